"""Clouds of the batched voxel head's tests (test_vox_head_cpu.py asserts their conditions with
numpy and the oracle alone, test_gpu_vosch_head.py runs them).  Plain functions, no GPU.

long_run_cloud: 5,000 points in the one voxel (50, 20, 70) at leaf 0.01, interleaved every third
  row with grsd_clouds.edge_cloud(): a voxel's points are far apart in the input and many, so
  its fp32 centroid depends on the summation order.
face_cloud: single points with x = z = float32(k) * float32(0.01), k = 1 .. 40, and their one-ulp
  neighbours below and above, each of the three families in a y band of its own so that every
  point keeps a voxel to itself: points on cell faces, where floor(p * (1 / leaf)) and
  floor(p / leaf) part and the voxel's centroid -- the point -- lies in another cell.
wide_key_cloud: the edge cloud with two anchor points that stretch its box to 513 x 513 x 257
  voxels (>= 2^26): with 64 frames the composite voxel key needs more than 32 bits.
status_clouds: one cloud per way a frame fails."""
import functools

import numpy as np

import grsd_clouds

LEAF = 0.01
LONG_CELL = (50, 20, 70)
LONG_N = 5000


def _rgb(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 24, n).astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def long_run_points(seed=23):
    """(LONG_N, 4) float32: base + U(0.0005, 0.0095) per axis inside LONG_CELL."""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(LONG_CELL) * LEAF + rng.uniform(0.0005, 0.0095, (LONG_N, 3))
    pts = np.empty((LONG_N, 4), np.float32)
    pts[:, :3] = xyz
    pts[:, 3] = _rgb(LONG_N, seed + 1)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def long_run_cloud():
    """Rows 0, 3, 6, ... are the long run's while the edge cloud lasts, then the rest of the run.
    Returns (cloud, rows of the run in input order)."""
    run, edge = long_run_points(), grsd_clouds.edge_cloud()
    k = len(edge) // 2
    assert k < LONG_N
    head = np.empty((3 * k, 4), np.float32)
    head[0::3] = run[:k]
    head[1::3] = edge[0:2 * k:2]
    head[2::3] = edge[1:2 * k:2]
    cloud = np.concatenate([head, edge[2 * k:], run[k:]])
    rows = np.concatenate([np.arange(0, 3 * k, 3), np.arange(3 * k + len(edge) - 2 * k, len(cloud))])
    cloud.setflags(write=False)
    return cloud, rows


def centroids(xyz):
    """fp32 centroids sum * fl(1 / n) of (n, 3) float32 points by four summation orders:
    input order (sequential), numpy's pairwise sum, reversed order, sorted order."""
    xyz = np.asarray(xyz, np.float32)
    rn = np.float32(1) / np.float32(len(xyz))

    def seq(a):
        return np.cumsum(a, axis=0, dtype=np.float32)[-1] * rn

    pairwise = np.array([np.sum(np.ascontiguousarray(xyz[:, a]), dtype=np.float32) for a in range(3)], np.float32)
    return dict(input=seq(xyz), pairwise=pairwise * rn, reversed=seq(xyz[::-1]), sorted=seq(np.sort(xyz, axis=0)))


def cells(xyz, leaf=LEAF):
    """(floor(p * fl(1 / leaf)), floor(p / leaf)) in float32: the voxeliser's cell, the centroid's."""
    xyz = np.asarray(xyz, np.float32)
    leaf = np.float32(leaf)
    inv = np.float32(1) / leaf
    return np.floor(xyz * inv).astype(np.int64), np.floor(xyz / leaf).astype(np.int64)


def lattice_values(kmax=40, leaf=LEAF):
    return np.arange(1, kmax + 1, dtype=np.float32) * np.float32(leaf)


@functools.lru_cache(maxsize=None)
def face_cloud():
    """(120, 4): per k the points (u, 0.005 + 0.5 g, u), u = (v - ulp, v, v + ulp)[g], v = float32(k) * float32(0.01)."""
    v = lattice_values()
    vals = np.stack([np.nextafter(v, np.float32(-1)), v, np.nextafter(v, np.float32(1))], 1)
    pts = np.empty((vals.size, 4), np.float32)
    pts[:, 0] = pts[:, 2] = vals.reshape(-1)
    pts[:, 1] = np.tile(np.float32(0.005) + np.float32(0.5) * np.arange(3, dtype=np.float32), len(v))
    pts[:, 3] = _rgb(vals.size, 31)
    pts.setflags(write=False)
    return pts


WIDE_ANCHORS = np.array([[-2.555, -2.555, 0.005], [2.565, 2.565, 2.565]])


@functools.lru_cache(maxsize=None)
def wide_key_cloud():
    edge = grsd_clouds.edge_cloud()
    anchors = np.zeros((2, 4), np.float32)
    anchors[:, :3] = WIDE_ANCHORS
    cloud = np.concatenate([anchors[:1], edge, anchors[1:]])
    cloud.setflags(write=False)
    return cloud


def key_bits(nvox, nframes):
    """Bits of the composite voxel key (vosch_frames.h vh_key): the values 0 .. nvox, the frames."""
    return max(int(nvox).bit_length(), 1) + max(int(nframes - 1).bit_length(), 1)


@functools.lru_cache(maxsize=None)
def status_clouds():
    """{name: cloud}: no valid point twice over, a cell beyond +-2^20, a div_b product above
    INT32_MAX, a box of more than 2^27 search cells at normals radius 0.004."""

    def pts(xyz):
        a = np.zeros((len(xyz), 4), np.float32)
        a[:, :3] = xyz
        a[:, 3] = _rgb(len(xyz), 41)
        a.setflags(write=False)
        return a

    rng = np.random.default_rng(43)
    box = rng.uniform((0.0, 0.0, 0.5), (2.56, 2.56, 2.0), (3000, 3))
    box[0], box[1] = (0.001, 0.001, 0.501), (2.559, 2.559, 1.999)
    return dict(no_point=pts(np.zeros((0, 3))), all_nan=pts(np.full((5, 3), np.nan)),
                far_x=pts([[2.0e4, 0.1, 0.9], [0.1, 0.1, 0.9]]), thirteen=pts([[0.0, 0.0, 0.5], [13.0, 13.0, 13.5]]),
                fine_box=pts(box))
