"""The frames of the batched VOSCH / GRSD tests (test_vosch_frames_cpu.py,
test_gpu_vosch_frames.py).  Plain functions, no GPU.

One batch at leaf 0.01, normals radius 0.02, subdivision 4 with offset (1, 0, 2): the four
shape clouds of test_gpu_grsd.py, a real Kinect view (bowl1_0000.pcd), grsd_clouds.edge_cloud() with its non-finite rows and stragglers, a
one-point and a zero-point cloud.  z_limit is an argument of the call, not of a frame: the
batch runs once without a limit and once behind z_limit = 1.0, which cuts the edge cloud's
plane and sphere.  At leaf 0.01 the Kinect view has no voxel whose centroid lies in another
cell (206 voxels; the edge cloud has one), so a second, fine batch holds it and the torus at
leaf 0.004: 945 voxels, 14 of them with their centroid in another cell."""
import functools

import numpy as np

import c3hlac
import grsd_clouds
from conftest import GOLDEN

PCD = GOLDEN / "ref_fixtures" / "pcd"
SHAPES = ["noiseless_cone_red", "noisy_sphere_green", "noisy_torus_blue", "noisy_plane_purple"]
LEAF, RADIUS, SUBDIV, OFFSET = 0.01, 0.02, 4, (1, 0, 2)
Z_LIMITS = (float("inf"), 1.0)
FINE_LEAF = 0.004


@functools.lru_cache(maxsize=None)
def batch():
    """[(name, (n, 4) float32 points)], read-only arrays."""
    out = [(s, c3hlac.read_pcd(PCD / (s + ".pcd"))) for s in SHAPES]
    out.append(("bowl1_0000", c3hlac.read_pcd(PCD / "bowl1_0000.pcd")))
    out.append(("edge", grsd_clouds.edge_cloud()))
    out.append(("one_point", np.array([[0.1, 0.2, 0.7, 0.0]], np.float32)))
    out.append(("no_point", np.zeros((0, 4), np.float32)))
    for _, p in out:
        p.setflags(write=False)
    return out


def fine_batch():
    d = dict(batch())
    return [(k, d[k]) for k in ("bowl1_0000", "noisy_torus_blue")]


def moved_voxels(g, layout, cloud, leaf):
    """Occupied voxels whose centroid lies in another cell than their own (oracle voxelize)."""
    occ = np.flatnonzero(layout >= 0)
    d = np.array(g.div_b[:3])
    own = np.stack([occ % d[0], (occ // d[0]) % d[1], occ // (d[0] * d[1])], 1) + np.array(g.min_b[:3])
    c = cloud[layout[occ], :3]
    return int((np.floor(c / np.float32(leaf)) != own).any(1).sum())


def subdivisions(div_b, subdiv=SUBDIV, offset=OFFSET):
    """getSubdivNum of a grid (grsd_colorCHLAC_tools.hpp:150-162), (0, 0, 0) where an offset
    reaches the grid's end."""
    if any(int(div_b[a]) <= offset[a] for a in range(3)):
        return (0, 0, 0)
    inv_s = np.float32(1.0 / subdiv)
    return tuple(int(np.ceil(np.float32((int(div_b[a]) - offset[a]) * inv_s))) for a in range(3))


# ---- the dense-cell pin (test_gpu_vosch_frames.py::test_cell_staged_normals_equal_the_per_point_walk) ----
# In a batch a search cell (side = the normals radius r) of DENSE_MIN points and more is served by
# the cell-staged normals kernel, a cell of fewer by the per-point walk.  Cloud B keeps every cell
# below that; cloud A is B plus fillers that lift the chosen cells over it without entering any
# compared query's neighbourhood: the same queries go through the other kernel, with the same
# neighbours in the same order.
DENSE_MIN = 16
PIN_CELLS = [(2 + 3 * i, 2 + 3 * j, 2) for i in range(4) for j in range(2)]  # (cx, cy, cz) of the search grid
PIN_QUERIES, PIN_CONTEXT, PIN_FILL, PIN_FILL_BIG = 5, 9, 16, 62


@functools.lru_cache(maxsize=None)
def dense_pin_clouds(seed=11):
    """(A, B, query rows): B = two anchors that pin the voxel box to cells (0, 0, 98) .. (39, 39,
    105) at LEAF, a sparse noisy plane at z = 1.03, and per chosen cell PIN_QUERIES queries in its
    low corner (local [0.02, 0.18] r) among PIN_CONTEXT points scattered around that corner;
    A = B + PIN_FILL fillers per chosen cell (PIN_FILL_BIG in the first: 65 points and more) in
    the high corner (local [0.87, 0.98] r)."""
    rng = np.random.default_rng(seed)
    r = RADIUS
    origin = np.array([0.0, 0.0, 0.98]) - r  # of the search grid: min_b * leaf - r
    parts = [np.array([[0.005, 0.005, 0.985], [0.395, 0.395, 1.055]])]
    plane = np.empty((1500, 3))
    plane[:, :2] = rng.uniform(0.01, 0.39, (1500, 2))
    plane[:, 2] = 1.03 + rng.normal(0, 0.0005, 1500)
    parts.append(plane)
    n0 = sum(len(p) for p in parts)
    queries, fill = [], []
    for k, c in enumerate(PIN_CELLS):
        corner = origin + np.array(c) * r
        parts.append(corner + rng.uniform(-0.5 * r, 0.6 * r, (PIN_CONTEXT, 3)))
        parts.append(corner + rng.uniform(0.02 * r, 0.18 * r, (PIN_QUERIES, 3)))
        n0 += PIN_CONTEXT
        queries.extend(range(n0, n0 + PIN_QUERIES))
        n0 += PIN_QUERIES
        fill.append(corner + rng.uniform(0.87 * r, 0.98 * r, (PIN_FILL_BIG if k == 0 else PIN_FILL, 3)))

    def cloud(xyz):
        pts = np.zeros((len(xyz), 4), np.float32)
        pts[:, :3] = xyz
        pts[:, 3] = (np.arange(len(xyz), dtype=np.uint32) * 2654435761 >> 8).astype(np.uint32).view(np.float32)
        pts.setflags(write=False)
        return pts

    b = np.concatenate(parts)
    return cloud(np.concatenate([b] + fill)), cloud(b), np.array(queries)


def search_cells(pts, min_b, div_b, leaf=LEAF, radius=RADIUS):
    """The search cell (linear index, -1 outside) of every point, with the float32 formulas of
    vf_nbr_grid (vosch_frames.h) and cell_of (rsd_dev.h); also the grid's dims."""
    leaf32, r32 = np.float32(leaf), np.float32(radius)
    lo = np.asarray(min_b, np.float64) * np.float64(leaf32)
    hi = (np.asarray(min_b, np.float64) + np.asarray(div_b, np.float64)) * np.float64(leaf32)
    origin = (lo - np.float64(r32)).astype(np.float32)
    dim = np.ceil((hi - lo) / np.float64(r32)).astype(np.int64) + 3
    inv = np.float32(1) / r32
    t = np.floor((pts[:, :3].astype(np.float32) - origin) * inv)
    ok = ((t >= 0) & (t < dim.astype(np.float32))).all(1)
    c = t.astype(np.int64)
    return np.where(ok, c[:, 0] + dim[0] * (c[:, 1] + dim[1] * c[:, 2]), -1), dim


def check_dense_pin(a, b, queries, grid_a, grid_b, radius=RADIUS):
    """Asserts what the pin rests on; grid_x = (min_b, div_b) of cloud x's voxelization."""
    assert tuple(grid_a[0]) == tuple(grid_b[0]) and tuple(grid_a[1]) == tuple(grid_b[1])  # same box: same search grid
    assert np.array_equal(a[:len(b)], b)
    ca, dim = search_cells(a, *grid_a)
    cb, _ = search_cells(b, *grid_b)
    assert (ca >= 0).all() and np.bincount(cb).max() < DENSE_MIN  # B: the per-point walk everywhere
    chosen = np.unique(cb[queries])
    want = [c[0] + dim[0] * (c[1] + dim[1] * c[2]) for c in PIN_CELLS]
    assert sorted(chosen) == sorted(want) and len(chosen) >= 8 and len(queries) >= 32
    na = np.bincount(ca, minlength=int(dim.prod()))
    assert (na[chosen] >= DENSE_MIN).all() and na[chosen].max() >= 65  # A: cell-staged, one cell in two passes
    fillers = a[len(b):, :3].astype(np.float32)
    assert np.isin(ca[len(b):], chosen).all()
    q = b[queries, :3].astype(np.float32)
    d = fillers[:, None, :] - q[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]  # float32, as pair_d2 adds
    assert d2.dtype == np.float32 and (d2 >= np.float32(radius) * np.float32(radius)).all()  # no filler is a neighbour
    dq = q[:, None, :] - b[None, :, :3].astype(np.float32)
    nb = ((dq[..., 0] * dq[..., 0] + dq[..., 1] * dq[..., 1]) + dq[..., 2] * dq[..., 2]) < np.float32(radius) * np.float32(radius)
    assert (nb.sum(1) >= 3).all() and nb.sum(1).max() > PIN_QUERIES  # neighbours beyond the query cluster
    local = (q - ((np.asarray(grid_b[0]) * np.float64(np.float32(LEAF)) - radius).astype(np.float32)
                  + np.array([[(c % dim[0]), (c // dim[0]) % dim[1], c // (dim[0] * dim[1])] for c in cb[queries]]) * np.float32(radius)))
    assert (local >= 0).all() and (local <= 0.2 * radius).all()
