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
