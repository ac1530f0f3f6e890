"""The clouds of the ConVOSCH tests (test_convosch_cpu.py, test_gpu_convosch.py) beyond the
frames of vosch_frames_data.py.  Plain functions, no GPU.

Two clouds of one point per voxel at the cell centres (i + 0.5) * leaf, leaf 0.01, z from cell
100 (so every centroid lies in its own cell):

white_plane()  300 x 300 x 1 cells, colour (255, 255, 255), subdiv 0: one row whose second-order
               sums pass 2^32 (test_convosch_cpu.py), and a group of 90,000 voxels, which the
               sparse batched C3-HLAC-981 sums in several chunks.
dense_cube()   12 x 12 x 12 cells of seeded random colours, subdiv 10, offset 0: 8 rows of
               1,000, 200, 40 and 8 voxels; row 0 has every neighbour present."""
import functools

import numpy as np

LEAF = 0.01
Z0 = 100
PLANE_SUBDIV, CUBE_SUBDIV = 0, 10
CUBE_EXIST = [2528, 505, 512, 101, 505, 101, 100, 20]
THR_MID = (127, 127, 127)


def _cloud(cells, rgb):
    pts = np.zeros((len(cells), 4), np.float32)
    pts[:, :3] = ((cells + 0.5) * LEAF).astype(np.float32)
    word = (rgb[:, 0].astype(np.uint32) << 16) | (rgb[:, 1].astype(np.uint32) << 8) | rgb[:, 2].astype(np.uint32)
    pts[:, 3] = word.view(np.float32)
    pts.setflags(write=False)
    return pts


def _cells(nx, ny, nz):
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel() + Z0], 1).astype(np.float64)


@functools.lru_cache(maxsize=None)
def white_plane():
    cells = _cells(300, 300, 1)
    return _cloud(cells, np.full((len(cells), 3), 255, np.int64))


@functools.lru_cache(maxsize=None)
def dense_cube(seed=5):
    cells = _cells(12, 12, 12)
    return _cloud(cells, np.random.default_rng(seed).integers(0, 256, (len(cells), 3)))
