"""The clouds of the sparse batched C3-HLAC-981 tests (test_c3_sparse_data_cpu.py,
test_gpu_c3_sparse.py): shapes at the edges of csrc/c3_sparse.hip -- its chunks of 1,024 voxels,
LDS slices of 128, plan tiles of 2,048 sorted positions, launches of at most 4,096 and 16,384
workgroups -- and the oracle's rows of a frame, computed once and shared.  Plain functions, no
GPU, read-only arrays.

ladder(lens, seed)   one point per voxel at the cell centres (cell + 0.5) * leaf, leaf 0.01, z from
                     cell 100 (convosch_data.py), for subdivision 13 at offset 0: block b is the
                     cells x in [13 b, 13 b + 13), its first lens[b] cells filled x-fastest, then y,
                     then z.  Row b of the frame holds exactly lens[b] voxels and the sorted order of
                     the sparse pass is the blocks in order.  The points are shuffled; the colours
                     come per channel from PALETTE, around the thresholds LADDER_THR and the ends
                     of the byte.  At offset (0, 1, 0) the cells of y = 0 feed no row: a row of at
                     most 13 voxels loses them all, and "none" keys stand behind the groups.
LADDER_A             rows of 2047, 2, 2047, 1024, 1025, 2048, 0, 1023, 128, 129, 127, 1, 2049 and 5
                     voxels: heads at the sorted positions 0, 2047 (a plan tile's last position, the
                     group straddles), 2049 (ends on 4095, a tile's end), 4096 (a tile's first, one
                     full chunk), 5120 (its second chunk is the one voxel at 6144, a tile's first),
                     6145, 8193, ...; the last group of 5 ends at vtot.
LADDER_B             2,048 voxels in rows of 129, 1024, 0, 767, 127 and 1: behind A its last head is
                     position vtot - 1, in front of A it moves every position of A by one whole
                     tile, so A's tile conditions hold in both arrangements, and its own one-voxel
                     group takes position 2047 with A's first head on 2048.
many_rows()          27 x 26 x 25 cells at occupancy 0.6, subdivision 1: 17,550 rows (the fill launches
                     16,384 workgroups) of which more than 4,096 hold a voxel (a chunk each: the
                     accumulate launches 4,096).
mixed_boxes()        64 small frames of extents 1 .. 19 per axis at different origins, occupancy
                     0.1 .. 0.9, for subdivision 4 with offset (1, 0, 2): non-cubic grids of different
                     div_b in one batch, frames of one and two voxels, frames without a row.
face_frames()        the face-heavy and by-hand frames of test_gpu_points_exact.py (20 .. 256 voxels
                     whose centroid lies in another cell), per (subdivision, offset) one batch."""
import functools

import numpy as np

import convosch_data as cd
import pyoracle as po
import test_gpu_points_exact as tpe
from conftest import THR

LEAF = cd.LEAF
RADIUS = 0.02  # the normals radius of the batches
LADDER_SUBDIV = 13
LADDER_OFFSETS = ((0, 0, 0), (0, 1, 0))
LADDER_THR = (64, 127, 200)
PALETTE = np.array([0, 63, 64, 65, 126, 127, 128, 199, 200, 201, 254, 255])
LADDER_A = (2047, 2, 2047, 1024, 1025, 2048, 0, 1023, 128, 129, 127, 1, 2049, 5)
LADDER_B = (129, 1024, 0, 767, 127, 1)
COLOR_MODES = (po.COLOR_C3_FLOAT, po.COLOR_C3_DOUBLE, po.COLOR_CHLAC)
MANY_SUBDIV = 1
MIXED_SUBDIV, MIXED_OFFSET = 4, (1, 0, 2)
PLAN_TILE, CHUNK, SLICE = 2048, 1024, 128  # kC3sPlanTile, kC3sChunk, kC3sSlice


@functools.lru_cache(maxsize=None)
def ladder(lens, seed):
    rng = np.random.default_rng(seed)
    cells = []
    for b, n in enumerate(lens):
        i = np.arange(n)
        cells.append(np.stack([LADDER_SUBDIV * b + i % 13, (i // 13) % 13, cd.Z0 + i // 169], 1))
    cells = np.concatenate(cells).astype(np.float64)
    rgb = PALETTE[rng.integers(0, len(PALETTE), (len(cells), 3))]
    order = rng.permutation(len(cells))
    return cd._cloud(cells[order], rgb[order])


def ladder_a():
    return ladder(LADDER_A, 21)


def ladder_b():
    return ladder(LADDER_B, 22)


def _random_box(rng, ext, p, origin):
    """Cells of an ext[0] x ext[1] x ext[2] box at occupancy p with both corner cells kept, random
    colours, shuffled."""
    occ = rng.random(tuple(ext)) < p
    occ[0, 0, 0] = occ[-1, -1, -1] = True
    cells = (np.argwhere(occ) + np.asarray(origin)).astype(np.float64)
    cells = cells[rng.permutation(len(cells))]
    return cd._cloud(cells, rng.integers(0, 256, (len(cells), 3)))


@functools.lru_cache(maxsize=None)
def many_rows(seed=31):
    return _random_box(np.random.default_rng(seed), (27, 26, 25), 0.6, (0, 0, cd.Z0))


ONE_CELL, TWO_VOXELS = (5, 17, 33), (9, 23, 40)  # frames of mixed_boxes


@functools.lru_cache(maxsize=None)
def mixed_boxes(seed=41):
    """[(n, 4) points] * 64.  Frames ONE_CELL are a single cell, frames TWO_VOXELS the two corner
    cells of their box."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(64):
        ext = rng.integers(1, 20, 3)
        origin = np.append(rng.integers(0, 60, 2), cd.Z0 + rng.integers(0, 60))
        p = rng.uniform(0.1, 0.9)
        if k in ONE_CELL:
            ext = np.array([1, 1, 1])
        if k in TWO_VOXELS:
            ext, p = np.maximum(ext, 3), 0.0
        out.append(_random_box(rng, ext, p, origin))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def no_point():
    pts = np.zeros((0, 4), np.float32)
    pts.setflags(write=False)
    return pts


# ---- the frames of test_gpu_points_exact.py ---------------------------------------------------
FACE, FACE_ONE = tpe.FACE, tpe.FACE_ONE
CM = po.COLOR_C3_DOUBLE


def _frozen(pts):
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def face_case(name):
    """(points, subdivision, offset) of a frame built for that subdivision and offset, by-hand
    voxels included: test_gpu_points_exact.py's generator, seeds and sizes."""
    if name == "face_s6":
        S, off, fr, shift = 6, (0, 0, 0), FACE, 0
    elif name == "face_s5":
        S, off, fr, shift = 5, (2, 1, 0), FACE, 0
    elif name == "one_s0":
        S, off, fr, shift = 0, (0, 0, 0), FACE_ONE, 0
    elif name == "one_s16":
        S, off, fr, shift = 16, (0, 0, 0), FACE_ONE, 0
    elif name in ("far_plus", "far_minus"):
        S, off, fr, shift = 6, (0, 0, 0), dict(seed=1402, n=2400, g=24, ff=0.15), 20000 if name == "far_plus" else -20000
    elif name.startswith("good_"):
        S, off, fr, shift = 6, (0, 0, 0), dict(seed=1410 + "abc".index(name[-1]), n=3600, g=24, ff=0.15), 0
    else:
        raise KeyError(name)
    return _frozen(tpe._face_frame(fr["seed"], fr["n"], fr["g"], fr["ff"], shift, S, off)), S, off


# per (subdivision, offset) one batch: the frames built for it first, then frames built for another
# subdivision, which are here plain face-heavy clouds (of several rows beside the one-row frame)
FACE_BATCHES = {
    (6, (0, 0, 0)): ("face_s6", "far_plus", "far_minus", "good_a", "good_b", "good_c", "one_s16"),
    (5, (2, 1, 0)): ("face_s5", "one_s16"),
    (16, (0, 0, 0)): ("one_s16", "face_s6", "good_a"),
    (0, (0, 0, 0)): ("one_s0", "face_s6"),
}


def face_frames():
    """{(subdivision, offset): [(name, points, built for this subdivision and offset)]}."""
    out = {}
    for (S, off), names in FACE_BATCHES.items():
        out[(S, off)] = []
        for n in names:
            pts, s, o = face_case(n)
            out[(S, off)].append((n, pts, (s, o) == (S, off)))
    return out


# ---- the oracle's view ------------------------------------------------------------------------
class Ref:
    pass


_REFS = {}


def reference(pts, leaf, subdiv, offset, thr, color_mode):
    """The oracle's rows of one frame, computed once per argument set and kept unchanged: fe (exact
    integer sums, one float multiply per bin), ex (the exist of the exact=False rows, as
    test_gpu_parity.py::test_extract_subdivision_cases takes it), sb, hn, the grid and the number
    of voxels whose centroid lies in another cell."""
    key = (id(pts), leaf, subdiv, tuple(offset), tuple(thr), color_mode)
    if key not in _REFS:
        po.set_voxel_semantics(True)
        r = Ref()
        r.pts = pts  # (keeps id(pts) taken)
        g, layout, cloud = po.voxelize(pts, leaf)
        r.g, r.layout, r.cloud = g, layout, cloud
        r.n_occ, r.n_valid = int(g.n_occ), int(g.n_valid)
        r.div_b, r.min_b = tuple(g.div_b), tuple(g.min_b)
        r.acting = np.floor(cloud[:, :3] / np.float32(leaf)).astype(np.int64) - np.array(r.min_b)
        occ = np.flatnonzero(layout >= 0)
        d = np.array(r.div_b)
        own = np.stack([occ % d[0], (occ // d[0]) % d[1], occ // (d[0] * d[1])], 1)
        r.n_moved = int((r.acting[layout[occ]] != own).any(1).sum())
        r.fe, r.sb, r.hn = po.c3hlac(g, layout, cloud, 981, thr, leaf, subdiv, offset, color_mode, exact=True)
        fa = po.c3hlac(g, layout, cloud, 981, thr, leaf, subdiv, offset, color_mode, exact=False)[0]
        r.ex = po.exist(fa)
        _REFS[key] = r
    return _REFS[key]


def row_counts(r, subdiv, offset):
    """(voxels per row (hn,), voxels that feed no row) of a reference: the subdivision of every
    acting cell with the float32 arithmetic of c3_hlac.cpp:349-356."""
    if r.hn <= 0:
        return np.zeros(0, np.int64), r.n_occ
    if r.hn == 1:  # one histogram: no centre test, offsets ignored
        return np.array([r.n_occ]), 0
    t = r.acting - np.array(offset)
    ijk = np.floor(t.astype(np.float32) * np.float32(1.0 / subdiv)).astype(np.int64)
    ok = (t >= 0).all(1) & (ijk < np.array(r.sb)).all(1)
    lin = ijk[ok, 0] + r.sb[0] * (ijk[ok, 1] + r.sb[1] * ijk[ok, 2])
    return np.bincount(lin, minlength=r.hn), int((~ok).sum())


def batch_positions(refs, subdiv, offset):
    """The sorted order of the sparse pass for a batch: (head position, length) of every group, in
    order, then the total number of voxels and the number of "none" keys behind the groups."""
    groups, pos, none, vtot = [], 0, 0, 0
    for r in refs:
        counts, n = row_counts(r, subdiv, offset)
        for c in counts:
            if c:
                groups.append((pos, int(c)))
                pos += int(c)
        none += n
        vtot += r.n_occ
    assert pos + none == vtot
    return groups, vtot, none

