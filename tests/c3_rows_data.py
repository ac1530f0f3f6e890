"""The clouds and oracle rows of the batched C3-HLAC rows tests (test_c3_rows_data_cpu.py,
test_gpu_c3_rows.py): c3h_extract_c3_frames at variants 981 and 117.  The clouds of
c3_sparse_data.py (imported, not copied) stand at the edges the 117 kernel shares with the 981
one -- chunks of 1,024 voxels, plan tiles of 2,048 sorted positions, the launches' workgroup counts
-- and, with group lengths 1, 127 .. 129, 1023 .. 1025 and 2047 .. 2049, on both sides of its own
slices of 64 voxels (kC3s117Slice: 127, 128, 129 = 2 x 64 - 1, 2 x 64, 2 x 64 + 1; 1023 .. 1025 the
same around 16 slices); SLICE_LADDER adds the lengths around one slice.

white_cube()   20 x 20 x 20 cells, one point per cell at the cell centre, colour (255, 255, 255),
               z from convosch_data.Z0: 8,000 voxels in one row at subdivision 0 and 20.  Its
               first-order 117 sums (13 neighbours x 255 x 255 per voxel) pass 2^32: the 64-bit
               cross-chunk slots.
reference()    the oracle's rows of one frame at a variant, computed once and kept unchanged."""
import functools

import numpy as np

import c3_sparse_data as sd
import convosch_data as cd
import pyoracle as po

LEAF = sd.LEAF
VARIANTS = (981, 117)
SLICE117 = 64  # kC3s117Slice
SLICE_LADDER = (63, 64, 65, 1, 191, 0, 192, 193)
NORM117_1 = np.float32(1.0 / 845325.0)  # kNorm117_1: columns 6 .. 41 of a 117 row


@functools.lru_cache(maxsize=None)
def white_cube():
    cells = cd._cells(20, 20, 20)
    return cd._cloud(cells, np.full((len(cells), 3), 255, np.int64))


def slice_ladder():
    return sd.ladder(SLICE_LADDER, 23)


class Ref:
    pass


_REFS = {}


def reference(pts, leaf, subdiv, offset, thr, color_mode, variant):
    """As c3_sparse_data.reference, with fe / ex of `variant`: the geometry, counts and n_moved are
    that reference's own (shared with the 981 tests), the 117 rows are computed here once."""
    base = sd.reference(pts, leaf, subdiv, offset, thr, color_mode)
    if variant == 981:
        return base
    key = (id(pts), leaf, subdiv, tuple(offset), tuple(thr), color_mode, variant)
    if key not in _REFS:
        po.set_voxel_semantics(True)
        r = Ref()
        r.__dict__.update(base.__dict__)
        r.fe, r.sb, r.hn = po.c3hlac(base.g, base.layout, base.cloud, variant, thr, leaf, subdiv, offset, color_mode,
                                     exact=True)
        fa = po.c3hlac(base.g, base.layout, base.cloud, variant, thr, leaf, subdiv, offset, color_mode, exact=False)[0]
        r.ex = po.exist(fa)
        assert tuple(r.sb) == tuple(base.sb) and r.hn == base.hn
        _REFS[key] = r
    return _REFS[key]


def raw_first_order(r):
    """The largest raw first-order sum of a 117 reference: a bin of columns 6 .. 41 divided by
    fl(1 / 845325), in float64."""
    return float((r.fe[:, 6:42].astype(np.float64) / np.float64(NORM117_1)).max())
