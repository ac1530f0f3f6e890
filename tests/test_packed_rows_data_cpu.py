"""The clouds of the packed C3-HLAC rows tests without a GPU: the oracle alone shows the conditions
test_gpu_packed_rows.py and test_gpu_pca_from_clouds.py rely on.  Per case the number of rows with
exist > 0 (what c3h_extract_c3_frames_packed writes) and of rows without (what it leaves out); in
every case the non-empty groups of the sparse pass -- the rows that hold a voxel -- are exactly the
rows with exist > 0, so packing by group is packing by exist; in ladder_a an empty row lies between
groups; many_rows has more group heads than a plan tile has positions, so the packed ordinals
cross plan tiles; mixed_boxes has 12 frames without a row.  packed() itself builds the c3h_packed_row
fields from a c3h_extract_c3_frames_packed call's arguments.  Conditions on the inputs, not tolerances."""
import numpy as np
import pytest

import c3_rows_data as rd
import c3_sparse_data as sd
import packed_rows_data as pd_


@pytest.mark.parametrize("name", list(pd_.CASES))
def test_packed_and_empty_rows(name):
    make, subdiv, offset, thr, want_packed, want_empty = pd_.CASES[name]
    clouds = make()
    for variant in rd.VARIANTS:
        p = pd_.packed(clouds, subdiv, offset, thr, sd.CM, variant)
        total = sum(max(r.hn, 0) for r in p.refs)
        assert (p.n, total - p.n) == (want_packed, want_empty), (name, variant, p.n, total - p.n)
        assert p.rows.shape == (p.n, variant) and p.frame_first[-1] == p.n and (p.exist >= 1).all()
        # ordered by frame, then by row
        key = p.frame.astype(np.int64) * (1 << 40) + p.row
        assert (np.diff(key) > 0).all()
        for k, r in enumerate(p.refs):
            a, b = p.frame_first[k], p.frame_first[k + 1]
            assert (p.frame[a:b] == k).all()
            # the groups of the sparse pass are the rows with a voxel: exactly those with exist > 0
            counts, _ = sd.row_counts(r, subdiv, offset)
            assert np.array_equal(counts > 0, r.ex[:len(counts)] > 0) if r.hn > 0 else b == a, (name, variant, k)
            if r.hn > 0:
                assert np.array_equal(p.row[a:b], np.flatnonzero(counts > 0))


def test_ladder_a_has_an_empty_row_between_groups():
    r = rd.reference(sd.ladder_a(), rd.LEAF, sd.LADDER_SUBDIV, (0, 0, 0), sd.LADDER_THR, sd.CM, 117)
    empty = np.flatnonzero(r.ex == 0)
    assert empty.tolist() == [6] and r.ex[5] > 0 and r.ex[7] > 0


def test_many_rows_heads_cross_plan_tiles():
    r = rd.reference(sd.many_rows(), rd.LEAF, sd.MANY_SUBDIV, (0, 0, 0), pd_.THR, sd.CM, 117)
    counts, none = sd.row_counts(r, sd.MANY_SUBDIV, (0, 0, 0))
    heads = int((counts > 0).sum())
    assert heads == 10491 > sd.PLAN_TILE and none == 0
    assert (counts[counts > 0] == 1).all()  # a head per sorted position: tiles 0 .. 4 full of heads, tile 5 partly
    assert -(-r.n_occ // sd.PLAN_TILE) == 6


def test_mixed_boxes_frames_without_a_row():
    p = pd_.packed(list(sd.mixed_boxes()), sd.MIXED_SUBDIV, sd.MIXED_OFFSET, pd_.THR, sd.CM, 117)
    rowless = int((np.diff(p.frame_first) == 0).sum())
    assert rowless == pd_.MIXED_ROWLESS and len(p.refs) == 64
