"""The clouds of c3_rows_data.py without a GPU: the oracle alone shows the conditions
test_gpu_c3_rows.py relies on at variant 117 -- first-order sums beyond 2^32 (white_cube in one
row), below it at subdivision 10, between 2^31 and 2^32 (ladder_a in one row: the signed-overflow
edge of a 32-bit cross-chunk sum), and group lengths around the 117 kernel's slice of 64 voxels.
Conditions on the inputs, not tolerances."""
import numpy as np
import pytest

import c3_rows_data as rd
import c3_sparse_data as sd
import pyoracle as po

ZERO = (0, 0, 0)
THR = sd.LADDER_THR


# A raw sum is recovered from an f32 bin (one conversion and one multiply: two roundings of 2^-24
# each) by a float64 division, so it is known to 2^-22 of its value
REL = 2.0 ** -22


def _near(raw, want):
    return abs(raw - want) <= REL * want


def _raw(pts, subdiv, cm):
    return rd.raw_first_order(rd.reference(pts, rd.LEAF, subdiv, ZERO, THR, cm, 117))


def test_white_cube_shape():
    r = rd.reference(rd.white_cube(), rd.LEAF, 0, ZERO, THR, po.COLOR_CHLAC, 117)
    assert r.div_b == (20, 20, 20) and r.n_occ == 8000 and r.n_moved == 0 and r.hn == 1
    assert rd.reference(rd.white_cube(), rd.LEAF, 20, ZERO, THR, po.COLOR_CHLAC, 117).hn == 1
    assert rd.reference(rd.white_cube(), rd.LEAF, 10, ZERO, THR, po.COLOR_CHLAC, 117).hn == 8
    assert sd.row_counts(r, 0, ZERO)[0].tolist() == [8000]  # 8 chunks: 7 full ones and one of 832


@pytest.mark.parametrize("cm", sd.COLOR_MODES)
def test_white_cube_sums_pass_2_32(cm):
    for subdiv in (0, 20):
        raw = _raw(rd.white_cube(), subdiv, cm)
        assert raw > 2.0 ** 32, (subdiv, raw)
        if cm in (po.COLOR_CHLAC, po.COLOR_C3_FLOAT):
            assert _near(raw, 6_083_478_900), (subdiv, raw)
        else:
            assert 6.03e9 < raw < 6.04e9, (subdiv, raw)
    raw10 = _raw(rd.white_cube(), 10, cm)
    assert 7.0e8 < raw10 < 2.0 ** 32 and raw10 < 8.7e8, raw10


def test_white_cube_bin6_is_pairs_times_65025():
    r = rd.reference(rd.white_cube(), rd.LEAF, 0, ZERO, THR, po.COLOR_CHLAC, 117)
    raw6 = float(np.float64(r.fe[0, 6]) / np.float64(rd.NORM117_1))
    assert _near(raw6, 93_556 * 65_025) and 93_556 * 65_025 == 6_083_478_900


def test_ladder_a_one_row_sits_between_2_31_and_2_32():
    raw = _raw(sd.ladder_a(), 0, sd.CM)
    assert 2.0 ** 31 < raw < 2.0 ** 32, raw
    assert _near(raw, 3_729_551_872), raw
    r = rd.reference(sd.ladder_a(), rd.LEAF, 0, ZERO, THR, sd.CM, 117)
    assert r.hn == 1 and -(-r.n_occ // sd.CHUNK) == 12  # one row of 12 chunks


def test_slice_ladder_group_lengths():
    """The 117 kernel stages 64 voxels at a time: groups of a slice less one, one slice, a slice and
    one, three slices less one, three slices, three slices and one; the ladders of c3_sparse_data
    add 2 x 64 and 16 x 64 with their neighbours."""
    S = rd.SLICE117
    r = rd.reference(rd.slice_ladder(), rd.LEAF, sd.LADDER_SUBDIV, ZERO, THR, sd.CM, 117)
    counts, none = sd.row_counts(r, sd.LADDER_SUBDIV, ZERO)
    assert counts.tolist() == list(rd.SLICE_LADDER) and none == 0 and r.n_moved == 0
    for n in (1, S - 1, S, S + 1, 3 * S - 1, 3 * S, 3 * S + 1):
        assert n in counts
    assert sd.CHUNK % S == 0 and sd.SLICE == 2 * S
    for n in (2 * S - 1, 2 * S, 2 * S + 1, 16 * S - 1, 16 * S, 16 * S + 1, 32 * S - 1, 32 * S, 32 * S + 1):
        assert n in sd.LADDER_A + sd.LADDER_B
    assert r.ex[5] == 0 and (np.delete(r.ex, 5) > 0).all()
