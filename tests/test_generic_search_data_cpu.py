"""The inputs of the generic-route cases (generic_search_data.py), checked with the oracle alone:
every case stays off the fast route, leaves a partial last workgroup, gates about half of its
positions, carries rows whose exist is 0, and has a clear rank-1 pick per model; and the fp32
restatement of the route meets the float64 oracle within half of SCORE_RTOL_F64, so that bound is
within reach of a faithful fp32 kernel.

Worst relative error of the restatement against the float64 oracle, as this test measures it
(printed with -s; the bound is 5e-6):
  G1 5.1e-7   G2 4.6e-7   G3 2.2e-7   G4 3.2e-7   G5 6.3e-7   G6 5.2e-7   G7 2.4e-7   G8 4.1e-7"""
import numpy as np
import pytest

import generic_search_data as gd
import pyoracle as po
from generic_search_data import SCORE_RTOL_F64


@pytest.mark.parametrize("name", gd.NAMES)
def test_case_stays_off_the_fast_route(name):
    c = gd.CASES[name]
    assert c["D"] > 160  # score_fast_ok, score_mfma_ok and score_tick_wide_ok all need D <= 160
    assert c["F"] >= c["D"] and (c["r"] <= c["D"] or c.get("random_q"))
    if c.get("uncompressed"):
        assert c["F"] == c["D"] and gd.case(name)["ap"] is None
    else:
        assert gd.case(name)["ap"].shape == (c["D"], c["F"])
    assert gd.case(name)["axis_q"].shape == (c["M"], c["r"], c["D"])


def test_table_reaches_what_it_names():
    C = gd.CASES
    assert C["G1"]["D"] % 128 == 36 and C["G1"]["D"] % 16 == 4      # second column block, 4-column tail
    assert C["G2"]["r"] > 64 and C["G2"]["r"] % 4 != 0
    assert len(gd.modes(C["G2"]["sb"], C["G2"]["box"], True)) == 6
    assert C["G3"]["D"] == 256 and C["G4"]["D"] > 256               # both sides of the kernel threshold
    assert -(-C["G5"]["D"] // 128) == 8
    assert C["G6"]["D"] % 4 != 0 and C["G6"]["F"] % 128 == 72 and C["G6"]["r"] < 4
    assert C["G7"]["D"] > 256 and C["G7"]["r"] < 16
    assert [gd.positions_per_workgroup(C[n]["D"], C[n]["r"]) for n in gd.NAMES] == [64, 64, 64, 16, 16, 64, 16, 16]
    assert C["G8"]["D"] <= 256 and gd.positions_per_workgroup(164, 473) == 64  # the last r that fits 64 positions
    for name in ("G4", "G5"):  # feature_max: a zero entry, an entry equal to a row's value
        c = gd.case(name)
        assert (c["fmax"] == 0).sum() == 1 and (c["f"][:, c["fmax"] > 0] == c["fmax"][c["fmax"] > 0]).any()
        fn = gd.normalise(c["f"], c["fmax"])
        assert not fn[:, c["fmax"] == 0].any() and fn.max() > 1  # values above the max stay above 1


@pytest.mark.parametrize("name", gd.NAMES)
def test_some_mode_leaves_a_partial_workgroup(name):
    c = gd.CASES[name]
    sp = gd.positions_per_workgroup(c["D"], c["r"])
    ps = [e[0] * e[1] * e[2] for _, _, e in gd.modes(c["sb"], c["box"], c["rotate"])]
    assert ps and any(p % sp for p in ps), (sp, ps)
    assert max(ps) > sp  # more than one workgroup


@pytest.mark.parametrize("name", gd.NAMES)
def test_gate(name):
    c = gd.case(name)
    f, ex = c["f"], c["ex"]
    assert (f >= 0).all() and np.array_equal(f, np.floor(f))
    empty = ~f.any(1)
    assert 0.2 < empty.mean() < 0.4
    assert not ex[empty].any() and (ex >= 0).all()
    assert ((ex == 0) & ~empty).sum() >= 10  # rows with data that the gate does not count
    eb = np.concatenate(gd.exist_box_sums(c["sb"], ex, c["box"], c["rotate"]))
    share = (eb > c["thr"]).mean()
    assert 0.25 <= share <= 0.75, share
    # the oracle gates the same positions, and none of them holds a zero compressed box
    _, scd = gd.oracle(name)
    blocks = gd.mode_blocks(scd, c["M"], c["sb"], c["box"], c["rotate"])
    gate = np.concatenate([np.repeat((b > c["thr"])[None], c["M"], 0).reshape(-1)
                           for b in gd.exist_box_sums(c["sb"], ex, c["box"], c["rotate"])])
    assert np.array_equal(scd >= 0, gate)
    for (_, sc), nrm in zip(blocks, gd.box_norms64(name)):
        assert (nrm[sc[0] >= 0] > 0).all()
    assert np.isfinite(scd).all() and (scd[scd >= 0] > 0).all()
    # a row with exist 0 and data lies in some passing box: dropping its data would show
    sb = c["sb"]
    hid = ((ex == 0) & ~empty).reshape(sb[2], sb[1], sb[0]).astype(np.int64)
    hits = sum(int(((gd._box_sum(hid, r3, e) > 0) & (sc[0] >= 0)).sum())
               for (_, r3, e), (_, sc) in zip(gd.modes(sb, c["box"], c["rotate"]), blocks))
    assert hits >= 10, hits


@pytest.mark.parametrize("name", gd.NAMES)
def test_fp32_restatement_meets_the_oracle(name):
    _, scd = gd.oracle(name)
    s32 = gd.restate32(name)
    assert s32.shape == scd.shape
    assert np.array_equal(s32 == -1.0, scd == -1.0)
    ok = scd > 0
    assert ok.any()
    err = np.abs(s32[ok] - scd[ok]) / scd[ok]
    print("%s: fp32 restatement vs float64 oracle, worst relative error %.3g" % (name, err.max()))
    assert err.max() <= SCORE_RTOL_F64 / 2, err.max()


@pytest.mark.parametrize("name", gd.NAMES)
def test_float64_compress_agrees_with_the_oracle_scores(name):
    """compress64 is the compress the oracle's scores come from: scores recomputed from it in
    float64 (direct box sums) meet the oracle's to 1e-9."""
    c = gd.case(name)
    _, scd = gd.oracle(name)
    sb = c["sb"]
    gv = gd.compress64(name)[0].reshape(sb[2], sb[1], sb[0], -1)
    q = c["axis_q"].astype(np.float64)
    for (_, r3, e), (_, sc) in zip(gd.modes(sb, c["box"], c["rotate"]),
                                   gd.mode_blocks(scd, c["M"], sb, c["box"], c["rotate"])):
        fb = gd._box_sum(gv, r3, e)
        pr = np.einsum("mrd,pd->mpr", q, fb)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.sqrt((pr * pr).sum(2)) / np.sqrt((fb * fb).sum(1))[None]
        ok = sc > 0
        np.testing.assert_allclose(s[ok], sc[ok], rtol=1e-9)


def _clear_picks(c, sb, L, scd):
    blocks = gd.mode_blocks(scd, c["M"], sb, c["box"], c["rotate"])
    for m in range(c["M"]):
        allm = np.concatenate([sc[m] for _, sc in blocks])
        top2 = np.sort(allm)[-2:]
        assert top2[1] > 0 and (top2[1] - top2[0]) / top2[1] > 4 * SCORE_RTOL_F64, (m, top2)
        assert L.records()[m][0][0] == top2[1]


@pytest.mark.parametrize("name", ["G1", "G4"])
def test_batch_frames(name):
    """The three frames of the batch entry points: every frame gates some positions and not all,
    the flat one fits the box in some modes only, and every pick is clear."""
    c = gd.batch_case(name)
    assert [len(gd.modes(sb, c["box"], c["rotate"])) for sb in gd.BATCH_SUBDIVS] == [6, 6, 2]
    for i, (sb, f, ex) in enumerate(gd.batch_frames()):
        L, scd = gd.batch_oracle(name, i)
        assert 0.1 < (scd >= 0).mean() < 0.9
        _clear_picks(c, sb, L, scd)


@pytest.mark.parametrize("route", ["generic", "fast"])
def test_list_state_cases(route):
    c = gd.list_state_case(route)
    assert (c["D"] > 160) == (route == "generic") and c["rank"] == 4 and c["rotate"]
    if route == "fast":
        assert c["D"] % 4 == 0 and c["r"] <= 64  # score_fast_ok
    eb = np.concatenate(gd.exist_box_sums(c["sb"], c["ex"], c["box"], c["rotate"]))
    assert 0.25 <= (eb > c["thr"]).mean() <= 0.75
    # the records fill every rank, span several modes, and removeOverlap has something to remove
    L, _ = gd.oracle_search(c, c["sb"], c["f"], c["ex"], c["rank"])
    before = L.records()
    assert all(e[0] > 0 for m in before for e in m) and len({e[4] for m in before for e in m}) > 1
    assert po.remove_overlap(L, c["box"]).records() != before


@pytest.mark.parametrize("name", gd.NAMES)
def test_rank1_pick_is_clear(name):
    """Every model's best float64 score leads every other position by more than 4 x the score
    tolerance, so a GPU within tolerance must pick the oracle's position: no tie clause."""
    c = gd.case(name)
    L, scd = gd.oracle(name)
    blocks = gd.mode_blocks(scd, c["M"], c["sb"], c["box"], c["rotate"])
    for m in range(c["M"]):
        allm = np.concatenate([sc[m] for _, sc in blocks])
        top2 = np.sort(allm)[-2:]
        assert top2[1] > 0 and (top2[1] - top2[0]) / top2[1] > 4 * SCORE_RTOL_F64, (m, top2)
        assert L.records()[m][0][0] == top2[1]
