"""The inputs of the fast-route cases (fast_search_data.py), checked with the oracle alone: every
case reaches the kernel edges its table row names (the route restated as plain arithmetic), lists
a ragged number of positions, keeps its scores away from 0, has a clear rank-1 pick per model and
sees its own edge (one fault of the kind the edge invites moves a float64 score by more than
10 x the bound); and the fp32 restatement of the route meets the float64 oracle within a quarter
of SCORE_RTOL_F64, so that bound is within reach of a faithful fp32 kernel.

Worst relative error of the restatement against the float64 oracle, as this test measures it
(printed with -s; the bound is 2.5e-6):
  F1 2.2e-7   F2 2.2e-7   F3 9.9e-7   F4 4.4e-7   F5 2.8e-7   F6 3.7e-7   F7 2.7e-7   F8 2.5e-7
  F9 3.7e-7   F10 4.0e-7  F11 4.1e-7  F12 3.7e-7  F13 4.5e-7  F14 4.6e-7  F15 8.1e-7  F16 4.3e-7
  F17 3.7e-7  F18 2.9e-7  W1 2.6e-7   W2 4.3e-7   F19 3.4e-7  W3 3.2e-7"""
import numpy as np
import pytest

import fast_search_data as fs
import generic_search_data as gd
from conftest import THR
from fast_search_data import SCORE_RTOL_F64


def test_route_facts():
    """What each table row says it reaches, from the code's own arithmetic."""
    C = fs.CASES
    D = {n: fs.dpad(c["D"]) for n, c in C.items()}
    assert all(d <= 160 and d % 4 == 0 for d in D.values())                  # score_mfma_ok; score_fast_ok with r <= 64
    assert D["F2"] == 8 and D["F15"] == 132 and all(D[n] == C[n]["D"] for n in C if n not in ("F2", "F15"))
    # score_mfma_kernel<KP>: both ends of every instantiation
    kp = {n: fs.mfma_kp(C[n]["D"]) for n in C}
    assert kp["F19"] == 52 and kp["W3"] == 64
    assert [kp[n] for n in fs.NAMES[:18]] == [16, 16, 16, 16, 24, 24, 32, 32, 40, 40, 52, 52, 64, 64, 72, 72, 80, 80]
    for lo, hi in (("F5", "F6"), ("F7", "F8"), ("F9", "F10"), ("F11", "F12"), ("F13", "F14"), ("F15", "F16"), ("F17", "F18")):
        assert fs.mfma_kp(D[lo] - 4) < kp[lo] == kp[hi] < (fs.mfma_kp(D[hi] + 4) if D[hi] < 160 else 99)
    assert kp["F4"] == 16 and fs.mfma_kp(D["F4"] + 4) == 24 and 16 - D["F1"] // 2 == 14  # zero k-pairs of F1
    # VALU groups
    assert fs.valu_groups(1, 1) == (64, [1])
    assert fs.valu_groups(33, 2) == (32, [32, 1])                            # F3: a second group of one model
    assert fs.valu_groups(4, 32) == (2, [2, 2]) and 2 * 32 == fs.KOC         # F4: the full window
    assert fs.valu_groups(7, 12) == (5, [5, 2])                              # F5
    assert fs.valu_groups(2, 33) == (1, [1, 1]) and (33 + 15) // 16 * 16 == 48  # F6: 48-column window
    assert fs.valu_groups(2, 64) == (1, [1, 1])                              # F8
    assert fs.valu_groups(1, 63) == (1, [1]) and (63 + 15) // 16 * 16 - 63 == 1  # F10: one padding column
    assert fs.valu_groups(9, 7) == (9, [9])                                  # F11: one group of 9
    assert fs.valu_groups(9, 64) == (1, [1] * 9)                             # F18
    # the group loop switches on between D = 32 and D = 36
    assert not fs.group_loop(32, 4, 32) and fs.group_loop(36, 7, 12)
    assert 32 * fs.KOC < fs.KFP * (fs.KOC + 1) <= 36 * fs.KOC
    assert not fs.group_loop(84, 9, 7)                                       # one group: nothing to loop over
    # chunks of 32 basis columns (score_mfma_kernel, the tick's tiles)
    cols = {n: C[n]["M"] * C[n]["r"] for n in C}
    assert cols["F2"] == 6 and cols["F9"] == 65 and cols["F9"] % fs.KSMC == 1  # a last chunk of one column
    assert all((m + 1) * 32 % fs.KSMC == 0 for m in range(4))                # F4: models end on chunk ends
    assert 33 % fs.KSMC == 1                                                 # F6: one column into the next chunk
    # F14: 9 tiles; 8 models would be 8 tiles, but the VALU body's LDS holds 7: two passes (7 + 2 models)
    assert cols["F14"] == 270 and -(-270 // 32) == 9 and -(-8 * 30 // 32) == 8 and fs.tick_mpp(128, 9, 30) == 7
    assert fs.tick_mpp(160, 9, 64) == 4 and fs.tick_mpp(4, 1, 1) == 1       # F18: three passes (4 + 4 + 1)
    assert fs.tick_mpp(8, 33, 2) == 32 and fs.tick_mpp(32, 4, 32) == 2      # F3: 32 + 1 models; F4: 2 + 2
    assert all(fs.tick_mpp(c["D"], c["M"], c["r"]) >= 1 for c in C.values() if c["r"] <= fs.KOC)
    # the tick and the compress
    assert [n for n in C if not fs.in_tick(C[n]["D"])] == ["F15", "F16", "F17", "F18"]
    assert D["F14"] == D["W1"] == 128                                        # all 128 columns of Bs live
    assert [fs.column_blocks(C[n]["D"]) for n in ("F14", "F15", "F18")] == [1, 2, 2] and D["F15"] - 128 == 4
    assert D["F1"] // 2 < 8 and D["F2"] // 2 < 8 and D["F3"] // 2 < 8          # under the 8-pair prefetch kTickPF
    # wide models: both ends of score_tick_wide_ok
    assert C["W1"]["r"] == fs.KOC + 1 and fs.tiles_per_model(65) == 3
    assert C["W2"]["r"] == 256 and fs.tiles_per_model(256) == 8 and fs.tiles_per_model(257) == 9
    assert fs.NARROW == fs.NAMES[:18] + ["F19"]
    assert [fs.wide_tpp(C[n]["D"], C[n]["M"], C[n]["r"]) for n in ("W1", "W2", "W3")] == [7, 3, 7]
    assert fs.wide_finishing(128, 3, 65) == [3]                             # W1: one pass
    assert fs.wide_finishing(64, 2, 256) == [0, 0, 1, 0, 0, 1]              # W2: a model is carried twice
    assert fs.wide_finishing(128, 10, 65) == [3, 3, 4]                      # W3: kTickWideFin models finish
    assert all(max(fs.wide_finishing(128, M, r)) <= 4 for M in range(1, 16) for r in (65, 66, 70, 75, 100, 256))
    # score_mfma_kernel's model groups on 512 .. 1,024 resident workgroups (256 CUs x 2 .. 4)
    for slots in (512, 768, 1024):
        for n in fs.NAMES:
            c = C[n]
            ng, sizes = fs.mfma_groups(fs.total_positions(c), c["M"], c["r"], slots)
            assert sum(sizes) == c["M"] and len(sizes) == ng
            assert fs.mfma_straddles(sizes, c["r"]) == (n == "F19"), (n, slots, sizes)
        assert fs.mfma_groups(fs.total_positions(C["F19"]), 6, 21, slots) == (2, [3, 3])
        assert fs.mfma_groups(fs.total_positions(C["F2"]), 3, 2, slots) == (1, [3])   # three models, one chunk
        assert fs.mfma_groups(fs.total_positions(C["F5"]), 7, 12, slots) == (4, [1, 2, 2, 2])
        assert fs.mfma_groups(fs.total_positions(C["F9"]), 5, 13, slots) == (3, [1, 2, 2])
        assert fs.mfma_groups(fs.total_positions(C["F18"]), 9, 64, slots)[0] == 9
    assert fs.total_positions(C["F19"]) == 26014 and -(-26014 // fs.KSMP) == 204
    # feature_max: a zero entry, an entry equal to a row's value (G4's construction)
    c = fs.case("F12")
    assert (c["fmax"] == 0).sum() == 1 and (c["f"][:, c["fmax"] > 0] == c["fmax"][c["fmax"] > 0]).any()
    fn = gd.normalise(c["f"], c["fmax"])
    assert not fn[:, c["fmax"] == 0].any() and fn.max() > 1
    assert [n for n in C if C[n].get("with_fmax")] == ["F12"]
    assert [n for n in C if C[n].get("common")] == [n for n in C if C[n]["r"] <= 2] == ["F1", "F2", "F3"]


@pytest.mark.parametrize("name", fs.NAMES)
def test_shapes(name):
    c = fs.case(name)
    sb = c["sb"]
    assert sb == ((18, 17, 17) if name == "F19" else (13, 11, 9))
    assert c["f"].shape == (sb[0] * sb[1] * sb[2], c["F"]) and c["F"] >= c["D"]
    assert c["ap"].shape == (c["D"], c["F"]) and c["axis_q"].shape == (c["M"], c["r"], c["D"])
    assert c["r"] <= c["D"] or c.get("random_q")
    assert len(gd.modes(c["sb"], c["box"], c["rotate"])) == (6 if c["rotate"] else 1)
    assert c["f"].shape[0] * c["F"] <= 1287 * 981


@pytest.mark.parametrize("name", fs.NAMES)
def test_gate_and_list(name):
    c = fs.case(name)
    f, ex = c["f"], c["ex"]
    assert (f >= 0).all() and (c.get("common") or np.array_equal(f, np.floor(f)))
    empty = ~f.any(1)
    assert 0.2 < empty.mean() < 0.4
    assert not ex[empty].any() and (ex >= 0).all()
    assert ((ex == 0) & ~empty).sum() == gd.EXIST0_ROWS
    gates = fs.gates(c)
    share = np.concatenate(gates).mean()
    assert 0.25 <= share <= 0.75, share
    # ragged: the list ends inside a 32-position chunk and inside a 128-position block
    n_mode = [int(g.sum()) for g in gates]
    n = sum(n_mode)
    assert n % fs.KFP and n % fs.KSMP, n
    assert any(k % fs.KFP and k % fs.KSMP for k in n_mode), n_mode
    assert n > fs.KSMP  # more than one block of score_mfma_kernel
    if name in ("F4", "F8", "F16"):  # more chunks than the tick's score workgroups: its chunk loop runs
        assert n > fs.TICK_GX * fs.KFP, n
    # the oracle gates the same positions; no passing position holds a zero box, every score is clear of 0
    _, scd = fs.oracle(name)
    want = np.concatenate([np.repeat(g[None], c["M"], 0).reshape(-1) for g in gates])
    assert np.array_equal(scd >= 0, want) and np.array_equal(scd == -1.0, ~want)
    assert np.isfinite(scd).all()
    print("%s: %d listed positions, smallest passing score %.4f" % (name, n, scd[want].min()))
    assert scd[want].min() >= 0.01, scd[want].min()
    for (_, sc), nrm in zip(gd.mode_blocks(scd, c["M"], c["sb"], c["box"], c["rotate"]),
                            gd.box_norms64_case(c, fs.compress64(name)[0])):
        assert (nrm[sc[0] >= 0] > 0).all()
    # a row with exist 0 and data lies in some passing box: dropping its data would show
    sb = c["sb"]
    hid = ((ex == 0) & ~empty).reshape(sb[2], sb[1], sb[0]).astype(np.int64)
    hits = sum(int(((gd._box_sum(hid, r3, e) > 0) & g).sum())
               for (_, r3, e), g in zip(gd.modes(sb, c["box"], c["rotate"]), gates))
    assert hits >= 10, hits


@pytest.mark.parametrize("name", fs.NAMES)
def test_fp32_restatement_meets_the_oracle(name):
    _, scd = fs.oracle(name)
    s32 = fs.restate32(name)
    assert s32.shape == scd.shape
    assert np.array_equal(s32 == -1.0, scd == -1.0)
    ok = scd > 0
    assert ok.any()
    err = np.abs(s32[ok] - scd[ok]) / scd[ok]
    print("%s: fp32 restatement vs float64 oracle, worst relative error %.3g" % (name, err.max()))
    assert err.max() <= SCORE_RTOL_F64 / 4, err.max()


@pytest.mark.parametrize("name", fs.NAMES)
def test_float64_scores_and_teeth(name):
    """scores64 without a fault is the oracle (1e-9); with one fault of the kind the case's edge
    invites, some passing score moves by more than 10 x SCORE_RTOL_F64."""
    c = fs.case(name)
    _, scd = fs.oracle(name)
    G64 = fs.compress64(name)[0]
    ok = scd > 0
    np.testing.assert_allclose(fs.scores64(c, G64)[ok], scd[ok], rtol=1e-9)
    faults = ["last_dim", "last_group"] + (["row_to_next"] if c["M"] > 1 else [])
    for fault in faults:
        s = fs.scores64(c, G64, fault)
        assert np.array_equal(s == -1.0, scd == -1.0)
        moved = (np.abs(s[ok] - scd[ok]) / scd[ok]).max()
        print("%s: fault %s moves a score by %.3g relative" % (name, fault, moved))
        assert moved > 10 * SCORE_RTOL_F64, (name, fault, moved)


@pytest.mark.parametrize("name", fs.NAMES)
def test_rank1_pick_is_clear(name):
    """Every model's best float64 score leads every other position by more than 4 x the score
    tolerance, so a GPU within tolerance must pick the oracle's position: no tie clause."""
    c = fs.case(name)
    L, scd = fs.oracle(name)
    blocks = gd.mode_blocks(scd, c["M"], c["sb"], c["box"], c["rotate"])
    worst = 1.0
    for m in range(c["M"]):
        allm = np.concatenate([sc[m] for _, sc in blocks])
        top2 = np.sort(allm)[-2:]
        lead = (top2[1] - top2[0]) / top2[1]
        worst = min(worst, lead)
        assert top2[1] > 0 and lead > 4 * SCORE_RTOL_F64, (m, top2)
        assert L.records()[m][0][0] == top2[1]
    print("%s: smallest rank-1 lead %.3g relative" % (name, worst))
    if c["rank"] > 1:  # the lists fill
        assert all(e[0] > 0 for m in L.records() for e in m)


def test_tick_frames():
    """The batch of the tick test: 11 frames at 8 per batch, four kinds, the last the case's rows."""
    assert fs.TICK_FRAMES == fs.TICK_BATCH + 3
    kinds = [fs.tick_kind(i) for i in range(fs.TICK_FRAMES)]
    assert set(kinds) == set(fs.TICK_KINDS) and kinds[-1] == "rows"
    assert {fs.tick_kind(i) for i in range(fs.TICK_BATCH, fs.TICK_FRAMES)} != {"empty"}
    c = fs.case("F5")
    f, ex = fs.tick_frame(c, "reversed")
    assert np.array_equal(f[0], c["f"][-1]) and ex[3] == c["ex"][-4]
    f, ex = fs.tick_frame(c, "halved")
    assert not f[::2].any() and not ex[::2].any() and np.array_equal(f[1::2], c["f"][1::2])
    assert np.array_equal(fs.tick_frame(c, "rows")[0], c["f"]) and c["f"][::2].any()
    f, ex = fs.tick_frame(c, "empty")
    assert not f.any() and not ex.any()
    # every kind but the empty one lists positions at the case's threshold
    for name in fs.NAMES:
        c = fs.case(name)
        for kind in ("reversed", "halved"):
            _, ex = fs.tick_frame(c, kind)
            n = sum(int((b > c["thr"]).sum()) for b in gd.exist_box_sums(c["sb"], ex, c["box"], c["rotate"]))
            assert n > 0, (name, kind)


def test_sparse_compress_rows():
    """The grid behind the sparse-compress comparison: 512 rows, the rows with data no multiple of
    the compress's 16-row blocks, empty rows among them."""
    fe, ex, sb = fs.sparse_rows(THR)
    assert sb == (8, 8, 8) and fe.shape == (512, 117)
    live = int((ex > 0).sum())
    print("sparse compress: %d rows with data of 512" % live)
    assert 0 < live < 512 and live % 16 != 0
    assert np.array_equal(ex > 0, fe.any(1))
    assert fs.dpad(6) == 8 and max(fs.SPARSE_D) == 128 and all(fs.dpad(d) <= 128 for d in fs.SPARSE_D)
    for D in fs.SPARSE_D:
        axis_t, var, axis_q, fmax = fs.sparse_setup(D, fe)
        assert axis_t.shape == (D, 117) and var.shape == (D,) and axis_q.shape[2] == D
        assert (fmax is not None) == (D == 100)
