"""The fp32 fast search route (compressed dimension D <= 160) against the float64 oracle, at the
shape edges of its kernels.  The cases and their references are in fast_search_data.py;
test_fast_search_data_cpu.py checks them without a GPU.

Single frame, per case and projection engine (1 the VALU list kernel score_list_body -- the
generic kernel for the wide models W1, W2 --, 2 the matrix cores score_mfma_kernel<KP>, 0
automatic): the compressed rows within the forward bound of a length-F fp32 chain of the float64
compress, the gate pattern exactly and the scores within SCORE_RTOL_F64 of the float64 oracle, the
lists the exact replay of the GPU's own scores, every model's rank-1 record at the oracle's
position; for r <= 64 the engines' scores and lists bit for bit (c3h_set_score_engine's contract).

Through the tick (c3h_run_feature_frames, 8 frames per batch, 11 frames): every record
byte-identical to the frame's single-frame search at the same engine and the last frame's scores
bit-identical; D <= 128 goes through the tick (the wide models at engines 0 and 2), D > 128 and
the wide models at engine 1 do not, with the same records.

The sparse compress behind an extract (compress_rows_body) against the dense one behind
set_features (compress_kernel): the same bits on every row with data, and within the derived
bound of the float64 compress of the oracle's rows."""
import numpy as np
import pytest

import c3hlac
import fast_search_data as fs
import generic_search_data as gd
import np_ref as npr
from conftest import THR
from fast_search_data import SCORE_RTOL_F64
from test_gpu_parity import _assert_replay_matches

pytestmark = pytest.mark.gpu

ENGINES = (1, 2, 0)


def _restore(ctx):
    ctx.timing(False)
    ctx.set_score_engine(0)
    ctx.set_remove_overlap(False)
    ctx.set_lanes(3)
    ctx.set_pipeline(True)
    ctx.set_batch(32)
    ctx.set_rank(1)


def _records(lists):
    return [[(float(e["score"]), int(e["x"]), int(e["y"]), int(e["z"]), int(e["mode"])) for e in m] for m in lists]


def _check_scores(sc, scd, tag):
    assert sc.shape == scd.shape, tag
    assert np.array_equal(sc == -1.0, scd == -1.0), tag  # the gate, exactly
    ok = scd > 0
    assert ok.any() and np.array_equal(ok, scd != -1.0), tag
    err = np.abs(sc[ok] - scd[ok]) / scd[ok]
    print("%s: scores vs float64 oracle, worst relative error %.3g" % (tag, err.max()))
    np.testing.assert_allclose(sc[ok], scd[ok], rtol=SCORE_RTOL_F64, err_msg=str(tag))


def _check_picks(lists, L, tag):
    for m, recs in enumerate(L.records()):
        got = _records(lists[m:m + 1])[0][0]
        assert got[1:] == tuple(recs[0][1:]), (tag, "model %d" % m, got, recs[0])
        assert abs(got[0] - recs[0][0]) <= SCORE_RTOL_F64 * recs[0][0], (tag, m)


def _check_compress(ctx, name):
    c = fs.case(name)
    G = ctx.compressed()
    G64, bound = fs.compress64(name)
    assert G.shape == G64.shape == (c["f"].shape[0], c["D"])  # the caller's D, not the padded one
    err = np.abs(G.astype(np.float64) - G64)
    worst = (err / np.where(bound > 0, bound, 1)).max()
    print("%s: compress |G - G64| / bound, worst %.3g" % (name, worst))
    assert (err <= bound).all(), (name, worst)
    assert not G[~c["f"].any(1)].any()


def _search(ctx, c, engine):
    ctx.set_score_engine(engine)
    ctx.set_features(c["f"], c["sb"], c["ex"])
    ctx.search_setup(c["axis_t"], c["var"], c["axis_q"], feature_max=c["fmax"])
    ctx.set_rank(c["rank"])
    ctx.clean_max()
    return ctx.search(c["box"], c["thr"], rotate=c["rotate"])


@pytest.mark.parametrize("name", fs.NAMES)
def test_case_vs_float64_oracle(ctx, name):
    c = fs.case(name)
    L, scd = fs.oracle(name)
    first = None
    try:
        for engine in ENGINES:
            tag = "%s engine %d" % (name, engine)
            lists, nm = _search(ctx, c, engine)
            assert nm == len(npr.mode_schedule(c["box"], c["rotate"]))
            assert np.array_equal(ctx.exist(), c["ex"]), tag
            _check_compress(ctx, name)
            sc = ctx.scores()
            _check_scores(sc, scd, tag)
            _assert_replay_matches(ctx, c["box"], c["rank"], lists, rotate=c["rotate"])
            _check_picks(lists, L, tag)
            if name in fs.NARROW:  # one set of scores whichever engine projects
                if first is None:
                    first = (sc.copy(), lists.copy())
                else:
                    assert sc.tobytes() == first[0].tobytes(), (tag, "scores differ from engine %d's" % ENGINES[0])
                    assert lists.tobytes() == first[1].tobytes(), (tag, "lists differ from engine %d's" % ENGINES[0])
    finally:
        _restore(ctx)


def _tick(ctx, c, dev, kinds):
    """-> (records (n, M, rank), kernel_times) of run_feature_frames over the frame kinds."""
    import torch
    M, rank, n = c["M"], c["rank"], len(kinds)
    d_out = torch.full((n, M * rank * 3), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.timing(c3hlac.timing_mask("pipeline", "replay"))
    ctx.kernel_times(reset=True)
    try:
        nm = ctx.run_feature_frames([dev[k][0] for k in kinds], [c["sb"]] * n, c["sb"], exist=[dev[k][1] for k in kinds],
                                    ranges=c["box"], exist_threshold=c["thr"], rotate=c["rotate"], d_out=d_out)
        ctx.synchronize()
        kt = ctx.kernel_times(reset=True)
    finally:
        ctx.timing(False)
    assert nm == len(npr.mode_schedule(c["box"], c["rotate"]))
    return d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(n, M, rank), kt


@pytest.mark.parametrize("name", fs.NAMES)
def test_case_through_the_tick(ctx, name):
    import torch
    c = fs.case(name)
    L, scd = fs.oracle(name)
    kinds = [fs.tick_kind(i) for i in range(fs.TICK_FRAMES)]
    frames = {k: fs.tick_frame(c, k) for k in fs.TICK_KINDS}
    dev = {k: (torch.from_numpy(f).to("cuda:0"), torch.from_numpy(ex).to("cuda:0")) for k, (f, ex) in frames.items()}
    torch.cuda.synchronize()
    wide = c["r"] > fs.KOC
    try:
        for engine in ENGINES:
            tag = "%s engine %d" % (name, engine)
            # each distinct frame on the single-frame route, from the setRank state
            ctx.set_score_engine(engine)
            ctx.search_setup(c["axis_t"], c["var"], c["axis_q"], feature_max=c["fmax"])
            ref = {}
            for k in fs.TICK_KINDS[::-1]:  # the case's own rows last
                ctx.set_features(frames[k][0], c["sb"], frames[k][1])
                ctx.set_rank(c["rank"])
                lists, _ = ctx.search(c["box"], c["thr"], rotate=c["rotate"])
                ref[k] = (lists.copy(), ctx.scores().copy())
            assert not ref["empty"][0].tobytes().strip(b"\0"), tag  # the setRank state
            assert (ref["empty"][1] == -1.0).all(), tag
            _check_scores(ref["rows"][1], scd, tag + " single frame")
            ctx.set_rank(c["rank"])
            ctx.set_batch(fs.TICK_BATCH)
            ctx.set_pipeline(True)
            got, kt = _tick(ctx, c, dev, kinds)
            through = fs.in_tick(c["D"]) and not (wide and engine == 1)
            assert kt["pipeline"][1] == (fs.TICK_FRAMES if through else 0), (tag, "frames through the tick", kt["pipeline"])
            for i, k in enumerate(kinds):
                assert got[i].tobytes() == ref[k][0].tobytes(), (tag, "frame %d (%s)" % (i, k), got[i], ref[k][0])
            assert tuple(ctx.subdiv) == c["sb"] and kinds[-1] == "rows"
            assert ctx.scores().tobytes() == ref["rows"][1].tobytes(), (tag, "scores of the last frame")
            _check_picks(got[-1], L, tag + " last frame")
    finally:
        _restore(ctx)


def test_sparse_compress_is_the_dense_one(ctx):
    """extract leaves a row list: the search compresses the listed rows (compress_rows_body).
    set_features of the same rows leaves none: compress_kernel over every row.  Both claim the
    ascending-j fma chain."""
    fe, ex_ref, sb = fs.sparse_rows(THR)
    try:
        ctx.set_score_engine(0)
        ctx.set_grid(fs.sparse_words().reshape(-1), (fs.SPARSE_GRID,) * 3)
        got_sb, H = ctx.extract(fs.SPARSE_F, THR, fs.SPARSE_S)
        assert tuple(got_sb) == sb and H == 512
        f, ex = ctx.features(), ctx.exist()
        assert np.array_equal(f, fe) and np.array_equal(ex, ex_ref)
        thr = gd.threshold(sb, ex, fs.SPARSE_BOX, False)
        rows = ex > 0
        for D in fs.SPARSE_D:
            axis_t, var, axis_q, fmax = fs.sparse_setup(D, fe)
            ctx.set_grid(fs.sparse_words().reshape(-1), (fs.SPARSE_GRID,) * 3)
            ctx.extract(fs.SPARSE_F, THR, fs.SPARSE_S)
            ctx.search_setup(axis_t, var, axis_q, feature_max=fmax)
            ctx.set_rank(1)
            lists_s, _ = ctx.search(fs.SPARSE_BOX, thr, rotate=False)
            G_s, sc_s = ctx.compressed().copy(), ctx.scores().copy()
            assert G_s.shape == (512, D)
            ctx.set_features(f, sb, ex)
            ctx.set_rank(1)
            lists_d, _ = ctx.search(fs.SPARSE_BOX, thr, rotate=False)
            G_d = ctx.compressed()
            assert rows.any() and np.array_equal(G_s[rows].view(np.uint32), G_d[rows].view(np.uint32)), \
                ("D = %d: sparse compress != dense compress" % D)
            assert np.array_equal(ctx.scores(), sc_s) and np.array_equal(lists_d, lists_s), D
            assert (sc_s > 0).sum() > 100, D
            G64, bound = gd.compress64_rows(fe, c3hlac.synth.whiten(axis_t, var), fmax)
            err = np.abs(G_d.astype(np.float64) - G64)
            worst = (err / np.where(bound > 0, bound, 1)).max()
            print("sparse compress D = %d: |G - G64| / bound, worst %.3g" % (D, worst))
            assert (err[rows] <= bound[rows]).all() and not G_d[~rows].any(), (D, worst)
    finally:
        _restore(ctx)
