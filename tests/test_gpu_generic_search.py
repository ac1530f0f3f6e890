"""The generic search route (compressed dimension D > 160) against the float64 oracle.

Every D above 160 -- a wide compression, or uncompressed 981-float C3-HLAC / 1001-float ConVOSCH
rows -- runs compress_kernel over every row, score_kernel<64> (D <= 256) or score_kernel<16>
(D > 256) over every position, and replay_kernel.  The cases and their references are in
generic_search_data.py; test_generic_search_data_cpu.py checks them without a GPU.

Per case: the compressed rows within the forward bound of a length-F fp32 chain of the float64
compress (derived, see compress64; bit for bit where the projection is the identity), the gate
pattern exactly and the scores within SCORE_RTOL_F64 of the float64 oracle, the lists the exact
replay of the GPU's own scores, and every model's rank-1 record at the oracle's position.

Then the list state across searches (continue, cleanMax with the stale modes kept, removeOverlap)
on this route and on the fast route, the batch entry points' frame-by-frame fall-back, and the
refusal of a D whose box rows do not fit the device's LDS."""
import numpy as np
import pytest

import batch_grids as bg
import c3hlac
import generic_search_data as gd
import np_ref as npr
import pyoracle as po
from c3hlac import synth
from conftest import THR
from generic_search_data import SCORE_RTOL_F64
from test_gpu_parity import _assert_replay_matches

pytestmark = pytest.mark.gpu


def _setup(ctx, c):
    ctx.set_score_engine(0)
    ctx.search_setup(c["axis_t"], c["var"], c["axis_q"], feature_max=c["fmax"])


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


def _check_case(ctx, name):
    c = gd.case(name)
    _setup(ctx, c)
    ctx.set_features(c["f"], c["sb"], c["ex"])
    ctx.set_rank(c["rank"])
    ctx.clean_max()
    lists, nm = ctx.search(c["box"], c["thr"], rotate=c["rotate"])
    assert nm == len(npr.mode_schedule(c["box"], c["rotate"]))
    assert np.array_equal(ctx.exist(), c["ex"])
    # compress
    G = ctx.compressed()
    G64, bound = gd.compress64(name)
    assert G.shape == G64.shape == (c["f"].shape[0], c["D"])
    if c.get("uncompressed"):  # identity projection: fma(f, 1, acc) and fma(f, 0, acc) are exact
        assert np.array_equal(G.view(np.uint32), gd.normalise(c["f"], c["fmax"]).view(np.uint32))
    err = np.abs(G.astype(np.float64) - G64)
    worst = (err / np.where(bound > 0, bound, 1)).max()
    print("%s: compress |G - G64| / bound, worst %.3g" % (name, worst))
    assert (err <= bound).all(), (name, worst)
    assert not G[~c["f"].any(1)].any()
    # scores
    L, scd = gd.oracle(name)
    _check_scores(ctx.scores(), scd, name)
    # lists
    _assert_replay_matches(ctx, c["box"], c["rank"], lists, rotate=c["rotate"])
    _check_picks(lists, L, name)


@pytest.mark.parametrize("name", gd.NAMES)
def test_case_vs_float64_oracle(ctx, name):
    _check_case(ctx, name)


def _replay_own_scores(ctx, c, prior):
    """npr.replay of the context's scores from `prior` -> (M, rank) records."""
    ms = [(mode, e[0], e[1], sc) for (mode, _, e), (_, sc) in
          zip(gd.modes(c["sb"], c["box"], c["rotate"]),
              gd.mode_blocks(ctx.scores(), c["M"], c["sb"], c["box"], c["rotate"]))]
    nl = npr.replay(ms, c["box"], c["rank"], [[list(e) for e in m] for m in prior])
    out = np.zeros((c["M"], c["rank"]), c3hlac.DET_DTYPE)
    for m in range(c["M"]):
        for i, e in enumerate(nl[m]):
            out[m, i] = tuple(e)
    return out


def _cleaned(lists):
    """cleanMax (search.cpp:716-732): score, x, y, z to 0, the modes stay."""
    return [[(0.0, 0, 0, 0, e[4]) for e in m] for m in _records(lists)]


@pytest.mark.parametrize("route", ["generic", "fast"])
def test_list_state_across_searches(ctx, route):
    """Continue without cleanMax, cleanMax with stale modes, removeOverlap: one semantics on the
    generic route (G2, D = 236) and on the fast route (G1's rows at D = 40), rank 4, six modes."""
    c = gd.list_state_case(route)
    box, rank, thr = c["box"], c["rank"], c["thr"]
    _setup(ctx, c)
    ctx.set_features(c["f"], c["sb"], c["ex"])
    ctx.set_rank(rank)
    ctx.clean_max()
    first, _ = ctx.search(box, thr)
    _assert_replay_matches(ctx, box, rank, first)
    assert (first["score"] > 0).all() and len(set(first["mode"].reshape(-1).tolist())) > 1
    # a second search continues from the first lists
    second, _ = ctx.search(box, thr)
    _assert_replay_matches(ctx, box, rank, second, prior=[[list(e) for e in m] for m in _records(first)])
    # cleanMax: the third starts from zeroed records that keep their modes (checkOverlap reads them)
    ctx.clean_max()
    third, _ = ctx.search(box, thr)
    stale = _cleaned(second)
    assert any(e[4] != 0 for m in stale for e in m)
    _assert_replay_matches(ctx, box, rank, third, prior=[[list(e) for e in m] for m in stale])
    # removeOverlap: the plain search's records through SearchObjMulti::removeOverlap
    ctx.clean_max()
    plain, _ = ctx.search(box, thr)
    assert np.array_equal(plain, _replay_own_scores(ctx, c, _cleaned(third)))
    ctx.clean_max()
    removed, _ = ctx.search(box, thr, remove_overlap=True)
    want = c3hlac.remove_overlap(_replay_own_scores(ctx, c, _cleaned(plain)), box)
    assert np.array_equal(removed, want)
    assert not np.array_equal(removed, plain)  # removeOverlap moved something


def _restore(ctx):
    ctx.set_score_engine(0)
    ctx.set_lanes(3)
    ctx.set_batch(32)
    ctx.set_pipeline(True)
    ctx.set_rank(1)


@pytest.mark.parametrize("name", ["G1", "G4"])
def test_run_feature_frames_falls_back_frame_by_frame(ctx, name):
    """D > 160 is not pipelinable: with the pipeline on, c3h_run_feature_frames searches every
    frame as c3h_set_features + c3h_set_rank + c3h_search_async.  Records byte-identical to the
    single-frame search from the setRank state; rank-1 records at the oracle's positions."""
    import torch
    c = gd.batch_case(name)
    frames = gd.batch_frames()
    M, rank = c["M"], c["rank"]
    _setup(ctx, c)
    ref = []
    for sb, f, ex in frames:
        ctx.set_features(f, sb, ex)
        ctx.set_rank(rank)
        lists, _ = ctx.search(c["box"], c["thr"], rotate=c["rotate"])
        ref.append(lists.copy())
    try:
        ctx.set_rank(rank)
        ctx.set_batch(4)
        ctx.set_pipeline(True)
        feats = [torch.from_numpy(f).to("cuda:0") for _, f, _ in frames]
        exist = [torch.from_numpy(ex).to("cuda:0") for _, _, ex in frames]
        d_out = torch.full((len(frames), M * rank * 3), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        nm = ctx.run_feature_frames(feats, [sb for sb, _, _ in frames], (9, 7, 6), exist=exist, ranges=c["box"],
                                    exist_threshold=c["thr"], rotate=c["rotate"], d_out=d_out)
        ctx.synchronize()
        assert nm == 6
        got = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(len(frames), M, rank)
        for i, (sb, f, ex) in enumerate(frames):
            assert got[i].tobytes() == ref[i].tobytes(), (name, i, got[i], ref[i])
            L, scd = gd.batch_oracle(name, i)
            _check_picks(got[i], L, (name, "frame %d" % i))
        # the context holds the last frame, in its own layout
        assert tuple(ctx.subdiv) == frames[-1][0]
        _check_scores(ctx.scores(), gd.batch_oracle(name, len(frames) - 1)[1], (name, "last frame"))
    finally:
        _restore(ctx)


def test_run_frames_takes_the_lanes(ctx):
    """c3h_run_frames with D = 164 on two 40^3 grids (C3-HLAC-981, S = 4: 1000 rows): one frame per
    chunk down the lanes.  Records byte-identical to set_grid + extract + search per frame; the
    last frame's scores against the float64 oracle on the extracted rows."""
    import torch
    G, S, box = 40, 4, (2, 2, 2)
    words = [np.ascontiguousarray(bg.words()[k].reshape(bg.G, bg.G, bg.G)[:G, :G, :G]).reshape(-1)
             for k in ("dense", "sparse")]
    axis_t, var, axis_q = synth.random_bases(981, 164, 2, 5, seed=synth.BASE_SEED + 9)
    ctx.set_score_engine(0)
    ctx.search_setup(axis_t, var, axis_q)
    ctx.set_grid(words[0], (G, G, G))
    sb, hn = ctx.extract(981, THR, S)
    assert tuple(sb) == (10, 10, 10) and hn == 1000
    thr = gd.threshold(sb, ctx.exist(), box, True)
    ref = []
    for w in words:
        ctx.set_grid(w, (G, G, G))
        ctx.set_rank(1)
        ctx.extract(981, THR, S)
        det, _ = ctx.search(box, thr)
        ref.append(det.copy())
    f, ex = ctx.features(), ctx.exist()
    _, _, scd = po.search(sb, f, ex, synth.whiten(axis_t, var), axis_q, box, 1, thr, dbl=True, want_scores=True)
    _check_scores(ctx.scores(), scd, "per-frame search, last frame")
    try:
        dev = torch.device("cuda", 0)
        d_grids = [torch.from_numpy(w.view(np.int32)).to(dev) for w in words]
        d_out = torch.full((len(words), 2 * 3), -1, dtype=torch.int64, device=dev)
        ctx.set_lanes(2)
        ctx.set_batch(4)
        ctx.set_pipeline(True)
        torch.cuda.synchronize()
        ctx.run_frames(np.array([g.data_ptr() for g in d_grids], np.uint64), (G, G, G), (0, 0, 0), 0.01, 981, THR, S,
                       box, thr, True, d_out.data_ptr())
        ctx.synchronize()
        got = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(len(words), 2, 1)
        for i in range(len(words)):
            assert got[i].tobytes() == ref[i].tobytes(), (i, got[i], ref[i])
        _check_scores(ctx.scores(), scd, "run_frames, last frame")
    finally:
        _restore(ctx)


def test_refusal_beyond_the_lds_budget(ctx):
    """D = 2600 uncompressed: 16 box rows of 2601 floats are 166,464 B, more than a workgroup's
    LDS.  c3h_search refuses it with a message naming D before anything launches (set_features
    with an explicit exist only copies), and the context searches G1 correctly afterwards."""
    D = 2600
    rng = np.random.default_rng(5)
    f = np.floor(rng.random((27, D)) * 4).astype(np.float32)
    ex = np.ones(27, np.int32)
    ctx.set_score_engine(0)
    ctx.search_setup(None, None, rng.standard_normal((1, 1, D)).astype(np.float32))
    ctx.set_features(f, (3, 3, 3), ex)
    ctx.set_rank(1)
    with pytest.raises(c3hlac._capi.C3HError) as e:
        ctx.search((1, 1, 1), 0)
    assert "D = %d" % D in str(e.value), str(e.value)
    _check_case(ctx, "G1")
