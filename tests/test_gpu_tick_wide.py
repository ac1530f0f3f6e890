"""Wide model subspaces (r > 64) through the pipelined tick: their score role
(score_tick_wide_body, a launch of its own behind the tick of the batch's score slot) projects
them on the matrix cores in passes of whole column tiles, so the batch entry points no longer
send such model sets down the lanes one frame at a time.

64^3 grids, leaf 0.04, C3-HLAC-117, exist threshold 10, 8 frames per batch over 5 full batches
and a ragged one of 3, so every one of the four buffer sets is reused; the frames cycle over
the three grids of batch_grids.py (dense, sparse, empty) with a shift after four batches.

Cases (D, M, r, S):
  (100, 3, 70, 4)   the reference's r = 70 (detect_object_vosch_multi's models_offline_r)
  (100, 7, 70, 4)   490 columns: several passes of the role
  (100, 7, 70, 8)   343 positions, fewer list chunks than score workgroups
  (80, 2, 80, 4)    r = D
  (116, 2, 116, 4)  4 column tiles per model; D a multiple of 4 just under F
  (20, 2, 70, 4)    more rows than dimensions: the LDS an r <= 64 search at D = 20 allocates
                    holds 2 tiles, so each model spans two passes and is carried twice

No model set with r <= 256 is rejected by score_tick_wide_ok (a model of 256 columns is 8
tiles, and one tile's pass, 128 D + 6,432 bytes, always fits the 384 D + 1,184 or more that
an r <= 64 search allocates), so the route that is left to the lanes is engine 1.

The reference is each distinct grid on the single-frame path at engine 2 (set_grid, extract,
search: score_mfma_kernel), code this feature does not touch: every record and the last
frame's scores() must be byte-identical to it.  Against the float64 oracle: scores within 1e-5
relative, another position only on a tie within 2e-5, the oracle's gated-out pattern.  A CPU
test on the oracle alone shows that the position check is not vacuous: the best score of a
(grid, model) pair is clear of the second by more than 1e-3 relative in at least two thirds
of the pairs of every case."""
import numpy as np
import pytest

import batch_grids as bg
import c3hlac
from batch_grids import BATCH, EXIST, F, G, LEAF, NFR
from c3hlac import synth
from conftest import THR

RTOL = 1e-5
BOX = (2, 2, 2)
# (D, M, r, S)
CASES = [(100, 3, 70, 4), (100, 7, 70, 4), (100, 7, 70, 8), (80, 2, 80, 4), (116, 2, 116, 4), (20, 2, 70, 4)]
RANK_CASE, RANK_BOX, RANK = (100, 7, 70, 4), (1, 2, 3), 4


def _id(c):
    return "D%d_M%d_r%d_S%d" % c


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_oracle_best_scores_are_clear_of_the_second(case):
    """CPU, the oracle alone: measured 6 of 6, 14 of 14, 12 of 14, 3 of 4, 3 of 4 and 4 of 4."""
    D, M, r, s = case
    clear = total = 0
    for k in ("dense", "sparse"):
        _, sc, _ = bg.oracle_search(D, M, r, s, BOX, k)
        sc = sc.reshape(M, -1)
        assert (sc[0] >= 0).sum() >= 100, (case, k)
        for m in range(M):
            v = np.sort(sc[m])[::-1]
            clear += bool(v[0] - v[1] > 1e-3 * v[0])
            total += 1
    assert 3 * clear >= 2 * total, (case, clear, total)


@pytest.fixture(scope="module")
def d_words(ctx):
    import torch
    d = {k: torch.from_numpy(w.view(np.int32)).to("cuda:0") for k, w in bg.words().items()}
    torch.cuda.synchronize()
    return d


_SINGLE = {}


def _single(ctx, case, box, rank):
    """Each grid on the single-frame path at engine 2: (lists, scores) per grid, computed once."""
    key = (case, box, rank)
    if key not in _SINGLE:
        D, M, r, s = case
        ctx.search_setup(*bg.bases(D, M, r))
        ctx.set_score_engine(2)
        try:
            ref = {}
            for k in bg.NAMES:
                ctx.set_grid(bg.words()[k], (G,) * 3, (0, 0, 0), LEAF)
                ctx.set_rank(rank)
                ctx.extract(F, THR, s)
                lists, _ = ctx.search(box, EXIST)
                ref[k] = (lists.copy(), ctx.scores().copy())
        finally:
            ctx.set_score_engine(0)
        assert np.array_equal(ref["empty"][0], np.zeros((M, rank), c3hlac.DET_DTYPE)), case  # the setRank state
        _SINGLE[key] = ref
    return _SINGLE[key]


def _run(ctx, d_words, names, case, box, rank, stream_cuts=None):
    """-> (records (NFR, M, rank), kernel_times) of run_frames / stream_frames over the cycle."""
    import torch
    D, M, r, s = case
    ptrs = np.array([d_words[k].data_ptr() for k in names], np.uint64)
    d_out = torch.full((NFR, M * rank * 3), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.timing(c3hlac.timing_mask("pipeline", "replay"))
    ctx.kernel_times(reset=True)
    try:
        if stream_cuts is None:
            ctx.run_frames(ptrs, (G,) * 3, (0, 0, 0), LEAF, F, THR, s, box, EXIST, True, d_out.data_ptr())
        else:
            for a, b in zip(stream_cuts[:-1], stream_cuts[1:]):
                ctx.run_frames(ptrs[a:b], (G,) * 3, (0, 0, 0), LEAF, F, THR, s, box, EXIST, True,
                               d_out[a:].data_ptr(), stream=True)
            ctx.stream_flush()
        ctx.synchronize()
        kt = ctx.kernel_times(reset=True)
    finally:
        ctx.timing(False)
    return d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(NFR, M, rank), kt


def _check_records(got, names, ref, tag):
    for i, k in enumerate(names):
        assert got[i].tobytes() == ref[k][0].tobytes(), (tag, "frame %d (%s)" % (i, k), got[i], ref[k][0])


def _check_det(rec, scores_f64, shape, tag):
    """rec: (M,) records of one frame at rank 1; scores_f64: (M, P) oracle scores of the single
    mode (box 2x2x2), P in (z, y, x) scan order."""
    ze, ye, xe = shape
    for m in range(rec.shape[0]):
        s, x, y, z, mode = float(rec[m]["score"]), int(rec[m]["x"]), int(rec[m]["y"]), int(rec[m]["z"]), int(rec[m]["mode"])
        ref = scores_f64[m]
        best = int(np.argmax(ref))  # first maximum in scan order = searchPart's strict '>'
        assert mode == 0, (tag, m, mode)
        p = (z * ye + y) * xe + x
        assert abs(s - ref[p]) <= RTOL * ref[p], (tag, m, s, ref[p])
        if p != best:  # only a tie within tolerance may pick another position
            assert ref[p] >= ref[best] * (1 - 2 * RTOL), (tag, m, (x, y, z), np.unravel_index(best, shape))


def _check_scores(gs, sc, tag):
    assert gs.shape == sc.shape, tag
    assert np.array_equal(gs < 0, sc < 0), tag
    ok = sc > 0
    np.testing.assert_allclose(gs[ok], sc[ok], rtol=RTOL)


def _setup(ctx, case, rank):
    ctx.search_setup(*bg.bases(*case[:3]))
    ctx.set_rank(rank)
    ctx.set_batch(BATCH)
    ctx.set_pipeline(True)


def _restore(ctx):
    ctx.timing(False)
    ctx.set_score_engine(0)
    ctx.set_batch(32)
    ctx.set_rank(1)


@pytest.mark.gpu
@pytest.mark.parametrize("last", ["dense", "sparse"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_wide_models_go_through_the_tick(ctx, d_words, case, last):
    D, M, r, s = case
    ref = _single(ctx, case, BOX, 1)
    names = bg.frame_names(last)
    _setup(ctx, case, 1)
    try:
        for engine in (0, 2):
            ctx.set_score_engine(engine)
            got, kt = _run(ctx, d_words, names, case, BOX, 1)
            assert kt["pipeline"][1] == NFR, ("frames through the tick", engine, kt["pipeline"])
            _check_records(got, names, ref, (case, "engine", engine))
            gs = ctx.scores()
            assert gs.tobytes() == ref[last][1].tobytes(), (case, "scores of the last frame", engine)
    finally:
        _restore(ctx)
    # against the float64 oracle
    for i, k in enumerate(names):
        if k != "empty":
            _, sc, sb = bg.oracle_search(D, M, r, s, BOX, k)
            shape = tuple(int(n) - b + 1 for n, b in zip(sb[::-1], BOX))  # (z, y, x) positions
            _check_det(got[i][:, 0], sc.reshape(M, -1), shape, "%s frame %d (%s)" % (case, i, k))
    _check_scores(gs, bg.oracle_search(D, M, r, s, BOX, last)[1], case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[0], CASES[5]], ids=_id)
def test_engine_1_takes_the_lanes(ctx, d_words, case):
    """Engine 1 has no VALU role for r > 64: no frame goes through a tick and the lanes (the
    generic VALU kernel, one frame per launch) give the single-frame path's records."""
    D, M, r, s = case
    engine = 1
    ref = _single(ctx, case, BOX, 1)
    names = bg.frame_names("dense")
    _setup(ctx, case, 1)
    try:
        ctx.set_score_engine(engine)
        got, kt = _run(ctx, d_words, names, case, BOX, 1)
        assert kt["pipeline"][1] == 0, ("frames through the tick", kt["pipeline"])
        _check_records(got, names, ref, (case, "engine", engine))
        gs = ctx.scores()
        assert gs.tobytes() == ref["dense"][1].tobytes(), (case, "scores of the last frame")
    finally:
        _restore(ctx)
    _, sc, sb = bg.oracle_search(D, M, r, s, BOX, "dense")
    shape = tuple(int(n) - b + 1 for n, b in zip(sb[::-1], BOX))
    _check_det(got[-1][:, 0], sc.reshape(M, -1), shape, (case, "last frame"))
    _check_scores(gs, sc, case)


@pytest.mark.gpu
def test_rank_4_over_six_modes(ctx, d_words):
    """Box (1, 2, 3): six modes; the batched replay follows the wide score role.  The lists are
    the single-frame path's; the last frame's are the sequential update replayed on the host
    over its scores, and those scores are the oracle's within 1e-5 (the rule of the rank tests:
    lists are compared through the scores they were built from)."""
    case = RANK_CASE
    D, M, r, s = case
    ref = _single(ctx, case, RANK_BOX, RANK)
    assert (ref["dense"][0]["score"][:, -1] > 0).all(), "a list did not fill"
    assert len({int(v) for v in ref["dense"][0]["mode"].reshape(-1)}) >= 3, "the lists hold few modes"
    names = bg.frame_names("dense")
    _setup(ctx, case, RANK)
    try:
        got, kt = _run(ctx, d_words, names, case, RANK_BOX, RANK)
        assert kt["pipeline"][1] == NFR and kt["replay"][1] == NFR, kt
        _check_records(got, names, ref, (case, "rank", RANK))
        gs = ctx.scores()
        fresh = np.zeros((M, RANK), c3hlac.DET_DTYPE)
        again = c3hlac.replay_scores(gs, ctx.subdiv, RANK_BOX, fresh, rotate=True)
        assert np.array_equal(again, got[-1])
    finally:
        _restore(ctx)
    L, sc, sb = bg.oracle_search(D, M, r, s, RANK_BOX, "dense", rank=RANK)
    _check_scores(gs, sc, case)
    # the float64 lists themselves: c3h_replay_scores over the oracle's scores is the oracle's update
    fresh = np.zeros((M, RANK), c3hlac.DET_DTYPE)
    assert np.array_equal(c3hlac.replay_scores(sc, sb, RANK_BOX, fresh, rotate=True), bg.lists_records(L))


@pytest.mark.gpu
def test_streamed_uneven_pushes_equal_run_frames(ctx, d_words):
    case = RANK_CASE
    ref = _single(ctx, case, RANK_BOX, RANK)
    names = bg.frame_names("dense")
    _setup(ctx, case, RANK)
    try:
        whole, _ = _run(ctx, d_words, names, case, RANK_BOX, RANK)
        got, kt = _run(ctx, d_words, names, case, RANK_BOX, RANK, stream_cuts=[0, 5, 6, 3 * BATCH + 1, NFR])
        # each push goes in batches of its own: 1 + 1 + 3 + 3 batches
        assert kt["pipeline"][1] == NFR and kt["replay"][1] == NFR, kt
        assert got.tobytes() == whole.tobytes()
        _check_records(got, names, ref, (case, "streamed"))
    finally:
        _restore(ctx)


P_LEAF, P_S, P_CANVAS = 0.02, 8, 64


@pytest.mark.gpu
def test_point_frames_of_wide_models_stay_in_the_batch(ctx):
    """Three small clouds of different extents on a 64^3 canvas: batched (status 0), with the
    records of the single-frame path (voxelize, extract, search)."""
    import torch
    dev = torch.device("cuda", 0)
    case = CASES[0]
    D, M, r, _ = case
    frames = [torch.from_numpy(synth.kinect_scene(n, grid=g, leaf=P_LEAF, seed=synth.BASE_SEED + 2 + i)).to(dev)
              for i, (n, g) in enumerate([(20_000, 40), (30_000, 48), (60_000, 64)])]
    torch.cuda.synchronize()
    ctx.search_setup(*bg.bases(D, M, r))
    ctx.set_rank(1)
    ctx.set_batch(BATCH)
    ctx.set_pipeline(True)
    try:
        d_out = torch.full((len(frames), M * 3), -1, dtype=torch.int64, device=dev)
        nm, info = ctx.run_point_frames(frames, P_LEAF, (P_CANVAS,) * 3, F, THR, P_S, BOX, EXIST, True, d_out)
        assert nm == 1
        assert (info["status"] == 0).all(), info["status"]
        assert len({tuple(d) for d in info["div_b"].tolist()}) == len(frames), info["div_b"]
        got = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(len(frames), M, 1)
        assert (got["score"] > 0).all()
        ctx.set_score_engine(2)
        for i, fr in enumerate(frames):
            ctx.voxelize(fr, P_LEAF)
            ctx.set_rank(1)
            ctx.extract(F, THR, P_S)
            ref, _ = ctx.search(BOX, EXIST)
            assert got[i].tobytes() == ref.tobytes(), (i, got[i], ref)
    finally:
        _restore(ctx)
