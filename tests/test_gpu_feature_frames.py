"""c3h_run_feature_frames / c3h_stream_feature_frames: batches of caller-computed feature rows
(SearchObj::setData as setVOSCH / setConVOSCH / setGRSD call it) through the pipelined tick.

Frames of feature_frames_data.py on the (16, 16, 16) canvas, 8 frames per batch over 5 full
batches and a ragged one of 3 (every buffer set is reused), the kinds cycling as
batch_grids.frame_names does, so a slot holds another kind than the time before.

The reference is code this feature does not touch: each distinct frame through set_features
(its own counts) + set_rank + search, once per case.  Every record must be byte-identical to
it, and the last frame's scores(), mapped from the canvas to the frame's layout, bit-identical
inside the frame and -1 outside.  Against the float64 oracle: the gated-out pattern, scores
within 1e-5 (the project's fp32 bound), another position only on a tie within 2e-5."""
import numpy as np
import pytest

import batch_grids as bg
import c3hlac
import feature_frames_data as fd
from batch_grids import BATCH, NFR
from conftest import THR
from test_gpu_tick_wide import _check_det, _check_scores

pytestmark = pytest.mark.gpu

BOX = (2, 2, 2)
RANK_BOX, RANK = (1, 2, 3), 4
CUTS = [0, 3, 11, 12, 30, NFR]


@pytest.fixture(scope="module")
def dev():
    """(kind, name) -> (rows, exist) device tensors, uploaded on first use."""
    import torch
    cache = {}

    def get(kind, name):
        if (kind, name) not in cache:
            f, e, _ = fd.frame(kind, name)
            cache[kind, name] = (torch.from_numpy(f).to("cuda:0"), torch.from_numpy(e).to("cuda:0"))
            torch.cuda.synchronize()
        return cache[kind, name]
    return get


def _frames(last, kinds):
    """The frame cycle: [(kind, name)] of NFR frames ending in `last`; kinds(i) names frame i's kind."""
    return [(kinds(i), k) for i, k in enumerate(bg.frame_names(last))]


def _mixed(i):
    """Full-canvas and cropped frames mixed, two slabs; the last frame (NFR - 1 = 42) is cropped."""
    return "slab" if i in (7, 20) else ("crop" if i % 3 == 0 else "vosch")


_SINGLE = {}


def _single(ctx, case, frames, box, rank, rotate, engine=0):
    """Each distinct frame on the single-frame route: (kind, name) -> (lists, scores), computed once."""
    key = (case["dim"], case["M"], case["r"], box, rank, rotate, engine)
    ref = _SINGLE.setdefault(key, {})
    todo = sorted(set(frames) - set(ref))
    if todo:
        axis_t, var, axis_q, fmax = fd.setup(case)
        ctx.search_setup(axis_t, var, axis_q, feature_max=fmax)
        ctx.set_score_engine(engine)
        try:
            for kind, name in todo:
                f, _, counts = fd.frame(kind, name)
                ctx.set_features(f, counts, None, case["rule"])
                ctx.set_rank(rank)
                lists, _ = ctx.search(box, case["thr"], rotate=rotate)
                ref[kind, name] = (lists.copy(), ctx.scores().copy())
        finally:
            ctx.set_score_engine(0)
    return ref


def _setup(ctx, case, rank, batch=BATCH):
    axis_t, var, axis_q, fmax = fd.setup(case)
    ctx.search_setup(axis_t, var, axis_q, feature_max=fmax)
    ctx.set_rank(rank)
    ctx.set_batch(batch)
    ctx.set_pipeline(True)


def _restore(ctx):
    ctx.timing(False)
    ctx.set_score_engine(0)
    ctx.set_remove_overlap(False)
    ctx.set_pipeline(True)
    ctx.set_batch(32)
    ctx.set_rank(1)


def _run(ctx, dev, frames, case, box, rank, rotate, with_exist=False, cuts=None, flush=True):
    """-> (records (N, M, rank), kernel_times, d_out) of run_feature_frames over the frames."""
    import torch
    M, n = case["M"], len(frames)
    feats = [dev(*fr)[0] for fr in frames]
    exist = [dev(*fr)[1] for fr in frames] if with_exist else None
    subdivs = [fd.frame(*fr)[2] for fr in frames]
    d_out = torch.full((n, M * rank * 3), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.timing(c3hlac.timing_mask("pipeline", "replay"))
    ctx.kernel_times(reset=True)
    try:
        if cuts is None:
            ctx.run_feature_frames(feats, subdivs, fd.CANVAS, rule=case["rule"], exist=exist, ranges=box,
                                   exist_threshold=case["thr"], rotate=rotate, d_out=d_out)
        else:
            for a, b in zip(cuts[:-1], cuts[1:]):
                ctx.run_feature_frames(feats[a:b], subdivs[a:b], fd.CANVAS, rule=case["rule"],
                                       exist=None if exist is None else exist[a:b], ranges=box,
                                       exist_threshold=case["thr"], rotate=rotate, d_out=d_out[a:].data_ptr(),
                                       stream=True)
            if flush:
                ctx.stream_flush()
        if flush:
            ctx.synchronize()
        kt = ctx.kernel_times(reset=True) if flush else None
    finally:
        if flush:
            ctx.timing(False)
    return (d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(n, M, rank) if flush else None), kt, d_out


def _check_records(got, frames, ref, tag):
    for i, fr in enumerate(frames):
        assert got[i].tobytes() == ref[fr][0].tobytes(), (tag, "frame %d %s" % (i, fr), got[i], ref[fr][0])


def _check_last_scores(ctx, case, frames, ref, box):
    """scores() of the last frame: canvas layout -> the frame's own; one mode."""
    M = case["M"]
    assert tuple(ctx.subdiv) == fd.CANVAS
    counts = fd.frame(*frames[-1])[2]
    inside, outside = fd.canvas_to_frame_scores(ctx.scores(), M, counts, box)
    assert np.ascontiguousarray(inside).tobytes() == ref[frames[-1]][1].tobytes(), "scores inside the frame"
    assert (outside == -1).all(), "positions outside the frame"
    return np.ascontiguousarray(inside).reshape(-1)


def _check_oracle(got, frames, case, box, rotate):
    M = case["M"]
    checked = 0
    for i, (kind, name) in enumerate(frames):
        if name == "empty" or kind == "slab":
            assert not got[i].tobytes().strip(b"\0"), ("setRank state", i, kind, name)
            continue
        _, sc = fd.oracle(case, kind, name, box, rotate=rotate)
        counts = fd.frame(kind, name)[2]
        shape = tuple(int(n) - b + 1 for n, b in zip(counts[::-1], box))  # (z, y, x) positions
        _check_det(got[i][:, 0], sc.reshape(M, -1), shape, "frame %d (%s %s)" % (i, kind, name))
        checked += 1
    assert checked >= NFR // 2


@pytest.mark.parametrize("last", ["dense", "sparse"])
def test_vosch_frames_go_through_the_tick(ctx, dev, last):
    case = fd.VOSCH
    frames = _frames(last, _mixed if last == "sparse" else (lambda i: "vosch" if i % 4 else "crop"))
    ref = _single(ctx, case, frames, BOX, 1, True)
    _setup(ctx, case, 1)
    try:
        for with_exist in (False, True):
            got, kt, _ = _run(ctx, dev, frames, case, BOX, 1, True, with_exist=with_exist)
            assert kt["pipeline"][1] == NFR, ("frames through the tick", with_exist, kt["pipeline"])
            _check_records(got, frames, ref, ("exist arrays", with_exist))
            inside = _check_last_scores(ctx, case, frames, ref, BOX)
            with pytest.raises(c3hlac.C3HError, match="C3H_ERR_STATE"):
                ctx.features()
    finally:
        _restore(ctx)
    _check_oracle(got, frames, case, BOX, True)
    _check_scores(inside, fd.oracle(case, *frames[-1], BOX)[1], (case, last))


@pytest.mark.parametrize("last", ["dense", "sparse"])
def test_grsd_rule_without_rotation(ctx, dev, last):
    case = fd.GRSD
    frames = _frames(last, lambda i: "grsd")
    ref = _single(ctx, case, frames, BOX, 1, False)
    _setup(ctx, case, 1)
    try:
        for with_exist in (False, True):
            got, kt, _ = _run(ctx, dev, frames, case, BOX, 1, False, with_exist=with_exist)
            assert kt["pipeline"][1] == NFR, ("frames through the tick", with_exist, kt["pipeline"])
            _check_records(got, frames, ref, ("exist arrays", with_exist))
            inside = _check_last_scores(ctx, case, frames, ref, BOX)
    finally:
        _restore(ctx)
    _check_oracle(got, frames, case, BOX, False)
    _check_scores(inside, fd.oracle(case, *frames[-1], BOX, rotate=False)[1], (case, last))


def test_rank_4_over_six_modes(ctx, dev):
    """Box (1, 2, 3) with rotation: six modes, the batched replay behind the score role; with
    set_remove_overlap the reference is c3hlac.remove_overlap on the single-frame lists."""
    case = fd.VOSCH
    frames = _frames("dense", _mixed)
    ref = _single(ctx, case, frames, RANK_BOX, RANK, True)
    full = ref["vosch", "dense"][0]
    assert (full["score"][:, -1] > 0).all(), "a list did not fill"
    assert len({int(v) for v in full["mode"].reshape(-1)}) >= 3, "the lists hold few modes"
    # the (1, 16, 16) slab: no 2x2x2 box fits it (the rank-1 tests see its setRank state), but
    # the modes of this box whose x range is 1 do, so here it must give its own search's lists
    assert (ref["slab", "dense"][0]["score"] > 0).any() and not ref["vosch", "empty"][0].tobytes().strip(b"\0")
    removed = {fr: (c3hlac.remove_overlap(v[0].copy(), RANK_BOX), None) for fr, v in ref.items()}
    assert any(removed[fr][0].tobytes() != ref[fr][0].tobytes() for fr in ref), "removeOverlap changes no list"
    _setup(ctx, case, RANK)
    try:
        for overlap, want in ((False, ref), (True, removed)):
            ctx.set_remove_overlap(overlap)
            got, kt, _ = _run(ctx, dev, frames, case, RANK_BOX, RANK, True)
            assert kt["pipeline"][1] == NFR and kt["replay"][1] == NFR, kt
            _check_records(got, frames, want, ("rank", RANK, "remove_overlap", overlap))
            assert frames[20] == ("slab", "dense") and got[20].tobytes() == want["slab", "dense"][0].tobytes()
    finally:
        _restore(ctx)
    # the lists are compared through the scores they were built from (the rule of the rank tests)
    _, sc = fd.oracle(case, "vosch", "dense", RANK_BOX, rank=RANK)
    _check_scores(ref["vosch", "dense"][1], sc, "single-frame scores against the oracle")


def test_wide_models(ctx, dev):
    """M = 3, r = 70 at engine 0: the score launch behind the tick; reference at engine 2."""
    case = fd.WIDE
    frames = _frames("sparse", _mixed)
    ref = _single(ctx, case, frames, BOX, 1, True, engine=2)
    _setup(ctx, case, 1)
    try:
        ctx.set_score_engine(0)
        got, kt, _ = _run(ctx, dev, frames, case, BOX, 1, True)
        assert kt["pipeline"][1] == NFR, kt["pipeline"]
        _check_records(got, frames, ref, "wide models")
        _check_last_scores(ctx, case, frames, ref, BOX)
    finally:
        _restore(ctx)
    _check_oracle(got, frames, case, BOX, True)


def test_streamed_uneven_pushes_and_a_grid_call_after(ctx, dev):
    import torch
    case = fd.VOSCH
    frames = _frames("dense", _mixed)
    ref = _single(ctx, case, frames, RANK_BOX, RANK, True)
    _setup(ctx, case, RANK)
    try:
        whole, _, _ = _run(ctx, dev, frames, case, RANK_BOX, RANK, True)
        got, kt, _ = _run(ctx, dev, frames, case, RANK_BOX, RANK, True, cuts=CUTS)
        assert kt["pipeline"][1] == NFR and kt["replay"][1] == NFR, kt
        assert got.tobytes() == whole.tobytes()
        _check_records(got, frames, ref, "streamed")
        # the stream left open; a grid call on the same context is another key: it drains the
        # stream, and its own records are those of the single-frame path
        _, _, d_open = _run(ctx, dev, frames, case, RANK_BOX, RANK, True, cuts=CUTS, flush=False)
        D, M, r, s = 100, 3, 20, 4
        ctx.search_setup(*bg.bases(D, M, r))
        ctx.set_rank(1)
        names = ["dense", "sparse", "empty", "sparse", "dense"]
        words = {k: torch.from_numpy(w.view(np.int32)).to("cuda:0") for k, w in bg.words().items()}
        d_grid = torch.full((len(names), M * 3), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ptrs = np.array([words[k].data_ptr() for k in names], np.uint64)
        ctx.run_frames(ptrs, (bg.G,) * 3, (0, 0, 0), bg.LEAF, bg.F, THR, s, BOX, bg.EXIST, True,
                       d_grid.data_ptr())
        ctx.synchronize()
        ctx.timing(False)
        late = d_open.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(NFR, case["M"], RANK)
        assert late.tobytes() == whole.tobytes(), "the open stream was not drained"
        grid = d_grid.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(len(names), M, 1)
        for i, k in enumerate(names):
            ctx.set_grid(bg.words()[k], (bg.G,) * 3, (0, 0, 0), bg.LEAF)
            ctx.set_rank(1)
            ctx.extract(bg.F, THR, s)
            lists, _ = ctx.search(BOX, bg.EXIST)
            assert grid[i].tobytes() == lists.tobytes(), ("grid frame", i, k)
    finally:
        _restore(ctx)


FALLBACK = [("vosch", "dense"), ("crop", "sparse"), ("slab", "dense"), ("vosch", "empty"), ("vosch", "sparse"),
            ("crop", "dense")]


@pytest.mark.parametrize("route", ["no_pipeline", "rank_65", "engine_1_r70"])
def test_routes_the_pipeline_does_not_cover(ctx, dev, route):
    case = fd.WIDE if route == "engine_1_r70" else fd.VOSCH
    rank = 65 if route == "rank_65" else 1
    engine = 1 if route == "engine_1_r70" else 0
    ref = _single(ctx, case, FALLBACK, BOX, rank, True, engine=engine)
    _setup(ctx, case, rank)
    try:
        ctx.set_pipeline(route != "no_pipeline")
        ctx.set_score_engine(engine)
        got, kt, _ = _run(ctx, dev, FALLBACK, case, BOX, rank, True)
        assert kt["pipeline"][1] == 0, ("no frame goes through a tick", kt["pipeline"])
        _check_records(got, FALLBACK, ref, route)
        if route == "rank_65":
            ctx.set_remove_overlap(True)
            with pytest.raises(c3hlac.C3HError, match="C3H_ERR_ARG"):
                _run(ctx, dev, FALLBACK, case, BOX, rank, True)
    finally:
        _restore(ctx)


def test_argument_errors(ctx, dev):
    import torch
    _setup(ctx, fd.VOSCH, 1)
    try:
        f, _ = dev("vosch", "dense")
        d_out = torch.zeros((2, fd.VOSCH["M"] * 3), dtype=torch.int64, device="cuda:0")
        kw = dict(rule=1, ranges=BOX, exist_threshold=10, d_out=d_out)
        with pytest.raises(c3hlac.C3HError, match="C3H_ERR_ARG"):  # a frame larger than the canvas
            ctx.run_feature_frames([dev("crop", "dense")[0], f], [fd.CROP, fd.CANVAS], (16, 16, 15), **kw)
        g, _ = dev("grsd", "dense")
        with pytest.raises(c3hlac.C3HError):  # dim != F of search_setup
            ctx.run_feature_frames([g], [fd.CANVAS], fd.CANVAS, **dict(kw, rule=2))
        _setup(ctx, fd.GRSD, 1)
        with pytest.raises(c3hlac.C3HError, match="C3H_ERR_ARG"):  # the VOSCH rule reads f20, f21
            ctx.run_feature_frames([g], [fd.CANVAS], fd.CANVAS, **kw)
        assert not d_out.any().item(), "nothing was enqueued"
    finally:
        _restore(ctx)


def test_no_word_of_the_previous_call_survives(ctx, dev):
    """Two calls on one context: all dense frames, then sparse / empty ones (full and cropped)
    on the same buffer sets.  An exist or has-data word, a list entry or a compressed row of the
    first call left in a set would change the second call's records."""
    case = fd.VOSCH
    first = [("vosch", "dense")] * NFR
    second = [(("crop" if i % 2 else "vosch"), ("sparse", "empty", "sparse")[i % 3]) for i in range(NFR)]
    ref = _single(ctx, case, first + second, BOX, 1, True)
    _setup(ctx, case, 1)
    try:
        got1, kt, _ = _run(ctx, dev, first, case, BOX, 1, True)
        _check_records(got1, first, ref, "first call")
        got2, kt, _ = _run(ctx, dev, second, case, BOX, 1, True)
        assert kt["pipeline"][1] == NFR, kt["pipeline"]
        _check_records(got2, second, ref, "second call")
        _check_last_scores(ctx, case, second, ref, BOX)
    finally:
        _restore(ctx)
