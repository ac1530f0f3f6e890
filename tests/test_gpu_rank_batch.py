"""Rank > 1 through the batch entry points: the batched rank replay (replay_frames_kernel)
behind the pipelined tick and on the lanes, against the single-frame path's replay_kernel.

64^3 grids, leaf 0.04, C3-HLAC-117, exist threshold 10, the four resident grids of
test_gpu_tick_score.py (scene, rolled, dense, empty), 8 frames per batch over 5 full batches
and a ragged one of 3, so every one of the four buffer sets is reused; the frame cycle is
shifted by one after four batches, so a set's slot holds another grid than the last time.

Cases (D, M, r) / S / box / rank:
  (20, 7, 12)   / 4 / (2, 2, 2) /  4   3,375 positions: one full chunk of 2,048 and a ragged one
  (20, 7, 12)   / 4 / (2, 2, 1) /  2   three modes
  (100, 10, 20) / 4 / (1, 2, 3) /  4   six modes, the bench's bases
  (100, 10, 20) / 8 / (2, 2, 2) / 33   343 positions, less than one chunk
  (20, 7, 12)   / 8 / (1, 2, 3) / 33   six modes
  (100, 10, 20) / 4 / (2, 2, 2) / 64   the largest rank whose list lives on the lanes of a wave
  (20, 7, 12)   / 8 / (2, 2, 2) / 65   stays on the per-frame replay (lanes)

The reference is each distinct grid searched on the single-frame path (set_grid, set_rank,
extract, search): code this feature does not touch.  Every frame's M x rank records must be
bit-identical to it with the pipeline on and with it off; with the pipeline on and rank <= 64
every frame goes through the tick and the batched replay (kernel_times); afterwards the
context holds the last frame's scores and lists.  The reference
records themselves must show that the update was exercised: full lists at ranks 2 and 4,
lists that never fill at rank 33 (setRank-state slots take part in the overlap test), both
at rank 64.

Points-in: c3h_run_point_frames at rank 3 keeps every frame in the batch (status 0) with the
single-frame path's records."""
import numpy as np
import pytest

import c3hlac
from c3hlac import synth
from conftest import THR

pytestmark = pytest.mark.gpu

G, LEAF, F, EXIST = 64, 0.04, 117, 10
BATCH, NFR = 8, 5 * 8 + 3
NAMES = ["scene", "rolled", "dense", "empty"]
CYCLE = ["empty", "scene", "rolled", "dense"]
# (D, M, r), S, box, rank
CASES = [((20, 7, 12), 4, (2, 2, 2), 4), ((20, 7, 12), 4, (2, 2, 1), 2), ((100, 10, 20), 4, (1, 2, 3), 4),
         ((100, 10, 20), 8, (2, 2, 2), 33), ((20, 7, 12), 8, (1, 2, 3), 33), ((100, 10, 20), 4, (2, 2, 2), 64),
         ((20, 7, 12), 8, (2, 2, 2), 65)]
IDS = ["D%d_M%d_r%d_S%d_box%d%d%d_rank%d" % (c[0] + (c[1],) + c[2] + (c[3],)) for c in CASES]


@pytest.fixture(scope="module")
def grids(ctx):
    """The four resident grids: host words and device copies."""
    import torch
    gi = ctx.voxelize(synth.kinect_scene(60_000, grid=G, leaf=LEAF, seed=synth.BASE_SEED + 1), LEAF)
    assert list(gi.div_b) == [G] * 3
    scene = ctx.grid().reshape(G, G, G).copy()
    rng = np.random.default_rng(5)
    occ = rng.random(G ** 3) < 0.05
    dense = np.where(occ, (1 << 24) | rng.integers(0, 1 << 24, G ** 3, dtype=np.uint32), 0).astype(np.uint32)
    words = dict(scene=scene.reshape(-1), rolled=np.ascontiguousarray(np.roll(scene, 5, axis=2)).reshape(-1),
                 dense=dense, empty=np.zeros(G ** 3, np.uint32))
    d_words = {k: torch.from_numpy(w.view(np.int32)).to("cuda:0") for k, w in words.items()}
    torch.cuda.synchronize()
    return dict(words=words, d_words=d_words)


_REFS = {}


def _refs(ctx, grids, case):
    """The single-frame path's records of the four grids for one case: computed once."""
    if case not in _REFS:
        (D, M, r), s, box, rank = case
        bases = synth.random_bases(F, D, M, r, seed=synth.BASE_SEED + 3)
        ctx.search_setup(*bases)
        ref = {}
        for k in NAMES:
            ctx.set_grid(grids["words"][k], (G,) * 3, (0, 0, 0), LEAF)
            ctx.set_rank(rank)
            ctx.extract(F, THR, s)
            lists, _ = ctx.search(box, EXIST)
            assert lists.shape == (M, rank)
            ref[k] = lists.copy()
        # the cases exercise the update (conditions on the reference alone)
        if rank in (2, 4):
            for k in ("scene", "dense"):
                assert (ref[k]["score"][:, -1] > 0).all(), (case, k, "a list did not fill")
        if rank == 33:
            for k in ("scene", "rolled", "dense"):
                assert (ref[k]["score"][:, -1] == 0).all(), (case, k, "a list filled")
        if rank == 64:
            assert (ref["dense"]["score"] > 0).all(), (case, "dense leaves a slot empty")
            assert (ref["scene"]["score"][:, -1] == 0).all(), (case, "scene fills a list")
        empty = np.zeros((M, rank), c3hlac.DET_DTYPE)  # the setRank state
        assert np.array_equal(ref["empty"], empty), case
        _REFS[case] = dict(bases=bases, ref=ref)
    return _REFS[case]


def _frame_name(i):
    return CYCLE[(i + i // (4 * BATCH)) % 4]  # shifted by one once every buffer set was used


def _names():
    names = [_frame_name(i) for i in range(NFR)]
    assert names[-1] == "dense" and set(names[:BATCH]) == set(NAMES)
    assert any(names[i] != names[i + 4 * BATCH] for i in range(NFR - 4 * BATCH))  # a set's slot changes grid
    return names


def _check_records(got, names, ref, tag):
    for i, k in enumerate(names):
        assert np.array_equal(got[i], ref[k]), (tag, "frame %d (%s)" % (i, k), got[i], ref[k])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_batched_rank_replay_matches_single_frame_path(ctx, grids, case):
    import torch
    (D, M, r), s, box, rank = case
    refs = _refs(ctx, grids, case)
    names = _names()
    ptrs = np.array([grids["d_words"][k].data_ptr() for k in names], np.uint64)
    ctx.search_setup(*refs["bases"])
    ctx.set_rank(rank)
    ctx.set_batch(BATCH)
    try:
        for pipeline in (True, False):
            ctx.set_pipeline(pipeline)
            d_out = torch.full((NFR, M * rank * 3), -1, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            ctx.timing(c3hlac.timing_mask("pipeline", "replay"))
            ctx.kernel_times(reset=True)
            ctx.run_frames(ptrs, (G,) * 3, (0, 0, 0), LEAF, F, THR, s, box, EXIST, True, d_out.data_ptr())
            ctx.synchronize()
            kt = ctx.kernel_times(reset=True)
            ctx.timing(False)
            got = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(NFR, M, rank)
            _check_records(got, names, refs["ref"], (case, "pipeline", pipeline))
            if pipeline and rank <= 64:
                assert kt["pipeline"][1] == NFR, ("frames through the tick", kt["pipeline"])
                assert kt["replay"][1] == NFR, ("frames through the batched replay", kt["replay"])
            # the context holds the last frame: its scores replayed on the host from fresh lists
            fresh = np.zeros((M, rank), c3hlac.DET_DTYPE)
            again = c3hlac.replay_scores(ctx.scores(), ctx.subdiv, box, fresh.copy(), rotate=True)  # (in place)
            assert np.array_equal(again, got[-1]), (case, "host replay of the last frame's scores", pipeline)
            # the empty frames' lists are the setRank state
            for i, k in enumerate(names):
                if k == "empty":
                    assert np.array_equal(got[i], fresh), (case, i)
            # ... and the last frame's lists: a search of the empty grid continues from the lists
            # the context holds and finds no candidate, so it hands them out as they are
            ctx.set_grid(grids["words"]["empty"], (G,) * 3, (0, 0, 0), LEAF)
            ctx.extract(F, THR, s)
            held, _ = ctx.search(box, EXIST)
            assert np.array_equal(held, got[-1]), (case, "the context's lists after run_frames", pipeline)
    finally:
        ctx.timing(False)
        ctx.set_pipeline(True)
        ctx.set_batch(32)
        ctx.set_rank(1)


def test_streamed_batches_at_rank_4(ctx, grids):
    """c3h_stream_frames in two calls and a flush: the same records as c3h_run_frames."""
    import torch
    case = CASES[0]
    (D, M, r), s, box, rank = case
    refs = _refs(ctx, grids, case)
    names = _names()
    ptrs = np.array([grids["d_words"][k].data_ptr() for k in names], np.uint64)
    ctx.search_setup(*refs["bases"])
    ctx.set_rank(rank)
    ctx.set_batch(BATCH)
    ctx.set_pipeline(True)
    try:
        d_out = torch.full((NFR, M * rank * 3), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ctx.timing(c3hlac.timing_mask("pipeline", "replay"))
        ctx.kernel_times(reset=True)
        cut = 3 * BATCH  # the second call ends on the ragged batch
        for a, b in ((0, cut), (cut, NFR)):
            ctx.run_frames(ptrs[a:b], (G,) * 3, (0, 0, 0), LEAF, F, THR, s, box, EXIST, True, d_out[a:].data_ptr(),
                           stream=True)
        ctx.stream_flush()
        ctx.synchronize()
        kt = ctx.kernel_times(reset=True)
        assert kt["pipeline"][1] == NFR and kt["replay"][1] == NFR, kt
        got = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(NFR, M, rank)
        _check_records(got, names, refs["ref"], (case, "streamed"))
    finally:
        ctx.timing(False)
        ctx.set_batch(32)
        ctx.set_rank(1)


P_G, P_LEAF, P_S, P_BOX, P_RANK, P_M, P_BATCH, P_NFR = 64, 0.02, 8, (2, 2, 1), 3, 3, 4, 12


def test_point_frames_at_rank_3_stay_in_the_batch(ctx):
    """12 device frames (colours varied, x shifted by whole cells so min_b varies) on a 64^3
    canvas: every frame batched (status 0), records those of the single-frame path."""
    import torch
    dev = torch.device("cuda", 0)
    base = torch.from_numpy(synth.kinect_scene(60_000, grid=P_G, leaf=P_LEAF, seed=synth.BASE_SEED + 2)).to(dev)
    frames = []
    for k in range(P_NFR):
        t = base.clone()
        bits = t[:, 3].view(torch.int32)
        t[:, 3] = (bits ^ ((k * 0x2F1D37) & 0xFFFFFF)).view(torch.float32)
        t[:, 0] = (t[:, 0].double() + k * P_LEAF).float()
        frames.append(t)
    torch.cuda.synchronize()
    ctx.search_setup(*synth.random_bases(F, 20, P_M, 12, seed=synth.BASE_SEED + 3))
    ctx.set_rank(P_RANK)
    ctx.set_batch(P_BATCH)
    ctx.set_pipeline(True)
    try:
        d_out = torch.full((P_NFR, P_M * P_RANK * 3), -1, dtype=torch.int64, device=dev)
        nm, info = ctx.run_point_frames(frames, P_LEAF, (P_G,) * 3, F, THR, P_S, P_BOX, EXIST, True, d_out)
        assert nm == 3
        assert (info["status"] == 0).all(), info["status"]
        assert len(set(info["min_b"][:, 0].tolist())) == P_NFR  # the x shift moves min_b
        got = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(P_NFR, P_M, P_RANK)
        assert (got["score"][:, :, 0] > 0).all()
        for i in range(P_NFR):
            ctx.voxelize(frames[i], P_LEAF)
            ctx.set_rank(P_RANK)
            ctx.extract(F, THR, P_S)
            ref, _ = ctx.search(P_BOX, EXIST)
            assert np.array_equal(got[i], ref), (i, got[i], ref)
    finally:
        ctx.set_batch(32)
        ctx.set_rank(1)
