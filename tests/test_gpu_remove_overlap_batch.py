"""SearchObjMulti::removeOverlap on the device for the batch entry points
(c3h_set_remove_overlap, remove_overlap_frames_kernel): with the setting on, d_out must hold,
byte for byte and frame for frame, what the host function c3h_remove_overlap makes of the d_out
of the same call with the setting off.

64^3 dense grid (batch_grids.py), leaf 0.04, C3-HLAC-117, exist threshold 10, S = 4 and 8,
43 frames at 8 per batch (5 full batches and a ragged one).

Cases (D, M, r, rank, box, rotate):
  (40, 12, 20, 12, (2, 2, 2), off)   twelve models of the fast path
  (100, 7, 70, 4, (2, 2, 2), on)     the reference's r = 70 (the tick's wide score role)
  (100, 3, 70, 8, (1, 2, 3), on)     six modes: boxes of different shapes overlap
  (100, 7, 70, 7, (2, 2, 2), off)    rank = M, as detect_object_vosch_multi's setRank(rank * M) / M

A CPU test on the oracle alone shows that removeOverlap has work to do: it changes at least
half of the M lists in every case (measured 11 of 12, 6 of 7, 2 of 3 and 6 of 7 at both S)."""
import numpy as np
import pytest

import batch_grids as bg
import c3hlac
import pyoracle as po
from batch_grids import BATCH, EXIST, F, G, LEAF, NFR
from c3hlac import _capi, synth
from conftest import THR

# (D, M, r, rank, box, rotate)
CASES = [(40, 12, 20, 12, (2, 2, 2), False), (100, 7, 70, 4, (2, 2, 2), True), (100, 3, 70, 8, (1, 2, 3), True),
         (100, 7, 70, 7, (2, 2, 2), False)]
SUBDIVS = (4, 8)


def _id(c):
    return "D%d_M%d_r%d_rank%d_box%d%d%d_%s" % (c[:4] + c[4] + ("rot" if c[5] else "norot",))


def _oracle(case, s):
    """-> (lists as searched, lists after removeOverlap) of the float64 oracle on the dense grid."""
    D, M, r, rank, box, rotate = case
    L, _, _ = bg.oracle_search(D, M, r, s, box, "dense", rank=rank, rotate=rotate)
    before = bg.lists_records(L).copy()
    L2 = po.Lists(M, rank)
    for f in ("score", "x", "y", "z", "mode"):
        getattr(L2, f)[:] = getattr(L, f)
    po.remove_overlap(L2, box)
    return before, bg.lists_records(L2)


@pytest.mark.parametrize("s", SUBDIVS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_oracle_remove_overlap_changes_half_of_the_lists(case, s):
    before, after = _oracle(case, s)
    changed = sum(before[m].tobytes() != after[m].tobytes() for m in range(case[1]))
    assert 2 * changed >= case[1], (case, s, changed)


@pytest.fixture(scope="module")
def d_dense(ctx):
    import torch
    d = torch.from_numpy(bg.words()["dense"].view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    return d


def _setup(ctx, case, rank=None):
    D, M, r = case[:3]
    ctx.search_setup(*bg.bases(D, M, r))
    ctx.set_rank(case[3] if rank is None else rank)
    ctx.set_batch(BATCH)
    ctx.set_pipeline(True)


def _restore(ctx):
    ctx.timing(False)
    ctx.set_remove_overlap(False)
    ctx.set_pipeline(True)
    ctx.set_batch(32)
    ctx.set_rank(1)


def _run(ctx, d_dense, case, s, rank, nfr=NFR):
    import torch
    D, M, r, _, box, rotate = case
    ptrs = np.full(nfr, d_dense.data_ptr(), np.uint64)
    d_out = torch.full((nfr, M * rank * 3), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.run_frames(ptrs, (G,) * 3, (0, 0, 0), LEAF, F, THR, s, box, EXIST, rotate, d_out.data_ptr())
    ctx.synchronize()
    return d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(nfr, M, rank)


def _host(recs, box):
    return np.stack([c3hlac.remove_overlap(fr.copy(), box) for fr in recs])


@pytest.mark.gpu
@pytest.mark.parametrize("s", SUBDIVS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_device_remove_overlap_equals_the_host_function(ctx, d_dense, case, s):
    D, M, r, rank, box, rotate = case
    _setup(ctx, case)
    try:
        ctx.timing(c3hlac.timing_mask("pipeline"))
        ctx.kernel_times(reset=True)
        off = _run(ctx, d_dense, case, s, rank)
        assert ctx.kernel_times(reset=True)["pipeline"][1] == NFR  # (r = 70 included: the wide score role)
        ctx.set_remove_overlap(True)
        on = _run(ctx, d_dense, case, s, rank)
        assert ctx.kernel_times(reset=True)["pipeline"][1] == NFR
        # the context's own lists stay as searched: a search of the empty grid continues from
        # them, finds no candidate and hands them out as they are
        ctx.set_grid(bg.words()["empty"], (G,) * 3, (0, 0, 0), LEAF)
        ctx.extract(F, THR, s)
        held, _ = ctx.search(box, EXIST, rotate=rotate)
        # the lanes
        ctx.set_pipeline(False)
        on_lanes = _run(ctx, d_dense, case, s, rank, nfr=BATCH + 3)
    finally:
        _restore(ctx)
    want = _host(off, box)
    assert (off[0].tobytes() != want[0].tobytes()), "removeOverlap changed nothing"
    for i in range(NFR):
        assert on[i].tobytes() == want[i].tobytes(), (case, s, "frame %d" % i, on[i], want[i])
    for i in range(BATCH + 3):
        assert on_lanes[i].tobytes() == want[i].tobytes(), (case, s, "lanes, frame %d" % i)
    assert held.tobytes() == off[-1].tobytes(), (case, s, "the context's lists", held, off[-1])
    # frame 0 against the float64 oracle: its lists after po.remove_overlap
    _, ref = _oracle(case, s)
    for f in ("x", "y", "z", "mode"):
        assert np.array_equal(on[0][f], ref[f]), (case, s, f, on[0], ref)
    np.testing.assert_allclose(on[0]["score"], ref["score"], rtol=1e-5)


@pytest.mark.gpu
def test_rank_1_launches_nothing_and_rank_65_is_refused(ctx, d_dense):
    import torch
    case = CASES[1]
    D, M, r, _, box, rotate = case
    try:
        _setup(ctx, case, rank=1)
        off = _run(ctx, d_dense, case, 4, 1, nfr=BATCH + 3)
        ctx.set_remove_overlap(True)
        on = _run(ctx, d_dense, case, 4, 1, nfr=BATCH + 3)
        assert on.tobytes() == off.tobytes()
        assert (on["score"] > 0).all()
        ctx.set_rank(65)
        ptrs = np.full(2, d_dense.data_ptr(), np.uint64)
        d_out = torch.zeros((2, M * 65 * 3), dtype=torch.int64, device="cuda:0")
        pts = synth.kinect_scene(5_000, grid=32, leaf=0.02, seed=synth.BASE_SEED)
        for stream in (False, True):
            with pytest.raises(_capi.C3HError, match="C3H_ERR_ARG.*rank <= 64"):
                ctx.run_frames(ptrs, (G,) * 3, (0, 0, 0), LEAF, F, THR, 4, box, EXIST, rotate, d_out.data_ptr(),
                               stream=stream)
        with pytest.raises(_capi.C3HError, match="C3H_ERR_ARG.*rank <= 64"):
            ctx.run_point_frames([pts], 0.02, (64,) * 3, F, THR, 8, box, EXIST, rotate, d_out)
        ctx.set_remove_overlap(False)  # rank 65 with the setting off runs as before
        ctx.run_frames(ptrs, (G,) * 3, (0, 0, 0), LEAF, F, THR, 4, box, EXIST, rotate, d_out.data_ptr())
        ctx.synchronize()
    finally:
        _restore(ctx)


@pytest.mark.gpu
def test_toggling_the_setting_drains_an_open_stream(ctx, d_dense):
    """stream_frames pushes with the setting off, on and off again without a flush in between:
    every frame has the records of the setting it was pushed with."""
    import torch
    case = CASES[1]
    D, M, r, rank, box, rotate = case
    cuts = [0, 2 * BATCH, 4 * BATCH + 3, NFR]
    try:
        _setup(ctx, case)
        off = _run(ctx, d_dense, case, 4, rank, nfr=1)[0]
        ptrs = np.full(NFR, d_dense.data_ptr(), np.uint64)
        d_out = torch.full((NFR, M * rank * 3), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            ctx.set_remove_overlap(k == 1)
            ctx.run_frames(ptrs[a:b], (G,) * 3, (0, 0, 0), LEAF, F, THR, 4, box, EXIST, rotate, d_out[a:].data_ptr(),
                           stream=True)
        ctx.stream_flush()
        ctx.synchronize()
        got = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(NFR, M, rank)
    finally:
        _restore(ctx)
    on = c3hlac.remove_overlap(off.copy(), box)
    assert on.tobytes() != off.tobytes()
    for i in range(NFR):
        want = on if cuts[1] <= i < cuts[2] else off
        assert got[i].tobytes() == want.tobytes(), ("frame %d" % i, got[i], want)


@pytest.mark.gpu
def test_point_frames_batched_and_single_frame_route(ctx):
    """Points-in: a frame the canvas holds stays in the batch, one whose extent is beyond the
    canvas takes the single-frame path; both get removeOverlap."""
    import torch
    dev = torch.device("cuda", 0)
    M, rank, box, leaf, s, canvas = 3, 3, (2, 2, 1), 0.02, 8, 48
    frames = [torch.from_numpy(synth.kinect_scene(n, grid=g, leaf=leaf, seed=synth.BASE_SEED + 2)).to(dev)
              for n, g in ((30_000, 40), (60_000, 64))]
    torch.cuda.synchronize()
    try:
        ctx.search_setup(*synth.random_bases(F, 20, M, 12, seed=synth.BASE_SEED + 3))
        ctx.set_rank(rank)
        ctx.set_batch(4)
        ctx.set_pipeline(True)
        res = {}
        for on in (False, True):
            ctx.set_remove_overlap(on)
            d_out = torch.full((2, M * rank * 3), -1, dtype=torch.int64, device=dev)
            _, info = ctx.run_point_frames(frames, leaf, (canvas,) * 3, F, THR, s, box, EXIST, True, d_out)
            assert info["status"].tolist() == [0, 1], info["status"]
            res[on] = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(2, M, rank)
    finally:
        _restore(ctx)
    want = _host(res[False], box)
    assert want.tobytes() != res[False].tobytes()
    assert res[True].tobytes() == want.tobytes(), (res[True], want)
