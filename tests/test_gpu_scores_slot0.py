"""The pipelined tick at rank 1 keeps the per-position score arrays of slot 0 of a batch only
(SparseSearch::scores_slot0_only): for the slots behind it the gate loads no previous score and
writes no -1, and the score role stores no score.  Records must not change, slot 0's array must
stay exact, and a batch that reads every slot again (rank 2) must find them refilled.

Grids of 40^3 with S = 4 (10^3 subdivisions), C3-HLAC-117, D = 30, 3 models x r = 5, 4 frames
per batch.  9 frames are two batches and a ragged one of a single frame; 8 frames are two full
batches, so the draining call's last frame sits in slot 0 of a four-frame batch.  Every call
runs twice on the context, the second time in another frame order, so each buffer set's slots
hold another frame than the last time under an equal score layout (the sparse -1 bookkeeping
of slot 0 then works against the previous frame's pattern).

The reference is every distinct grid on the single-frame path (set_grid, extract, set_rank,
search) of a context of its own: records bit for bit, and scores() byte for byte.

  sparse, sparse2   0.2 % random occupancy
  dense             30 % occupancy: every subdivision holds voxels, every position passes
  empty             no voxel: the cleared record
  tie_first / tie_last / tie_mid
                    a 4^3 block of random colours filling one subdivision, at the grid's first
                    corner, its last corner and at (4, 5, 6); with threshold 0 every position
                    whose box holds it passes and has the same box feature, so the record is
                    the first of them in scan order, and at the corners the only one

Boxes: 2x2x2 (one mode, 729 positions) and 3x2x1 with its six rotation modes.  Threshold 0,
and threshold -1, which passes all-empty boxes too.  Stale slots: rank-1 batches do not keep the score arrays of slots >= 1, so a
rank-2 batch of the same layout afterwards (whose replay reads every slot) must refill them --
records and scores() equal a fresh context's at rank 2 -- and the same the other way round."""
import numpy as np
import pytest

import c3hlac
from c3hlac import synth
from conftest import THR

pytestmark = pytest.mark.gpu

G, S, LEAF, F = 40, 4, 0.04, 117
DMR = (30, 3, 5)
M = DMR[1]
BATCH = 4
ORDER_A = ["sparse", "tie_first", "empty", "dense", "sparse2", "tie_last", "tie_mid", "empty", "sparse"]
ORDER_B = ["dense", "empty", "tie_mid", "sparse2", "tie_last", "sparse", "empty", "tie_first", "dense"]
TIE_SUB = {"tie_first": (0, 0, 0), "tie_last": (9, 9, 9), "tie_mid": (4, 5, 6)}
BOXES = {"box222": ((2, 2, 2), False), "box321r": ((3, 2, 1), True)}


def _words():
    rng = np.random.default_rng(11)

    def rand(p):
        occ = rng.random(G ** 3) < p
        return np.where(occ, (1 << 24) | rng.integers(0, 1 << 24, G ** 3, dtype=np.uint32), 0).astype(np.uint32)

    out = dict(sparse=rand(0.002), sparse2=rand(0.002), dense=rand(0.3), empty=np.zeros(G ** 3, np.uint32))
    for name, (sx, sy, sz) in TIE_SUB.items():
        w = np.zeros((G, G, G), np.uint32)  # z, y, x
        w[S * sz:S * sz + S, S * sy:S * sy + S, S * sx:S * sx + S] = (1 << 24) | rng.integers(
            0, 1 << 24, (S, S, S), dtype=np.uint32)
        out[name] = w.reshape(-1)
    return out


WORDS = _words()


def _setup(c, rank=1):
    c.search_setup(*synth.random_bases(F, *DMR, seed=synth.BASE_SEED + 7))
    c.set_rank(rank)
    c.set_batch(BATCH)
    c.set_pipeline(True)


@pytest.fixture(scope="module")
def grids(ctx):
    import torch
    out = {k: torch.from_numpy(w.view(np.int32)).to("cuda:0") for k, w in WORDS.items()}
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def single(ctx):
    """The single-frame path on a context of its own: (name, box, rotate, thr, rank) ->
    (records (M, rank), scores()), computed once per key."""
    cache = {}
    with c3hlac.Context(0) as c:
        _setup(c)

        def ref(name, box, rotate, thr, rank=1):
            key = (name, box, rotate, thr, rank)
            if key not in cache:
                c.set_grid(WORDS[name], (G,) * 3, (0, 0, 0), LEAF)
                sb, hn = c.extract(F, THR, S)
                assert sb == (G // S,) * 3 and hn == (G // S) ** 3
                c.set_rank(rank)
                lists, _ = c.search(box, thr, rotate=rotate)
                cache[key] = (lists.copy(), c.scores().copy())
            return cache[key]

        yield ref


def _run(c, grids, names, box, rotate, thr, rank=1, pushes=None, through_tick=True):
    """One draining c3h_run_frames (pushes: c3h_stream_frames in pieces and a flush) over the
    named frames: (frames, M, rank) records."""
    import torch
    n = len(names)
    ptrs = np.array([grids[k].data_ptr() for k in names], np.uint64)
    d_out = torch.full((n, M * rank * 3), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    c.timing(c3hlac.timing_mask("pipeline"))
    c.kernel_times(reset=True)
    args = ((G,) * 3, (0, 0, 0), LEAF, F, THR, S, box, thr, rotate)
    try:
        if pushes is None:
            c.run_frames(ptrs, *args, d_out.data_ptr())
        else:
            f0 = 0
            for k in pushes:
                c.run_frames(ptrs[f0:f0 + k], *args, d_out[f0:].data_ptr(), stream=True)
                f0 += k
            assert f0 == n
            c.stream_flush()
        c.synchronize()
        ticked = c.kernel_times(reset=True)["pipeline"][1]
    finally:
        c.timing(False)
    if through_tick:
        assert ticked == n, ("frames through the tick", ticked, n)
    return d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(n, M, rank)


def _check(got, names, single, box, rotate, thr, rank=1):
    bad = [(i, k) for i, k in enumerate(names)
           if got[i].tobytes() != single(k, box, rotate, thr, rank)[0].tobytes()]
    assert not bad, (bad, got[bad[0][0]], single(bad[0][1], box, rotate, thr, rank)[0])


@pytest.fixture()
def tick(ctx):
    _setup(ctx)
    yield ctx
    ctx.timing(False)
    ctx.set_rank(1)
    ctx.set_batch(32)
    ctx.set_pipeline(True)


@pytest.mark.parametrize("key", sorted(BOXES))
def test_reference_frames(single, key):
    """What the frames are meant to exercise holds on the single-frame path itself."""
    box, rotate = BOXES[key]
    nmodes = 6 if rotate else 1
    xr, yr, zr = box
    n = G // S
    P0 = (n - xr + 1) * (n - yr + 1) * (n - zr + 1)  # positions of mode 0 (x, y, z ranges as given)
    if key == "box222":
        assert P0 == 729
    rec, sc = single("dense", box, rotate, 0)
    assert sc.size == nmodes * M * P0 and (sc >= 0).all() and (rec["score"] > 0).all()  # every position passes
    rec, sc = single("empty", box, rotate, 0)
    assert (sc == -1).all() and rec.tobytes() == np.zeros((M, 1), c3hlac.DET_DTYPE).tobytes()
    for name in ("sparse", "sparse2"):
        sc = single(name, box, rotate, 0)[1]
        assert 0.1 < (sc >= 0).mean() < 0.9  # a ragged gate list
    for name, sub in TIE_SUB.items():
        rec, sc = single(name, box, rotate, 0)
        first = tuple(max(0, s - (r - 1)) for s, r in zip(sub, box))  # mode 0 comes first in the schedule
        # a corner's subdivision lies in one position's box only
        passing = int((sc.reshape(nmodes, M, P0)[0, 0] >= 0).sum())
        assert passing == {"tie_first": 1, "tie_last": 1, "tie_mid": xr * yr * zr}[name]
        for m in range(M):
            r = rec[m, 0]
            assert r["score"] > 0 and (int(r["mode"]), int(r["x"]), int(r["y"]), int(r["z"])) == (0,) + first, (name, r)
        ok = sc[sc >= 0].reshape(-1)
        per_model = sc.reshape(nmodes, M, P0)
        for m in range(M):  # all passing positions share one box feature: exact ties
            v = per_model[:, m][per_model[:, m] >= 0]
            assert v.size and np.unique(v).size == 1, (name, m)
        assert ok.size


@pytest.mark.parametrize("key", sorted(BOXES))
@pytest.mark.parametrize("nfr", [9, 8])
def test_records_and_scores_equal_the_single_frame_path(tick, grids, single, key, nfr):
    box, rotate = BOXES[key]
    for order in (ORDER_A, ORDER_B):  # the second call meets the first one's score arrays
        names = order[:nfr]
        got = _run(tick, grids, names, box, rotate, 0)
        _check(got, names, single, box, rotate, 0)
        # the context holds the last frame: slot 0 of its batch, whose arrays are kept
        want = single(names[-1], box, rotate, 0)[1]
        assert tick.scores().tobytes() == want.tobytes(), (key, nfr, names[-1])


@pytest.mark.parametrize("key", sorted(BOXES))
def test_streamed_equals_the_single_frame_path(tick, grids, single, key):
    box, rotate = BOXES[key]
    for order, pushes in ((ORDER_A, (4, 4, 1)), (ORDER_B, (3, 5, 1)), (ORDER_A, (9,))):
        got = _run(tick, grids, order, box, rotate, 0, pushes=pushes)
        _check(got, order, single, box, rotate, 0)


@pytest.mark.parametrize("key", sorted(BOXES))
def test_negative_threshold(tick, grids, single, key):
    """thr = -1: all-empty boxes pass as well."""
    box, rotate = BOXES[key]
    for order in (ORDER_A, ORDER_B):
        got = _run(tick, grids, order[:8], box, rotate, -1)
        _check(got, order[:8], single, box, rotate, -1)
        assert tick.scores().tobytes() == single(order[7], box, rotate, -1)[1].tobytes()
    assert (single("sparse", box, rotate, -1)[1] != -1).all()  # every position passed


def _fresh(grids, names, box, rotate, rank):
    with c3hlac.Context(0) as c:
        _setup(c, rank)
        got = _run(c, grids, names, box, rotate, 0, rank=rank)
        return got, c.scores().copy()


@pytest.mark.parametrize("ranks", [(1, 2), (2, 1)], ids=["rank1_then_rank2", "rank2_then_rank1"])
def test_stale_slots_are_refilled_when_the_rank_changes(tick, grids, single, ranks):
    """Rank-1 batches leave the score arrays of slots >= 1 stale; the rank-2 replay reads every
    slot, so a rank-2 batch of the same layout must dense-fill them (and a rank-1 batch after
    rank-2 ones must still keep slot 0)."""
    box, rotate = BOXES["box321r"]
    first, second = ranks
    tick.set_rank(first)
    for order in (ORDER_A, ORDER_B):
        _run(tick, grids, order[:8], box, rotate, 0, rank=first)
    tick.set_rank(second)
    for order in (ORDER_B, ORDER_A):
        names = order[:8]
        got = _run(tick, grids, names, box, rotate, 0, rank=second)
        want, want_scores = _fresh(grids, names, box, rotate, second)
        assert got.tobytes() == want.tobytes(), (ranks, [i for i in range(8) if got[i].tobytes() != want[i].tobytes()])
        assert tick.scores().tobytes() == want_scores.tobytes()
        _check(got, names, single, box, rotate, 0, rank=second)
