"""The tick's occupancy stream at the chunk sizes of its two paths (csrc/occ_sched.h).

The row-wave path (gx = 256, 512, 1024) streams chunks of C = 16,384 voxels (16 loads of
16 B per lane, C3H_OCC_ROW_UNROLL); whole chunks take unclamped loads, a frame's partial
last chunk a uniform test per wave and load.  The grids below sit on the edges of that
scheme: less than one chunk, exactly one, one plus a partial chunk, 33 1/8 chunks (tail
stealing on, the partial chunk in the pooled tail), gx = 512 (1 3/4 chunks), and a grid of
the general path (16 loads per lane, per-lane clamp).  Every frame holds ~0.5 % random
voxels, voxel 0, the last voxel and both voxels either side of every chunk boundary (of
16,384 and of 24,576 voxels, the other depth measured); one frame of five is empty.

Batches of 8 through the pipelined c3h_run_frames (two full batches and a ragged one), at
S = 4 and S = 10 (ragged last subdivision).  Every frame's detections are compared with the
float64 oracle on its grid (scores within 1e-5 relative, position the oracle's unless tied
within that tolerance); the last frame's exist() and features() with the exact-integer
oracle, no tolerance.  All six grids run in one sequence on one context (the stamps and
buffers of one shape are reused by the next); the parameter chooses which comes last."""
import numpy as np
import pytest

import pyoracle as po
from c3hlac import synth
from conftest import THR

pytestmark = pytest.mark.gpu

RTOL = 1e-5
C_ROW, C_ALT = 256 * 16 * 4, 256 * 24 * 4  # the chunk in voxels; the other measured depth's
GRIDS = [(256, 8, 5), (256, 8, 8), (256, 8, 9), (256, 40, 53), (512, 8, 7), (200, 9, 11)]
assert 256 * 8 * 5 < C_ROW == 256 * 8 * 8 < 256 * 8 * 9 and 8 * 256 * 40 * 53 == 265 * C_ROW
SUBDIVS = [4, 10]
LEAF, F, D, M, R, BOX, EXIST = 0.01, 117, 30, 3, 5, (1, 1, 1), 4
BATCH, NFR, NDISTINCT = 8, 2 * 8 + 5, 5
EMPTY = 3  # the all-empty one of the NDISTINCT frames


def _frame_words(dims, k):
    nvox = dims[0] * dims[1] * dims[2]
    words = np.zeros(nvox, np.uint32)
    if k == EMPTY:
        return words
    rng = np.random.default_rng(1000 * k + dims[1] * 17 + dims[2])
    idx = [rng.choice(nvox, max(1, nvox // 200), replace=False), [0, nvox - 1]]
    for c in (C_ROW, C_ALT):
        b = np.arange(c, nvox + 1, c)
        idx += [b - 1, b[b < nvox]]
    idx = np.unique(np.concatenate([np.asarray(i, np.int64) for i in idx]))
    words[idx] = (1 << 24) | rng.integers(0, 1 << 24, idx.size, dtype=np.uint32)
    return words


@pytest.fixture(scope="module")
def cases(ctx):
    """Per grid: NDISTINCT resident frames; per (grid, S): the oracle's features, exist gate
    and float64 scores of each.  Computed once, shared by every parametrisation."""
    import torch
    axis_t, var, axis_q = synth.random_bases(F, D, M, R, seed=synth.BASE_SEED + 7)
    ap = synth.whiten(axis_t, var)
    out = {}
    for dims in GRIDS:
        words = [_frame_words(dims, k) for k in range(NDISTINCT)]
        d_words = [torch.from_numpy(w.view(np.int32)).to("cuda:0") for w in words]
        ref = {}
        for s in SUBDIVS:
            rs = []
            for w in words:
                g, layout, cloud = po.grid_inputs(w, dims, LEAF)
                fe, sb, _ = po.c3hlac(g, layout, cloud, F, THR, LEAF, s, exact=True)
                ex = po.exist(fe)
                _, _, sc = po.search(sb, fe, ex, ap, axis_q, BOX, 1, EXIST, dbl=True, want_scores=True)
                rs.append((fe, ex, sc, sb))
            ref[s] = rs
        out[dims] = dict(d_words=d_words, ref=ref)
    torch.cuda.synchronize()
    return dict(grids=out, bases=(axis_t, var, axis_q))


def _check_det(rec, scores_f64, shape, tag):
    """rec: (M, 3) int64 c3h_det words of one frame; scores_f64: (M, P) oracle scores of the
    single mode, P in (z, y, x) scan order, -1 where the exist gate rejects the position."""
    ze, ye, xe = shape
    for m in range(rec.shape[0]):
        s = float(rec[m, 0:1].view(np.float64)[0])
        x, y, z, mode = (int(v) for v in rec[m, 1:3].view(np.int32))
        ref = scores_f64[m]
        best = int(np.argmax(ref))  # first maximum in scan order = searchPart's strict '>'
        assert mode == 0, (tag, m, mode)
        if ref[best] <= 0:  # nothing passes the gate (the empty frame): the cleared record
            assert (s, x, y, z) == (0.0, 0, 0, 0), (tag, m, s, (x, y, z))
            continue
        p = (z * ye + y) * xe + x
        assert abs(s - ref[p]) <= RTOL * ref[p], (tag, m, s, ref[p])
        if p != best:  # only a tie within tolerance may pick another position
            assert ref[p] >= ref[best] * (1 - 2 * RTOL), (tag, m, (x, y, z), np.unravel_index(best, shape))


def _distinct(i):
    return (3 * i) % NDISTINCT  # neighbouring frames of a batch differ; the last (i = 20) is not the empty one


@pytest.mark.parametrize("subdiv", SUBDIVS)
@pytest.mark.parametrize("last", range(len(GRIDS)), ids=["%dx%dx%d" % g for g in GRIDS])
def test_tick_occupancy_at_chunk_edges_vs_oracle(ctx, cases, last, subdiv):
    import torch
    assert _distinct(NFR - 1) != EMPTY
    ctx.search_setup(*cases["bases"])
    ctx.set_rank(1)
    ctx.set_batch(BATCH)
    ctx.set_pipeline(True)
    order = [g for i, g in enumerate(GRIDS) if i != last] + [GRIDS[last]]
    try:
        for dims in order:
            case = cases["grids"][dims]
            ref = case["ref"][subdiv]
            ptrs = np.array([case["d_words"][_distinct(i)].data_ptr() for i in range(NFR)], np.uint64)
            d_out = torch.zeros((NFR, M * 3), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            ctx.run_frames(ptrs, dims, (0, 0, 0), LEAF, F, THR, subdiv, BOX, EXIST, True, d_out.data_ptr())
            ctx.synchronize()
            got = d_out.cpu().numpy().reshape(NFR, M, 3)
            for i in range(NFR):
                fe, ex, sc, sb = ref[_distinct(i)]
                shape = tuple(int(n) - b + 1 for n, b in zip(sb[::-1], BOX))  # (z, y, x) positions
                _check_det(got[i], sc.reshape(M, -1), shape, "%s S=%d frame %d" % (dims, subdiv, i))
        # the context holds the last frame of the last grid: exact feature rows and exist gate
        fe, ex, sc, sb = ref[_distinct(NFR - 1)]
        gex = ctx.exist()
        bad = np.flatnonzero(gex != ex)
        assert bad.size == 0, ("exist", bad.size, bad[:8].tolist(), gex[bad[:8]].tolist(), ex[bad[:8]].tolist())
        gf = ctx.features()
        assert gf.shape == fe.shape
        bad = np.flatnonzero((gf != fe).any(1))
        assert bad.size == 0, ("features", bad.size, bad[:8].tolist())
    finally:
        ctx.set_batch(32)
