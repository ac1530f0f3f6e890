"""The tick's segment-occupancy map (csrc/occ_sched.h): the row-wave stream writes one
uint16 per 256-voxel span, bit s = the span's s-th 64-byte segment holds a voxel, and the
tile role of the next tick does not fetch the halo words of empty segments.  A wrong or stale
bit is a voxel read as 0, i.e. a wrong feature row.

Grids: the row-wave grids of test_gpu_occ_depth.py (less than a chunk, one chunk, one plus a
partial chunk, 33 1/8 chunks with tail stealing, gx = 512: two spans per row) and 200x9x11,
which takes the general path with the map off.  S = 4 and S = 10, batches of 8.

Frames: five distinct per grid, one of them empty: ~0.5 % random voxels, voxel 0, the last
voxel, both sides of every chunk boundary, both sides of every 16-word segment boundary in x
(both in frames 2 and 4, one side alternating in the others, so a segment occupied in one
frame is empty in the next), and, in every frame but 0 and the empty one, tiles of both S whose
first centre has its -x, -y and -z neighbours in the segment, row and plane before the tile,
which hold none of its centres; the last frame, checked exactly, is frame 4.  69 frames = 2 x 4 full batches + a ragged
one: every buffer set is reused, frame i and frame i + 32 share set and slot and always
differ, the empty frame both follows and precedes an occupied one there.

Checks: every frame's M x 3 record words byte-identical between set_pipeline(True) and
set_pipeline(False) (the lanes never see the map); the detections against the float64 oracle
(score within 1e-5 relative, position the oracle's unless tied within 2e-5); the last
frame's features() and exist() equal to the exact-integer oracle.  A streamed sequence
(c3h_stream_frames) and a points-in sequence on a 256-wide canvas (stamped batches: no
stream, map off) agree with the single-frame path."""
import numpy as np
import pytest

import c3hlac
import pyoracle as po
from c3hlac import synth
from conftest import THR

pytestmark = pytest.mark.gpu

RTOL = 1e-5
C_ROW = 256 * 16 * 4  # the row-wave chunk in voxels
GRIDS = [(256, 8, 5), (256, 8, 8), (256, 8, 9), (256, 40, 53), (512, 8, 7), (200, 9, 11)]
SUBDIVS = [4, 10]
LEAF, F, D, M, R, BOX, EXIST = 0.01, 117, 30, 3, 5, (1, 1, 1), 4
BATCH, SETS, NDISTINCT, EMPTY = 8, 4, 5, 3
NFR = 2 * SETS * BATCH + 5


def _distinct(i):
    return (3 * i) % NDISTINCT


def _frame_words(dims, k):
    gx, gy, gz = dims
    nvox = gx * gy * gz
    words = np.zeros(nvox, np.uint32)
    if k == EMPTY:
        return words
    rng = np.random.default_rng(7000 * k + gy * 17 + gz)
    idx = [rng.choice(nvox, max(1, nvox // 200), replace=False), [0, nvox - 1]]
    b = np.arange(C_ROW, nvox + 1, C_ROW)
    idx += [b - 1, b[b < nvox]]
    # every 16-word boundary of one row: both sides (x = 16m - 1 and 16m) in frames 2 and 4,
    # one side in the others, alternating with m + k (the segment next to it is empty there)
    m = np.arange(1, gx // 16 + (1 if gx % 16 else 0))
    row = (((k + 1) % gz) * gy + (2 * k + 1) % gy) * gx
    idx.append(row + 16 * m - ((m + k) % 2 == 0))
    if k in (2, 4):
        idx += [row + 16 * m - 1, row + 16 * m]
    # tiles (S = 4: from x0 = 16; S = 10: from x0 = 80) with a first centre whose -x, -y, -z
    # neighbours lie in the segment / row / plane before the tile
    for s in SUBDIVS:
        x0 = 16 * s // np.gcd(16, s)
        y0, z0 = (s if s < gy else 0), (s if s < gz else 0)
        if x0 >= gx or k == 0:  # not in frame 0 (nor the empty one): the segment before is empty there
            continue
        for dx, dy, dz in [(0, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (-1, -1, -1)]:
            x, y, z = x0 + dx, y0 + dy, z0 + dz
            if min(x, y, z) >= 0:
                idx.append([(z * gy + y) * gx + x])
    idx = np.unique(np.concatenate([np.asarray(i, np.int64).ravel() for i in idx]))
    words[idx] = (1 << 24) | rng.integers(0, 1 << 24, idx.size, dtype=np.uint32)
    return words


@pytest.fixture(scope="module")
def cases(ctx):
    """Per grid: the resident frames; per (grid, S): the oracle's features, exist gate and
    float64 scores of each.  Computed once, shared by every test here."""
    import torch
    axis_t, var, axis_q = synth.random_bases(F, D, M, R, seed=synth.BASE_SEED + 11)
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
        out[dims] = dict(words=words, d_words=d_words, ref=ref)
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
        best = int(np.argmax(ref))
        assert mode == 0, (tag, m, mode)
        if ref[best] <= 0:  # nothing passes the gate (the empty frame): the cleared record
            assert (s, x, y, z) == (0.0, 0, 0, 0), (tag, m, s, (x, y, z))
            continue
        p = (z * ye + y) * xe + x
        assert abs(s - ref[p]) <= RTOL * ref[p], (tag, m, s, ref[p])
        if p != best:  # only a tie within tolerance may pick another position
            assert ref[p] >= ref[best] * (1 - 2 * RTOL), (tag, m, (x, y, z), np.unravel_index(best, shape))


def _run(ctx, case, dims, subdiv, nfr, pipeline, stream_sizes=None):
    import torch
    ptrs = np.array([case["d_words"][_distinct(i)].data_ptr() for i in range(nfr)], np.uint64)
    d_out = torch.zeros((nfr, M * 3), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.set_pipeline(pipeline)
    if stream_sizes is None:
        ctx.run_frames(ptrs, dims, (0, 0, 0), LEAF, F, THR, subdiv, BOX, EXIST, True, d_out.data_ptr())
    else:
        f0 = 0
        for n in stream_sizes:
            ctx.run_frames(ptrs[f0:f0 + n], dims, (0, 0, 0), LEAF, F, THR, subdiv, BOX, EXIST, True,
                           d_out.data_ptr() + f0 * M * 3 * 8, stream=True)
            f0 += n
        assert f0 == nfr
        ctx.stream_flush()
    ctx.synchronize()
    return d_out.cpu().numpy().reshape(nfr, M, 3)


def test_frame_sequence_reuses_every_set_with_other_occupancy(cases):
    """The sequence the tests below run does what the stale-map case needs."""
    per = SETS * BATCH
    pairs = [(_distinct(i), _distinct(i + per)) for i in range(NFR - per)]
    assert all(a != b for a, b in pairs)
    assert any(a == EMPTY for a, b in pairs) and any(b == EMPTY for a, b in pairs)
    assert _distinct(NFR - 1) != EMPTY
    for dims in GRIDS[:5]:  # segment bitmaps of the distinct frames differ pairwise, both ways
        w = cases["grids"][dims]["words"]
        seg = [np.add.reduceat(x != 0, np.arange(0, x.size, 16)) > 0 for x in w]
        for a in range(NDISTINCT):
            for b in range(NDISTINCT):
                if a != b and a != EMPTY:
                    assert (seg[a] & ~seg[b]).any(), (dims, a, b)


@pytest.mark.parametrize("subdiv", SUBDIVS)
@pytest.mark.parametrize("dims", GRIDS, ids=["%dx%dx%d" % g for g in GRIDS])
def test_tick_with_segment_map_vs_lanes_and_oracle(ctx, cases, dims, subdiv):
    ctx.search_setup(*cases["bases"])
    ctx.set_rank(1)
    ctx.set_batch(BATCH)
    case = cases["grids"][dims]
    ref = case["ref"][subdiv]
    try:
        lanes = _run(ctx, case, dims, subdiv, NFR, False)
        got = _run(ctx, case, dims, subdiv, NFR, True)
        # the context holds the last frame: exact feature rows and exist gate
        fe, ex, sc, sb = ref[_distinct(NFR - 1)]
        gex = ctx.exist()
        gf = ctx.features()
    finally:
        ctx.set_pipeline(True)
        ctx.set_batch(32)
    bad = [i for i in range(NFR) if got[i].tobytes() != lanes[i].tobytes()]
    assert not bad, ("pipeline != lanes", len(bad), bad[:8], [_distinct(i) for i in bad[:8]])
    for i in range(NFR):
        fe_i, ex_i, sc_i, sb_i = ref[_distinct(i)]
        shape = tuple(int(n) - b + 1 for n, b in zip(sb_i[::-1], BOX))
        _check_det(got[i], sc_i.reshape(M, -1), shape, "%s S=%d frame %d" % (dims, subdiv, i))
    bad = np.flatnonzero(gex != ex)
    assert bad.size == 0, ("exist", bad.size, bad[:8].tolist(), gex[bad[:8]].tolist(), ex[bad[:8]].tolist())
    assert gf.shape == fe.shape
    bad = np.flatnonzero((gf != fe).any(1))
    assert bad.size == 0, ("features", bad.size, bad[:8].tolist())


def _single_grid(ctx, words, dims, subdiv):
    """The single-frame path: c3h_set_grid + c3h_extract + search from fresh lists."""
    ctx.set_grid(words, dims, (0, 0, 0), LEAF)
    ctx.extract(F, THR, subdiv)
    ctx.set_rank(1)
    lists, _ = ctx.search(BOX, EXIST)
    return lists.copy()


@pytest.mark.parametrize("dims", [(256, 40, 53), (512, 8, 7)], ids=["256x40x53", "512x8x7"])
def test_streamed_frames_agree_with_single_frame_path(ctx, cases, dims):
    """c3h_stream_frames in ragged pushes (the pipeline stays filled, sets keep rotating):
    the same detections as the single-frame path of each distinct frame."""
    subdiv = 10
    ctx.search_setup(*cases["bases"])
    ctx.set_rank(1)
    ctx.set_batch(BATCH)
    case = cases["grids"][dims]
    try:
        got = _run(ctx, case, dims, subdiv, NFR, True, stream_sizes=[BATCH, 3 * BATCH, 5, BATCH + 7, NFR - 5 * BATCH - 12])
        single = [_single_grid(ctx, case["words"][k], dims, subdiv) for k in range(NDISTINCT)]
    finally:
        ctx.set_batch(32)
    for i in range(NFR):
        fe, ex, sc, sb = case["ref"][subdiv][_distinct(i)]
        shape = tuple(int(n) - b + 1 for n, b in zip(sb[::-1], BOX))
        _check_det(got[i], sc.reshape(M, -1), shape, "streamed %s frame %d" % (dims, i))
        one = single[_distinct(i)][:, 0]
        rec = got[i].reshape(-1).view(c3hlac.DET_DTYPE)
        for m in range(M):
            s1 = float(one[m]["score"])
            assert abs(float(rec[m]["score"]) - s1) <= RTOL * abs(s1), (dims, i, m)
            if (int(rec[m]["x"]), int(rec[m]["y"]), int(rec[m]["z"])) != (int(one[m]["x"]), int(one[m]["y"]), int(one[m]["z"])):
                ref = sc.reshape(M, -1)[m]
                p = (int(rec[m]["z"]) * shape[1] + int(rec[m]["y"])) * shape[2] + int(rec[m]["x"])
                assert ref[p] >= ref.max() * (1 - 2 * RTOL), (dims, i, m)


def test_points_in_on_a_row_wave_canvas_agrees_with_single_frame_path(ctx, cases):
    """Points-in batches are stamped by the voxeliser's scatter: no occupancy role in their
    first tick, so no map, on a canvas whose rows the stream would take as whole spans."""
    import torch
    canvas, subdiv, nfr = (256, 16, 16), 10, 2 * SETS * BATCH + 3
    frames = []
    for k in range(NDISTINCT):
        rng = np.random.default_rng(90 + k)
        nv = canvas[0] * canvas[1] * canvas[2]
        idx = np.unique(np.concatenate([rng.choice(nv, nv // (40 if k != EMPTY else 4000), replace=False), [0, nv - 1]]))
        xyz = np.stack([idx % canvas[0], idx // canvas[0] % canvas[1], idx // (canvas[0] * canvas[1])], 1)
        pts = np.empty((idx.size, 4), np.float32)
        pts[:, :3] = ((xyz + 0.5) * LEAF).astype(np.float32)
        pts[:, 3] = rng.integers(0, 1 << 24, idx.size, dtype=np.uint32).view(np.float32)
        frames.append(pts)
    ctx.search_setup(*cases["bases"])
    ctx.set_rank(1)
    ctx.set_batch(BATCH)
    ctx.set_pipeline(True)
    try:
        d_out = torch.zeros((nfr, M * 3), dtype=torch.int64, device="cuda:0")
        nm, info = ctx.run_point_frames([frames[_distinct(i)] for i in range(nfr)], LEAF, canvas, F, THR, subdiv, BOX,
                                        EXIST, True, d_out)
        got = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(nfr, M)
        assert (info["status"] == 0).all(), np.flatnonzero(info["status"])
        assert (info["div_b"] == np.array(canvas)).all()
        single = []
        for k in range(NDISTINCT):
            ctx.voxelize(frames[k], LEAF)
            ctx.extract(F, THR, subdiv)
            ctx.set_rank(1)
            lists, _ = ctx.search(BOX, EXIST)
            single.append(lists.copy())
    finally:
        ctx.set_batch(32)
    for i in range(nfr):
        assert np.array_equal(got[i], single[_distinct(i)][:, 0]), i
