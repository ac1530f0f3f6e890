"""The sparse batched C3-HLAC (csrc/c3_sparse.hip) behind c3h_extract_vosch_frames at head 1: columns
20 .. 1000 of every ConVOSCH row of a batch (dim 1001, the 981 bins) and columns 20 .. 136 of every
VOSCH row (dim 137, the 117 bins, rows of stride 137 from column 20), against the oracle, at the
edges of its chunks, slices, plan tiles and launches.

One reference and no tolerance.  For every frame fe, sb, hn = po.c3hlac(..., variant, ..., exact=True)
and ex = po.exist of the exact=False rows (c3_rows_data.reference); columns 20 .. of the frame's
rows, as uint32 views, equal fe where ex > 0 and are all zero bits where ex == 0 -- the sums are
integers and every bin takes one float multiply, the standard the dense c3h_extract meets.  The row
count is hn, info["subdiv_b"] the oracle's counts ((1, 1, 1) for one histogram, as the GRSD front
reports it), info["n_moved"] the oracle's number of voxels whose centroid lies in another cell,
status 0.  Columns 0 .. 19 are compared as bytes with a dim-20 call on the same batch.  No row is
left out; where a rows tensor is passed, every slot past a frame's rows keeps the sentinel.  Head 0
(the per-frame dense extract) and the single-frame c3h_extract_convosch go against the same oracle
rows where stated.  The clouds: c3_sparse_data.py, whose conditions test_c3_sparse_data_cpu.py
asserts with the oracle alone.

What stays uncovered, because a test of a few seconds cannot reach it: more than 4,096 groups of
several chunks (the stride of c3s_final_kernel: over 4.2 million voxels), more than 2,097,152
voxels in a batch (the stride of c3s_keys_kernel), and more than 8,192 plan tiles (16.8 million
voxels, the stride of c3s_plan_kernel)."""
import numpy as np
import pytest

import c3_rows_data as rd
import c3_sparse_data as sd
import c3hlac
import convosch_data as cd
from c3hlac import synth
from conftest import THR

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
SENTINEL = np.float32(-12345.5)
DIM = 1001
VOSCH = 137  # [GRSD-20 | C3-HLAC-117]: the dim - 20 bins of a row are the oracle's variant
ZERO = (0, 0, 0)


@pytest.fixture(scope="module")
def hctx():
    c = c3hlac.Context(0)
    c.set_batch(64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref_ctx():
    c = c3hlac.Context(0)
    yield c
    c.close()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def refs_of(clouds, subdiv, offset, thr, cm, dim=DIM):
    """The oracle's rows per frame at variant dim - 20; None for a frame without a valid point."""
    return [rd.reference(p, sd.LEAF, subdiv, offset, thr, cm, dim - 20) if len(p) else None for p in clouds]


def cap_of(refs):
    return max([r.hn for r in refs if r is not None] + [1])


def extract(ctx, clouds, dim, cap, subdiv, offset, thr=THR, cm=sd.CM, rows=None):
    return ctx.extract_vosch_frames(clouds, sd.LEAF, dim=dim, row_cap=cap, thr=thr, subdiv=subdiv, offset=offset,
                                    normals_radius=sd.RADIUS, color_mode=cm, rows=rows)


_G20 = {}


def grsd20(ctx, clouds, cap, subdiv, offset):
    """Columns 0 .. 19: a dim-20 call on the same batch, once per batch (they depend on neither the
    thresholds nor the colour mode)."""
    key = (tuple(id(p) for p in clouds), subdiv, offset)
    if key not in _G20:
        views, info = extract(ctx, clouds, 20, cap, subdiv, offset)
        _G20[key] = [None if v is None else v.cpu().numpy().copy() for v in views]
    return _G20[key]


def check_rows(got, r, g20, tag, dim=DIM):
    """One frame's rows (H, dim) against the oracle's, every row."""
    assert got.shape == (max(r.hn, 0), dim) and r.fe.shape == (max(r.hn, 0), dim - 20), (tag, got.shape, r.hn)
    if r.hn <= 0:
        return
    c3 = u32(got[:, 20:])
    on = r.ex > 0
    bad = np.flatnonzero((c3[on] != u32(r.fe[on])).any(1))
    assert bad.size == 0, (tag, "rows that exist", bad.size, np.flatnonzero(on)[bad[:8]].tolist(),
                           np.flatnonzero(c3[on][bad[0]] != u32(r.fe[on][bad[0]]))[:8].tolist())
    bad = np.flatnonzero(c3[~on].any(1))
    assert bad.size == 0, (tag, "rows that do not exist", bad.size, np.flatnonzero(~on)[bad[:8]].tolist())
    assert np.array_equal(u32(got[:, :20]), u32(g20)), (tag, "columns 0 .. 19")


def check_batch(views, info, refs, g20, subdiv, tag, rows=None, cap=None, dim=DIM):
    assert len(views) == len(refs)
    slots = None if rows is None else rows.view(len(refs), cap * dim)
    for k, r in enumerate(refs):
        t = (tag, k)
        if r is None:
            assert info["status"][k] == ERR_STATE and views[k] is None, t
            h = 0
        else:
            assert info["status"][k] == 0, (t, info["status"][k])
            assert tuple(info["subdiv_b"][k]) == ((1, 1, 1) if subdiv == 0 else r.sb), (t, info["subdiv_b"][k], r.sb)
            assert tuple(info["div_b"][k]) == r.div_b and tuple(info["min_b"][k]) == r.min_b, t
            assert info["n_occ"][k] == r.n_occ and info["n_valid"][k] == r.n_valid, t
            assert info["n_moved"][k] == r.n_moved, (t, info["n_moved"][k], r.n_moved)
            check_rows(views[k].cpu().numpy(), r, g20[k], t, dim)
            h = max(r.hn, 0)
        if slots is not None:
            assert bool((slots[k, h * dim:] == float(SENTINEL)).all()), (t, "the sentinel past the frame's rows")


def sentinel_rows(n, cap, dim=DIM):
    import torch
    rows = torch.full((n * cap * dim,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()  # torch's fill before the context's stream writes
    return rows


def run_and_check(ctx, gctx, clouds, subdiv, offset, thr, cm, tag, head=1, sentinel=True, dim=DIM):
    """One head-`head` call of dim `dim` on ctx against the oracle; the dim-20 columns from gctx."""
    refs = refs_of(clouds, subdiv, offset, thr, cm, dim)
    cap = cap_of(refs)
    gctx.set_vosch_head(1)
    g20 = grsd20(gctx, clouds, cap, subdiv, offset)
    ctx.set_vosch_head(head)
    rows = sentinel_rows(len(clouds), cap, dim) if sentinel else None
    views, info = extract(ctx, clouds, dim, cap, subdiv, offset, thr, cm, rows=rows)
    check_batch(views, info, refs, g20, subdiv, (tag, "dim", dim, "head", head), rows, cap, dim)
    return refs, g20


def single_and_check(rc, pts, r, g20, subdiv, offset, thr, cm, tag):
    """The single-frame route (c3h_voxelize + c3h_compute_normals + c3h_extract_convosch)."""
    rc.voxelize(pts, sd.LEAF)
    rc.compute_normals(sd.RADIUS)
    sb, hn = rc.extract_convosch(thr, subdiv, offset, color_mode=cm)
    assert tuple(sb) == r.sb and hn == r.hn, (tag, sb, hn)
    check_rows(rc.features(), r, g20, (tag, "single frame"))


# ---- a. the ladders ----------------------------------------------------------------------------
LADDERS = {"a": sd.ladder_a, "b": sd.ladder_b}


@pytest.mark.parametrize("offset", sd.LADDER_OFFSETS, ids=["off000", "off010"])
@pytest.mark.parametrize("arr", ["ab", "ba"])
def test_ladders(hctx, ref_ctx, arr, offset):
    """Group lengths 1, 127 .. 129, 1023 .. 1025, 2047 .. 2049 and an empty row; heads on a plan
    tile's last and first position, a group's end on a tile's end, the last group ending at vtot
    (of one voxel behind A, of five behind B) or followed by "none" keys (offset (0, 1, 0)); three
    thresholds that differ and colours on either side of each, under every colour mode."""
    hctx.set_batch(64)
    clouds = [LADDERS[n]() for n in arr]
    sub = sd.LADDER_SUBDIV
    for cm in sd.COLOR_MODES:
        refs, g20 = run_and_check(hctx, hctx, clouds, sub, offset, sd.LADDER_THR, cm, (arr, offset, cm))
    # head 0 and the single-frame route, one colour mode per case, against the same oracle rows
    cm = sd.COLOR_MODES[((arr == "ba") + 2 * (offset != ZERO)) % 3]
    refs, g20 = run_and_check(hctx, hctx, clouds, sub, offset, sd.LADDER_THR, cm, (arr, offset, cm), head=0)
    for k, pts in enumerate(clouds):
        single_and_check(ref_ctx, pts, refs[k], g20[k], sub, offset, sd.LADDER_THR, cm, (arr, offset, cm, k))


def test_ladder_a_alone_at_batch_1(hctx):
    hctx.set_batch(1)
    try:
        run_and_check(hctx, hctx, [sd.ladder_a()], sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "A at batch 1")
    finally:
        hctx.set_batch(64)


# ---- b. more rows and chunks than one launch ---------------------------------------------------
def test_many_rows(hctx):
    """17,550 rows (c3s_fill_kernel launches 16,384 workgroups) and 10,491 chunks of one voxel
    (c3s_accum_kernel launches 4,096 and reuses its LDS behind barriers): alone, then between
    LADDER_B and a frame without a point, which has no row and status C3H_ERR_STATE; head 0 once."""
    hctx.set_batch(64)
    many = sd.many_rows()
    run_and_check(hctx, hctx, [many], sd.MANY_SUBDIV, ZERO, THR, sd.CM, "many rows alone")
    run_and_check(hctx, hctx, [sd.ladder_b(), many, sd.no_point()], sd.MANY_SUBDIV, ZERO, THR, sd.CM, "many rows in the middle")
    run_and_check(hctx, hctx, [many], sd.MANY_SUBDIV, ZERO, THR, sd.CM, "many rows alone", head=0)


# ---- c. non-cubic and tiny frames of different div_b --------------------------------------------
def test_mixed_boxes(hctx):
    hctx.set_batch(64)
    clouds = list(sd.mixed_boxes())
    order = np.random.default_rng(7).permutation(len(clouds))
    for cm in (c3hlac.COLOR_C3_DOUBLE, c3hlac.COLOR_CHLAC):
        run_and_check(hctx, hctx, clouds, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, cm, ("mixed", cm), sentinel=False)
        run_and_check(hctx, hctx, [clouds[i] for i in order], sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, cm,
                      ("mixed, permuted", cm), sentinel=False)


# ---- d. voxels whose centroid lies in another cell ----------------------------------------------
@pytest.mark.parametrize("key", list(sd.FACE_BATCHES), ids=["S6", "S5-off210", "S16-one", "S0"])
def test_face_frames(hctx, key):
    """The frames of test_gpu_points_exact.py, 36 .. 100 moved voxels each: onto an occupied cell,
    across a subdivision border, into cell -1, into an empty subdivision and out of one that then
    empties.  The one-subdivision frame (S 16) and the frames with a voxel in cell -1 stand in a
    batch with frames of several rows."""
    subdiv, offset = key
    hctx.set_batch(64)
    clouds = [p for _, p, _ in sd.face_frames()[key]]
    for head in (1, 0):
        refs, _ = run_and_check(hctx, hctx, clouds, subdiv, offset, THR, sd.CM, ("face", key), head=head)
    assert all(r.n_moved >= 20 for r in refs)


# ---- e. one context, call after call ------------------------------------------------------------
def test_one_context_call_after_call(hctx):
    """c3s_cnt and c3s_acc are the context's and cleared per call: the white plane and LADDER_A at
    subdivision 50 (39 groups of several chunks, the most of any call here), then mixed_boxes
    (none), LADDER_A, many_rows (none), LADDER_A -- every later call on grown buffers that hold the
    sums of the calls before."""
    a = sd.ladder_a()
    with c3hlac.Context(0) as c:
        c.set_batch(64)
        run_and_check(c, hctx, [cd.white_plane(), a], 50, ZERO, sd.LADDER_THR, sd.CM, "plane + A", sentinel=False)
        run_and_check(c, hctx, list(sd.mixed_boxes()), sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, "mixed", sentinel=False)
        run_and_check(c, hctx, [a], sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "A, second", sentinel=False)
        run_and_check(c, hctx, [sd.many_rows()], sd.MANY_SUBDIV, ZERO, THR, sd.CM, "many rows", sentinel=False)
        run_and_check(c, hctx, [a], sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "A, third", sentinel=False)


# ---- f. the search on top -----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ladders", "face"])
def test_search_records(hctx, which):
    """c3h_run_vosch_point_frames at dim 1001, rank 1, head 1: the records are, as int64 bytes, those
    of c3h_run_feature_frames fed the oracle's rows [dim-20 columns | fe or zeros] with the
    setConVOSCH exist rule."""
    import torch
    dev = torch.device("cuda", 0)
    if which == "ladders":
        clouds, subdiv, offset, thr, box = [sd.ladder_a(), sd.ladder_b()], sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, (2, 1, 1)
    else:
        subdiv, offset, thr, box = 6, ZERO, THR, (2, 2, 2)
        clouds = [p for _, p, _ in sd.face_frames()[(subdiv, offset)]]
    hctx.set_batch(64)
    hctx.set_vosch_head(1)
    refs = refs_of(clouds, subdiv, offset, thr, sd.CM)
    g20 = grsd20(hctx, clouds, cap_of(refs), subdiv, offset)
    M, exist_thr, nf = 2, 5, len(clouds)
    axis_t, var, axis_q = synth.random_bases(DIM, 30, M, 5, seed=78)
    hctx.search_setup(axis_t, var, axis_q)
    hctx.set_rank(1)
    hctx.set_remove_overlap(False)
    feats = []
    for r, g in zip(refs, g20):
        rows = np.concatenate([g, np.where((r.ex > 0)[:, None], r.fe, np.float32(0))], 1)
        feats.append(torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(dev))
    canvas = tuple(max(r.sb[a] for r in refs) for a in range(3))
    want = torch.zeros((nf, M * 3), dtype=torch.int64, device=dev)
    got = torch.full((nf, M * 3), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # torch's uploads and fills before the context's stream reads and writes
    nm_ref = hctx.run_feature_frames(feats, [r.sb for r in refs], canvas, rule=1, ranges=box, exist_threshold=exist_thr,
                                     rotate=True, d_out=want)
    hctx.synchronize()
    want = want.cpu().numpy()
    assert want.view(c3hlac.DET_DTYPE)["score"].max() > 0
    nm, info = hctx.run_vosch_point_frames(clouds, sd.LEAF, canvas, box, exist_thr, dim=DIM, thr=thr, subdiv=subdiv,
                                           offset=offset, normals_radius=sd.RADIUS, color_mode=sd.CM, d_out=got)
    hctx.synchronize()
    assert [int(s) for s in info["status"]] == [0] * nf
    assert [int(n) for n in info["n_moved"]] == [r.n_moved for r in refs]
    assert nm == nm_ref and np.array_equal(got.cpu().numpy(), want)


# ---- g. dim 137: the 117 bins into rows of stride 137 from column 20 ------------------------------
# The same clouds as above, the smallest that reach the kernels' edges: what c3s117_accum_kernel,
# c3s_fill_kernel<4> and c3s_final_kernel<117> write with (variant, stride, col0) = (117, 137, 20)
# against po.c3hlac(..., 117, ..., exact=True).  A slot's rows start at every four-byte alignment of
# a 16-byte quad in turn (137 floats a row), which the fill's head / body / tail split depends on:
# the sentinel past a frame's rows is checked in every case that passes a rows tensor.
@pytest.mark.parametrize("offset", sd.LADDER_OFFSETS, ids=["off000", "off010"])
@pytest.mark.parametrize("arr", ["ab", "ba"])
def test_ladders_137(hctx, arr, offset):
    """test_ladders' batches at dim 137, head 1: a chunk per wave and groups of several chunks, heads
    on plan-tile edges; one colour mode per case (all three: test_color_modes_137)."""
    hctx.set_batch(64)
    clouds = [LADDERS[n]() for n in arr]
    cm = sd.COLOR_MODES[((arr == "ba") + 2 * (offset != ZERO)) % 3]
    run_and_check(hctx, hctx, clouds, sd.LADDER_SUBDIV, offset, sd.LADDER_THR, cm, (arr, offset, cm), dim=VOSCH)


def test_color_modes_137(hctx):
    hctx.set_batch(64)
    for cm in sd.COLOR_MODES:
        run_and_check(hctx, hctx, [sd.ladder_a(), sd.ladder_b()], sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, cm, ("modes", cm),
                      dim=VOSCH)


def test_ladder_a_alone_at_batch_1_137(hctx):
    hctx.set_batch(1)
    try:
        run_and_check(hctx, hctx, [sd.ladder_a()], sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "A at batch 1", dim=VOSCH)
    finally:
        hctx.set_batch(64)


def test_many_rows_137(hctx):
    """17,550 rows: c3s_fill_kernel<4> launches 4,096 workgroups of four rows and sweeps twice."""
    hctx.set_batch(64)
    many = sd.many_rows()
    run_and_check(hctx, hctx, [many], sd.MANY_SUBDIV, ZERO, THR, sd.CM, "many rows alone", dim=VOSCH)
    run_and_check(hctx, hctx, [sd.ladder_b(), many, sd.no_point()], sd.MANY_SUBDIV, ZERO, THR, sd.CM,
                  "many rows in the middle", dim=VOSCH)


@pytest.mark.parametrize("key", list(sd.FACE_BATCHES), ids=["S6", "S5-off210", "S16-one", "S0"])
def test_face_frames_137(hctx, key):
    """test_face_frames' batches: the moved voxels count in the row of the cell their centroid lies
    in, as the dense extract's off-cell correction has it."""
    subdiv, offset = key
    hctx.set_batch(64)
    clouds = [p for _, p, _ in sd.face_frames()[key]]
    refs, _ = run_and_check(hctx, hctx, clouds, subdiv, offset, THR, sd.CM, ("face", key), dim=VOSCH)
    assert all(r.n_moved >= 20 for r in refs)


def test_dims_in_turn_on_one_context():
    """Dim 137, dim 1001 and c3h_extract_c3_frames(117) share the context's c3s_* buffers: in turn,
    twice, each against its own oracle rows."""
    import torch
    clouds = [sd.ladder_a(), sd.ladder_b()]
    sub, thr = sd.LADDER_SUBDIV, sd.LADDER_THR
    r117 = refs_of(clouds, sub, ZERO, thr, sd.CM, VOSCH)
    cap = cap_of(r117)
    with c3hlac.Context(0) as c:
        c.set_batch(64)
        for turn in range(2):
            run_and_check(c, c, clouds, sub, ZERO, thr, sd.CM, ("in turn", turn), dim=VOSCH)
            run_and_check(c, c, clouds, sub, ZERO, thr, sd.CM, ("in turn", turn), dim=DIM)
            rows = torch.full((len(clouds) * cap * 117,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()  # torch's fill before the context's stream writes
            views, eviews, info = c.extract_c3_frames(clouds, sd.LEAF, 117, thr, cap, subdiv=sub, color_mode=sd.CM, rows=rows)
            for k, r in enumerate(r117):
                t = ("in turn", turn, "c3 frames", k)
                got = views[k].cpu().numpy()
                assert info["status"][k] == 0 and got.shape == (r.hn, 117), t
                assert np.array_equal(eviews[k].cpu().numpy(), r.ex), t
                on = r.ex > 0
                assert np.array_equal(u32(got[on]), u32(r.fe[on])) and not u32(got[~on]).any(), t
                assert bool((rows.view(len(clouds), cap * 117)[k, r.hn * 117:] == float(SENTINEL)).all()), t


def test_statuses_137(hctx):
    """The colour mode and the thresholds belong to the call, so the frames that differ are those
    with and without rows: LADDER_B (rows), a frame without a point, and a single cell that offset
    (1, 0, 0) leaves without a row.  Head 1 at dim 137 refuses per frame what the dense 117 extract
    of head 0 refuses, with its status and message: a negative threshold on a frame with rows is
    C3H_ERR_STATE; an invalid colour mode is C3H_ERR_ARG on a frame with rows and -- unlike dim 1001
    and head 0 -- status 0 on the frame without rows (kept, not aligned).  The frame
    without a point stays C3H_ERR_STATE.  No slot is written.  The same batch with good arguments right after is
    exact."""
    hctx.set_batch(64)
    hctx.set_vosch_head(1)
    clouds = [sd.ladder_b(), sd.no_point(), sd.mixed_boxes()[sd.ONE_CELL[0]]]
    sub, thr, off = sd.LADDER_SUBDIV, sd.LADDER_THR, (1, 0, 0)
    refs = refs_of(clouds, sub, off, thr, sd.CM, VOSCH)
    assert refs[0].hn > 0 and refs[2].hn == 0
    cap = cap_of(refs)
    bad_mode = "c3h_extract: variant must be 981 or 117, color_mode a C3H_COLOR_* value"
    bad_thr = "extract_vosch: GRSD / C3 subdivisions differ"
    for dim, kw, want, msg in ((VOSCH, dict(cm=7), [ERR_ARG, ERR_STATE, 0], bad_mode),
                               (DIM, dict(cm=7), [ERR_ARG, ERR_STATE, ERR_ARG], bad_mode),
                               (VOSCH, dict(thr=(thr[0], -1, thr[2])), [ERR_STATE, ERR_STATE, 0], bad_thr)):
        rows = sentinel_rows(len(clouds), cap, dim)
        views, info = extract(hctx, clouds, dim, cap, sub, off, rows=rows, **{"thr": thr, **kw})
        assert [int(v) for v in info["status"]] == want, (dim, kw, info["status"])
        assert [v is None for v in views] == [w < 0 for w in want], (dim, kw)
        assert all(v is None or v.shape[0] == 0 for v in views), (dim, kw, "a frame has rows")
        assert bool((rows == float(SENTINEL)).all()), (dim, kw, "a slot was written")
        assert hctx.lib.c3h_last_error(hctx.h).decode() == msg, (dim, kw)
    run_and_check(hctx, hctx, clouds, sub, off, thr, sd.CM, "after the refused calls", dim=VOSCH)
