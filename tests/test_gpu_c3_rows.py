"""c3h_extract_c3_frames (point clouds in, C3-HLAC 981 / 117 rows out: the batched voxel head and the
sparse pass of csrc/c3_sparse.hip alone) against the oracle.

One reference and no tolerance.  For every frame fe, sb, hn = po.c3hlac(..., variant, ...,
exact=True) and ex = po.exist of the exact=False rows (c3_rows_data.reference); the frame's rows, as
uint32 views, equal fe where ex > 0 and are all zero bits where ex == 0; its exist values equal ex;
info equals the oracle's geometry, counts and n_moved, subdiv_b its counts ((1, 1, 1) for one
histogram), status 0.  No row is left out.  Where sentinel-filled tensors are passed, every element
past a frame's rows and every slot of a failed frame keeps the sentinel, in rows and in exist.
Where stated the rows and exist are also compared, as bytes, with c3h_voxelize + c3h_extract +
c3h_get_features / c3h_get_exist on a second context, and at 981 with columns 20 .. 1000 of a
dim-1001 c3h_extract_vosch_frames call.  The clouds: c3_sparse_data.py and c3_rows_data.py, whose
conditions test_c3_sparse_data_cpu.py and test_c3_rows_data_cpu.py assert with the oracle alone.

What stays uncovered, because a test of a few seconds cannot reach it: more than 4,096 groups of
several chunks (the stride of c3s_final_kernel: over 4.2 million voxels), more than 2,097,152
voxels in a batch (the stride of c3s_keys_kernel), more than 8,192 plan tiles (16.8 million voxels,
the stride of c3s_plan_kernel) and, at 117, more than 16,384 chunks in a batch (the stride of
c3s117_accum_kernel, four chunks a workgroup; the 981 kernel's stride of 4,096 chunks is passed by
many_rows)."""
import numpy as np
import pytest

import c3_rows_data as rd
import c3_sparse_data as sd
import c3hlac
from c3hlac import _capi
from conftest import THR

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_RANGE = -1, -3, -5
SENTINEL = np.float32(-12345.5)
ESENTINEL = -777
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


def refs_of(clouds, variant, subdiv, offset, thr, cm):
    """The oracle's rows per frame; None for a frame without a valid point."""
    return [rd.reference(p, rd.LEAF, subdiv, offset, thr, cm, variant) if len(p) else None for p in clouds]


def cap_of(refs):
    return max([r.hn for r in refs if r is not None] + [1])


def sentinels(n, cap, variant):
    import torch
    rows = torch.full((n * cap * variant,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    exist = torch.full((n * cap,), ESENTINEL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()  # torch's fills before the context's stream writes
    return rows, exist


def check_rows(got, gex, r, variant, tag):
    """One frame's rows (H, variant) and exist (H,) against the oracle's, every row."""
    assert got.shape == (max(r.hn, 0), variant) and gex.shape == (max(r.hn, 0),), (tag, got.shape, gex.shape, r.hn)
    if r.hn <= 0:
        return
    assert np.array_equal(gex, r.ex), (tag, "exist", np.flatnonzero(gex != r.ex)[:8].tolist())
    g = u32(got)
    on = r.ex > 0
    bad = np.flatnonzero((g[on] != u32(r.fe[on])).any(1))
    assert bad.size == 0, (tag, "rows that exist", bad.size, np.flatnonzero(on)[bad[:8]].tolist(),
                           np.flatnonzero(g[on][bad[0]] != u32(r.fe[on][bad[0]]))[:8].tolist())
    bad = np.flatnonzero(g[~on].any(1))
    assert bad.size == 0, (tag, "rows that do not exist", bad.size, np.flatnonzero(~on)[bad[:8]].tolist())


def check_batch(views, eviews, info, refs, variant, subdiv, tag, rows=None, exist=None, cap=None):
    assert len(views) == len(refs) == len(eviews)
    slots = None if rows is None else rows.view(len(refs), cap * variant)
    eslots = None if exist is None else exist.view(len(refs), cap)
    for k, r in enumerate(refs):
        t = (tag, k)
        if r is None:
            assert info["status"][k] == ERR_STATE and views[k] is None and eviews[k] is None, t
            h = 0
        else:
            assert info["status"][k] == 0, (t, info["status"][k])
            assert tuple(info["subdiv_b"][k]) == ((1, 1, 1) if subdiv == 0 else tuple(r.sb)), (t, info["subdiv_b"][k], r.sb)
            assert tuple(info["div_b"][k]) == r.div_b and tuple(info["min_b"][k]) == r.min_b, t
            assert info["n_occ"][k] == r.n_occ and info["n_valid"][k] == r.n_valid, t
            assert info["n_moved"][k] == (r.n_moved if r.hn > 0 else 0), (t, info["n_moved"][k], r.n_moved)
            check_rows(views[k].cpu().numpy(), eviews[k].cpu().numpy(), r, variant, t)
            h = max(r.hn, 0)
        if slots is not None:
            assert bool((slots[k, h * variant:] == float(SENTINEL)).all()), (t, "the sentinel past the frame's rows")
            assert bool((eslots[k, h:] == ESENTINEL).all()), (t, "the exist sentinel past the frame's rows")


def run_and_check(ctx, clouds, variant, subdiv, offset, thr, cm, tag, sentinel=True):
    refs = refs_of(clouds, variant, subdiv, offset, thr, cm)
    cap = cap_of(refs)
    rows, exist = sentinels(len(clouds), cap, variant) if sentinel else (None, None)
    views, eviews, info = ctx.extract_c3_frames(clouds, rd.LEAF, variant, thr, cap, subdiv=subdiv, offset=offset,
                                                color_mode=cm, rows=rows, exist=exist)
    check_batch(views, eviews, info, refs, variant, subdiv, (tag, variant), rows, exist, cap)
    return refs, views, eviews


def single_equal(rc, clouds, views, eviews, variant, subdiv, offset, thr, cm, tag):
    """c3h_voxelize + c3h_extract + c3h_get_features / c3h_get_exist on context rc, as bytes."""
    for k, pts in enumerate(clouds):
        rc.voxelize(pts, rd.LEAF)
        sb, hn = rc.extract(variant, thr, subdiv, offset, color_mode=cm)
        assert hn == views[k].shape[0], (tag, k, hn, views[k].shape)
        assert np.array_equal(u32(rc.features()), u32(views[k].cpu().numpy())), (tag, k, "rows of the single-frame route")
        assert np.array_equal(rc.exist(), eviews[k].cpu().numpy()), (tag, k, "exist of the single-frame route")


# ---- a. the ladders ----------------------------------------------------------------------------
LADDERS = {"a": sd.ladder_a, "b": sd.ladder_b}


@pytest.mark.parametrize("variant", rd.VARIANTS)
@pytest.mark.parametrize("offset", sd.LADDER_OFFSETS, ids=["off000", "off010"])
@pytest.mark.parametrize("arr", ["ab", "ba"])
def test_ladders(hctx, ref_ctx, arr, offset, variant):
    """Group lengths 1, 127 .. 129, 1023 .. 1025, 2047 .. 2049 and an empty row, on either side of the
    981 kernel's slices of 128 and the 117 kernel's of 64; the plan-tile conditions of
    c3_sparse_data; every colour mode; one mode per case also against the single-frame route."""
    hctx.set_batch(64)
    clouds = [LADDERS[n]() for n in arr]
    for cm in sd.COLOR_MODES:
        refs, views, eviews = run_and_check(hctx, clouds, variant, sd.LADDER_SUBDIV, offset, sd.LADDER_THR, cm, (arr, offset, cm))
        if cm == sd.COLOR_MODES[((arr == "ba") + 2 * (offset != ZERO)) % 3]:
            single_equal(ref_ctx, clouds, views, eviews, variant, sd.LADDER_SUBDIV, offset, sd.LADDER_THR, cm, (arr, offset, cm))


@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_ladder_a_alone_at_batch_1(hctx, variant):
    hctx.set_batch(1)
    try:
        run_and_check(hctx, [sd.ladder_a()], variant, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "A at batch 1")
    finally:
        hctx.set_batch(64)


@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_ladder_a_in_one_row(hctx, variant):
    """Subdivision 0: one row of 12 chunks; at 117 its largest sum lies between 2^31 and 2^32."""
    hctx.set_batch(64)
    run_and_check(hctx, [sd.ladder_a()], variant, 0, ZERO, sd.LADDER_THR, sd.CM, "A in one row")


@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_slice_ladder(hctx, variant):
    """Groups of 63, 64, 65, 191, 192 and 193 voxels: around one and three slices of the 117 kernel."""
    hctx.set_batch(64)
    run_and_check(hctx, [rd.slice_ladder(), sd.ladder_b()], variant, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "slices")


# ---- b. sums beyond 2^32 -------------------------------------------------------------------------
@pytest.mark.parametrize("cm", sd.COLOR_MODES)
def test_white_cube(hctx, ref_ctx, cm):
    """8,000 white voxels in one row: first-order 117 sums of 6.0e9, held in the 64-bit slots of a
    group of 8 chunks; at subdivision 10 eight rows of one chunk each (8.0e8 in u32).  The oracle
    is the only standard; whether the single-frame c3h_extract agrees is printed, not asserted."""
    hctx.set_batch(64)
    cube = rd.white_cube()
    run_and_check(hctx, [cube, sd.ladder_b()], 117, 0, ZERO, sd.LADDER_THR, cm, ("cube + B", cm))
    for subdiv in (20, 10):
        refs, views, eviews = run_and_check(hctx, [cube], 117, subdiv, ZERO, sd.LADDER_THR, cm, ("cube", subdiv, cm))
        ref_ctx.voxelize(cube, rd.LEAF)
        ref_ctx.extract(117, sd.LADDER_THR, subdiv, ZERO, color_mode=cm)
        same = np.array_equal(u32(ref_ctx.features()), u32(views[0].cpu().numpy()))
        print("white cube, subdivision %d, colour mode %d: single-frame c3h_extract %s" %
              (subdiv, cm, "agrees" if same else "DIFFERS"))


# ---- c. more rows and chunks than one launch ------------------------------------------------------
@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_many_rows(hctx, variant):
    """17,550 rows (more than the 16,384 of one sweep of the fill: 16,384 workgroups at 981, 4,096 of
    four rows at 117) and 10,491 chunks of one voxel: alone, then
    between LADDER_B and a frame without a point, which has status C3H_ERR_STATE and keeps its
    sentinel slot."""
    hctx.set_batch(64)
    many = sd.many_rows()
    run_and_check(hctx, [many], variant, sd.MANY_SUBDIV, ZERO, THR, sd.CM, "many rows alone")
    run_and_check(hctx, [sd.ladder_b(), many, sd.no_point()], variant, sd.MANY_SUBDIV, ZERO, THR, sd.CM, "many rows in the middle")


# ---- d. non-cubic and tiny frames of different div_b ----------------------------------------------
@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_mixed_boxes(hctx, ref_ctx, variant):
    hctx.set_batch(64)
    clouds = list(sd.mixed_boxes())
    order = np.random.default_rng(7).permutation(len(clouds))
    refs, views, eviews = run_and_check(hctx, clouds, variant, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, "mixed")
    single_equal(ref_ctx, clouds, views, eviews, variant, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, "mixed")
    run_and_check(hctx, [clouds[i] for i in order], variant, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, "mixed, permuted")


# ---- e. voxels whose centroid lies in another cell --------------------------------------------------
@pytest.mark.parametrize("variant", rd.VARIANTS)
@pytest.mark.parametrize("key", list(sd.FACE_BATCHES), ids=["S6", "S5-off210", "S16-one", "S0"])
def test_face_frames(hctx, ref_ctx, key, variant):
    """The frames of test_gpu_points_exact.py: moved voxels, cell -1, the one-row frame among frames
    of several rows; the S 6 batch also against the single-frame route."""
    subdiv, offset = key
    hctx.set_batch(64)
    clouds = [p for _, p, _ in sd.face_frames()[key]]
    refs, views, eviews = run_and_check(hctx, clouds, variant, subdiv, offset, THR, sd.CM, ("face", key))
    assert all(r.n_moved >= 20 for r in refs)
    if key == (6, ZERO):
        single_equal(ref_ctx, clouds, views, eviews, variant, subdiv, offset, THR, sd.CM, ("face", key))


# ---- f. the dim-1001 route is unchanged -------------------------------------------------------------
def test_981_rows_are_columns_20_of_dim_1001(hctx):
    hctx.set_batch(64)
    hctx.set_vosch_head(1)
    clouds = [sd.ladder_a(), sd.ladder_b()]
    refs, views, _ = run_and_check(hctx, clouds, 981, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "981 | 1001")
    v1001, info = hctx.extract_vosch_frames(clouds, rd.LEAF, dim=1001, row_cap=cap_of(refs), thr=sd.LADDER_THR,
                                            subdiv=sd.LADDER_SUBDIV, offset=ZERO, normals_radius=sd.RADIUS, color_mode=sd.CM)
    for k in range(len(clouds)):
        assert info["status"][k] == 0
        assert np.array_equal(u32(v1001[k].cpu().numpy()[:, 20:]), u32(views[k].cpu().numpy())), k


# ---- g. statuses -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_statuses(hctx, variant):
    import torch
    hctx.set_batch(64)
    a, b = sd.ladder_a(), sd.ladder_b()
    ra, rb = refs_of([a, b], variant, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM)
    assert ra.hn == 14 and rb.hn == 6

    def call(clouds, cap, subdiv=sd.LADDER_SUBDIV, offset=ZERO, thr=sd.LADDER_THR, var=variant):
        rows, exist = sentinels(len(clouds), cap, variant)
        return hctx.extract_c3_frames(clouds, rd.LEAF, var, thr, cap, subdiv=subdiv, offset=offset, color_mode=sd.CM,
                                      rows=rows, exist=exist) + (rows.view(len(clouds), -1), exist.view(len(clouds), -1))

    # row_cap one below A's row count: C3H_ERR_RANGE for A only
    views, eviews, info, rows, exist = call([a, b], ra.hn - 1)
    assert info["status"].tolist() == [ERR_RANGE, 0] and views[0] is None and eviews[0] is None
    assert bool((rows[0] == float(SENTINEL)).all()) and bool((exist[0] == ESENTINEL).all())
    check_rows(views[1].cpu().numpy(), eviews[1].cpu().numpy(), rb, variant, "B beside a refused A")
    # an offset at div_b on an axis, and a negative threshold: status 0, no rows, the slot untouched
    for kw in (dict(offset=(0, ra.div_b[1], 0)), dict(offset=(0, 0, ra.div_b[2] + 5)), dict(thr=(64, -1, 200))):
        views, eviews, info, rows, exist = call([a], ra.hn, **kw)
        assert info["status"][0] == 0 and tuple(info["subdiv_b"][0]) == ZERO, (kw, info)
        assert views[0].shape == (0, variant) and eviews[0].shape == (0,) and info["n_moved"][0] == 0, kw
        assert tuple(info["div_b"][0]) == ra.div_b and info["n_occ"][0] == ra.n_occ, kw
        assert bool((rows == float(SENTINEL)).all()) and bool((exist == ESENTINEL).all()), kw
    # a bad variant: C3H_ERR_ARG for the call, nothing written
    rows, exist = sentinels(1, ra.hn, 981)
    with pytest.raises(_capi.C3HError, match="C3H_ERR_ARG"):
        hctx.extract_c3_frames([a], rd.LEAF, 137, sd.LADDER_THR, ra.hn, subdiv=sd.LADDER_SUBDIV, rows=rows, exist=exist)
    with pytest.raises(_capi.C3HError, match="C3H_ERR_ARG"):
        hctx.extract_c3_frames([a], rd.LEAF, variant, sd.LADDER_THR, ra.hn, subdiv=sd.LADDER_SUBDIV, color_mode=7,
                               rows=rows, exist=exist)
    hctx.synchronize()
    assert bool((rows == float(SENTINEL)).all()) and bool((exist == ESENTINEL).all())
    # a caller's tensors are checked
    with pytest.raises(ValueError):
        hctx.extract_c3_frames([a], rd.LEAF, variant, sd.LADDER_THR, ra.hn, subdiv=sd.LADDER_SUBDIV,
                               rows=torch.zeros(3, dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        hctx.extract_c3_frames([a], rd.LEAF, variant, sd.LADDER_THR, ra.hn, subdiv=sd.LADDER_SUBDIV,
                               exist=torch.zeros(ra.hn, dtype=torch.int64, device="cuda:0"))


def test_context_holds_no_grid_afterwards():
    with c3hlac.Context(0) as c:
        c.set_batch(64)
        b = sd.ladder_b()
        c.voxelize(b, rd.LEAF)
        c.extract(117, sd.LADDER_THR, sd.LADDER_SUBDIV)
        run_and_check(c, [b], 117, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "state")
        with pytest.raises(_capi.C3HError, match="C3H_ERR_STATE"):
            c.extract(117, sd.LADDER_THR, sd.LADDER_SUBDIV)
        c.voxelize(b, rd.LEAF)
        sb, hn = c.extract(117, sd.LADDER_THR, sd.LADDER_SUBDIV)
        r = rd.reference(b, rd.LEAF, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, 117)
        check_rows(c.features(), c.exist(), r, 117, "after voxelize")


def test_point_frames_and_device_clouds(hctx):
    """A PointFrames of device tensors is accepted; new tensors come back zeroed past the rows."""
    import torch
    hctx.set_batch(64)
    clouds = [sd.ladder_b(), sd.ladder_a()]
    dev = [torch.from_numpy(np.array(p)).to("cuda:0") for p in clouds]
    torch.cuda.synchronize()
    frames = hctx.prepare_point_frames(dev)
    refs = refs_of(clouds, 117, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM)
    views, eviews, info = hctx.extract_c3_frames(frames, rd.LEAF, 117, sd.LADDER_THR, cap_of(refs), subdiv=sd.LADDER_SUBDIV,
                                                 color_mode=sd.CM)
    check_batch(views, eviews, info, refs, 117, sd.LADDER_SUBDIV, "device clouds")


# ---- h. one context, call after call ------------------------------------------------------------------
def test_one_context_call_after_call(hctx):
    """c3s_cnt and c3s_acc are the context's and cleared per call, the slots 117 or 981 words wide:
    the white cube at 117 (a 64-bit slot beyond 2^32), mixed_boxes at 981 (no slot), LADDER_A at
    117, a dim-1001 c3h_extract_vosch_frames (981-wide slots over the 117 ones), LADDER_A at 117
    again -- every later call on grown buffers that hold the sums of the calls before."""
    a = sd.ladder_a()
    with c3hlac.Context(0) as c:
        c.set_batch(64)
        run_and_check(c, [rd.white_cube()], 117, 0, ZERO, sd.LADDER_THR, sd.CM, "cube", sentinel=False)
        run_and_check(c, list(sd.mixed_boxes()), 981, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, "mixed", sentinel=False)
        run_and_check(c, [a], 117, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "A, first", sentinel=False)
        r = sd.reference(a, sd.LEAF, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM)
        views, info = c.extract_vosch_frames([a], sd.LEAF, dim=1001, row_cap=r.hn, thr=sd.LADDER_THR, subdiv=sd.LADDER_SUBDIV,
                                             offset=ZERO, normals_radius=sd.RADIUS, color_mode=sd.CM)
        assert info["status"][0] == 0
        c3 = u32(views[0].cpu().numpy()[:, 20:])
        on = r.ex > 0
        assert np.array_equal(c3[on], u32(r.fe[on])) and not c3[~on].any()
        run_and_check(c, [a], 117, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "A, second", sentinel=False)
