"""c3h_extract_c3_frames_packed (point clouds in, only the C3-HLAC 981 / 117 rows with exist > 0 out,
frame after frame in row order: the packed mode of csrc/c3_sparse.hip) against the oracle.

One reference and no tolerance.  packed_rows_data.packed concatenates fe[ex > 0] of
c3_rows_data.reference in frame order; the call's rows, as uint32 views, equal it; frame, row and
exist of the id records, n_packed (the number of rows returned), frame_first and info equal the
oracle's; every element past row n_packed of the sentinel-filled rows and ids tensors keeps the
sentinel.  The same bytes come from c3h_extract_c3_frames on the same context (rows and exist where
exist > 0).  set_batch(5) and set_batch(64) give identical bytes; the count query gives the full
call's count; with cap = n - 1 and cap = 1 the call returns C3H_ERR_RANGE with the count needed,
the rows and ids below cap are right and everything from cap on keeps the sentinel.  The clouds:
c3_sparse_data.py and c3_rows_data.py, whose packed conditions test_packed_rows_data_cpu.py asserts
with the oracle alone.

What stays uncovered, because a test of a few seconds cannot reach it: more than 256 plan tiles in
a batch (the second round of c3s_pack_scan_kernel's one workgroup, 256 tiles a round: over 524,288
voxels), more than 8,192 plan tiles (the stride of c3s_pack_count_kernel and of c3s_plan_kernel:
16.8 million voxels), and the strides test_gpu_c3_rows.py names for the kernels the packed mode
shares with the dense one (c3s_keys_kernel, c3s_final_kernel, c3s117_accum_kernel).
c3s_pack_frames_kernel has a workgroup per frame and one more, at most 65: no stride."""
import numpy as np
import pytest

import c3_rows_data as rd
import c3_sparse_data as sd
import c3hlac
import packed_rows_data as pd_
from c3hlac import _capi
from conftest import THR

pytestmark = pytest.mark.gpu
ERR_STATE = -3
SENTINEL = np.float32(-12345.5)
ISENTINEL = -777
ZERO = (0, 0, 0)
SLACK = 3  # sentinel rows behind the capacity


@pytest.fixture(scope="module")
def hctx():
    c = c3hlac.Context(0)
    c.set_batch(64)
    yield c
    c.close()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sentinels(cap, variant):
    import torch
    rows = torch.full(((cap + SLACK) * variant,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    ids = torch.full(((cap + SLACK) * 4,), ISENTINEL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()  # torch's fills before the context's stream writes
    return rows, ids


def check_prefix(rows, ids, p, k, variant, tag):
    """The first k packed rows and id records against the oracle's, and the sentinel from k on."""
    g = rows.cpu().numpy().reshape(-1, variant)
    rec = ids.cpu().numpy().reshape(-1, 4)
    bad = np.flatnonzero((u32(g[:k]) != u32(p.rows[:k])).any(1))
    assert bad.size == 0, (tag, "rows", bad.size, bad[:8].tolist(), p.frame[bad[:8]].tolist(), p.row[bad[:8]].tolist())
    assert np.array_equal(rec[:k, 0], p.frame[:k]), (tag, "frame")
    assert np.array_equal(np.ascontiguousarray(rec[:k, 2:4]).view(np.int64)[:, 0], p.row[:k]), (tag, "row")
    assert np.array_equal(rec[:k, 1], p.exist[:k]), (tag, "exist")
    assert (g[k:] == SENTINEL).all(), (tag, "the sentinel past the rows")
    assert (rec[k:] == ISENTINEL).all(), (tag, "the id sentinel past the rows")


def check_info(info, refs, subdiv, tag):
    for k, r in enumerate(refs):
        if r is None:
            assert info["status"][k] == ERR_STATE, (tag, k)
            continue
        assert info["status"][k] == 0, (tag, k, info["status"][k])
        assert tuple(info["subdiv_b"][k]) == ((1, 1, 1) if subdiv == 0 else tuple(r.sb)), (tag, k)
        assert tuple(info["div_b"][k]) == r.div_b and tuple(info["min_b"][k]) == r.min_b, (tag, k)
        assert info["n_occ"][k] == r.n_occ and info["n_valid"][k] == r.n_valid, (tag, k)
        assert info["n_moved"][k] == (r.n_moved if r.hn > 0 else 0), (tag, k)


def run_and_check(ctx, clouds, variant, subdiv, offset, thr, cm, tag, dense=False):
    p = pd_.packed(clouds, subdiv, offset, thr, cm, variant)
    rows, ids = sentinels(p.n, variant)
    out, frame, row, exist, first, info = ctx.extract_c3_frames_packed(clouds, rd.LEAF, variant, thr, subdiv=subdiv, offset=offset,
                                                                      color_mode=cm, cap=p.n, rows=rows, ids=ids)
    assert out.shape == (p.n, variant) and frame.shape == row.shape == exist.shape == (p.n,), (tag, out.shape, p.n)
    assert np.array_equal(first, p.frame_first), (tag, first.tolist(), p.frame_first.tolist())
    check_prefix(rows, ids, p, p.n, variant, tag)
    assert np.array_equal(row.cpu().numpy(), p.row) and np.array_equal(frame.cpu().numpy(), p.frame), tag
    check_info(info, p.refs, subdiv, tag)
    if dense:  # the same bytes as the dense route on the same context
        cap = max([r.hn for r in p.refs if r is not None] + [1])
        views, eviews, dinfo = ctx.extract_c3_frames(clouds, rd.LEAF, variant, thr, cap, subdiv=subdiv, offset=offset, color_mode=cm)
        got = out.cpu().numpy()
        for k, r in enumerate(p.refs):
            a, b = first[k], first[k + 1]
            if views[k] is None or views[k].shape[0] == 0:
                assert a == b, (tag, k)
                continue
            ex = eviews[k].cpu().numpy()
            on = ex > 0
            assert np.array_equal(u32(views[k].cpu().numpy()[on]), u32(got[a:b])), (tag, k, "rows of the dense route")
            assert np.array_equal(ex[on], exist.cpu().numpy()[a:b]), (tag, k, "exist of the dense route")
            assert np.array_equal(np.flatnonzero(on), row.cpu().numpy()[a:b]), (tag, k)
    return p, rows, ids


LADDERS = {"a": sd.ladder_a, "b": sd.ladder_b}


@pytest.mark.parametrize("variant", rd.VARIANTS)
@pytest.mark.parametrize("offset", sd.LADDER_OFFSETS, ids=["off000", "off010"])
@pytest.mark.parametrize("arr", ["a", "ab", "ba"])
def test_ladders(hctx, arr, offset, variant):
    """Groups of several chunks (their slot beside multi_row), an empty row between groups, "none"
    keys behind the groups at offset (0, 1, 0), heads on both sides of the plan tiles' edges."""
    hctx.set_batch(64)
    run_and_check(hctx, [LADDERS[n]() for n in arr], variant, sd.LADDER_SUBDIV, offset, sd.LADDER_THR, sd.CM, (arr, offset),
                  dense=arr == "ba")


@pytest.mark.parametrize("variant", rd.VARIANTS)
@pytest.mark.parametrize("cm", sd.COLOR_MODES)
def test_colour_modes(hctx, variant, cm):
    hctx.set_batch(64)
    run_and_check(hctx, [sd.ladder_b(), sd.ladder_a()], variant, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, cm, ("modes", cm))


@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_slice_ladder(hctx, variant):
    hctx.set_batch(64)
    run_and_check(hctx, [rd.slice_ladder(), sd.ladder_b()], variant, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "slices", dense=True)


def mixed_with_no_point():
    clouds = list(sd.mixed_boxes())
    clouds.insert(7, sd.no_point())
    return clouds


@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_mixed_boxes_with_a_frame_without_a_point(hctx, variant):
    """65 frames: two batches at 64, frames without a row, a failed frame with an empty range."""
    hctx.set_batch(64)
    p, _, _ = run_and_check(hctx, mixed_with_no_point(), variant, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, "mixed + none")
    assert p.n == 1067 and p.frame_first[7] == p.frame_first[8]
    run_and_check(hctx, list(sd.mixed_boxes()), variant, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, "mixed", dense=True)


@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_many_rows(hctx, variant):
    """10,491 heads over six plan tiles: the tiles' scan and the ordinals inside a tile full of heads;
    then between LADDER_B and a frame without a point."""
    hctx.set_batch(64)
    many = sd.many_rows()
    run_and_check(hctx, [many], variant, sd.MANY_SUBDIV, ZERO, THR, sd.CM, "many rows alone")
    run_and_check(hctx, [sd.ladder_b(), many, sd.no_point()], variant, sd.MANY_SUBDIV, ZERO, THR, sd.CM, "many rows in the middle")


@pytest.mark.parametrize("variant", rd.VARIANTS)
@pytest.mark.parametrize("key", list(sd.FACE_BATCHES), ids=["S6", "S5-off210", "S16-one", "S0"])
def test_face_frames(hctx, key, variant):
    subdiv, offset = key
    hctx.set_batch(64)
    clouds = [p for _, p, _ in sd.face_frames()[key]]
    run_and_check(hctx, clouds, variant, subdiv, offset, THR, sd.CM, ("face", key), dense=key == (6, ZERO))


@pytest.mark.parametrize("cm", sd.COLOR_MODES)
def test_white_cube(hctx, cm):
    """One row of 8 chunks with 64-bit sums (c3s_final_kernel's packed epilogue), then eight rows."""
    hctx.set_batch(64)
    run_and_check(hctx, [rd.white_cube(), sd.ladder_b()], 117, 0, ZERO, sd.LADDER_THR, cm, ("cube + B", cm))
    run_and_check(hctx, [rd.white_cube()], 117, 10, ZERO, sd.LADDER_THR, cm, ("cube", 10, cm))


@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_batch_sizes_give_identical_bytes(hctx, variant):
    """set_batch(5) (13 batches, the packed base carried on the host) and set_batch(64)."""
    clouds = mixed_with_no_point()
    got = []
    try:
        for b in (5, 64):
            hctx.set_batch(b)
            _, rows, ids = run_and_check(hctx, clouds, variant, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, ("batch", b))
            got.append((rows.cpu().numpy().view(np.uint32), ids.cpu().numpy()))
    finally:
        hctx.set_batch(64)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("variant", rd.VARIANTS)
def test_count_query_and_overflow(hctx, variant):
    hctx.set_batch(64)
    clouds = [sd.ladder_b(), sd.ladder_a()]
    args = dict(subdiv=sd.LADDER_SUBDIV, offset=ZERO, color_mode=sd.CM)
    p = pd_.packed(clouds, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, variant)
    # cap=None: the count query first, tensors of exactly that size
    out, frame, row, exist, first, info = hctx.extract_c3_frames_packed(clouds, rd.LEAF, variant, sd.LADDER_THR, **args)
    assert out.shape == (p.n, variant) and np.array_equal(u32(out.cpu().numpy()), u32(p.rows))
    assert np.array_equal(exist.cpu().numpy(), p.exist) and np.array_equal(first, p.frame_first)
    # cap=0 is the query alone
    out0, _, _, _, first0, _ = hctx.extract_c3_frames_packed(clouds, rd.LEAF, variant, sd.LADDER_THR, cap=0, **args)
    assert out0.shape == (0, variant) and np.array_equal(first0, p.frame_first)
    for cap in (p.n - 1, 1):
        rows, ids = sentinels(cap, variant)
        with pytest.raises(_capi.C3HError, match="C3H_ERR_RANGE") as e:
            hctx.extract_c3_frames_packed(clouds, rd.LEAF, variant, sd.LADDER_THR, cap=cap, rows=rows, ids=ids, **args)
        assert e.value.needed == p.n, (cap, e.value.needed)
        check_prefix(rows, ids, p, cap, variant, ("overflow", cap))


def test_statuses_and_arguments(hctx):
    import torch
    hctx.set_batch(64)
    a = sd.ladder_a()
    # a negative threshold: the silent-empty frame, status 0 and no rows
    out, frame, row, exist, first, info = hctx.extract_c3_frames_packed([a, sd.ladder_b()], rd.LEAF, 117, (64, -1, 200),
                                                                       subdiv=sd.LADDER_SUBDIV)
    assert out.shape == (0, 117) and first.tolist() == [0, 0, 0] and info["status"].tolist() == [0, 0]
    with pytest.raises(_capi.C3HError, match="C3H_ERR_ARG"):
        hctx.extract_c3_frames_packed([a], rd.LEAF, 137, sd.LADDER_THR, subdiv=sd.LADDER_SUBDIV, cap=4)
    with pytest.raises(ValueError):
        hctx.extract_c3_frames_packed([a], rd.LEAF, 117, sd.LADDER_THR, subdiv=sd.LADDER_SUBDIV, cap=14,
                                      rows=torch.zeros(3, dtype=torch.float32, device="cuda:0"))


def test_dense_dim_1001_and_packed_on_one_context():
    """c3s_cnt, c3s_acc and the chunks are the context's: a dense call, a dim-1001 call and a packed
    call one after another, then the dense call again."""
    a = sd.ladder_a()
    with c3hlac.Context(0) as c:
        c.set_batch(64)
        c.set_vosch_head(1)
        r = rd.reference(a, rd.LEAF, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, 981)
        on = r.ex > 0
        for _ in range(2):
            views, eviews, info = c.extract_c3_frames([a], rd.LEAF, 981, sd.LADDER_THR, r.hn, subdiv=sd.LADDER_SUBDIV, color_mode=sd.CM)
            g = u32(views[0].cpu().numpy())
            assert np.array_equal(g[on], u32(r.fe[on])) and not g[~on].any() and np.array_equal(eviews[0].cpu().numpy(), r.ex)
            v1001, info = c.extract_vosch_frames([a], rd.LEAF, dim=1001, row_cap=r.hn, thr=sd.LADDER_THR, subdiv=sd.LADDER_SUBDIV,
                                                 offset=ZERO, normals_radius=sd.RADIUS, color_mode=sd.CM)
            c3 = u32(v1001[0].cpu().numpy()[:, 20:])
            assert info["status"][0] == 0 and np.array_equal(c3[on], u32(r.fe[on])) and not c3[~on].any()
            run_and_check(c, [a], 981, sd.LADDER_SUBDIV, ZERO, sd.LADDER_THR, sd.CM, "packed after dense and 1001")
            run_and_check(c, [rd.white_cube()], 117, 0, ZERO, sd.LADDER_THR, sd.CM, "packed 117 after 981")
