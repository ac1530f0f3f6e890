"""The batched voxel head of c3h_extract_vosch_frames / c3h_run_vosch_point_frames
(c3h_set_vosch_head(1); csrc/voxelize.hip vh_*) against the single-frame route -- c3h_voxelize +
c3h_compute_normals + c3h_extract_vosch / c3h_extract_grsd on a second context, as
test_gpu_vosch_frames.py -- and against the per-frame head (c3h_set_vosch_head(0)) on the same
inputs.  Every test sets the head itself, on a context of this module.  Every comparison is of
bytes (uint32 views): rows, info, per-point normals, per-voxel radii and types, search records.
The clouds: vosch_frames_data.py and vox_head_data.py, whose conditions test_vox_head_cpu.py
asserts with numpy and the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import c3hlac
import pyoracle as po
import vosch_frames_data as vd
import vox_head_data as hd
from c3hlac import _capi, synth
from conftest import THR
from test_gpu_vosch_frames import cap_of, check_frames, run_batch, single, single_on, u32

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_RANGE = -1, -3, -5
SENTINEL = np.float32(-12345.5)
INF = float("inf")
HEADS = (1, 0)


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


def on_device(clouds):
    import torch
    out = [torch.from_numpy(np.array(c, np.float32)).to("cuda:0") for c in clouds]
    torch.cuda.synchronize()
    return out


def test_the_setter_takes_0_and_1_only(hctx):
    for head in (0, 1):
        hctx.set_vosch_head(head)
    for head in (-1, 2, 137):
        with pytest.raises(_capi.C3HError, match="C3H_ERR_ARG"):
            hctx.set_vosch_head(head)


@pytest.mark.parametrize("z_limit", vd.Z_LIMITS, ids=["plain", "z1"])
@pytest.mark.parametrize("dim,normalize", [(137, False), (137, True), (20, False), (20, True)])
def test_routes_agree(hctx, ref_ctx, dim, normalize, z_limit):
    names = [n for n, _ in vd.batch()]
    clouds = [p for _, p in vd.batch()]
    refs = [single(ref_ctx, p, vd.LEAF, z_limit, vd.RADIUS, dim, normalize) for p in clouds]
    hctx.set_batch(64)
    for head in HEADS:
        hctx.set_vosch_head(head)
        for frames in (clouds, on_device(clouds)):
            views, info = run_batch(hctx, frames, vd.LEAF, z_limit, vd.RADIUS, dim, normalize, cap_of(refs))
            check_frames(hctx, refs, views, info)
            if z_limit == vd.Z_LIMITS[0]:
                assert info["n_moved"][names.index("edge")] == 1
    # this batch's composite voxel key would fit 32 bits (test_wide_voxel_keys holds one that does not)
    nvox = max(int(np.prod(np.array(r["div_b"], np.int64))) for r in refs if r["status"] == 0)
    assert hd.key_bits(nvox, len(clouds)) <= 32


def test_fine_leaf_with_off_cell_centroids(hctx, ref_ctx):
    clouds = [p for _, p in vd.fine_batch()]
    refs = [single(ref_ctx, p, vd.FINE_LEAF, INF, vd.RADIUS, 137, False) for p in clouds]
    for head in HEADS:
        hctx.set_vosch_head(head)
        for frames in (clouds, on_device(clouds)):
            views, info = run_batch(hctx, frames, vd.FINE_LEAF, INF, vd.RADIUS, 137, False, cap_of(refs))
            check_frames(hctx, refs, views, info)
            assert info["n_moved"][0] == 14 and info["n_occ"][0] == 945


def test_long_run_is_summed_in_input_order(hctx, ref_ctx):
    d = dict(vd.batch())
    cloud, _ = hd.long_run_cloud()
    clouds = [d["noisy_sphere_green"], cloud, d["noiseless_cone_red"]]
    for dim in (137, 20):
        refs = [single(ref_ctx, p, vd.LEAF, INF, vd.RADIUS, dim, False) for p in clouds]
        assert refs[1]["status"] == 0 and len(refs[1]["rows"]) > 100
        for head in HEADS:
            hctx.set_vosch_head(head)
            views, info = run_batch(hctx, clouds, vd.LEAF, INF, vd.RADIUS, dim, False, cap_of(refs))
            check_frames(hctx, refs, views, info)  # rows, and the RSD getter's per-voxel arrays


def test_face_points_feed_the_off_cell_correction(hctx, ref_ctx):
    face = hd.face_cloud()
    g, layout, cloud = po.voxelize(face, vd.LEAF)
    moved = vd.moved_voxels(g, layout, cloud, vd.LEAF)
    assert moved > 0
    clouds = [dict(vd.batch())["edge"], face, dict(vd.batch())["noisy_sphere_green"]]
    refs = [single(ref_ctx, p, vd.LEAF, INF, vd.RADIUS, 137, False) for p in clouds]
    assert refs[1]["status"] == 0 and refs[1]["n_occ"] == g.n_occ and len(refs[1]["rows"]) > 100
    for head in HEADS:
        hctx.set_vosch_head(head)
        views, info = run_batch(hctx, clouds, vd.LEAF, INF, vd.RADIUS, 137, False, cap_of(refs))
        check_frames(hctx, refs, views, info)
        assert info["n_moved"][1] == moved and info["n_moved"][0] == 1


def test_wide_voxel_keys(hctx, ref_ctx):
    """64 frames, one of them with a box of 2^26 voxels and more: the composite voxel key holds
    more than 32 bits (the head sorts 64-bit words whatever the batch; a key cut to 32 bits would
    file this frame's points under other frames)."""
    small = [p for _, p in vd.batch() if len(p) > 1]
    wide = hd.wide_key_cloud()
    clouds = [small[i % len(small)] for i in range(63)]
    clouds.insert(40, wide)
    sub, off = 32, (0, 0, 0)
    refs = [single(ref_ctx, p, vd.LEAF, INF, vd.RADIUS, 20, False, subdiv=sub, offset=off) for p in clouds]
    assert all(r["status"] == 0 for r in refs)
    hctx.set_batch(64)
    for head in HEADS:
        hctx.set_vosch_head(head)
        views, info = run_batch(hctx, clouds, vd.LEAF, INF, vd.RADIUS, 20, False, cap_of(refs), subdiv=sub, offset=off)
        check_frames(hctx, refs, views, info, getters=False)
        nvox = int(np.prod(info["div_b"][40].astype(np.int64)))
        assert nvox >= 2 ** 26 and hd.key_bits(nvox, len(clouds)) > 32
    for i in (39, 40, 41):
        assert np.array_equal(u32(hctx.frame_normals(i)), u32(refs[i]["normals"]))


def test_statuses_in_one_batch(hctx, ref_ctx):
    import torch
    d, s = dict(vd.batch()), hd.status_clouds()
    good = [d["noisy_sphere_green"], d["noiseless_cone_red"], d["edge"], d["bowl1_0000"]]
    clouds = [good[0], s["no_point"], good[1], s["all_nan"], s["far_x"], good[2], s["thirteen"], good[3]]
    refs = [single(ref_ctx, p, vd.LEAF, INF, vd.RADIUS, 137, False) for p in clouds]
    assert [r["status"] for r in refs] == [0, ERR_STATE, 0, ERR_STATE, ERR_RANGE, 0, ERR_RANGE, 0]
    e = 5  # the edge cloud: row_cap one below its rows
    small = len(refs[e]["rows"]) - 1
    assert small >= max(len(r["rows"]) for k, r in enumerate(refs) if k != e)
    cut = [dict(r, status=ERR_RANGE) if k == e else r for k, r in enumerate(refs)]
    for head in HEADS:
        hctx.set_vosch_head(head)
        rows = torch.full((len(clouds) * small * 137,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        views, info = run_batch(hctx, clouds, vd.LEAF, INF, vd.RADIUS, 137, False, small, rows=rows)
        check_frames(hctx, cut, views, info)
        slots = rows.view(len(clouds), small * 137)
        for k, r in enumerate(cut):
            h = len(r["rows"]) if r["status"] == 0 else 0
            assert (slots[k, h * 137:] == float(SENTINEL)).all(), k
            if r["status"] < 0:
                with pytest.raises(_capi.C3HError, match="C3H_ERR_STATE"):
                    hctx.frame_normals(k)
    # more than 2^27 search cells: a call of its own, at the normals radius that makes them
    radius = 0.004
    clouds = [good[1], s["fine_box"], good[0]]
    refs = [single(ref_ctx, p, vd.LEAF, INF, radius, 20, False) for p in clouds]
    assert [r["status"] for r in refs] == [0, ERR_RANGE, 0]
    for head in HEADS:
        hctx.set_vosch_head(head)
        views, info = run_batch(hctx, clouds, vd.LEAF, INF, radius, 20, False, cap_of(refs))
        check_frames(hctx, refs, views, info)


def test_batch_sizes_and_order(hctx, ref_ctx):
    clouds = [p for _, p in vd.batch()]
    refs = [single(ref_ctx, p, vd.LEAF, INF, vd.RADIUS, 137, False) for p in clouds]
    cap = cap_of(refs)
    hctx.set_vosch_head(1)
    for B in (1, 3, 64):
        hctx.set_batch(B)
        views, info = run_batch(hctx, clouds, vd.LEAF, INF, vd.RADIUS, 137, False, cap)
        check_frames(hctx, refs, views, info, getters=B >= len(clouds))
        if B < len(clouds):  # the getters speak of one batch only
            with pytest.raises(_capi.C3HError, match="C3H_ERR_STATE"):
                hctx.frame_normals(0)
            with pytest.raises(_capi.C3HError, match="C3H_ERR_STATE"):
                hctx.frame_rsd(0)
    hctx.set_batch(64)
    order = np.random.default_rng(3).permutation(len(clouds))
    views, info = run_batch(hctx, [clouds[i] for i in order], vd.LEAF, INF, vd.RADIUS, 137, False, cap)
    check_frames(hctx, [refs[i] for i in order], views, info)


def test_state_after_a_batched_head_call():
    """After a head-1 call the context holds no single-frame grid; the single-frame route then
    gives a fresh context's bytes, and so do head-1 batches, head-0 batches and single frames
    interleaved on one context."""
    named = vd.batch()
    clouds = [p for _, p in named]
    edge = dict(named)["edge"]
    narrow = (edge, vd.LEAF, INF, vd.RADIUS, 137, False)
    wide = (edge, 0.1, INF, vd.RADIUS, 20, False, 0, (0, 0, 0))  # leaf 0.1: the RSD grid of its own

    def batch_on(c, head):
        c.set_batch(64)
        c.set_vosch_head(head)
        views, info = run_batch(c, clouds, vd.LEAF, INF, vd.RADIUS, 137, False, cap)
        out = []
        for i, v in enumerate(views):
            if v is None:
                out.append(None)
                continue
            radii, types = c.frame_rsd(i)
            out.append(dict(rows=v.cpu().numpy().copy(), normals=c.frame_normals(i), radii=radii, types=types))
        return out, np.array(info["status"]).copy()

    def fresh(fn, *args):
        with c3hlac.Context(0) as c:
            return fn(c, *args)

    def same(got, want):
        assert got.keys() == want.keys() and got["status"] == 0
        for k in want:
            if isinstance(want[k], np.ndarray):
                assert want[k].size > 0 and np.array_equal(u32(got[k]), u32(want[k])), k
            else:
                assert got[k] == want[k], k

    def same_batch(got, want):
        assert np.array_equal(got[1], want[1])
        for g, w in zip(got[0], want[0]):
            assert (g is None) == (w is None)
            if g is not None:
                for k in w:
                    assert np.array_equal(u32(g[k]), u32(w[k])), k

    want_narrow, want_wide = fresh(single_on, *narrow), fresh(single_on, *wide)
    cap = len(want_narrow["rows"])
    want_batch = fresh(batch_on, 0)
    same_batch(fresh(batch_on, 1), want_batch)
    with c3hlac.Context(0) as c:
        same(single_on(c, *narrow), want_narrow)
        for _ in range(2):
            same_batch(batch_on(c, 1), want_batch)
            with pytest.raises(_capi.C3HError, match="C3H_ERR_STATE"):
                c.compute_normals(vd.RADIUS)
            gi = _capi.GridInfo()
            assert c.lib.c3h_get_grid_info(c.h, C.byref(gi)) == ERR_STATE
            same(single_on(c, *narrow), want_narrow)
            same(single_on(c, *wide), want_wide)
            same_batch(batch_on(c, 0), want_batch)
            same_batch(batch_on(c, 1), want_batch)
            same(single_on(c, *wide), want_wide)
            same(single_on(c, *narrow), want_narrow)
            with pytest.raises(_capi.C3HError, match="C3H_ERR_STATE"):
                c.frame_normals(0)


@pytest.mark.parametrize("rank,overlap", [(1, False), (4, True)])
def test_search_records(hctx, ref_ctx, rank, overlap):
    import torch
    dev = torch.device("cuda", 0)
    clouds = [p for _, p in vd.batch()]
    refs = [single(ref_ctx, p, vd.LEAF, INF, vd.RADIUS, 137, False) for p in clouds]
    M = 2
    axis_t, var, axis_q = synth.random_bases(137, 30, M, 5, seed=78)
    hctx.search_setup(axis_t, var, axis_q)
    hctx.set_rank(rank)
    hctx.set_remove_overlap(overlap)
    hctx.set_batch(64)
    canvas = tuple(max(r["sb"][a] for r in refs) for a in range(3))
    box, thr = (2, 2, 2), 5
    nf = len(clouds)
    feats = [torch.from_numpy(np.ascontiguousarray(r["rows"])).to(dev) for r in refs]
    want = torch.zeros((nf, M * rank * 3), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    nm_ref = hctx.run_feature_frames(feats, [r["sb"] for r in refs], canvas, rule=1, ranges=box, exist_threshold=thr,
                                     rotate=True, d_out=want)
    hctx.synchronize()
    want = want.cpu().numpy()
    assert want.view(c3hlac.DET_DTYPE)["score"].max() > 0
    try:
        for head in HEADS:
            hctx.set_vosch_head(head)
            got = torch.full((nf, M * rank * 3), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            nm, info = hctx.run_vosch_point_frames(clouds, vd.LEAF, canvas, box, thr, dim=137, thr=THR, subdiv=vd.SUBDIV,
                                                   offset=vd.OFFSET, normals_radius=vd.RADIUS, d_out=got)
            hctx.synchronize()
            assert nm == nm_ref and np.array_equal(got.cpu().numpy(), want), head
            assert [int(s) for s in info["status"]] == [r["status"] for r in refs]
    finally:
        hctx.set_rank(1)
        hctx.set_remove_overlap(False)
