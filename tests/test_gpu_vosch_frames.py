"""Point clouds in, VOSCH / GRSD rows out for a batch (c3h_extract_vosch_frames,
c3h_run_vosch_point_frames; csrc/vosch_front.hip) against the single-frame route --
c3h_voxelize + c3h_compute_normals + c3h_extract_vosch / c3h_extract_grsd on a second context,
which test_gpu_grsd.py and test_gpu_grsd_edges.py pin to the float64 oracle.  Both run the same
front, the single-frame route as a batch of one: the comparison shows that a frame's results do
not depend on its batch, and it pins the cell-staged normals of a batch to the per-point walk
that a table of one frame takes (test_cell_staged_normals_equal_the_per_point_walk does so
without leaning on that).  Every comparison is of bytes (uint32 views), unconditional: rows,
info, per-point normals (NaNs in the same rows), per-voxel radii and types, search records.
The frames: vosch_frames_data.py (test_vosch_frames_cpu.py shows with the oracle alone that they
hold different grids and subdivision counts, several filled subdivisions, every type, voxels
whose centroid lies in another cell, frames without rows and frames without valid points)."""
import ctypes as C

import numpy as np
import pytest

import c3hlac
import vosch_frames_data as vd
from c3hlac import _capi, synth
from c3hlac._capi import ptr
from conftest import THR

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_RANGE = -1, -3, -5
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def ref_ctx():
    c = c3hlac.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def _restore(ctx):
    yield
    ctx.set_batch(32)
    ctx.set_rank(1)
    ctx.set_remove_overlap(False)


_REFS = {}


def single(rc, pts, leaf, z_limit, radius, dim, normalize, subdiv=vd.SUBDIV, offset=vd.OFFSET):
    """The single-frame route on the reference context: status, rows, info fields, normals, RSD.
    Computed once per argument set and kept unchanged."""
    key = (id(pts), leaf, z_limit, radius, dim, normalize, subdiv, offset)
    if key not in _REFS:
        _REFS[key] = single_on(rc, pts, leaf, z_limit, radius, dim, normalize, subdiv, offset)
    return _REFS[key]


def single_on(rc, pts, leaf, z_limit, radius, dim, normalize, subdiv=vd.SUBDIV, offset=vd.OFFSET):
    """The single-frame route on context rc."""
    lib, h = rc.lib, rc.h
    out = {"status": 0, "rows": np.zeros((0, dim), np.float32), "sb": (0, 0, 0)}
    gi = _capi.GridInfo()
    p = rc._grsd_params(subdiv, offset, 0.01, normalize)
    sb = (C.c_int32 * 3)()
    hn = C.c_int64()
    st = lib.c3h_voxelize(h, ptr(np.ascontiguousarray(pts)), len(pts), 0, float(leaf), float(z_limit), C.byref(gi))
    if st >= 0:
        st = lib.c3h_compute_normals(h, float(radius), None)
    if st >= 0:
        if dim == 137:
            st = lib.c3h_extract_vosch(h, C.byref(p), (C.c_int32 * 3)(*THR), 1, sb, C.byref(hn))
        else:
            st = lib.c3h_extract_grsd(h, C.byref(p), sb, C.byref(hn))
    out["status"] = min(st, 0)
    if st >= 0:
        out["div_b"], out["min_b"] = tuple(gi.div_b), tuple(gi.min_b)
        out["n_valid"], out["n_occ"], out["sb"] = int(gi.n_valid), int(gi.n_occ), tuple(sb)
        rc.hist_num, rc.variant = int(hn.value), dim
        out["rows"] = rc.features()
        out["normals"] = rc.normals(len(pts))
        out["radii"], out["types"] = rc.rsd()
    return out


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_batch(ctx, clouds, leaf, z_limit, radius, dim, normalize, row_cap, rows=None, subdiv=vd.SUBDIV,
              offset=vd.OFFSET):
    return ctx.extract_vosch_frames(clouds, leaf, dim=dim, row_cap=row_cap, thr=THR, subdiv=subdiv, offset=offset,
                                    normalize=normalize, normals_radius=radius, z_limit=z_limit, rows=rows)


def check_frames(ctx, refs, views, info, getters=True):
    for i, r in enumerate(refs):
        assert info["status"][i] == r["status"], (i, info["status"][i], r["status"])
        if r["status"] < 0:
            assert views[i] is None
            continue
        for f in ("div_b", "min_b"):
            assert tuple(info[f][i]) == r[f], (i, f)
        assert tuple(info["subdiv_b"][i]) == r["sb"] and info["n_valid"][i] == r["n_valid"] and info["n_occ"][i] == r["n_occ"], i
        got = views[i].cpu().numpy()
        assert got.shape == r["rows"].shape, (i, got.shape, r["rows"].shape)
        assert np.array_equal(u32(got), u32(r["rows"])), (i, "rows")
        if getters:
            assert np.array_equal(u32(ctx.frame_normals(i)), u32(r["normals"])), (i, "normals")
            radii, types = ctx.frame_rsd(i)
            assert np.array_equal(u32(radii), u32(r["radii"])) and np.array_equal(types, r["types"]), (i, "rsd")


def cap_of(refs):
    return max([len(r["rows"]) for r in refs] + [1])


@pytest.mark.parametrize("z_limit", vd.Z_LIMITS, ids=["plain", "z1"])
@pytest.mark.parametrize("dim,normalize", [(137, False), (137, True), (20, False), (20, True)])
def test_rows_info_and_getters(ctx, ref_ctx, dim, normalize, z_limit):
    clouds = [p for _, p in vd.batch()]
    refs = [single(ref_ctx, p, vd.LEAF, z_limit, vd.RADIUS, dim, normalize) for p in clouds]
    names = [n for n, _ in vd.batch()]
    # the frames are what the CPU module says: rows, no rows (H = 0, status 0), no valid point (STATE)
    st = dict(zip(names, refs))
    assert len(st["edge"]["rows"]) > 100 and st["noisy_plane_purple"]["status"] == 0 and len(st["noisy_plane_purple"]["rows"]) == 0
    assert st["no_point"]["status"] == ERR_STATE and st["one_point"]["status"] == 0
    ctx.set_batch(64)
    views, info = run_batch(ctx, clouds, vd.LEAF, z_limit, vd.RADIUS, dim, normalize, cap_of(refs))
    check_frames(ctx, refs, views, info)
    if z_limit == vd.Z_LIMITS[0]:
        assert info["n_moved"][names.index("edge")] == 1  # (the oracle's count: test_vosch_frames_cpu.py)


def test_fine_leaf_with_off_cell_centroids(ctx, ref_ctx):
    clouds = [p for _, p in vd.fine_batch()]
    refs = [single(ref_ctx, p, vd.FINE_LEAF, float("inf"), vd.RADIUS, 137, False) for p in clouds]
    ctx.set_batch(64)
    views, info = run_batch(ctx, clouds, vd.FINE_LEAF, float("inf"), vd.RADIUS, 137, False, cap_of(refs))
    check_frames(ctx, refs, views, info)
    assert info["n_moved"][0] == 14 and info["n_occ"][0] == 945


def test_kinect_scene_in_a_batch_of_its_own(ctx, ref_ctx):
    pts = synth.kinect_scene(150_000, grid=48, leaf=0.02, seed=77)
    refs = [single(ref_ctx, pts, 0.02, float("inf"), 0.04, 137, False)]
    assert len(refs[0]["rows"]) > 500
    ctx.set_batch(64)
    views, info = run_batch(ctx, [pts], 0.02, float("inf"), 0.04, 137, False, cap_of(refs))
    check_frames(ctx, refs, views, info)


def test_batch_sizes_order_and_row_cap(ctx, ref_ctx):
    import torch
    named = vd.batch()
    clouds = [p for _, p in named]
    refs = [single(ref_ctx, p, vd.LEAF, float("inf"), vd.RADIUS, 137, False) for p in clouds]
    cap = cap_of(refs)
    for B in (1, 3, 64):
        ctx.set_batch(B)
        views, info = run_batch(ctx, clouds, vd.LEAF, float("inf"), vd.RADIUS, 137, False, cap)
        check_frames(ctx, refs, views, info, getters=B >= len(clouds))
        if B < len(clouds):  # the getters speak of one batch only
            with pytest.raises(_capi.C3HError, match="C3H_ERR_STATE"):
                ctx.frame_normals(0)
    ctx.set_batch(64)
    for i in (1, 5):  # a batch of one frame
        views, info = run_batch(ctx, [clouds[i]], vd.LEAF, float("inf"), vd.RADIUS, 137, False, cap)
        check_frames(ctx, [refs[i]], views, info)
    order = np.random.default_rng(3).permutation(len(clouds))
    views, info = run_batch(ctx, [clouds[i] for i in order], vd.LEAF, float("inf"), vd.RADIUS, 137, False, cap)
    check_frames(ctx, [refs[i] for i in order], views, info)
    # row_cap one below the edge cloud's count: that frame alone fails, its slot keeps the sentinel
    e = [n for n, _ in named].index("edge")
    small = len(refs[e]["rows"]) - 1
    assert small >= max(len(r["rows"]) for k, r in enumerate(refs) if k != e)
    rows = torch.full((len(clouds) * small * 137,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()  # torch's fill before the context's stream writes
    views, info = run_batch(ctx, clouds, vd.LEAF, float("inf"), vd.RADIUS, 137, False, small, rows=rows)
    assert info["status"][e] == ERR_RANGE and views[e] is None
    assert (rows.view(len(clouds), small * 137)[e] == float(SENTINEL)).all()
    cut = [dict(r, status=ERR_RANGE) if k == e else r for k, r in enumerate(refs)]
    check_frames(ctx, cut, views, info, getters=False)
    for k in (e - 1, e + 1):  # its neighbours: their rows, then the sentinel
        h = len(refs[k]["rows"])
        assert (rows.view(len(clouds), small * 137)[k, h * 137:] == float(SENTINEL)).all()


def test_empty_frames_do_not_disturb_their_neighbours(ctx, ref_ctx):
    d = dict(vd.batch())
    empty = [d["no_point"], np.full((5, 4), np.nan, np.float32), d["no_point"]]
    full = [d["noisy_sphere_green"], d["edge"], d["noiseless_cone_red"]]
    clouds = [empty[0], full[0], empty[1], empty[2], full[1], full[2], empty[0]]
    refs = [single(ref_ctx, p, vd.LEAF, float("inf"), vd.RADIUS, 20, True) for p in clouds]
    assert [r["status"] for r in refs] == [ERR_STATE, 0, ERR_STATE, ERR_STATE, 0, 0, ERR_STATE]
    cap = cap_of(refs)
    ctx.set_batch(64)
    views, info = run_batch(ctx, clouds, vd.LEAF, float("inf"), vd.RADIUS, 20, True, cap)
    check_frames(ctx, refs, views, info)
    with pytest.raises(_capi.C3HError, match="C3H_ERR_STATE"):
        ctx.frame_rsd(0)
    got = [views[i].cpu().numpy().copy() for i in (1, 4, 5)]
    views2, info2 = run_batch(ctx, full, vd.LEAF, float("inf"), vd.RADIUS, 20, True, cap)
    for a, b in zip(got, views2):
        assert np.array_equal(u32(a), u32(b.cpu().numpy()))


def test_wide_leaf_takes_the_rsd_grid_of_its_own(ctx, ref_ctx):
    d = dict(vd.batch())
    clouds = [d["noisy_sphere_green"], d["noiseless_cone_red"]]
    assert 0.1 * np.sqrt(3) / 2 > 4 * vd.RADIUS
    refs = [single(ref_ctx, p, 0.1, float("inf"), vd.RADIUS, 20, False, subdiv=0, offset=(0, 0, 0)) for p in clouds]
    assert all(len(r["rows"]) == 1 and r["rows"].sum() > 0 for r in refs)
    ctx.set_batch(64)
    views, info = run_batch(ctx, clouds, 0.1, float("inf"), vd.RADIUS, 20, False, 1, subdiv=0, offset=(0, 0, 0))
    check_frames(ctx, refs, views, info)


@pytest.mark.parametrize("rank,overlap", [(1, False), (4, True)])
def test_search_records(ctx, ref_ctx, rank, overlap):
    import torch
    dev = torch.device("cuda", 0)
    clouds = [p for _, p in vd.batch()]
    refs = [single(ref_ctx, p, vd.LEAF, float("inf"), vd.RADIUS, 137, False) for p in clouds]
    M = 2
    axis_t, var, axis_q = synth.random_bases(137, 30, M, 5, seed=78)
    ctx.search_setup(axis_t, var, axis_q)
    ctx.set_rank(rank)
    ctx.set_remove_overlap(overlap)
    ctx.set_batch(64)
    canvas = tuple(max(r["sb"][a] for r in refs) for a in range(3))
    box, thr = (2, 2, 2), 5
    nf = len(clouds)
    # the reference records: run_feature_frames on the single-frame rows
    feats = [torch.from_numpy(np.ascontiguousarray(r["rows"])).to(dev) for r in refs]
    want = torch.zeros((nf, M * rank * 3), dtype=torch.int64, device=dev)
    got = torch.full((nf, M * rank * 3), -1, dtype=torch.int64, device=dev)
    want2 = torch.zeros((nf, M * rank * 3), dtype=torch.int64, device=dev)
    got2 = torch.full((nf, M * rank * 3), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # torch's uploads and fills before the context's stream reads and writes
    nm_ref = ctx.run_feature_frames(feats, [r["sb"] for r in refs], canvas, rule=1, ranges=box, exist_threshold=thr,
                                    rotate=True, d_out=want)
    ctx.synchronize()
    want = want.cpu().numpy()
    assert want.view(c3hlac.DET_DTYPE)["score"].max() > 0
    nm, info = ctx.run_vosch_point_frames(clouds, vd.LEAF, canvas, box, thr, dim=137, thr=THR, subdiv=vd.SUBDIV,
                                          offset=vd.OFFSET, normals_radius=vd.RADIUS, d_out=got)
    ctx.synchronize()
    assert nm == nm_ref and np.array_equal(got.cpu().numpy(), want)
    assert [int(s) for s in info["status"]] == [r["status"] for r in refs]
    # a canvas smaller than the edge cloud's counts: that frame keeps the setRank state and a negative status
    e = [n for n, _ in vd.batch()].index("edge")
    small = tuple(max(r["sb"][a] for k, r in enumerate(refs) if k != e) for a in range(3))
    assert any(refs[e]["sb"][a] > small[a] for a in range(3))
    sbs = [(0, 0, 0) if k == e else r["sb"] for k, r in enumerate(refs)]
    feats2 = [f if k != e else f[:0] for k, f in enumerate(feats)]
    nm_ref2 = ctx.run_feature_frames(feats2, sbs, small, rule=1, ranges=box, exist_threshold=thr, rotate=True, d_out=want2)
    nm2, info2 = ctx.run_vosch_point_frames(clouds, vd.LEAF, small, box, thr, dim=137, thr=THR, subdiv=vd.SUBDIV,
                                            offset=vd.OFFSET, normals_radius=vd.RADIUS, d_out=got2)
    ctx.synchronize()
    assert nm2 == nm_ref2 and nm2 > 0 and info2["status"][e] == ERR_RANGE
    g2 = got2.cpu().numpy()
    assert np.array_equal(g2, want2.cpu().numpy())
    rec = g2[e].view(c3hlac.DET_DTYPE)
    assert not rec["score"].any() and not rec["x"].any() and not rec["mode"].any()  # the setRank state


def test_model_size_is_checked_before_anything_runs(ctx):
    import torch
    axis_t, var, axis_q = synth.random_bases(117, 30, 2, 5, seed=79)
    ctx.search_setup(axis_t, var, axis_q)
    ctx.set_rank(1)
    ctx.set_remove_overlap(False)
    clouds = [p for _, p in vd.batch()][:2]
    got = torch.full((2, 2 * 3), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(_capi.C3HError, match="C3H_ERR_ARG"):
        ctx.run_vosch_point_frames(clouds, vd.LEAF, (4, 4, 4), (2, 2, 2), 5, dim=137, thr=THR, subdiv=vd.SUBDIV,
                                   offset=vd.OFFSET, normals_radius=vd.RADIUS, d_out=got)
    ctx.synchronize()
    assert (got.cpu().numpy() == -1).all()


def test_cell_staged_normals_equal_the_per_point_walk(ctx):
    """vosch_frames_data.dense_pin_clouds in one batch: the chosen cells hold 16 points and more
    in frame A (cell-staged kernel, one of them in two passes of 64 queries) and fewer in frame B
    (per-point walk); the fillers that make the difference are nobody's neighbour among the
    compared queries, so their normals must agree bit for bit -- a summation-order slip in
    either kernel would not."""
    a, b, queries = vd.dense_pin_clouds()
    ctx.set_batch(64)
    views, info = run_batch(ctx, [a, b], vd.LEAF, float("inf"), vd.RADIUS, 20, False, 1, subdiv=0, offset=(0, 0, 0))
    assert list(info["status"]) == [0, 0]
    vd.check_dense_pin(a, b, queries, (info["min_b"][0], info["div_b"][0]), (info["min_b"][1], info["div_b"][1]))
    na, nb = ctx.frame_normals(0), ctx.frame_normals(1)
    assert np.isfinite(nb[queries]).all()
    assert np.array_equal(u32(na[queries]), u32(nb[queries]))


def test_single_frames_and_batches_share_a_context(ctx):
    """Single-frame calls and batches use the same buffers: interleaved on one context, every
    result is the one a fresh context gives, and a single-frame c3h_compute_normals takes the
    batch getters' frames away."""
    named = vd.batch()
    clouds = [p for _, p in named]
    edge = dict(named)["edge"]
    inf = float("inf")
    narrow = (edge, vd.LEAF, inf, vd.RADIUS, 137, False)
    wide = (edge, 0.1, inf, vd.RADIUS, 20, False, 0, (0, 0, 0))  # leaf 0.1: the RSD grid of its own
    assert 0.1 * np.sqrt(3) / 2 > 4 * vd.RADIUS

    def batch_on(c):
        c.set_batch(64)
        views, info = run_batch(c, clouds, vd.LEAF, inf, vd.RADIUS, 137, False, cap)
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

    want_narrow, want_wide = fresh(single_on, *narrow), fresh(single_on, *wide)
    cap = len(want_narrow["rows"])
    want_batch, want_status = fresh(batch_on)
    with c3hlac.Context(0) as c:
        same(single_on(c, *narrow), want_narrow)
        for _ in range(2):
            got, status = batch_on(c)
            assert np.array_equal(status, want_status)
            for g, w in zip(got, want_batch):
                assert (g is None) == (w is None)
                if g is not None:
                    for k in w:
                        assert np.array_equal(u32(g[k]), u32(w[k])), k
            same(single_on(c, *wide), want_wide)
            same(single_on(c, *narrow), want_narrow)
            with pytest.raises(_capi.C3HError, match="C3H_ERR_STATE"):
                c.frame_normals(0)
