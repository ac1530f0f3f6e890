"""Normals / RSD / GRSD / VOSCH (csrc/vosch_front.hip and its host code in csrc/capi_vosch.hip) on
tests/grsd_clouds.py: what the reference's clean shape clouds of test_gpu_grsd.py never
reach.  The reference is oracle/grsd_oracle.py (float64); tests/test_grsd_oracle_cpu.py
establishes on the oracle alone what the cloud contains and that the masks used here are
small.

- non-finite rows, isolated points, a pair (NaN normals), exactly three neighbours, a
  collinear triple (degenerate covariance), duplicates, a viewpoint off the origin;
- RSD radii of 0.5 (reach 1), 1.3 (reach 2) and 4.3 (rebuilt grid) normal radii, voxels
  with fewer than two points in range, NaN normals among the RSD neighbours;
- transition counts bit-exact from the device's own types, never under a condition;
- z_limit: normals and GRSD of the kept points are those of limitPoint-then-compute;
- a context that has held a wider search grid and larger buffers;
- VOSCH with offset and normalize, the silent-empty returns, and a cloud of more than
  8192 x 256 points (the second pass of the grid-stride loops).

Every exclusion mask comes from the reference alone and is asserted to be under its cap
(0.5 % of the normals for the eigengap, 1 % of the voxels for the thresholds) before use."""
import numpy as np
import pytest

import feature_frames_data as ffd
import grsd_clouds as gc
import grsd_oracle as go
import pyoracle as po
import vosch_frames_data as vd
from conftest import THR

pytestmark = pytest.mark.gpu
RADIUS = 0.02
VP = gc.SPHERE_C
SUB = dict(subdiv=3, offset=(1, 0, 2))
INF = float("inf")


@pytest.fixture(scope="module")
def edge():
    pts, ix = gc.edge_cloud(with_index=True)
    return dict(pts=pts, ix=ix, fin=np.isfinite(pts[:, :3]).all(1))


def _gap_ok(pts):
    """Rows whose normal is determined (relative eigengap >= 1e-3), from the reference."""
    gap, _ = gc.eigengap(pts, RADIUS)
    excluded = gap < 1e-3
    assert excluded.sum() <= 0.005 * np.isfinite(gap).sum()
    return np.isfinite(gap) & ~excluded


def _run(ctx, pts, leaf, z_limit=INF, vp=VP, vosch=False, **kw):
    """One voxelize / normals / GRSD pass; everything the device returns."""
    gi = ctx.voxelize(pts, leaf, z_limit)
    ctx.compute_normals(RADIUS, vp)
    nrm = ctx.normals(len(pts))
    sb, H = ctx.extract_vosch(THR, **kw) if vosch else ctx.extract_grsd(**kw)
    radii, types = ctx.rsd()
    return dict(div=list(gi.div_b), nrm=nrm, sb=sb, H=H, radii=radii, types=types, feat=ctx.features(),
                exist=ctx.exist())


def _check_grsd(out, pts, kept, leaf, z_limit=INF, subdiv=0, offset=(0, 0, 0), normalize=False):
    """Radii, types and counts of a _run against the oracle on the kept points and the
    device normals."""
    g, layout, cloud = po.voxelize(pts, leaf, z_limit)
    sub, dn = pts[kept], out["nrm"][kept].astype(np.float64)
    _, sb_ref, radii_ref, types_ref = go.grsd(sub, dn, g, layout, cloud, leaf, subdiv=subdiv, offset=offset)
    assert list(out["sb"]) == list(sb_ref) and len(out["types"]) == len(cloud)
    np.testing.assert_allclose(out["radii"], radii_ref, rtol=1e-5, atol=1e-7)
    near = gc.near_threshold(radii_ref)
    assert near.sum() <= 0.01 * len(cloud)
    mism = int((out["types"] != types_ref).sum())
    print("leaf", leaf, "z_limit", z_limit, "voxels", len(cloud), "near a threshold", int(near.sum()),
          "type mismatches", mism, "types", np.bincount(out["types"], minlength=5).tolist())
    assert np.array_equal(out["types"][~near], types_ref[~near])
    # fewer than two points in range: radii (0, 0), the oracle's voxels
    assert np.array_equal((out["radii"] == 0).all(1), (radii_ref == 0).all(1))
    # the counts, from the device's own types: bit-exact
    feat_ref = go.grsd(sub, dn, g, layout, cloud, leaf, subdiv=subdiv, offset=offset, types=out["types"])[0]
    assert out["H"] == len(feat_ref) and feat_ref.sum() > 0
    scale = np.float32(20.0 / 26) if normalize else np.float32(1)
    np.testing.assert_array_equal(out["feat"][:, :20], (feat_ref * scale).astype(np.float32))
    return types_ref


def test_normals_edge_cases(ctx, edge):
    pts, ix, fin = edge["pts"], edge["ix"], edge["fin"]
    ctx.voxelize(pts, 0.01)
    ctx.compute_normals(RADIUS, VP)
    nrm = ctx.normals(len(pts)).astype(np.float64)
    ref = go.normals(pts, RADIUS, VP)
    nan = np.isnan(nrm).any(1)
    assert np.array_equal(nan, np.isnan(ref[:, 0]))
    assert sorted(np.flatnonzero(nan)) == sorted(np.concatenate([ix["nonfinite"], ix["singles"], ix["pair"]]))
    assert np.isnan(nrm[nan]).all()
    ok = _gap_ok(pts)
    assert ok[ix["corner"]].all() and ok[ix["dup"]].all() and not ok[ix["line"]].any()
    np.testing.assert_allclose(nrm[ok, :3], ref[ok, :3], atol=1e-5)  # signs included
    np.testing.assert_allclose(nrm[ok, 3], ref[ok, 3], atol=1e-5)
    # the collinear triple: any unit vector across the line, no curvature
    ln = nrm[ix["line"]]
    assert np.isfinite(ln).all()
    assert np.abs(np.linalg.norm(ln[:, :3], axis=1) - 1).max() < 1e-6
    assert np.abs(ln[:, :3] @ gc.LINE_DIR).max() < 1e-5
    assert np.abs(ln[:, 3]).max() < 1e-6
    # the default viewpoint (the origin): other signs on the sphere, the oracle's
    ctx.compute_normals(RADIUS)
    n0 = ctx.normals(len(pts)).astype(np.float64)
    ref0 = go.normals(pts, RADIUS)
    sp = ix["sphere"]
    assert ((n0[sp, :3] * nrm[sp, :3]).sum(1) < 0).sum() >= len(sp) // 4
    assert np.array_equal(np.isnan(n0).any(1), nan)
    np.testing.assert_allclose(n0[ok], ref0[ok], atol=1e-5)


@pytest.mark.parametrize("leaf,reach,kw", [(0.01, 1, SUB), (0.01, 1, dict(subdiv=0)), (0.03, 2, SUB)])
def test_rsd_grsd_edge_cloud(ctx, edge, leaf, reach, kw):
    # cells of the search grid that vf_rsd_kernel visits around a centroid, per side
    max_dist = np.float32(max(0.01, leaf / 2 * np.sqrt(3)))
    assert int(np.ceil(max_dist * (np.float32(1) / np.float32(RADIUS)))) == reach and max_dist <= 4 * RADIUS
    out = _run(ctx, edge["pts"], leaf, **kw)
    types_ref = _check_grsd(out, edge["pts"], edge["fin"], leaf, **kw)
    assert (np.bincount(types_ref, minlength=5) > 0).all()  # every class takes part
    assert (out["radii"] == 0).all(1).sum() == 3  # the three isolated points' voxels


@pytest.mark.parametrize("leaf", [0.01, 0.03])
def test_z_limit_drops_points_before_normals(ctx, edge, leaf):
    """limitPoint comes first in the reference: a point at z >= z_limit is nobody's
    neighbour and has no normal.  Measured on the library before NbrGrid carried z_limit
    (the search grid held every finite point inside its one-cell margin): 699 of the 700
    dropped finite points had a normal (the 700th is isolated), and 236 of the 3015 kept
    normals differed from the oracle's by more than 1e-4 (max 0.078), at both leaves."""
    pts, fin = edge["pts"], edge["fin"]
    kept = fin & (pts[:, 2] < 1.0)
    assert kept.sum() == 3015 and (fin & ~kept).sum() == 700
    out = _run(ctx, pts, leaf, 1.0, **SUB)
    nrm = out["nrm"].astype(np.float64)
    ref = go.normals(pts[kept], RADIUS, VP)
    ok = _gap_ok(pts[kept])
    err = np.abs(nrm[kept][ok] - ref[ok]).max(1)
    print("z_limit normals: dropped rows with a normal:", int(np.isfinite(nrm[~kept]).all(1).sum()),
          "kept rows off by > 1e-4:", int((err > 1e-4).sum()), "max", np.nanmax(err))
    assert np.isnan(nrm[~kept]).all()
    assert np.array_equal(np.isnan(nrm[kept]).any(1), np.isnan(ref[:, 0]))
    np.testing.assert_allclose(nrm[kept][ok], ref[ok], atol=1e-5)
    _check_grsd(out, pts, kept, leaf, 1.0, **SUB)


def test_context_reuse_after_wider_grid(ctx, edge):
    """The same call before and after one that rebuilt the search grid at 4.3 normal radii
    (leaf 0.1: fewer, wider cells, other ranges) gives the same bits: no stale cell range,
    grid or buffer length survives into it."""
    pts, fin = edge["pts"], edge["fin"]
    first = _run(ctx, pts, 0.01, 1.0, **SUB)
    wide = _run(ctx, pts, 0.1, **SUB)
    assert np.float32(0.1 / 2 * np.sqrt(3)) > 4 * RADIUS  # extract_grsd builds a grid of its own
    _check_grsd(wide, pts, fin, 0.1, **SUB)
    again = _run(ctx, pts, 0.01, 1.0, **SUB)
    for k in first:
        np.testing.assert_array_equal(again[k], first[k], err_msg=k)
    _check_grsd(again, pts, fin & (pts[:, 2] < 1.0), 0.01, 1.0, **SUB)


def test_vosch_offset_normalize(ctx, edge):
    pts = edge["pts"]
    kw = dict(normalize=True, **SUB)
    grsd = _run(ctx, pts, 0.01, **kw)
    _check_grsd(grsd, pts, edge["fin"], 0.01, **kw)
    sb, H = ctx.extract(117, THR, SUB["subdiv"], SUB["offset"])
    c3, ex = ctx.features().copy(), ctx.exist().copy()
    assert sb == grsd["sb"] and H == grsd["H"] and (ex > 0).any() and (ex == 0).any()
    v = _run(ctx, pts, 0.01, vosch=True, **kw)
    assert v["sb"] == sb and v["H"] == H and v["feat"].shape == (H, 137)
    np.testing.assert_array_equal(v["feat"][:, :20], grsd["feat"])
    np.testing.assert_array_equal(v["feat"][:, 20:][ex > 0], c3[ex > 0])
    assert (v["feat"][:, 20:][ex == 0] == 0).all()
    np.testing.assert_array_equal(v["exist"], ffd.vosch_exist(v["feat"]))
    np.testing.assert_array_equal(v["exist"], ex)
    np.testing.assert_array_equal(grsd["exist"], ffd.grsd_exist(grsd["feat"]))


def test_silent_empty_returns(ctx, edge):
    """extractGRSDSignature21 returns no histogram for a negative subdivision size
    (grsd_colorCHLAC_tools.hpp:159-162) and for an offset beyond the grid (:150-153)."""
    pts = edge["pts"]
    gi = ctx.voxelize(pts, 0.03)
    ctx.compute_normals(RADIUS, VP)
    div = list(gi.div_b)
    for kw in (dict(subdiv=-1), dict(subdiv=3, offset=(div[0], 0, 0)), dict(subdiv=3, offset=(0, 0, div[2]))):
        sb, H = ctx.extract_grsd(**kw)
        assert H == 0 and sb == (0, 0, 0), kw
        assert ctx.features().shape == (0, 20)
    # the last offset inside the grid: one layer of subdivisions
    sb, H = ctx.extract_grsd(3, offset=(0, 0, div[2] - 1))
    assert sb[2] == 1 and H == sb[0] * sb[1]
    out = _run(ctx, pts, 0.03, **SUB)  # and a valid extract after the empty ones
    _check_grsd(out, pts, edge["fin"], 0.03, **SUB)


def test_normals_second_grid_stride_pass(ctx):
    """2^21 + 1000 points: the kernels that serve c3h_compute_normals (vf_keys_kernel,
    vf_ranges_kernel and vf_normals_frame_kernel, the per-point walk of a one-frame table) run
    8192 x 256 threads, so the last 1000 rows, and the last 1000 positions of the sort by
    cell, are reached only by a thread's second iteration.  Cells sort by z, then y, then
    x, about 46 points each here: those positions are the upper z layer (z >= 1) of the last
    row of cells (y in [1.48, 1.5)) at the largest x, and ten samples are taken there."""
    n = 2 ** 21 + 1000
    pts = gc.big_plane(n)
    rng = np.random.default_rng(3)
    top = np.flatnonzero((pts[:, 2] >= 1.0) & (pts[:, 1] >= 1.485))
    top = top[np.argsort(pts[top, 0])[-10:]]
    assert pts[top, 0].min() > 1.45  # within the last three of that row's 150 cells
    rows = np.concatenate([rng.choice(2 ** 21, 40, replace=False), top,
                           [2 ** 21, n - 1], 2 ** 21 + 1 + rng.choice(998, 48, replace=False)])
    assert len(rows) == 100 and (rows >= 2 ** 21).sum() == 50
    gi = ctx.voxelize(pts, 0.02)
    pos = _sorted_positions(pts, gi, 0.02)
    assert (pos[top] >= 2 ** 21).all()  # the ten samples: second-pass positions of the sort by cell
    ctx.compute_normals(RADIUS)
    nrm = ctx.normals(n).astype(np.float64)
    ref = go.normals(pts, RADIUS, rows=rows)
    assert np.isfinite(ref).all()
    np.testing.assert_allclose(nrm[rows], ref, atol=1e-5)
    # every row of the second pass: a unit normal of the plane z = 1, towards the origin
    last = nrm[2 ** 21:]
    assert np.isfinite(last).all()
    assert np.abs(np.linalg.norm(last[:, :3], axis=1) - 1).max() < 1e-6
    assert (last[:, 2] < -0.9).all()


def _sorted_positions(pts, gi, leaf):
    """Every row's position in the stable sort by search cell (float32 formulas of the library)."""
    cells, _ = vd.search_cells(pts, gi.min_b[:3], gi.div_b[:3], leaf, RADIUS)
    assert (cells >= 0).all()
    pos = np.empty(len(pts), np.int64)
    pos[np.argsort(cells, kind="stable")] = np.arange(len(pts))
    return pos


def test_batch_normals_second_grid_stride_pass(ctx):
    """gc.big_cells ahead of a small cloud in one batch: every grid-stride loop of the batch's
    normals reaches a second iteration.  More than 65536 cells of 16 points and more:
    vf_normals_kernel's 65536 one-wave workgroups take a second cell each.  Sorted positions from
    2^21 on in cells of fewer than 16 points: vf_keys_kernel, vf_ranges_kernel and
    vf_normals_sparse_kernel (8192 x 256 threads) serve them in a second pass.  Both are asserted
    here first.  Sampled rows against the float64 oracle, the second-pass rows unit normals, and every row bit for bit the per-point walk's that c3h_compute_normals runs."""
    pts = gc.big_cells()
    n = len(pts)
    small = gc.edge_cloud()
    ctx.set_batch(64)
    try:
        _, info = ctx.extract_vosch_frames([pts, small], 0.02, dim=20, row_cap=1, normals_radius=RADIUS)
        assert list(info["status"]) == [0, 0]
        nrm = ctx.frame_normals(0)
    finally:
        ctx.set_batch(32)
    cells, dim = vd.search_cells(pts, info["min_b"][0], info["div_b"][0], 0.02, RADIUS)
    assert (cells >= 0).all()
    per_cell = np.bincount(cells, minlength=int(dim.prod()))
    assert (per_cell >= vd.DENSE_MIN).sum() > 65536
    order = np.argsort(cells, kind="stable")
    tail = order[2 ** 21:]  # the rows at sorted positions >= 2^21
    assert len(tail) >= 1000 and (per_cell[cells[tail]] < vd.DENSE_MIN).all()
    dense_rows = np.flatnonzero(per_cell[cells] >= vd.DENSE_MIN)
    rng = np.random.default_rng(4)
    rows = np.concatenate([rng.choice(dense_rows, 50, replace=False), rng.choice(tail, 50, replace=False)])
    ref = go.normals(pts, RADIUS, rows=rows)
    ok = np.isfinite(ref[:, 0])
    assert ok[:50].all() and ok[50:].sum() >= 40 and np.array_equal(np.isfinite(nrm[rows, 0]), ok)
    np.testing.assert_allclose(nrm[rows][ok].astype(np.float64), ref[ok], atol=1e-5)
    # every row of the second pass: NaN with fewer than three points in range (float32 distances, as
    # the library compares them; the strip is thin), else a unit normal, the plane's towards the origin where a dozen points fix it
    near = pts[pts[:, 1] > 5.37, :3]
    d = pts[tail, None, :3] - near[None, :, :]
    cnt = (((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < np.float32(RADIUS) * np.float32(RADIUS)).sum(1)
    last = nrm[tail].astype(np.float64)
    assert np.array_equal(np.isfinite(last).all(1), cnt >= 3) and (cnt >= 3).sum() >= 1000
    assert np.isnan(last[cnt < 3]).all()
    assert np.abs(np.linalg.norm(last[cnt >= 3, :3], axis=1) - 1).max() < 1e-6
    assert (last[cnt >= 12, 2] < -0.9).sum() >= 0.99 * (cnt >= 12).sum() > 500  # (few points: any direction)
    ctx.voxelize(pts, 0.02)
    ctx.compute_normals(RADIUS)
    assert np.array_equal(nrm.view(np.uint32), ctx.normals(n).view(np.uint32))
