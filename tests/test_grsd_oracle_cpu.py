"""The conditions that tests/test_gpu_grsd_edges.py relies on, established on the CPU
oracle alone (oracle/grsd_oracle.py on tests/grsd_clouds.py): what edge_cloud contains,
that its exclusion masks are small, that the oracle's new arguments change nothing, and
that the z_limit case cannot pass vacuously."""
import numpy as np
import pytest

import grsd_clouds as gc
import grsd_oracle as go
import pyoracle as po

RADIUS = 0.02
SUB = dict(subdiv=3, offset=(1, 0, 2))


@pytest.fixture(scope="module")
def edge():
    pts, ix = gc.edge_cloud(with_index=True)
    fin = np.isfinite(pts[:, :3]).all(1)
    nrm = go.normals(pts, RADIUS, gc.SPHERE_C)
    gap, cnt = gc.eigengap(pts, RADIUS)
    return dict(pts=pts, ix=ix, fin=fin, nrm=nrm, gap=gap, cnt=cnt)


@pytest.fixture(scope="module")
def rsd_cases(edge):
    """(z_limit, leaf) -> (kept points, their normals, grid, layout, centroids, grsd result)."""
    out = {}
    for zl in (np.inf, 1.0):
        kept = edge["fin"] & (edge["pts"][:, 2] < zl)
        sub = edge["pts"][kept]
        nk = go.normals(sub, RADIUS, gc.SPHERE_C)
        for leaf in (0.01, 0.03):
            g, layout, cloud = po.voxelize(edge["pts"], leaf, zl)
            out[zl, leaf] = (sub, nk, g, layout, cloud, go.grsd(sub, nk, g, layout, cloud, leaf, **SUB))
    return out


def test_edge_cloud_contents(edge):
    pts, ix, fin, nrm, cnt = edge["pts"], edge["ix"], edge["fin"], edge["nrm"], edge["cnt"]
    assert pts.shape == (3718, 4) and pts.dtype == np.float32
    assert ix["nonfinite"].tolist() == [100, 2000, 2001] and int(fin.sum()) == 3715
    # NaN normals: the non-finite rows, the three singles and the pair; nothing else
    nan = np.isnan(nrm[:, 0])
    assert sorted(np.flatnonzero(nan)) == sorted(np.concatenate([ix["nonfinite"], ix["singles"], ix["pair"]]))
    assert cnt[ix["singles"]].tolist() == [1, 1, 1] and cnt[ix["pair"]].tolist() == [2, 2]
    assert cnt[ix["line"]].tolist() == [3, 3, 3] and cnt[ix["corner"]].tolist() == [3, 3, 3]
    assert (cnt[fin].min(), cnt[fin].max()) == (1, 85)
    # the duplicates sit on their originals: equal neighbourhoods, equal normals
    assert np.array_equal(pts[ix["dup"], :3], pts[ix["plane"][:4], :3])
    assert np.array_equal(nrm[ix["dup"]], nrm[ix["plane"][:4]])
    # the right-angle triple spans z = const: normal +-z, towards the sphere centre (above it)
    np.testing.assert_allclose(nrm[ix["corner"]], [[0, 0, 1, 0]] * 3, atol=1e-12)
    # stragglers: every group at least 0.05 from all other points
    xyz = pts[fin, :3].astype(np.float64)
    rows = np.flatnonzero(fin)
    for name in ("singles", "pair", "line", "corner"):
        for k, i in enumerate(ix[name]):
            own = ix[name] if name != "singles" else ix[name][k:k + 1]
            d = np.linalg.norm(xyz - pts[i, :3].astype(np.float64), axis=1)
            assert d[~np.isin(rows, own)].min() >= 0.05, (name, k)


def test_eigengap_mask_is_the_collinear_triple(edge):
    gap, ix = edge["gap"], edge["ix"]
    small = np.flatnonzero(gap < 1e-3)
    assert small.tolist() == ix["line"].tolist()
    assert np.sort(gap[np.isfinite(gap)])[3] > 0.1  # the next gap is two orders wider
    assert len(small) <= 0.005 * np.isfinite(edge["nrm"][:, 0]).sum()
    # the triple's own properties, on the oracle: a unit vector across the line, no curvature
    n = edge["nrm"][ix["line"]]
    np.testing.assert_allclose(np.linalg.norm(n[:, :3], axis=1), 1, atol=1e-12)
    assert np.abs(n[:, :3] @ gc.LINE_DIR).max() < 1e-5 and np.abs(n[:, 3]).max() < 1e-6


def test_viewpoint_changes_signs_on_the_sphere(edge):
    n0 = go.normals(edge["pts"], RADIUS)
    sp = edge["ix"]["sphere"]
    flipped = (edge["nrm"][sp, :3] * n0[sp, :3]).sum(1) < 0
    assert flipped.sum() == 654  # of 1400: far above the quarter the GPU test asks for
    np.testing.assert_allclose(np.abs(edge["nrm"][sp, :3]), np.abs(n0[sp, :3]), atol=1e-12)


@pytest.mark.parametrize("zl,leaf,nvox,types,zero", [
    (np.inf, 0.01, 923, [3, 335, 6, 527, 52], 3),
    (np.inf, 0.03, 134, [3, 52, 15, 49, 15], 3),
    (1.0, 0.01, 753, [2, 167, 5, 526, 53], 2),
    (1.0, 0.03, 113, [2, 32, 15, 49, 15], 2),
])
def test_types_zero_radii_and_thresholds(rsd_cases, zl, leaf, nvox, types, zero):
    sub, nk, g, layout, cloud, (feat, sb, radii, ty) = rsd_cases[zl, leaf]
    assert len(cloud) == nvox
    assert np.bincount(ty, minlength=5).tolist() == types and min(types) > 0  # all five classes
    # fewer than two points in range of the centroid: radii (0, 0), NOISE.  These are the
    # isolated points' voxels (one of the singles is beyond z = 1)
    z = (radii == 0).all(1)
    assert z.sum() == zero and (ty[z] == go.NOISE).all()
    near = gc.near_threshold(radii)
    assert near.sum() <= 0.01 * nvox
    assert feat.shape == (sb[0] * sb[1] * sb[2], 20) and feat.sum() > 0
    # given its own types, grsd() counts the same transitions
    f2, sb2, r2, t2 = go.grsd(sub, nk, g, layout, cloud, leaf, types=ty, **SUB)
    assert np.array_equal(f2, feat) and sb2 == sb and r2 is None and np.array_equal(t2, ty)
    # and other types give other counts (the argument is used)
    f3 = go.grsd(sub, nk, g, layout, cloud, leaf, types=(ty + 1) % 5, **SUB)[0]
    assert not np.array_equal(f3, feat)


def test_z_limit_keeps_3015_points(edge):
    assert int((edge["fin"] & (edge["pts"][:, 2] < 1.0)).sum()) == 3015


def test_grsd_types_whole_cloud(rsd_cases):
    sub, nk, g, layout, cloud, (_, _, _, ty) = rsd_cases[np.inf, 0.01]
    f, sb, radii, _ = go.grsd(sub, nk, g, layout, cloud, 0.01)
    f2 = go.grsd(sub, nk, g, layout, cloud, 0.01, types=ty)[0]
    assert sb == [1, 1, 1] and np.array_equal(f, f2)
    # every voxel sees 26 neighbours; only transitions (i, j >= i) are kept
    assert 0 < f.sum() <= 26 * len(cloud)


def test_normals_rows_equal_the_full_call(edge):
    rows = [0, 99, 100, 101, 1999, 2000, 2002, 3703, 3706, 3709, 3712, 3717, 5, 5]
    got = go.normals(edge["pts"], RADIUS, gc.SPHERE_C, rows=rows)
    assert got.shape == (len(rows), 4)
    np.testing.assert_array_equal(got, edge["nrm"][rows])
    assert np.isnan(got[2]).all() and np.isfinite(got[0]).all()


def test_dropped_neighbours_change_kept_normals(edge):
    """z_limit = 1.0 cuts the tilted plane in two.  Normals of the kept points computed
    with the dropped ones as neighbours (a search grid over all input points) differ from
    limitPoint-then-normals: the z_limit GPU test can tell the two apart."""
    kept = edge["fin"] & (edge["pts"][:, 2] < 1.0)
    nk = go.normals(edge["pts"][kept], RADIUS, gc.SPHERE_C)
    assert np.array_equal(np.isnan(nk[:, 0]), np.isnan(edge["nrm"][kept, 0]))
    changed = np.nanmax(np.abs(nk[:, :3] - edge["nrm"][kept, :3]), axis=1) > 1e-4
    assert changed.sum() == 236
    assert changed.sum() >= 100


def test_big_plane_shape():
    pts = gc.big_plane(5000)
    assert pts.shape == (5000, 4) and np.isfinite(pts[:, :3]).all()
    assert np.abs(pts[:, :2]).max() <= 1.5 and abs(pts[:, 2].std() - 0.001) < 1e-4
