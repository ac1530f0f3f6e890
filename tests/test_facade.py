"""The reference-named C++ facade (mapping-private_amd/host/c3hlac_host.h), driven by
tests/cpp/facade_demo.cpp the way detect_object*.cpp drive the reference.

CPU: the facade compiles and links against the C-ABI library; Param / PCA readers agree
with the reference's files (param.cpp:43-222, pca.cpp:119-185) and with the oracle.
GPU: getVoxelGrid -> extractC3HLACSignature981/117 -> SearchC3HLACMulti through the
facade equals the same pipeline through the Python binding and the oracle.
"""
import json
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT as REPO

import pyoracle as po
import c3hlac
from c3hlac import synth

PKG = REPO / "mapping-private_amd"
FIX = GOLDEN / "ref_fixtures"


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    if not (PKG / "lib" / "libc3hlac_host.so").exists():
        pytest.fail("libc3hlac_host.so not built (make -C mapping-private_amd)")
    exe = tmp_path_factory.mktemp("facade") / "facade_demo"
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", str(REPO / "include"), "-I", str(PKG / "host"),
           str(REPO / "tests" / "cpp" / "facade_demo.cpp"), "-L", str(PKG / "lib"), "-lc3hlac_host",
           "-lc3hlac_mi355x", "-Wl,-rpath," + str(PKG / "lib"), "-o", str(exe)]
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_facade_params_and_pca(demo):
    out = subprocess.run([str(demo), "params", str(FIX / "param_v1"), str(FIX / "models_offline_r")],
                         check=True, capture_output=True, text=True).stdout
    j = json.loads(out)
    assert j["voxel_size"] == pytest.approx(0.02, rel=1e-7)
    assert (j["dim"], j["box_scene"], j["box_model"], j["rotate_num"], j["c3_hlac_flg"]) == (100, 10, 10, 1, 1)
    assert j["missing_key"] == -1  # Param::readDim on a file without "dim:" returns -1
    assert j["thr"] == [147, 146, 148]
    axis, var, _ = po.pca_read(FIX / "models_offline_r" / "compress_axis")
    assert j["scene_dim"] == axis.shape[0] == 137
    # getAxis()(i, 0) = eigenvector 0, component i
    assert np.float32(j["scene_axis_00"]) == axis[0, 0] and np.float32(j["scene_axis_10"]) == axis[1, 0]
    assert np.float32(j["scene_var0"]) == var[0]
    assert j["model_dim"] == 100


def _lcg(seed, n):
    s = np.uint64(seed)
    out = np.empty(n, np.float32)
    for i in range(n):
        s = (s * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)
        out[i] = np.float32(int((s >> np.uint64(8)) & np.uint64(0xFFFF)) / 65536.0) - np.float32(0.5)
    return out, s


@pytest.mark.gpu
def test_facade_pipeline_matches_binding(demo, tmp_path, ctx):
    pts = synth.kinect_scene(40_000, grid=40, leaf=0.01, seed=synth.BASE_SEED + 5)
    cloud = tmp_path / "cloud.bin"
    pts.astype(np.float32).tofile(cloud)
    feat = tmp_path / "feat.bin"
    r = subprocess.run([str(demo), "run", str(cloud), str(feat)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)

    # the same pipeline through the Python binding (same context type, same kernels) and the oracle
    gi = ctx.voxelize(pts, 0.01)
    assert j["div"] == list(gi.div_b) and j["n_occ"] == gi.n_occ
    sb, hn = ctx.extract(981, (147, 146, 148), 8)
    f981 = ctx.features()
    ctx.extract(117, (147, 146, 148), 0)
    f117 = ctx.features()
    got = np.fromfile(feat, np.float32)
    assert j["hist_num"] == hn and j["subdiv"] == list(sb)
    np.testing.assert_array_equal(got[:hn * 981].reshape(hn, 981), f981)
    np.testing.assert_array_equal(got[hn * 981:], f117.reshape(-1))
    g, layout, cl = po.voxelize(pts, 0.01)
    fo, _, _ = po.c3hlac(g, layout, cl, 981, (147, 146, 148), 0.01, 8, exact=True)
    np.testing.assert_array_equal(f981, fo)

    # search: the PCA files the demo wrote, its LCG scene axis, readAxis + setSceneAxis
    D, rdim, M = 16, 4, 2
    qs = []
    for m in range(M):
        a, v, _ = c3hlac.pca_read(str(feat) + ".m%d" % m)
        qs.append(c3hlac.read_axis(a, v, D, rdim, multiple_similarity=True))
    vals, _ = _lcg(3, D * 981)
    axis = vals.reshape(D, 981)
    var = np.arange(1, D + 1, dtype=np.float32)
    ctx.search_setup(axis, var, np.stack(qs))
    ctx.set_rank(1)
    ctx.extract(981, (147, 146, 148), 8)
    det, _ = ctx.search((2, 2, 1), 10, rotate=True)
    det = det[:, 0]
    assert j["xy"] == sb[0] * sb[1] and j["z"] == sb[2]
    for m in range(M):
        s, x, y, z, mode, xr = j["dets"][m]
        assert (s, x, y, z, mode) == (det["score"][m], det["x"][m], det["y"][m], det["z"][m], det["mode"][m])
        assert xr == (2 if mode in (0, 1) else (2 if mode in (2, 3) else 1))


PCD = FIX / "pcd"


def test_facade_pcd_and_feature_io(demo, tmp_path):
    """loadPCDFile / readFeature / writeFeature through the facade (host only)."""
    out = tmp_path / "f.pcd"
    j = json.loads(subprocess.run([str(demo), "io", str(PCD / "bowl1_0000.pcd"),
                                   str(PCD / "noisy_cube_black_GRSD_CCHLAC.pcd"), str(out)],
                                  check=True, capture_output=True, text=True).stdout)
    ref = c3hlac.read_pcd(PCD / "bowl1_0000.pcd")
    assert j["n_points"] == ref.shape[0] and j["missing"] == -1
    assert np.float32(j["p0"][0]) == ref[0, 0] and j["p0"][3] == int(ref[0:1, 3].view(np.uint32)[0])
    assert (j["rows"], j["dim"]) == (1, 137)
    # the c3_hlac writer names the field "descriptor"; everything else is the reference's file
    a = out.read_text().splitlines()
    b = (PCD / "noisy_cube_black_GRSD_CCHLAC.pcd").read_text().splitlines()
    assert a[1] == "FIELDS descriptor" and b[1] == "FIELDS vfh" and a[:1] + a[2:] == b[:1] + b[2:]


@pytest.mark.gpu
def test_facade_auto_threshold(demo, ctx):
    import np_ref as npr
    j = json.loads(subprocess.run([str(demo), "thr", str(PCD / "noisy_torus_blue.pcd"), "0.005"],
                                  check=True, capture_output=True, text=True).stdout)
    ctx.voxelize(c3hlac.read_pcd(PCD / "noisy_torus_blue.pcd"), 0.005)
    h = 2 * npr.color_histogram(ctx.grid())
    t, ave = npr.auto_threshold(h)
    assert j["n_occ"] == h[0].sum() // 2 and j["h_sum"] == h[0].sum()
    assert j["thr"] == list(t) and j["ave"] == list(ave)


@pytest.mark.parametrize("dim", [981, 495])
def test_facade_rotate_feature90(demo, dim):
    import pca_oracle as pco
    for mode in range(4):
        out = subprocess.run([str(demo), "rot", str(dim), str(mode)], check=True, capture_output=True,
                             text=True).stdout
        assert json.loads(out) == pco.rotate_map(dim, mode).tolist()


@pytest.mark.gpu
def test_facade_pca_training(ctx, demo, tmp_path):
    """pca_scene + pca_models through the facade (host rows batched into the GPU
    accumulator) against the oracle: variances, subspaces and the file format."""
    import pca_oracle as pco
    rng = np.random.default_rng(11)
    n, F, D, nm = 1200, 981, 40, 60
    X = (rng.random((n, 8)) @ rng.random((8, F)) + 0.01 * rng.random((n, F))).astype(np.float32)
    rows = tmp_path / "rows.bin"
    rows.write_bytes(np.array([n, F], np.int32).tobytes() + X.tobytes())
    out = subprocess.run([str(demo), "train", str(rows), str(tmp_path), str(D), str(nm)], check=True,
                         capture_output=True, text=True).stdout
    j = json.loads(out)
    assert (j["scene_dim"], j["model_dim"]) == (F, D)
    sa, sv, sm = c3hlac.pca_read(tmp_path / "scene_pca")
    assert sm is None
    ref_s = pco.train(X)
    np.testing.assert_allclose(sv, ref_s[1].astype(np.float32), rtol=0, atol=1e-9 * ref_s[1][0])
    ma, mv, _ = c3hlac.pca_read(tmp_path / "model_pca")
    ref_m = pco.train(X[:nm], sa[:, :D], sv[:D], rotate=True, exact=True)
    np.testing.assert_allclose(mv, ref_m[1].astype(np.float32), rtol=1e-6, atol=1e-9 * ref_m[1][0])
    # leading model subspace (r = 10 as in the demos) equals the oracle's
    P1, P2 = ma[:, :10].astype(np.float64), ref_m[0][:, :10]
    assert np.abs(P1 @ P1.T - P2 @ P2.T).max() < 1e-4


@pytest.mark.gpu
def test_facade_vosch_flow(ctx, demo):
    """example_GRSD_CCHLAC.cpp through the facade: GRSD equals the binding's, VOSCH is
    [GRSD-20 | C3-117] with the C3 part equal to extractC3HLACSignature117."""
    path = FIX / "pcd" / "noisy_torus_blue.pcd"
    out = subprocess.run([str(demo), "vosch", str(path), "0.01"], check=True, capture_output=True,
                         text=True).stdout
    j = json.loads(out)
    pts = c3hlac.read_pcd(path)
    ctx.voxelize(pts, 0.01)
    ctx.compute_normals(0.02)
    ctx.extract_grsd(0)
    g = ctx.features()[0]
    assert np.array_equal(np.float32(j["grsd"]), g)
    assert j["vosch_dim"] == 137
    ctx.extract(117, (127, 127, 127), 0)
    c3 = ctx.features()[0]
    assert np.array_equal(np.float32(j["vosch_head"][:20]), g)
    assert np.array_equal(np.float32(j["vosch_head"][20:22]), c3[:2])


@pytest.mark.gpu
def test_facade_normals_with_dropped_points(ctx, demo):
    """getNormals returns a row per input point, NaN for the points getVoxelGrid's z_limit
    dropped (it used to size its buffer by the kept points while the library wrote a row
    for every input point); GRSD behind a z_limit equals the binding's."""
    path = FIX / "pcd" / "noisy_torus_blue.pcd"
    pts = c3hlac.read_pcd(path)
    zl = float(np.median(pts[:, 2]))
    out = subprocess.run([str(demo), "vosch", str(path), "0.01", repr(zl)], check=True, capture_output=True,
                         text=True).stdout
    j = json.loads(out)
    gi = ctx.voxelize(pts, 0.01, zl)
    assert 0 < gi.n_valid < len(pts)
    ctx.compute_normals(0.02)
    nrm = ctx.normals(len(pts))
    assert np.isnan(nrm[pts[:, 2] >= np.float32(zl)]).all()
    assert j["normal_rows"] == len(pts)
    assert j["normal_nan_rows"] == int(np.isnan(nrm[:, 0]).sum()) >= len(pts) - gi.n_valid
    ctx.extract_grsd(0)
    assert np.array_equal(np.float32(j["grsd"]), ctx.features()[0])


@pytest.mark.gpu
def test_facade_read_data_integral_tables(ctx, demo, tmp_path):
    """SearchObj::readData (search.cpp:169-210): binary integral tables of compressed
    features and exist counts -> search; the same lists as the binding's search on the
    per-subdivision values the tables difference to (readAxis of the same model files)."""
    rng = np.random.default_rng(5)
    X, Y, Z, D = 9, 8, 7, 16
    cells = rng.standard_normal((Z, Y, X, D))
    ex = rng.integers(0, 6, (Z, Y, X)).astype(np.int64)
    I = cells.cumsum(0).cumsum(1).cumsum(2)
    E = ex.cumsum(0).cumsum(1).cumsum(2)
    fF, fN = tmp_path / "F.bin", tmp_path / "N.bin"
    fF.write_bytes(np.array([X, Y, Z], np.int32).tobytes() + I.astype(np.float64).tobytes())
    fN.write_bytes(E.astype(np.int32).tobytes())
    out = subprocess.run([str(demo), "readdata", str(fF), str(fN), str(tmp_path), str(D)], check=True,
                         capture_output=True, text=True).stdout
    dets = json.loads(out)["dets"]
    # the facade's cells: 3-D differences (double) of the float-stored integral table
    If = I.astype(np.float32).astype(np.float64)
    P = np.pad(If, ((1, 0), (1, 0), (1, 0), (0, 0)))
    c = (P[1:, 1:, 1:] - P[1:, 1:, :-1] - P[1:, :-1, 1:] + P[1:, :-1, :-1]
         - P[:-1, 1:, 1:] + P[:-1, 1:, :-1] + P[:-1, :-1, 1:] - P[:-1, :-1, :-1]).astype(np.float32)
    qs = []
    for m in (0, 1):
        a, v, _ = c3hlac.pca_read(tmp_path / ("m%d" % m))
        qs.append(c3hlac.read_axis(a, v, D, 4))
    ctx.set_features(c.reshape(-1, D), (X, Y, Z), ex.reshape(-1).astype(np.int32))
    ctx.search_setup(None, None, np.stack(qs))
    ctx.set_rank(1)
    lists, _ = ctx.search((2, 2, 2), 5)
    for m in (0, 1):
        e = lists[m, 0]
        assert [float(e["score"]), int(e["x"]), int(e["y"]), int(e["z"]), int(e["mode"])] == dets[m]


def _write_pcd(path, pts):
    hdr = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\n"
           "TYPE F F F F\nCOUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n"
           % (len(pts), len(pts)))
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, np.float32).tobytes())


@pytest.mark.gpu
def test_facade_estimation_classes(demo, tmp_path):
    """extract_c3_hlac_scene.cpp's flow (Param -> loadPCDFile -> VoxelGrid -> features ->
    writeFeature) through C3HLAC981Estimation / C3HLAC117Estimation (c3_hlac.h:79-220) for
    PointXYZRGB and PointXYZRGBNormal: rows equal to extractC3HLACSignature981/117's,
    getSubdivNum, setVoxelFilter's false returns, the silent-empty threshold case; the
    written feature file against the oracle."""
    pts = synth.kinect_scene(200_000, grid=64, leaf=0.02, seed=synth.BASE_SEED + 77)
    pcd = tmp_path / "scene.pcd"
    _write_pcd(pcd, pts)
    r = subprocess.run([str(demo), "estim", str(FIX / "param_v1"), str(pcd), str(tmp_path / "f")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)
    assert j["filter_ok"] == 1 and j["rows"] == j["free_rows"] == 7 ** 3
    assert j["same981"] == 1 and j["subdiv"] == j["subdiv_free"] == [7, 7, 7]
    assert j["same117"] == 1 and j["rows117"] > 0 and j["wide117"] == 1 and j["narrow_throws"] == 1
    assert j["normal_down_same"] == 1 and j["normal_same981"] == 1
    assert j["offset_false"] == 1 and j["negative_subdiv_false"] == 1 and j["negative_thr_empty"] == 1
    assert j["unset_throws"] == 1 and j["name"] == "C3HLAC981Estimation"
    # ColorCHLAC_RI_Estimation == extractColorCHLACSignature117 == the oracle's ColorCHLAC table
    assert j["same_cc117"] == 1 and j["cc_name"] == "ColorCHLAC_RI_Estimation"
    cc = c3hlac.read_feature(tmp_path / "f_cc117.pcd")
    fc, _, _ = po.c3hlac(*po.voxelize(pts, 0.02), 117, (147, 146, 148), 0.02, 10, color_mode=po.COLOR_CHLAC,
                         exact=True)
    fc = fc[(fc != 0).any(1)]
    assert cc.shape == fc.shape
    np.testing.assert_allclose(cc, fc, atol=5e-7, rtol=1e-6)
    est = c3hlac.read_feature(tmp_path / "f_estim.pcd")
    free = c3hlac.read_feature(tmp_path / "f_free.pcd")
    assert np.array_equal(est, free)
    g, layout, cloud = po.voxelize(pts, 0.02)
    fe, _, _ = po.c3hlac(g, layout, cloud, 981, (147, 146, 148), 0.02, 10, exact=True)
    fe = fe[(fe != 0).any(1)]  # writeFeature drops all-zero rows (c3_hlac_tools.hpp:89-115)
    assert est.shape == fe.shape
    np.testing.assert_allclose(est, fe, atol=5e-7)  # "%f" text
