"""The facade's PCA::addClouds (host/c3hlac_host.h, on c3h_pca_add_c3_frames): tests/cpp/packed_rows_demo.cpp
trains one PCA from the batch extract's rows added one by one on the host (every row with a non-zero
value, what writeFeature keeps) and one with addClouds over the same three reference shape clouds,
variant 117 plain and variant 981 with the 24 rotations.  The same rows are added on both routes,
and the variances agree within 1e-6 of the largest: both accumulate exact products in f64 (the sums
agree to about 1e-15; the variances are returned as f32, 6e-8, and dsyevd's own error on a matrix
of this norm is of that order too)."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import vosch_frames_data as vd
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_add_clouds_equals_rows_added_one_by_one(tmp_path):
    pkg = ROOT / "mapping-private_amd"
    assert shutil.which("g++") and (pkg / "lib" / "libc3hlac_host.so").exists()
    exe = tmp_path / "packed_rows_demo"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-I", str(pkg / "host"),
                    str(ROOT / "tests" / "cpp" / "packed_rows_demo.cpp"), "-L", str(pkg / "lib"), "-lc3hlac_host",
                    "-lc3hlac_mi355x", "-Wl,-rpath," + str(pkg / "lib"), "-o", str(exe)], check=True, capture_output=True,
                   text=True)
    d = dict(vd.batch())
    files = []
    for i, k in enumerate(("noisy_sphere_green", "noiseless_cone_red", "bowl1_0000")):
        files.append(tmp_path / ("cloud%d.bin" % i))
        np.ascontiguousarray(d[k]).tofile(files[-1])
    r = subprocess.run([str(exe), repr(vd.LEAF), str(vd.SUBDIV)] + [str(f) for f in files], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)
    for variant in ("117", "981"):
        v = j[variant]
        assert v["kept"] == v["added"] and v["added"] >= 3, (variant, j)
        assert v["dim"] == [int(variant)] * 2, (variant, j)
        assert 0 <= v["variance_diff"] <= 1e-6, (variant, j)
