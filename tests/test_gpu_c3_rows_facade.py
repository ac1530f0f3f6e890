"""The facade's batch form of extractC3HLACSignature981 / 117 (host/c3hlac_host.h, on
c3h_extract_c3_frames): tests/cpp/c3_rows_demo.cpp runs the single-cloud function per cloud and the
batch function over all clouds of three reference shape clouds, for both variants, and compares
rows and subdivision counts as bytes."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import vosch_frames_data as vd
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_facade_batch_rows_equal_single(tmp_path):
    pkg = ROOT / "mapping-private_amd"
    assert shutil.which("g++") and (pkg / "lib" / "libc3hlac_host.so").exists()
    exe = tmp_path / "c3_rows_demo"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-I", str(pkg / "host"),
                    str(ROOT / "tests" / "cpp" / "c3_rows_demo.cpp"), "-L", str(pkg / "lib"), "-lc3hlac_host",
                    "-lc3hlac_mi355x", "-Wl,-rpath," + str(pkg / "lib"), "-o", str(exe)], check=True, capture_output=True,
                   text=True)
    d = dict(vd.batch())
    files = []
    for i, k in enumerate(("noisy_sphere_green", "noiseless_cone_red", "bowl1_0000")):
        files.append(tmp_path / ("cloud%d.bin" % i))
        np.ascontiguousarray(d[k]).tofile(files[-1])
    for subdiv in (vd.SUBDIV, 0):
        r = subprocess.run([str(exe), repr(vd.LEAF), str(subdiv)] + [str(f) for f in files], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        j = json.loads(r.stdout)
        for variant in ("981", "117"):
            assert j[variant]["differ"] == 0, (subdiv, variant, j)
            assert len(j[variant]["rows"]) == 3 and min(j[variant]["rows"]) >= 1, (subdiv, variant, j)
            assert j[variant]["nonzero"] >= 3, (subdiv, variant, j)
