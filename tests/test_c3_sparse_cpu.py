"""The sparse batched C3-HLAC-981's host arithmetic (csrc/c3_sparse.h) without a GPU:
c3_sparse_check.cpp (its own main) built with -fsanitize=address,undefined and run: the row key's
packing and order with the "none" value last at 1, 2 and 64 frames and up to 2^31 - 1 rows a frame,
the chunk plan of groups of 0, 1, a chunk, a chunk and one, and 90,000 voxels, the inverse bin
table as a bijection onto 0 .. 980 that agrees with the closed form for every (k, c, n), the
auto-product triangle and the twelve channel pairs, and the subdivision of an acting cell at
the skip and drop edges."""
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sparse C3 check"
    exe = tmp_path_factory.mktemp("c3_sparse") / "c3_sparse_check"
    src = ROOT / "tests" / "c3_sparse_check.cpp"
    inc = ROOT / "mapping-private_amd" / "csrc"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(inc), str(src),
                        "-o", str(exe)], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    return exe


def test_c3_sparse_arithmetic_on_the_host(checker):
    p = subprocess.run([str(checker)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "c3_sparse ok"
    stats = {ln.split(":")[0]: int(ln.split()[-1]) for ln in lines[:-1]}
    assert stats["key"] >= 3 * 4 * 3 and stats["plan"] >= 90 and stats["bin"] == 981 and stats["sub"] >= 30, stats
