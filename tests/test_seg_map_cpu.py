"""The segment-occupancy map's arithmetic (csrc/occ_sched.h) walked on the host: the tick's
row-wave stream, the tile role and this check share the voxel -> (entry, bit) helpers, the
span of a wave's load and the ballot fold as they are.  seg_map_check.cpp builds every
frame's map over the real chunk schedule (own chunks plus pooled units) and checks that every
span is written exactly once, every occupied voxel's bit is set and no bit is set over an
empty segment."""
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the segment-map check"
    exe = tmp_path_factory.mktemp("seg_map") / "seg_map_check"
    src = ROOT / "tests" / "seg_map_check.cpp"
    inc = ROOT / "mapping-private_amd" / "csrc"
    p = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(inc), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return exe


def test_map_written_once_per_span_and_matches_the_grid(checker):
    p = subprocess.run([str(checker)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "seg_map ok"
    # 5 grids x 3 workgroup counts x (stealing off, 3 pooled settings)
    assert len(lines) - 1 == 5 * 3 * 4
    # 256 x 40 x 53 at the shipped depth, the tick's stealing planned for 8 frames: 2,120 spans
    # in a map of 34 whole chunks, the partial last chunk in the pooled tail
    part = [l for l in lines if l.startswith("256x40x53 depth 16 wgs 4 frames 8 div 16 unit 8:")]
    assert len(part) == 1 and part[0].startswith(
        "256x40x53 depth 16 wgs 4 frames 8 div 16 unit 8: spans 2120 entries 2176 pooled units 8 ")
    # gx = 512: a grid row is two spans
    two = [l for l in lines if l.startswith("512x8x7 depth 16 wgs 4 frames 1 div 0 unit 0:")]
    assert len(two) == 1 and two[0].startswith("512x8x7 depth 16 wgs 4 frames 1 div 0 unit 0: spans 112 entries 128 ")
