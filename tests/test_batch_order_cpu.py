"""csrc/batch_order.h without a GPU: which frame goes into which slot of which batch, and the
batch number a draining call starts from.

batch_order_check.cpp (its own main) is built with -fsanitize=address,undefined and run as a
program.  For B in {1, 2, 3, 32}, nframes 1 .. 4 B + 1, draining and not, it asserts that every
frame appears exactly once, that only a draining call's last chunk is reordered (its last frame
in slot 0, the rest in order behind it), that the last chunk of a draining call lands on buffer
set 0, and that the header agrees slot by slot with a literal transcription of the expressions
the batch drivers carried before they shared it."""
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the batch order check"
    exe = tmp_path_factory.mktemp("batch_order") / "batch_order_check"
    src = ROOT / "tests" / "batch_order_check.cpp"
    inc = ROOT / "mapping-private_amd" / "csrc"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(inc), str(src),
                        "-o", str(exe)], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    return exe


def test_batch_order_header_on_the_host(checker):
    p = subprocess.run([str(checker)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "batch_order ok"
    # 4 batch sizes x (4 B + 1) frame counts x 2; per frame: its slot agrees with the
    # transcription, lies in range, follows the rule, and the frame is seen once
    frames = sum(n for B in (1, 2, 3, 32) for n in range(1, 4 * B + 2))
    assert int(lines[0].split()[-1]) >= 2 * 4 * frames
