"""bench.py's plain run and --dump-outputs: the options, the files written for a batch of
detection records, and (GPU) one small plain run from the command line: the result line
holds the headline keys and none of the --full passes, and the dumped arrays are the last
step's detections."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]
import bench  # noqa: E402

FULL_ONLY = ("kernel_ms_avg", "voxelize_mpoints_per_s", "detections_per_s_search_kernels", "points_in",
             "points_in_real_views", "single_frame", "cpu_baseline", "scored_detections_per_s")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_write_outputs_splits_records_into_float64_arrays(tmp_path):
    import c3hlac
    det = np.zeros((3, 5), c3hlac.DET_DTYPE)
    rng = np.random.default_rng(7)
    det["score"] = rng.random((3, 5))
    for k in ("x", "y", "z", "mode"):
        det[k] = rng.integers(-1, 1 << 20, (3, 5))
    words = det.view(np.int64).reshape(3, 5, 3)
    out = tmp_path / "a" / "b"  # created with its parents
    bench.write_outputs(out, words)
    assert sorted(p.name for p in out.iterdir()) == ["positions.npy", "scores.npy"]
    sc, pos = np.load(out / "scores.npy"), np.load(out / "positions.npy")
    assert sc.dtype == np.float64 and pos.dtype == np.float64
    assert np.array_equal(sc, det["score"])
    assert np.array_equal(pos, np.stack([det[k] for k in ("x", "y", "z", "mode")], -1))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_last_step(ctx, tmp_path):
    B, K, W = 8, 3, 4
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
           "--batch", str(B), "--frames", "8", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res
    assert res["steps"] == K and res["warmup"] == W and res["roofline"]["launches"] == K
    assert res["ms_per_step"] > 0 and res["value"] > 0
    assert not [k for k in FULL_ONLY if k in res]
    sc, pos = np.load(tmp_path / "out" / "scores.npy"), np.load(tmp_path / "out" / "positions.npy")
    assert sc.shape == (B, bench.M * bench.RANK) and pos.shape == (B, bench.M * bench.RANK, 4)
    assert sc.dtype == np.float64 and pos.dtype == np.float64
    assert np.all(sc > 0)
    n = res["config"]["positions"] ** (1 / 3)
    assert np.all((pos[..., :3] >= 0) & (pos[..., :3] < round(n))) and np.all(pos[..., 3] >= 0)
    # frames i and i + 8 of the stream read the same resident grid: with 8 grids and a batch of
    # 8, the last step's first record is scene 0's, as the one-frame API finds it
    import c3hlac
    from c3hlac import synth
    axis_t, var, axis_q = synth.random_bases(bench.VARIANT, bench.D, bench.M, bench.R, seed=synth.BASE_SEED)
    with c3hlac.Context(0) as c:
        c.search_setup(axis_t, var, axis_q)
        c.set_rank(bench.RANK)
        c.voxelize(bench.scene_points(synth, 0, 0), bench.LEAF)
        c.extract(bench.VARIANT, bench.THR, bench.SUBDIV)
        lists, _ = c.search(bench.BOX, bench.EXIST_THR)
    # (both search in fp32: equal best scores within its rounding; the position of a tie may differ)
    assert np.allclose(sc[0], lists[:, 0]["score"], rtol=1e-5, atol=0)
