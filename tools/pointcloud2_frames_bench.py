#!/usr/bin/env python3
"""c3h_run_pointcloud2_frames against what a caller of the same library could do before it,
at the points-in flagship's size: --frames (512) device-resident Kinect messages, organised
640 x 480, point_step 32 with rgb at byte 16 (9.83 MB each), 10 % NaN holes besides the
scene's own, 128^3 canvas, C3-HLAC-981, bench.py's points-in search settings, the batch size
of Context.point_batch.

  A  run_pointcloud2_frames: the batched voxeliser reads the messages in place;
  B  c3h_pointcloud2_to_xyzrgb per message on the context's stream (the C entry point, its
     arguments built beforehand), then one run_point_frames on the converted arrays;
  C  run_point_frames on arrays converted beforehand: the floor, no conversion at all.

One untimed sizing call of each, then --reps alternations of A, B, C in one process, each timed
on the host clock around a device synchronisation.  Pass: A is shorter than B in every
alternation by more than B's own spread (max - min).  A over C is reported, not gated.  The
records and frame info of A and C are compared (they must be equal).  Prints one JSON line."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mapping-private_amd"), str(ROOT / "oracle")]

import bench  # noqa: E402  (the flagship's constants)

W, H, STEP = 640, 480, 32
FIELDS = {"x": 0, "y": 4, "z": 8, "rgb": 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    import c3hlac
    from c3hlac import synth
    from c3hlac._capi import ptr

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = c3hlac.Context(0)
    ctx.set_stream(stream.cuda_stream)
    n = W * H
    G, leaf = bench.P_GRID, bench.P_LEAF
    base = []
    for s in range(args.scenes):
        pts = synth.kinect_scene(n, grid=G, leaf=leaf, seed=synth.BASE_SEED + 7100 + s)[:n].copy()
        holes = np.random.default_rng(s).random(n) < 0.1
        holes[:2] = False
        pts[holes, :3] = np.nan
        base.append(torch.from_numpy(pts).to(dev))

    def message(i):
        t = base[i % len(base)].clone()
        k = i // len(base)
        t[:, 3] = (t[:, 3].view(torch.int32) ^ ((k * 0x2F1D37) & 0xFFFFFF)).view(torch.float32)
        t[:, 0] = (t[:, 0].double() + k * leaf).float()
        b = t.view(torch.uint8).reshape(n, 16)
        rec = torch.full((n, STEP), 0xAB, dtype=torch.uint8, device=dev)
        rec[:, 0:12] = b[:, 0:12]
        rec[:, 16:20] = b[:, 12:16]
        return dict(height=H, width=W, point_step=STEP, row_step=W * STEP, is_bigendian=0, fields=FIELDS,
                    data=rec.reshape(-1)), t

    msgs, arrays = zip(*[message(i) for i in range(args.frames)])
    conv = [torch.empty((n, 4), dtype=torch.float32, device=dev) for _ in range(args.frames)]
    torch.cuda.synchronize(dev)
    ctx.search_setup(*synth.random_bases(bench.P_VARIANT, bench.D, bench.P_M, bench.R, seed=synth.BASE_SEED + 31))
    ctx.set_rank(1)
    ctx.set_pipeline(True)
    ctx.set_batch(ctx.point_batch(args.frames))
    run = (leaf, (G,) * 3, bench.P_VARIANT, bench.THR, bench.SUBDIV, bench.BOX, bench.EXIST_THR, True)
    out = {k: torch.zeros((args.frames, 3 * bench.P_M), dtype=torch.int64, device=dev) for k in "ABC"}
    p_msgs = ctx.prepare_pointcloud2_frames(list(msgs))
    p_conv = ctx.prepare_point_frames(conv)
    p_arrays = ctx.prepare_point_frames(list(arrays))
    off = (C.c_int32 * 4)(0, 4, 8, 16)
    to_xyzrgb = ctx.lib.c3h_pointcloud2_to_xyzrgb
    conv_args = [(ptr(m["data"]), H, W, STEP, W * STEP, off, 0, ptr(o), C.c_void_p(stream.cuda_stream))
                 for m, o in zip(msgs, conv)]
    info = {}

    def run_a():
        _, info["A"] = ctx.run_pointcloud2_frames(p_msgs, *run, out["A"])

    def run_b():
        for a in conv_args:
            to_xyzrgb(*a)
        _, info["B"] = ctx.run_point_frames(p_conv, *run, out["B"])

    def run_c():
        _, info["C"] = ctx.run_point_frames(p_arrays, *run, out["C"])

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    for fn in (run_c, run_b, run_a):  # untimed: sizes the buffers, loads the kernels
        fn()
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(out["A"], out["C"]) and torch.equal(out["B"], out["C"]) and
                np.array_equal(info["A"], info["C"]) and np.array_equal(info["B"], info["C"]))
    t = {k: [] for k in "ABC"}
    for _ in range(args.reps):
        t["A"].append(timed(run_a))
        t["B"].append(timed(run_b))
        t["C"].append(timed(run_c))
    spread = max(t["B"]) - min(t["B"])
    ok = all(b - a > spread for a, b in zip(t["A"], t["B"]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps({
        "label": args.label, "frames": args.frames, "points_per_message": n, "message_bytes": n * STEP,
        "batch": ctx.point_batch(args.frames), "canvas": G, "variant": bench.P_VARIANT,
        "build": c3hlac._capi.build_provenance().get("lib_src_sha256"),
        "statuses_batched": int((info["A"]["status"] == 0).sum()), "detections": int((out["A"][:, 0] != 0).sum()),
        "A_equals_C_and_B": same,
        "A_ms": t["A"], "B_ms": t["B"], "C_ms": t["C"], "B_spread_ms": spread, "pass_A_shorter_than_B": ok,
        "A_frames_per_s": args.frames / med["A"] * 1e3, "B_frames_per_s": args.frames / med["B"] * 1e3,
        "C_frames_per_s": args.frames / med["C"] * 1e3,
        "A_over_C": med["A"] / med["C"], "B_over_A": med["B"] / med["A"]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
