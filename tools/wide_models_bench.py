#!/usr/bin/env python3
"""The reference's multi-model caller at its own size on the batch path, measured: the bench
geometry (256^3 frames, C3-HLAC-117, S = 10, D = 100, box 2^3, exist threshold 100, 64 frames
per step) with detect_object_vosch_multi's 63 models of r = 70 (synth.random_bases) through
c3h_stream_frames,
  (a) at rank 1;
  (b) at rank 63 without rotation, every frame ending with removeOverlap: on the device
      (c3h_set_remove_overlap) where the library has it, else on the host after a download
      of the step's records (c3h_remove_overlap per frame), as a caller had to do before.

Per configuration: an allocation prime (one drained c3h_run_frames), --warmup steps, then
--steps steps timed on the host clock around a device synchronisation (the host's share --
the download and the host removeOverlap -- is part of (b)).  Prints one JSON line:
  {"lib": ..., "device_overlap": bool, "passing": positions of one frame that pass the gate,
   "rank1": {"ms_per_step": ..., "pipeline_frames": ...},
   "rank63": {"ms_per_step": ..., "ms_per_step_raw": (no removeOverlap), "pipeline_frames": ...}}

Select another build of the library with C3HLAC_LIB (tools/build_variant.sh, or an older
build's libc3hlac_mi355x.so), as tools/rank_bench.py does, to compare two builds in alternation."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mapping-private_amd"), str(ROOT / "oracle")]

import bench  # noqa: E402  (the flagship's constants and grid generator)

M, R, RANK = 63, 70, 63


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=24, help="resident 256^3 grids the steps cycle over")
    ap.add_argument("--skip-rank63", action="store_true")
    args = ap.parse_args()
    import torch
    import c3hlac
    from c3hlac import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = c3hlac.Context(0)
    ctx.set_stream(stream.cuda_stream)
    B, G = bench.BATCH, bench.GRID
    ctx.set_batch(B)
    ctx.set_pipeline(True)
    device_overlap = hasattr(ctx.lib, "c3h_set_remove_overlap")
    out = {"lib": os.environ.get("C3HLAC_LIB", "default"), "device_overlap": device_overlap}
    grids, _, _ = bench.make_grids(ctx, dev, args.frames, 0, synth, c3hlac, torch)
    ctx.search_setup(*synth.random_bases(bench.VARIANT, bench.D, M, R, seed=synth.BASE_SEED))
    n_total = (args.warmup + args.steps) * B
    gptr = np.array([grids[i % len(grids)].data_ptr() for i in range(n_total)], np.uint64)

    def run(rank, rotate, overlap):
        """overlap: None (raw records), "device" or "host".  -> (ms per step, frames through the tick)"""
        geom = ((G,) * 3, (0, 0, 0), bench.LEAF, bench.VARIANT, bench.THR, bench.SUBDIV, bench.BOX, bench.EXIST_THR,
                rotate)
        ctx.set_rank(rank)
        if device_overlap:
            ctx.set_remove_overlap(overlap == "device")
        rec = M * rank * 3
        dets = torch.zeros((n_total, rec), dtype=torch.int64, device=dev)
        host = torch.zeros((B, rec), dtype=torch.int64).pin_memory() if overlap == "host" else None
        ctx.run_frames(gptr[:bench.PIPE_DEPTH * B], *geom, dets.data_ptr())  # allocation prime, drained
        torch.cuda.synchronize(dev)
        if "passing" not in out:  # the context holds the prime's last frame
            out["passing"] = float((ctx.scores() >= 0).sum()) / M
        ctx.timing(c3hlac.timing_mask("pipeline"))
        ctx.kernel_times(reset=True)
        t0 = 0.0
        for step in range(args.warmup + args.steps):
            if step == args.warmup:
                ctx.stream_flush()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
            a = step * B
            ctx.run_frames(gptr[a:a + B], *geom, dets.data_ptr() + a * rec * 8, stream=True)
            if host is not None:  # the step's records: complete after a flush, down and through the host function
                ctx.stream_flush()
                host.copy_(dets[a:a + B], non_blocking=True)
                torch.cuda.synchronize(dev)
                lists = host.numpy().view(c3hlac.DET_DTYPE).reshape(B, M, rank)
                for f in range(B):
                    c3hlac.remove_overlap(lists[f], bench.BOX)
        ctx.stream_flush()
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        kt = ctx.kernel_times(reset=True)
        ctx.timing(False)
        if device_overlap:
            ctx.set_remove_overlap(False)
        return ms, kt["pipeline"][1]

    ms, nf = run(1, True, None)
    out["rank1"] = {"ms_per_step": ms, "pipeline_frames": nf}
    if not args.skip_rank63:
        raw, nf = run(RANK, False, None)
        ms, _ = run(RANK, False, "device" if device_overlap else "host")
        out["rank63"] = {"ms_per_step": ms, "ms_per_step_raw": raw, "pipeline_frames": nf}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
