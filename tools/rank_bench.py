#!/usr/bin/env python3
"""Rank > 1 through the batch entry points, measured: the bench shape (256^3 frames,
C3-HLAC-117, S = 10, D = 100, 10 models x r = 20, box 2^3, exist threshold 100, 64 frames
per batch) through c3h_stream_frames at several ranks, and one points-in call
(c3h_run_point_frames, bench.py's 128^3 C3-HLAC-981 frames) at one rank.

Per rank: an allocation prime (one drained c3h_run_frames over every buffer set), --warmup
streamed steps, then --steps streamed steps between two device events on the context's
stream; a second, untimed-for-the-step pass of the same steps with the library's own events
around the replay launches gives the `replay` slot.  Prints one JSON line:
  {"lib": ..., "ranks": {"1": {"ms_per_step": ..., "replay_ms_per_step": ..., "replay_frames": ...,
   "pipeline_frames": ...}, ...}, "points": {"rank": 2, "frames": 64, "ms": [...], "status_nonzero": n}}

Select another build of the library with C3HLAC_LIB (tools/build_variant.sh), as
tools/tick_ab.sh does, to compare two builds in alternation."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mapping-private_amd"), str(ROOT / "oracle")]

import bench  # noqa: E402  (the flagship's constants and grid generator)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="1,2,4,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=24, help="resident 256^3 grids the steps cycle over")
    ap.add_argument("--points", type=int, default=64, help="frames of the points-in call (0: skip)")
    ap.add_argument("--points-rank", type=int, default=2)
    ap.add_argument("--points-reps", type=int, default=5)
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
    out = {"lib": os.environ.get("C3HLAC_LIB", "default"), "ranks": {}}
    geom = ((G,) * 3, (0, 0, 0), bench.LEAF, bench.VARIANT, bench.THR, bench.SUBDIV, bench.BOX, bench.EXIST_THR, True)

    if args.ranks:
        grids, _, _ = bench.make_grids(ctx, dev, args.frames, 0, synth, c3hlac, torch)
        ctx.search_setup(*synth.random_bases(bench.VARIANT, bench.D, bench.M, bench.R, seed=synth.BASE_SEED))
        n_total = (args.warmup + args.steps) * B
        gptr = np.array([grids[i % len(grids)].data_ptr() for i in range(n_total)], np.uint64)
        for rank in (int(r) for r in args.ranks.split(",")):
            ctx.set_rank(rank)
            rec = bench.M * rank * 3
            dets = torch.zeros((n_total, rec), dtype=torch.int64, device=dev)
            ctx.run_frames(gptr[:bench.PIPE_DEPTH * B], *geom, dets.data_ptr())  # allocation prime, drained
            res = {}
            for timed_slots in (False, True):
                ctx.run_frames(gptr[:args.warmup * B], *geom, dets.data_ptr(), stream=True)
                torch.cuda.synchronize(dev)
                if timed_slots:
                    ctx.timing(c3hlac.timing_mask("pipeline", "replay"))
                    ctx.kernel_times(reset=True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.run_frames(gptr[args.warmup * B:], *geom, dets.data_ptr() + args.warmup * B * rec * 8, stream=True)
                e1.record(stream)
                torch.cuda.synchronize(dev)
                if timed_slots:
                    kt = ctx.kernel_times(reset=True)
                    ctx.timing(False)
                    res["replay_ms_per_step"] = kt["replay"][0] / args.steps
                    res["replay_frames"] = kt["replay"][1]
                    res["pipeline_ms_per_step"] = kt["pipeline"][0] / args.steps
                    res["pipeline_frames"] = kt["pipeline"][1]
                else:
                    res["ms_per_step"] = e0.elapsed_time(e1) / args.steps
                ctx.stream_flush()
                torch.cuda.synchronize(dev)
            res["records_nonzero"] = int((dets[:, 0] != 0).sum().item())
            out["ranks"][str(rank)] = res
            del dets
        del grids

    if args.points > 0:
        nb = 8
        base = [torch.from_numpy(synth.kinect_scene(bench.N_RAYS, grid=bench.P_GRID, leaf=bench.P_LEAF,
                                                    seed=synth.BASE_SEED + 7000 + s)).to(dev) for s in range(nb)]
        frames = []
        for i in range(args.points):
            t, k = base[i % nb].clone(), i // nb
            t[:, 3] = (t[:, 3].view(torch.int32) ^ ((k * 0x2F1D37) & 0xFFFFFF)).view(torch.float32)
            t[:, 0] = (t[:, 0].double() + k * bench.P_LEAF).float()
            frames.append(t)
        ctx.search_setup(*synth.random_bases(bench.P_VARIANT, bench.D, bench.P_M, bench.R, seed=synth.BASE_SEED + 31))
        ctx.set_rank(args.points_rank)
        ctx.set_batch(ctx.point_batch(len(frames)))
        d_out = torch.zeros((len(frames), bench.P_M * args.points_rank * 3), dtype=torch.int64, device=dev)
        pa = (bench.P_LEAF, (bench.P_GRID,) * 3, bench.P_VARIANT, bench.THR, bench.SUBDIV, bench.BOX, bench.EXIST_THR, True)
        frames = ctx.prepare_point_frames(frames)
        ms, info = [], None
        for rep in range(2 + args.points_reps):  # two untimed calls size the buffers
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record(stream)
            _, info = ctx.run_point_frames(frames, *pa, d_out)
            e1.record(stream)
            torch.cuda.synchronize(dev)
            if rep >= 2:
                ms.append(e0.elapsed_time(e1))
        out["points"] = {"rank": args.points_rank, "frames": args.points, "ms": ms,
                         "status_nonzero": int((info["status"] != 0).sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
