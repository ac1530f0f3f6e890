#!/usr/bin/env python3
"""Batched search of caller-computed feature rows (c3h_stream_feature_frames) against what a
caller of the same library could do before it, measured at the bench geometry: 256^3 grids of
bench.make_grids, S = 10 (26^3 subdivisions), C3-HLAC-117 rows extracted once on the device
with 20 columns prepended -- resident 137-dim VOSCH-shaped frames, exist by the VOSCH rule --
D = 100, box 2^3, exist threshold 100, 64 frames per step, in two settings:
  small   10 models of r = 20 at rank 1 (the flagship's models);
  multi   63 models of r = 70 at rank 63 without rotation, every frame ending with
          removeOverlap (detect_object_vosch_multi.cpp's size).

  batched  one c3h_stream_feature_frames push per step, c3h_set_remove_overlap on the device;
  loop     per frame c3h_set_features(on_device) + c3h_clean_max + c3h_search_async into the
           frame's records; at rank 63 a download of the step's records and the host
           c3h_remove_overlap per frame follow the loop.

After an allocation prime and --warmup steps of each, the two alternate --reps times in one
process, --steps steps each, timed on the host clock around a device synchronisation.
Pass: the batched step is shorter than the loop's in every alternation, by more than the
loop's own spread (max - min) across its repetitions.  No ratio is fixed in advance.

The front kernel alone (feat_front_kernel, the "c3hlac" timing slot of a feature-frames call)
is timed in a pass of its own: its time per step and the bytes of rows it reads per second.
Prints one JSON line per setting."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mapping-private_amd"), str(ROOT / "oracle")]

import bench  # noqa: E402  (the flagship's constants and grid generator)

DIM = 137
SETTINGS = {"small": (10, 20, 1, True), "multi": (63, 70, 63, False)}  # M, r, rank, rotate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=64, help="resident feature frames the steps cycle over")
    ap.add_argument("--settings", default="small,multi")
    args = ap.parse_args()
    import torch
    import c3hlac
    from c3hlac import synth
    from c3hlac._capi import i32x3, ptr

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = c3hlac.Context(0)
    ctx.set_stream(stream.cuda_stream)
    B, G = bench.BATCH, bench.GRID
    ctx.set_batch(B)
    ctx.set_pipeline(True)
    grids, _, _ = bench.make_grids(ctx, dev, args.frames, 0, synth, c3hlac, torch)
    # resident frames: the device extract's rows behind 20 columns kept on the rows with data
    feats, sb = [], None
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    for g in grids:
        ctx.set_grid(g, (G,) * 3, (0, 0, 0), bench.LEAF)
        sb, hn = ctx.extract(bench.VARIANT, bench.THR, bench.SUBDIV)
        c3 = torch.empty((hn, bench.VARIANT), dtype=torch.float32, device=dev)
        ctx._chk(ctx.lib.c3h_get_features(ctx.h, ptr(c3), 1), "get_features")
        head = torch.floor(torch.rand((hn, 20), generator=gen, device=dev) * 40)
        head = head * (c3 != 0).any(1, keepdim=True)
        feats.append(torch.cat([head, c3], 1).contiguous())
    del grids
    torch.cuda.synchronize(dev)
    H = int(feats[0].shape[0])
    subdivs = [sb] * B
    rng, thr = i32x3(bench.BOX), bench.EXIST_THR
    csb = i32x3(sb)

    for name in args.settings.split(","):
        M, r, rank, rotate = SETTINGS[name]
        ctx.search_setup(*synth.random_bases(DIM, bench.D, M, r, seed=synth.BASE_SEED))
        ctx.set_rank(rank)
        rec = M * rank * 3
        nsteps = args.warmup + args.steps
        dets = torch.zeros((nsteps * B, rec), dtype=torch.int64, device=dev)
        host = torch.zeros((B, rec), dtype=torch.int64).pin_memory()
        step_feats = [[feats[(s * B + i) % len(feats)] for i in range(B)] for s in range(nsteps)]

        def batched(steps, first=0):
            for s in range(first, first + steps):
                ctx.run_feature_frames(step_feats[s], subdivs, sb, rule=1, ranges=bench.BOX, exist_threshold=thr,
                                       rotate=rotate, d_out=dets.data_ptr() + s * B * rec * 8, stream=True)
            ctx.stream_flush()
            torch.cuda.synchronize(dev)

        def loop(steps, first=0):
            lib, h = ctx.lib, ctx.h
            for s in range(first, first + steps):
                for i, f in enumerate(step_feats[s]):
                    lib.c3h_set_features(h, C.c_void_p(f.data_ptr()), csb, DIM, None, 1, 1)
                    lib.c3h_clean_max(h)
                    rc = lib.c3h_search_async(h, rng, thr, int(rotate), C.c_void_p(dets.data_ptr() + (s * B + i) * rec * 8))
                    assert rc >= 0, rc
                if rank > 1:  # the step's records down and through the host removeOverlap
                    host.copy_(dets[s * B:(s + 1) * B], non_blocking=True)
                    torch.cuda.synchronize(dev)
                    lists = host.numpy().view(c3hlac.DET_DTYPE).reshape(B, M, rank)
                    for k in range(B):
                        c3hlac.remove_overlap(lists[k], bench.BOX)
            torch.cuda.synchronize(dev)

        def timed(fn):
            t0 = time.perf_counter()
            fn(args.steps, args.warmup)
            return (time.perf_counter() - t0) * 1e3 / args.steps

        ctx.set_remove_overlap(rank > 1)
        # allocation prime (one drained call) and warm-up of both routes
        ctx.run_feature_frames(step_feats[0], subdivs, sb, rule=1, ranges=bench.BOX, exist_threshold=thr, rotate=rotate,
                               d_out=dets)
        torch.cuda.synchronize(dev)
        passing = float((ctx.scores() >= 0).sum()) / M
        ctx.timing(c3hlac.timing_mask("pipeline"))
        ctx.kernel_times(reset=True)
        batched(args.warmup)
        through_tick = ctx.kernel_times(reset=True)["pipeline"][1]
        ctx.timing(False)
        ctx.set_rank(rank)
        loop(args.warmup)
        t_b, t_l = [], []
        for _ in range(args.reps):
            ctx.set_rank(rank)
            t_l.append(timed(loop))
            t_b.append(timed(batched))
        spread = max(t_l) - min(t_l)
        ok = all(l - b > spread for l, b in zip(t_l, t_b))
        # the front kernel alone
        ctx.timing(c3hlac.timing_mask("c3hlac"))
        ctx.kernel_times(reset=True)
        batched(args.steps, args.warmup)
        front_ms, front_frames = ctx.kernel_times(reset=True)["c3hlac"]
        ctx.timing(False)
        ctx.set_remove_overlap(False)
        nbytes = front_frames * H * DIM * 4
        print(json.dumps({
            "setting": name, "M": M, "r": r, "rank": rank, "rotate": rotate, "frames_per_step": B, "rows": H, "dim": DIM,
            "passing_positions": passing, "frames_through_tick_in_warmup": through_tick,
            "batched_ms_per_step": t_b, "loop_ms_per_step": t_l, "loop_spread_ms": spread,
            "ratio_loop_over_batched": [l / b for l, b in zip(t_l, t_b)], "pass": ok,
            "front_ms_per_step": front_ms / max(args.steps, 1), "front_frames": front_frames,
            "front_read_TB_per_s": nbytes / max(front_ms, 1e-9) * 1e-9}), flush=True)


if __name__ == "__main__":
    main()
