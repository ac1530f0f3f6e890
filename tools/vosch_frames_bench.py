#!/usr/bin/env python3
"""Point clouds in, detections out (c3h_run_vosch_point_frames) against what a caller of the
same library did before it, per frame: c3h_voxelize -> c3h_compute_normals -> c3h_extract_vosch
(--dim 137) or c3h_extract_convosch (--dim 1001) -> a device copy of the rows, then one
c3h_run_feature_frames over the frames' rows.

  A  resident synth.kinect_scene(300_000, grid=256, leaf=0.01) clouds (--scenes distinct ones,
     cycled to --frames), leaf 0.01, normals 0.02, RSD 0.01, subdivision 10;
  B  the reference's small shape clouds (tests/golden/ref_fixtures/pcd, a few thousand points
     each), cycled to --frames, same parameters;
each searched by 10 models of r = 20 at rank 1 ("small") and by 63 models of r = 70 at rank 63
with removeOverlap ("multi"), D = 100, box 2^3 -- detect_object_vosch_multi.cpp's sizes.

After a warm-up of both routes they alternate --reps times in one process, timed on the host
clock around a device synchronisation.  Pass: the batched call is shorter than the loop in every
alternation by more than the loop's own spread (max - min).  --route loop runs the loop alone (a
library without the batched entry, e.g. the parent commit's through C3HLAC_LIB).
--head 0 | 1 selects the batched call's head (c3h_set_vosch_head: 0 c3h_voxelize per frame, 1 the
batched voxel head; without --head the library's default runs and the setter is not called, so a
library without it can be timed).  --head both alternates the loop, the batched call at head 0 and
the batched call at head 1 in the one process, compares the records of all three and adds
"head_pass": head 1 is shorter than head 0 in every alternation by more than head 0's own spread.  A stage pass
drains the device after each of the loop's calls (voxelize | normals with their grid | RSD + GRSD |
C3 + rows: the granularity of the single-frame entry points, on the host clock); the kernels of
either route are split further by running this tool under rocprofv3 --kernel-trace --stats.
Prints one JSON line per setting and search; "row_buffer_bytes" is what the tool itself allocates
for the loop's rows (the batched call's rows are the context's: frames x canvas rows x dim floats,
"context_row_bytes")."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mapping-private_amd"), str(ROOT / "oracle")]

import numpy as np  # noqa: E402

import bench  # noqa: E402

LEAF, RADIUS, SUBDIV = 0.01, 0.02, 10
SEARCHES = {"small": (10, 20, 1), "multi": (63, 70, 63)}  # M, r, rank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setting", default="A", choices=["A", "B"])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--scenes", type=int, default=8, help="distinct kinect scenes of setting A")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--searches", default="small,multi")
    ap.add_argument("--route", default="both", choices=["both", "loop"])
    ap.add_argument("--head", default=None, choices=["0", "1", "both"], help="the batched call's head (c3h_set_vosch_head)")
    ap.add_argument("--dim", type=int, default=137, choices=[137, 1001], help="137 VOSCH | 1001 ConVOSCH")
    args = ap.parse_args()
    DIM = args.dim
    import torch
    import c3hlac
    from c3hlac import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = c3hlac.Context(0)
    ctx.set_batch(64)
    ctx.set_pipeline(True)
    extract_rows = ctx.extract_vosch if DIM == 137 else ctx.extract_convosch
    if args.setting == "A":
        base = [synth.kinect_scene(300_000, grid=256, leaf=LEAF, seed=synth.BASE_SEED + k) for k in range(args.scenes)]
    else:
        pcd = ROOT / "tests" / "golden" / "ref_fixtures" / "pcd"
        base = []
        for path in sorted(pcd.glob("*.pcd")):  # the x y z rgb clouds among them
            try:
                b = c3hlac.read_pcd(path)
            except c3hlac.C3HError:
                continue
            if 500 <= len(b) <= 20000:
                base.append(b)
    clouds = [torch.from_numpy(np.ascontiguousarray(base[i % len(base)])).to(dev) for i in range(args.frames)]
    torch.cuda.synchronize(dev)
    frames = ctx.prepare_point_frames(clouds)
    nf = len(clouds)

    # the frames' subdivision counts (one single-frame pass): the canvas and the loop's row buffers
    sbs = []
    for c in clouds:
        ctx.voxelize(c, LEAF)
        ctx.compute_normals(RADIUS)
        sbs.append(extract_rows(bench.THR, SUBDIV)[0])
    canvas = tuple(max(s[a] for s in sbs) for a in range(3))
    rows = [torch.zeros((s[0] * s[1] * s[2], DIM), dtype=torch.float32, device=dev) for s in sbs]
    torch.cuda.synchronize(dev)

    def stage_pass():
        tot = np.zeros(4)
        for c in clouds:  # every stage drained before the next starts
            t = [time.perf_counter()]
            for call in (lambda: ctx.voxelize(c, LEAF), lambda: ctx.compute_normals(RADIUS),
                         lambda: ctx.extract_grsd(SUBDIV), lambda: extract_rows(bench.THR, SUBDIV)):
                call()
                ctx.synchronize()
                t.append(time.perf_counter())
            tot += np.diff(t) * 1e3
        return {"voxelize_ms": tot[0], "normals_with_grid_ms": tot[1], "rsd_grsd_ms": tot[2],
                "c3_and_rows_ms": max(tot[3] - tot[2], 0.0), "frames": nf}

    stages = stage_pass()

    for name in args.searches.split(","):
        M, r, rank = SEARCHES[name]
        ctx.search_setup(*synth.random_bases(DIM, bench.D, M, r, seed=synth.BASE_SEED))
        ctx.set_rank(rank)
        ctx.set_remove_overlap(rank > 1)
        rec = M * rank * 3
        d_loop = torch.zeros((nf, rec), dtype=torch.int64, device=dev)
        d_batch = torch.zeros((nf, rec), dtype=torch.int64, device=dev)
        thr = 20
        torch.cuda.synchronize(dev)  # torch's fills before the context's stream writes

        def loop():
            for c, out in zip(clouds, rows):
                ctx.voxelize(c, LEAF)
                ctx.compute_normals(RADIUS)
                extract_rows(bench.THR, SUBDIV)
                ctx._chk(ctx.lib.c3h_get_features(ctx.h, c3hlac.ptr(out), 1), "get_features")  # the device copy
            ctx.run_feature_frames(rows, sbs, canvas, rule=1, ranges=bench.BOX, exist_threshold=thr, rotate=False,
                                   d_out=d_loop)
            ctx.synchronize()

        def batched(head=None, out=None):
            if head is not None:
                ctx.set_vosch_head(head)
            ctx.run_vosch_point_frames(frames, LEAF, canvas, bench.BOX, thr, dim=DIM, thr=bench.THR, subdiv=SUBDIV,
                                       normals_radius=RADIUS, rotate=False, d_out=d_batch if out is None else out)
            ctx.synchronize()

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        loop()
        t_l, t_b, t_h = [], [], {0: [], 1: []}
        heads = (0, 1) if args.head == "both" else ()
        one_head = int(args.head) if args.head in ("0", "1") else None
        if args.route == "both":
            batched(one_head)
            torch.cuda.synchronize(dev)
            same = bool(torch.equal(d_loop, d_batch))
            for h in heads:  # the warm-up of either head, and its records against the loop's
                d_head = torch.zeros((nf, rec), dtype=torch.int64, device=dev)
                torch.cuda.synchronize(dev)
                batched(h, d_head)
                torch.cuda.synchronize(dev)
                same = same and bool(torch.equal(d_loop, d_head))
        for _ in range(args.reps):
            t_l.append(timed(loop))
            if args.route == "both" and not heads:
                t_b.append(timed(lambda: batched(one_head)))
            for h in heads:
                t_h[h].append(timed(lambda: batched(h)))
        if heads:
            t_b = t_h[1]
        spread = max(t_l) - min(t_l)
        out = {"setting": args.setting, "search": name, "dim": DIM, "M": M, "r": r, "rank": rank, "frames": nf,
               "points_per_frame": int(np.mean([len(c) for c in clouds])), "canvas_b": canvas,
               "rows_per_frame": int(np.mean([len(x) for x in rows])),
               "row_buffer_bytes": int(sum(x.numel() * 4 for x in rows)),
               "context_row_bytes": int(nf * canvas[0] * canvas[1] * canvas[2] * DIM * 4), "loop_ms": t_l, "loop_spread_ms": spread,
               "loop_stage_ms_total": stages}
        if heads:
            spread0 = max(t_h[0]) - min(t_h[0])
            out.update({"head": "both", "batched_head0_ms": t_h[0], "batched_head1_ms": t_h[1], "head0_spread_ms": spread0,
                        "head_pass": all(a - b > spread0 for a, b in zip(t_h[0], t_h[1]))})
        elif one_head is not None:
            out["head"] = one_head
        if args.route == "both":
            out.update({"batched_ms": t_b, "records_equal": same,
                        "ratio_loop_over_batched": [a / b for a, b in zip(t_l, t_b)],
                        "pass": all(a - b > spread for a, b in zip(t_l, t_b))})
        print(json.dumps(out), flush=True)
        ctx.set_remove_overlap(False)


if __name__ == "__main__":
    main()
