#!/usr/bin/env python3
"""Point clouds in, C3-HLAC rows out (c3h_extract_c3_frames) against the loop a caller of the same
library writes without it, per frame: c3h_voxelize -> c3h_extract -> a device copy of the rows
(c3h_get_features).  For --frames clouds, variants 981 and 117:

  A   resident synth.kinect_scene(300_000, grid=256, leaf=0.01) clouds (--scenes distinct ones,
      cycled to --frames), leaf 0.01, subdivision 10;
  B   the reference's object clouds (tests/golden/ref_fixtures/pcd, a few thousand points each),
      cycled to --frames, leaf 0.01, subdivision 0 (one row per cloud) and 10.

After a warm-up of both routes they alternate --reps times in one process, timed on the host clock
around a device synchronisation.  Pass: the batched call is shorter than the loop in every
alternation by more than the loop's own spread (max - min).  The rows of the two routes are
compared as bytes ("rows_equal").  --route loop runs the loop alone (a library without the batched
entry, e.g. the parent commit's through C3HLAC_LIB).  Informational: the time of
c3h_extract_vosch_frames at dim 1001 (variant 981) / 137 (variant 117) on the same clouds, which
adds normals, RSD and GRSD.  Prints one JSON line per setting, subdivision and variant."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mapping-private_amd"), str(ROOT / "oracle")]

import numpy as np  # noqa: E402

import bench  # noqa: E402

LEAF, RADIUS = 0.01, 0.02
SETTINGS = {"A": (10,), "B": (0, 10)}  # subdivisions per setting


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="A,B")
    ap.add_argument("--variants", default="981,117")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--scenes", type=int, default=8, help="distinct kinect scenes of setting A")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--route", default="both", choices=["both", "loop"])
    args = ap.parse_args()
    import torch
    import c3hlac
    from c3hlac import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = c3hlac.Context(0)
    ctx.set_batch(64)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for setting in args.settings.split(","):
        if setting == "A":
            base = [synth.kinect_scene(300_000, grid=256, leaf=LEAF, seed=synth.BASE_SEED + k) for k in range(args.scenes)]
        else:
            base = []
            for path in sorted((ROOT / "tests" / "golden" / "ref_fixtures" / "pcd").glob("*.pcd")):
                try:
                    b = c3hlac.read_pcd(path)
                except c3hlac.C3HError:  # not an x y z rgb cloud
                    continue
                if 500 <= len(b) <= 20000:
                    base.append(b)
        clouds = [torch.from_numpy(np.ascontiguousarray(base[i % len(base)])).to(dev) for i in range(args.frames)]
        torch.cuda.synchronize(dev)
        frames = ctx.prepare_point_frames(clouds)
        nf = len(clouds)
        for subdiv in SETTINGS[setting]:
            for variant in [int(v) for v in args.variants.split(",")]:
                hn = []
                for c in clouds:  # the frames' row counts (one single-frame pass): the loop's row buffers, row_cap
                    ctx.voxelize(c, LEAF)
                    hn.append(ctx.extract(variant, bench.THR, subdiv)[1])
                cap = max(hn + [1])
                rows = [torch.zeros((h, variant), dtype=torch.float32, device=dev) for h in hn]
                rows_b = torch.zeros(nf * cap * variant, dtype=torch.float32, device=dev)
                exist_b = torch.zeros(nf * cap, dtype=torch.int32, device=dev)
                dim = 20 + variant
                rows_v = torch.zeros(nf * cap * dim, dtype=torch.float32, device=dev)
                torch.cuda.synchronize(dev)  # torch's fills before the context's stream writes

                def loop():
                    for c, out in zip(clouds, rows):
                        ctx.voxelize(c, LEAF)
                        ctx.extract(variant, bench.THR, subdiv)
                        if out.numel():
                            ctx._chk(ctx.lib.c3h_get_features(ctx.h, c3hlac.ptr(out), 1), "get_features")  # the device copy
                    ctx.synchronize()

                def batched():
                    return ctx.extract_c3_frames(frames, LEAF, variant, bench.THR, cap, subdiv=subdiv, rows=rows_b,
                                                 exist=exist_b)  # (synchronises)

                def vosch():
                    ctx.extract_vosch_frames(frames, LEAF, dim=dim, row_cap=cap, thr=bench.THR, subdiv=subdiv,
                                             normals_radius=RADIUS, rows=rows_v)

                loop()
                out = {"setting": setting, "subdiv": subdiv, "variant": variant, "frames": nf,
                       "points_per_frame": int(np.mean([len(c) for c in clouds])), "rows_per_frame": float(np.mean(hn)),
                       "row_cap": cap}
                t_l, t_b, t_v = [], [], []
                if args.route == "both":
                    views, _, info = batched()
                    torch.cuda.synchronize(dev)
                    same = all(int(s) == 0 for s in info["status"])
                    for v, r in zip(views, rows):
                        same = same and v is not None and v.shape == r.shape and \
                            bool(torch.equal(v.contiguous().view(torch.int32), r.view(torch.int32)))
                    out["rows_equal"] = same
                    vosch()
                for _ in range(args.reps):
                    t_l.append(timed(loop))
                    if args.route == "both":
                        t_b.append(timed(batched))
                        t_v.append(timed(vosch))
                spread = max(t_l) - min(t_l)
                out.update({"loop_ms": t_l, "loop_spread_ms": spread})
                if args.route == "both":
                    out.update({"batched_ms": t_b, "ratio_loop_over_batched": [a / b for a, b in zip(t_l, t_b)],
                                "pass": all(a - b > spread for a, b in zip(t_l, t_b)),
                                "vosch_frames_dim": dim, "vosch_frames_ms": t_v})
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
