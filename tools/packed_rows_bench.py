#!/usr/bin/env python3
"""Point clouds in, PCA::addData out: the routes from --frames clouds to a trained correlation
(PCA(False), no compression), variants 981 and 117:

  recipe   today's: c3h_extract_c3_frames into dense slots, per frame rows[exist > 0] in torch and
           c3h_pca_add_data (a host synchronisation, a gather and an add per frame);
  packed   c3h_extract_c3_frames_packed into a tensor sized by a count query made beforehand, one
           c3h_pca_add_data;
  clouds   c3h_pca_add_c3_frames.

  A   resident synth.kinect_scene(300_000, grid=256, leaf=0.01) clouds (--scenes distinct ones,
      cycled to --frames), leaf 0.01, subdivision 10;
  B   the reference's object clouds (tests/golden/ref_fixtures/pcd), cycled to --frames, leaf 0.01,
      subdivision 10.

After a warm-up of every route they alternate --reps times in one process, timed on the host clock
around a device synchronisation (every route ends with the PCA's stream idle).  Also timed: the dense
c3h_extract_c3_frames alone ("dense_ms").  Reported: the bytes of the row buffers per route, and
whether the correlations of the routes agree within 1e-12 of the largest entry (the bound of
test_gpu_pca_from_clouds.py).  Pass: packed and clouds are shorter than recipe in every alternation
by more than recipe's own spread (max - min).  --route recipe runs the recipe and the dense call alone
(a library without the packed entries, e.g. the parent commit's through C3HLAC_LIB, in a process of
its own).  Prints one JSON line per setting and variant."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mapping-private_amd"), str(ROOT / "oracle")]

import numpy as np  # noqa: E402

import bench  # noqa: E402

LEAF, SUBDIV = 0.01, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="A,B")
    ap.add_argument("--variants", default="981,117")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--scenes", type=int, default=8, help="distinct kinect scenes of setting A")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--route", default="all", choices=["all", "recipe"])
    args = ap.parse_args()
    import torch
    import c3hlac
    from c3hlac import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = c3hlac.Context(0)
    ctx.set_batch(64)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def correlation(pca):
        pca.solve()
        return pca.correlation()

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
        for variant in [int(v) for v in args.variants.split(",")]:
            hn = []
            for c in clouds:  # the frames' row counts (one single-frame pass): row_cap of the dense slots
                ctx.voxelize(c, LEAF)
                hn.append(ctx.extract(variant, bench.THR, SUBDIV)[1])
            cap = max(hn + [1])
            rows_d = torch.zeros(nf * cap * variant, dtype=torch.float32, device=dev)
            exist_d = torch.zeros(nf * cap, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)  # torch's fills before the context's stream writes
            pcas = {}

            def dense():
                return ctx.extract_c3_frames(frames, LEAF, variant, bench.THR, cap, subdiv=SUBDIV, rows=rows_d, exist=exist_d)

            def recipe():
                pca = pcas["recipe"] = c3hlac.PCA(False)
                views, eviews, _ = dense()
                for v, e in zip(views, eviews):
                    if v is not None and v.shape[0]:
                        keep = v[e > 0]
                        torch.cuda.current_stream(dev).synchronize()  # the gather, before the PCA's stream reads it
                        if keep.shape[0]:
                            pca.add_data(keep)

            out = {"setting": setting, "subdiv": SUBDIV, "variant": variant, "frames": nf,
                   "points_per_frame": int(np.mean([len(c) for c in clouds])), "rows_per_frame": float(np.mean(hn)),
                   "row_cap": cap, "dense_bytes": nf * cap * variant * 4}
            routes = {"recipe": recipe}
            if args.route == "all":
                n = int(ctx.extract_c3_frames_packed(frames, LEAF, variant, bench.THR, subdiv=SUBDIV, cap=0)[4][-1])
                rows_p = torch.zeros(max(n, 1) * variant, dtype=torch.float32, device=dev)
                ids_p = torch.zeros(max(n, 1) * 4, dtype=torch.int32, device=dev)
                torch.cuda.synchronize(dev)
                out.update({"packed_rows": n, "packed_bytes": n * variant * 4, "clouds_bytes": n * variant * 4})

                def packed():
                    pca = pcas["packed"] = c3hlac.PCA(False)
                    pca.add_data(ctx.extract_c3_frames_packed(frames, LEAF, variant, bench.THR, subdiv=SUBDIV, cap=n, rows=rows_p,
                                                              ids=ids_p)[0])

                def from_clouds():
                    pca = pcas["clouds"] = c3hlac.PCA(False)
                    pca.add_c3_frames(ctx, frames, LEAF, variant, bench.THR, subdiv=SUBDIV)

                routes.update({"packed": packed, "clouds": from_clouds})
            for fn in routes.values():  # warm-up
                fn()
            torch.cuda.synchronize(dev)
            if args.route == "all":
                C = {k: correlation(p) for k, p in pcas.items()}
                scale = np.abs(C["recipe"]).max()
                out["nsample"] = {k: int(p.nsample) for k, p in pcas.items()}
                out["correlation_diff"] = {k: float(np.abs(C[k] - C["recipe"]).max() / scale) for k in ("packed", "clouds")}
                out["correlations_agree"] = all(d <= 1e-12 for d in out["correlation_diff"].values())
            for p in pcas.values():
                p.close()
            t = {k: [] for k in routes}
            t_dense = []
            for _ in range(args.reps):
                for k, fn in routes.items():
                    t[k].append(timed(fn))
                    pcas[k].close()
                t_dense.append(timed(dense))
            spread = max(t["recipe"]) - min(t["recipe"])
            out.update({k + "_ms": v for k, v in t.items()})
            out.update({"recipe_spread_ms": spread, "dense_ms": t_dense, "dense_spread_ms": max(t_dense) - min(t_dense)})
            if args.route == "all":
                out["pass"] = all(r - x > spread for k in ("packed", "clouds") for r, x in zip(t["recipe"], t[k]))
            print(json.dumps(out), flush=True)
            del rows_d, exist_d


if __name__ == "__main__":
    main()
