#!/usr/bin/env python3
"""Adaptive sampling on the headline frame (cornell_plane_light 1024^2, depth 8): uniform 256 spp against drt_render_adaptive with
min 16, step 16, max 256 at rel_error 0.05, 0.02 and 0.01. One JSON line per run: wall time, paths traced, Mpaths/s over the traced
paths, rounds, pixels at max. Each run on a fresh context, after one warm-up render of its own shape.
    python3 tools/adaptive_probe.py [--size 1024] [--only 0.02]
    python3 tools/adaptive_probe.py --refine   (rel_error 0.05, then drt_render_adaptive_continue on the same film to 0.02; again to 0.01:
                                                 one line per leg, to set beside the fresh render at the tighter bound)
    python3 tools/adaptive_probe.py --kernel-stats <rocprofv3 *_kernel_stats.csv>   (the convergence kernels' share of kernel time)"""
import argparse
import csv
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))


def kernel_share(path):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    conv = sum(float(r["TotalDurationNs"]) for r in rows if "drt_converge" in r["Name"])
    return {"kernel_ms": round(total / 1e6, 3), "converge_ms": round(conv / 1e6, 3), "converge_share": round(conv / total, 5) if total else None,
            "converge_kernels": {r["Name"].split("(")[0]: round(float(r["TotalDurationNs"]) / 1e6, 3) for r in rows if "drt_converge" in r["Name"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--max-spp", type=int, default=256)
    ap.add_argument("--only", type=float, default=None, help="one adaptive run at this rel_error, no uniform run and no warm-up (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--refine", action="store_true", help="0.05 and then the continuation to 0.02, and to 0.01, each pair on a fresh context")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_share(a.kernel_stats)))
        return
    import pydrt
    W = a.size
    bundle = pydrt.load_scene(os.path.join(REPO, "scenes", "cornell_plane_light.scn"), W, W)
    params = pydrt.make_params(W, W, spp=a.max_spp, max_depth=a.depth, seed=1)
    if a.refine:
        for tight in (0.02, 0.01):
            r = pydrt.Renderer(bundle, params)
            try:
                r.render(0, 16)
                r.synchronize()
                r.reset_film()
                legs = []
                for leg, rel in (("first", 0.05), ("continuation", tight)):
                    t0 = time.perf_counter()
                    rep = r.render_adaptive(16, a.max_spp, 16, rel) if leg == "first" else r.render_adaptive_continue(a.max_spp, 16, rel)
                    legs.append((leg, rel, (time.perf_counter() - t0) * 1e3, rep))
                st = r.stats()
            finally:
                r.close()
            for leg, rel, wall, rep in legs:
                print(json.dumps({"mode": "refine " + leg, "rel_error": rel, "wall_ms": round(wall, 2), "paths": int(rep["paths"]),
                                  "mpaths_per_s": round(rep["paths"] / wall / 1e3, 1), "rounds": rep["rounds"],
                                  "pixels_at_max": rep["pixels_at_max"], "stats_paths": int(st.paths)}), flush=True)
        return
    runs = [None] + [0.05, 0.02, 0.01] if a.only is None else [a.only]
    for rel in runs:
        r = pydrt.Renderer(bundle, params)
        try:
            if a.only is None:  # warm-up: code objects loaded, pool touched (not under --only: its kernels would count in a trace)
                r.render(0, 16)
                r.synchronize()
                r.reset_film()
            t0 = time.perf_counter()
            if rel is None:
                r.render(0, a.max_spp)
                r.synchronize()
                rep = {"rounds": 1, "pixels_at_max": W * W, "paths": a.max_spp * W * W}
            else:
                rep = r.render_adaptive(16, a.max_spp, 16, rel)
            wall = (time.perf_counter() - t0) * 1e3
            st = r.stats()
        finally:
            r.close()
        print(json.dumps({"mode": "uniform" if rel is None else "adaptive", "rel_error": rel, "wall_ms": round(wall, 2),
                          "paths": int(rep["paths"]), "paths_frac": round(rep["paths"] / (a.max_spp * W * W), 4),
                          "mpaths_per_s": round(rep["paths"] / wall / 1e3, 1), "rounds": rep["rounds"],
                          "pixels_at_max": rep["pixels_at_max"], "kernel_ms": round(st.total_ms, 2), "stats_paths": int(st.paths)}),
              flush=True)


if __name__ == "__main__":
    main()
