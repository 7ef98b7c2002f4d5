#!/usr/bin/env python3
"""What sample maps cost (drt_render_sample_map), beside the dense path rendering the same samples.

    python3 tools/sample_map_probe.py [--size 1024] [--depth 8] [--reps 3] [--out FILE]
    python3 tools/sample_map_probe.py --only map255            (one configuration in this process: what rocprofv3 is given)
    python3 tools/sample_map_probe.py --kernel-stats <rocprofv3 *_kernel_stats.csv>   (the map's own kernels, per call and per round)

One process per configuration and run: the parent opens no device and starts the configurations one after the other, --reps rounds over
all of them, so the runs of two configurations alternate. A child creates its context (DRT_BATCH_RESIDENT), does its work once to warm
up (code objects, the pool measurement, the map's buffers), resets the film and does it once more, timed: the wall time of the call
(for drt_render: to the end of drt_synchronize) and the trace + shade times of its kernel pairs by HIP events (drt_stats).

The configurations, on cornell_plane_light.scn at --size^2:
    dense256, map256    drt_render(0, 256) against a uniform map of 256 (one round)
    dense256g           drt_render(0, 256) with DRT_NO_CLOSED_SHADE=1: the dense launch with the shade instantiation a list launch takes
    dense255, map255    drt_render(0, 255) against a uniform map of 255 (eight rounds)
    region              a map of 16 everywhere and 256 inside the centred region of a quarter of the width and height (two rounds: 16 samples
                        of the pixels outside, 256 of the pixels inside)
    dense16, tile256    its yardstick: the 16-spp frame, and a fresh context over the region's tile rendering 256 (created inside the timing)
Prints its lines and one JSON line (also written to --out)."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))

CONFIGS = ["dense256", "dense256g", "map256", "dense255", "map255", "region", "dense16", "tile256"]
MAP_KERNELS = ("drt_map_adopt_kernel", "drt_map_select_kernel", "drt_converge_scan", "drt_converge_scatter")


def kernel_stats(path):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    mine = {k: [0.0, 0] for k in MAP_KERNELS}
    for r in rows:
        for k in MAP_KERNELS:
            if k in r["Name"]:
                mine[k][0] += float(r["TotalDurationNs"])
                mine[k][1] += int(r["Calls"])
    return {"kernel_ms": round(total / 1e6, 3), "map_kernels_ms": round(sum(v[0] for v in mine.values()) / 1e6, 4),
            "per_kernel": {k: {"calls": v[1], "total_us": round(v[0] / 1e3, 2), "mean_us": round(v[0] / 1e3 / v[1], 2) if v[1] else None}
                           for k, v in mine.items()}}


def child(a):
    import numpy as np
    import pydrt
    W, name = a.size, a.only
    if name == "dense256g":
        os.environ["DRT_NO_CLOSED_SHADE"] = "1"  # read when the context is created
    bundle = pydrt.load_scene(os.path.join(REPO, "scenes", "cornell_plane_light.scn"), W, W)
    q = W // 4
    x0 = y0 = (W - q) // 2
    if name == "tile256":
        params = pydrt.make_params(W, W, spp=256, max_depth=a.depth, seed=1, x0=x0, y0=y0, tile_w=q, tile_h=q, batch_spp=pydrt.BATCH_RESIDENT)
    else:
        params = pydrt.make_params(W, W, spp=256, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    target = None
    if name.startswith("map"):
        target = np.full((W, W), int(name[3:]), dtype=np.uint32)
    elif name == "region":
        target = pydrt.region_map(W, W, 16, [(x0, y0, q, q, 256)])

    def work(r):
        if target is not None:
            return r.render_sample_map(target)
        r.render(0, 256 if name == "tile256" else int(name[5:8]))
        r.synchronize()
        return None

    r = pydrt.Renderer(bundle, params)
    try:
        work(r)
        r.reset_film()
        if name == "tile256":  # a caller without sample maps makes this context for the region: its creation is part of the price
            r.close()
            t0 = time.perf_counter()
            r = pydrt.Renderer(bundle, params)
            created = (time.perf_counter() - t0) * 1e3
        else:
            created = 0.0
            t0 = time.perf_counter()
        rep = work(r)
        wall = (time.perf_counter() - t0) * 1e3
        st = r.stats()
        paths = int(target.sum(dtype=np.uint64)) if target is not None else int(r.n_pixels) * (256 if name == "tile256" else int(name[5:8]))
        assert st.paths == paths and st.redone_launches == 0
        print(json.dumps({"config": name, "wall_ms": wall, "create_ms": created, "trace_ms": st.trace_ms, "shade_ms": st.shade_ms,
                          "kernel_ms": st.trace_ms + st.shade_ms, "launches": st.launches, "paths": paths, "rounds": rep["rounds"] if rep else 0}))
    finally:
        r.close()


def run_child(a, name):
    cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--size", str(a.size), "--depth", str(a.depth)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("sample_map_probe: configuration %s failed (%d)" % (name, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=[""] + CONFIGS)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_stats(a.kernel_stats)))
        return
    if a.only:
        return child(a)
    runs = {c: [] for c in CONFIGS}
    for rep in range(a.reps):
        for c in CONFIGS:
            runs[c].append(run_child(a, c))
            x = runs[c][-1]
            print("rep %d %-9s wall %8.2f ms  trace + shade %8.2f ms  %3d launches  %d rounds" % (rep, c, x["wall_ms"], x["kernel_ms"], x["launches"], x["rounds"]),
                  flush=True)
    keys = ("wall_ms", "kernel_ms", "trace_ms", "shade_ms", "create_ms")
    med = {c: {k: statistics.median(x[k] for x in runs[c]) for k in keys} for c in CONFIGS}
    out = {"size": a.size, "depth": a.depth, "reps": a.reps,
           "runs": [{"config": c, **med[c], "wall_min_max_ms": [min(x["wall_ms"] for x in runs[c]), max(x["wall_ms"] for x in runs[c])],
                     "kernel_min_max_ms": [min(x["kernel_ms"] for x in runs[c]), max(x["kernel_ms"] for x in runs[c])],
                     "launches": runs[c][0]["launches"], "rounds": runs[c][0]["rounds"], "paths": runs[c][0]["paths"]} for c in CONFIGS]}
    for m, d in (("map256", "dense256"), ("map255", "dense255"), ("dense256g", "dense256")):
        out[m + "_over_" + d] = {"wall": med[m]["wall_ms"] / med[d]["wall_ms"], "kernel": med[m]["kernel_ms"] / med[d]["kernel_ms"]}
        print("%s / %s: wall %.3f, trace + shade %.3f" % (m, d, out[m + "_over_" + d]["wall"], out[m + "_over_" + d]["kernel"]))
    yard = {k: med["dense16"][k] + med["tile256"][k] for k in ("wall_ms", "kernel_ms")}
    out["region_yardstick"] = yard
    out["region_over_yardstick"] = {"wall": med["region"]["wall_ms"] / yard["wall_ms"], "kernel": med["region"]["kernel_ms"] / yard["kernel_ms"]}
    print("region / (dense16 + fresh tile256): wall %.3f (%.2f against %.2f ms, %.2f of them creating the tile's context), trace + shade %.3f"
          % (out["region_over_yardstick"]["wall"], med["region"]["wall_ms"], yard["wall_ms"], med["tile256"]["create_ms"], out["region_over_yardstick"]["kernel"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
