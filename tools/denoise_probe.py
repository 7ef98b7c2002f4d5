#!/usr/bin/env python3
"""Times the variance-guided denoiser (drt_denoise_film: guide, weight and apply kernel) on a chosen workload: renders the frame
once, then filters the resident film --repeat times and prints the HIP-event time of each pass (the first one carries the
allocations) and one JSON line. Per-kernel times come from running this under `rocprofv3 --kernel-trace --stats -- python3 ...`.

    python3 tools/denoise_probe.py [--scene cornell_plane_light.scn] [--size 1024] [--spp 256] [--depth 8]
                                   [--radius 5] [--patch 1] [--k 1] [--alpha 1] [--repeat 5]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))

import pydrt  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", default="cornell_plane_light.scn")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--patch", type=int, default=1)
    ap.add_argument("--k", type=float, default=1.0)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    bundle = pydrt.load_scene(os.path.join(REPO, "scenes", a.scene), a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    r = pydrt.Renderer(bundle, params)
    r.render()
    st = r.stats()
    times, unusable = [], 0
    for _ in range(max(1, a.repeat)):
        rep = r.denoise(a.radius, a.patch, a.k, a.alpha)
        times.append(rep["kernel_ms"])
        unusable = rep["unusable"]
    r.close()
    S, n = bundle.S, a.size * a.size
    steady = sorted(times[1:] or times)
    # what the three kernels must move at least: the film's mean and variance in, the result out, the guide and the weights out and in
    floor_bytes = n * (4 * S * 8 + 2 * 64 + 2 * (2 * a.radius + 1) ** 2 * 8)
    line = {"scene": a.scene, "size": a.size, "spp": a.spp, "S": S, "radius": a.radius, "patch": a.patch, "k": a.k, "alpha": a.alpha,
            "render_ms": st.total_ms, "denoise_ms": times, "denoise_ms_median": steady[len(steady) // 2], "unusable": unusable,
            "compulsory_gb": floor_bytes / 1e9, "compulsory_gb_per_s": floor_bytes / 1e6 / steady[len(steady) // 2]}
    for i, t in enumerate(times):
        print("denoise pass %d: %.3f ms" % (i, t))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
