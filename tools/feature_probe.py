#!/usr/bin/env python3
"""Times the first-hit feature pass (drt_render_features: one kernel, one lane per pixel) on a chosen workload: renders the frame
once, then takes the features of the resident film --repeat times, every pixel at the count its film holds, and prints the HIP-event
time of each pass (the first one carries the allocations), the render's own trace-stage time beside it, and one JSON line. The
kernel's own line comes from running this under `rocprofv3 --kernel-trace --stats -- python3 ...`.

    python3 tools/feature_probe.py [--scene cornell_plane_light.scn] [--size 1024] [--spp 256] [--depth 8] [--repeat 5]
                                   [--spheres N]   (the many-sphere scene behind the hierarchy instead of --scene)"""
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
    ap.add_argument("--spheres", type=int, default=0)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    if a.spheres:
        bundle = pydrt.synthetic_sphere_scene(a.spheres, a.size, a.size)
    else:
        bundle = pydrt.load_scene(os.path.join(REPO, "scenes", a.scene), a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    r = pydrt.Renderer(bundle, params)
    r.render()
    st = r.stats()
    times, rep = [], None
    for _ in range(max(1, a.repeat)):
        rep = r.render_features(0)
        times.append(rep["kernel_ms"])
    mean, _, _ = r.read_features()
    r.close()
    steady = sorted(times[1:] or times)
    med = steady[len(steady) // 2]
    line = {"scene": "spheres:%d" % a.spheres if a.spheres else a.scene, "size": a.size, "spp": a.spp, "rays": rep["rays"],
            "empty_pixels": rep["empty_pixels"], "coverage": float(mean[:, 4].mean()), "render_trace_ms": st.trace_ms,
            "render_shade_ms": st.shade_ms, "closest_hit_scans": st.closest_hit_scans, "shadow_scans": st.shadow_scans,
            "features_ms": times, "features_ms_median": med, "mrays_per_s": rep["rays"] / 1e3 / med,
            "features_over_trace": med / st.trace_ms if st.trace_ms else None}
    for i, t in enumerate(times):
        print("feature pass %d: %.3f ms" % (i, t))
    print("render: trace %.3f ms, shade %.3f ms" % (st.trace_ms, st.shade_ms))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
