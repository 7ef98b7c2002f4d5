#!/usr/bin/env python3
"""Times the ID-matte pass (drt_render_mattes: one kernel, one lane per pixel) on a chosen workload, and the first-hit feature pass
beside it, which casts the same rays and runs the same scans: renders the frame once, then takes the mattes and the features of the
resident film --repeat times each, alternating, every pixel at the count its film holds, and prints the HIP-event time of each pass
(the first one carries the allocations) and one JSON line. The kernels' own lines come from running this under
`rocprofv3 --kernel-trace --stats -- python3 ...`.

    python3 tools/matte_probe.py [--scene cornell_plane_light.scn] [--size 1024] [--spp 256] [--depth 8] [--repeat 5]
                                 [--spheres N]   (the many-sphere scene behind the hierarchy instead of --scene)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))

import pydrt  # noqa: E402


def median(times):
    steady = sorted(times[1:] or times)
    return steady[len(steady) // 2]


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
    mattes, features, rep = [], [], None
    for _ in range(max(1, a.repeat)):
        rep = r.render_mattes(0)
        mattes.append(rep["kernel_ms"])
        features.append(r.render_features(0)["kernel_ms"])
    ids, counts, tail = r.read_mattes()
    r.close()
    m, f = median(mattes), median(features)
    line = {"scene": "spheres:%d" % a.spheres if a.spheres else a.scene, "size": a.size, "spp": a.spp, "rays": rep["rays"],
            "empty_pixels": rep["empty_pixels"], "overflow_pixels": list(rep["overflow_pixels"]),
            "pixels_with_two_surfaces": int((counts[:, 0, 1] > 0).sum()), "pixels_with_two_materials": int((counts[:, 1, 1] > 0).sum()),
            "render_trace_ms": st.trace_ms, "mattes_ms": mattes, "features_ms": features, "mattes_ms_median": m, "features_ms_median": f,
            "mattes_over_features": m / f, "mrays_per_s": rep["rays"] / 1e3 / m}
    for i, (tm, tf) in enumerate(zip(mattes, features)):
        print("pass %d: mattes %.3f ms, features %.3f ms" % (i, tm, tf))
    print("render: trace %.3f ms, shade %.3f ms" % (st.trace_ms, st.shade_ms))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
