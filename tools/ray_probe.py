#!/usr/bin/env python3
"""Times the ray queries in device mode (drt_cast_rays, drt_test_visibility: one kernel each, one lane per ray) on a chosen workload:
the frame's own camera rays, --samples of every pixel in sample-major order (so a wave holds neighbouring pixels, as the feature
kernel's does), and as many visibility pairs (each ray's hit position against a point on the scene's first light). With --second the
closest-hit list is the second generation instead: from every hit position a seeded random unit direction, the incoherent set.
Prints, per pass, the HIP-event time of each call, and beside the medians of the passes after the first two yardsticks taken in the
same process: drt_render_features over the same camera rays (the same scan with no per-ray input or output), and the time the rays'
152 bytes (48 in, 104 out) would take at the device-to-device copy bandwidth measured here. One JSON line at the end. The kernels'
own lines come from running this under `rocprofv3 --kernel-trace --stats -- python3 ...`.

    python3 tools/ray_probe.py [--scene cornell_plane_light.scn] [--size 1024] [--samples 32] [--repeat 5] [--second]
                               [--spheres N]   (the many-sphere scene behind the hierarchy instead of --scene)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))

import numpy as np  # noqa: E402
import pydrt  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", default="cornell_plane_light.scn")
    ap.add_argument("--spheres", type=int, default=0)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--second", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ray_probe: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    if a.spheres:
        bundle = pydrt.synthetic_sphere_scene(a.spheres, a.size, a.size)
    else:
        bundle = pydrt.load_scene(os.path.join(REPO, "scenes", a.scene), a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=1, max_depth=4, seed=1)
    r = pydrt.Renderer(bundle, params)
    stream = torch.cuda.Stream(device=dev)
    P, K = a.size * a.size, a.samples
    n = P * K

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    with torch.cuda.stream(stream):
        r.set_stream(stream.cuda_stream)
        x = torch.arange(a.size, dtype=torch.int32, device=dev).repeat(a.size)
        y = torch.arange(a.size, dtype=torch.int32, device=dev).repeat_interleave(a.size)
        xy = torch.stack([x, y], dim=1).repeat(K, 1).contiguous()
        smp = torch.arange(K, dtype=torch.int32, device=dev).repeat_interleave(P).contiguous()
        ro, rd, hits = r.cast_pixels(xy, smp)
        words = hits.view(torch.float64).reshape(n, 13)
        pos = words[:, 0:3].contiguous()
        index = hits.view(torch.int32).reshape(n, 26)[:, 22]
        hit_share = float((index >= 0).double().mean().item())
        sc = bundle.scene
        light = None
        for i in range(int(sc.num_surfaces)):
            s = sc.surfaces[i]
            if int(sc.materials[int(s.material)].is_emissive):
                light = np.array(list(s.position))
                if int(s.type) == pydrt.GEO_PLANE:
                    light = light + 0.5 * np.array(list(s.u)) + 0.5 * np.array(list(s.v))
                break
        if light is None:
            light = np.array(list(bundle.camera.aperture_position))
        p1 = torch.from_numpy(light).to(dev).repeat(n, 1).contiguous()
        if a.second:
            g = torch.Generator(device=dev)
            g.manual_seed(0x5EED)
            d2 = torch.randn((n, 3), dtype=torch.float64, device=dev, generator=g)
            rd = (d2 / d2.norm(dim=1, keepdim=True)).contiguous()
            ro = pos
        del xy, smp, x, y
        # the copy yardstick: a device-to-device copy of 1 GiB reads and writes 2 GiB
        src = torch.empty(1 << 27, dtype=torch.float64, device=dev).normal_()
        dst = torch.empty_like(src)
        copy_ms = sorted(timed(lambda: dst.copy_(src))[0] for _ in range(5))[2]
        copy_bw = 2.0 * src.numel() * 8 / (copy_ms * 1e-3)
        del src, dst
        cast_ms, vis_ms = [], []
        for _ in range(max(2, a.repeat)):
            t, out = timed(lambda: r.cast_rays(ro, rd))
            cast_ms.append(t)
            del out
            t, out = timed(lambda: r.test_visibility(pos, p1))
            vis_ms.append(t)
            visible_share = float(out.double().mean().item())
            del out
    feat_ms = []
    for _ in range(max(2, a.repeat)):
        feat_ms.append(r.render_features(K)["kernel_ms"])
    r.close()
    med = lambda v: sorted(v[1:])[len(v[1:]) // 2]
    bytes_ms = n * 152 / copy_bw * 1e3
    line = {"scene": "spheres:%d" % a.spheres if a.spheres else a.scene, "size": a.size, "samples": K, "rays": n, "second_generation": bool(a.second),
            "hit_share": hit_share, "visible_share": visible_share, "cast_ms": cast_ms, "visibility_ms": vis_ms, "features_ms": feat_ms,
            "cast_ms_median": med(cast_ms), "visibility_ms_median": med(vis_ms), "features_ms_median": med(feat_ms),
            "cast_mrays_per_s": n / 1e3 / med(cast_ms), "visibility_mpairs_per_s": n / 1e3 / med(vis_ms), "features_mrays_per_s": n / 1e3 / med(feat_ms),
            "copy_ms_1GiB": copy_ms, "copy_bytes_per_s": copy_bw, "ms_of_152_bytes_per_ray_at_copy_bandwidth": bytes_ms,
            "ms_of_49_bytes_per_pair_at_copy_bandwidth": n * 49 / copy_bw * 1e3}
    for i in range(len(cast_ms)):
        print("pass %d: cast_rays %.3f ms, test_visibility %.3f ms, features %.3f ms" % (i, cast_ms[i], vis_ms[i], feat_ms[i]))
    print("copy: %.3f ms per GiB copied, %.2f TB/s read + written; 152 bytes per ray: %.3f ms" % (copy_ms, copy_bw / 1e12, bytes_ms))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
