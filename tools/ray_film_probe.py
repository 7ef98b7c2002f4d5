#!/usr/bin/env python3
"""Rate of a ray film (drt_bind_rays) beside the camera render it must equal: on the headline scene a context is bound to its own
camera's centre rays (drt_cast_pixels under DRT_FILM_SAMPLE_CENTER gives them, the weights are dirs . forward) and renders the frame
--steps times after --warmup, resident, as bench.py times it (wall clock around the steps, the kernels' own HIP-event times beside
it); the same frame through the camera under the centre scheme is timed the same way, in the same process, before and after it.
Prints one line per leg and one JSON line. With --layers L the table is the same rays L times over, which only spreads a pixel's
samples over L entries (width * height entries apart): what the layered read costs.

    python3 tools/ray_film_probe.py [--scene cornell_plane_light.scn] [--size 1024] [--spp 256] [--depth 8] [--steps 3] [--warmup 1]
                                    [--layers 1] [--device-table]   (--device-table: torch tensors, used in place)"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))

import pydrt  # noqa: E402


def timed(r, spp, steps, warmup):
    for _ in range(warmup):
        r.render(0, spp)
    r.synchronize()
    st0 = r.stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        r.render(0, spp)
    r.synchronize()
    dt = time.perf_counter() - t0
    st1 = r.stats()
    paths = st1.paths - st0.paths
    return {"ms_per_step": dt * 1e3 / steps, "mpaths_per_s": paths / dt / 1e6, "trace_ms": (st1.trace_ms - st0.trace_ms) / steps,
            "shade_ms": (st1.shade_ms - st0.shade_ms) / steps, "path_flags": st1.path_flags}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", default="cornell_plane_light.scn")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--device-table", action="store_true")
    a = ap.parse_args()
    W = H = a.size
    bundle = pydrt.load_scene(os.path.join(REPO, "scenes", a.scene), W, H)
    bundle.camera.aperture_radius = 0.0
    params = pydrt.make_params(W, H, spp=a.spp, max_depth=a.depth, seed=1, pixel_scheme=pydrt.FILM_SAMPLE_CENTER, batch_spp=pydrt.BATCH_RESIDENT)
    legs = {}
    cam = pydrt.Renderer(bundle, params)
    try:
        xy = np.stack([np.tile(np.arange(W), H), np.repeat(np.arange(H), W)], axis=1)
        o, d, _ = cam.cast_pixels(xy, np.zeros(W * H, dtype=np.uint32))
        legs["camera"] = timed(cam, a.spp, a.steps, a.warmup)
    finally:
        cam.close()
    f = np.array(list(bundle.camera.forward))
    w = d[:, 0] * f[0] + d[:, 1] * f[1] + d[:, 2] * f[2]
    table = [np.ascontiguousarray(np.broadcast_to(t.reshape((1, H, W) + t.shape[1:]), (a.layers, H, W) + t.shape[1:])) for t in (o, d, w)]
    if a.device_table:
        import torch
        table = [torch.from_numpy(t).to("cuda:0").contiguous() for t in table]
        torch.cuda.synchronize()
    ray = pydrt.Renderer(bundle, params)
    try:
        ray.bind_rays(*table)
        legs["rays"] = timed(ray, a.spp, a.steps, a.warmup)
    finally:
        ray.close()
    cam = pydrt.Renderer(bundle, params)
    try:
        legs["camera_again"] = timed(cam, a.spp, a.steps, a.warmup)
    finally:
        cam.close()
    assert legs["rays"]["path_flags"] & pydrt.PATH_RAYS and not legs["camera"]["path_flags"] & pydrt.PATH_RAYS
    for name, leg in legs.items():
        print("%-13s %8.3f ms per step, %8.1f Mpaths/s (trace %.3f ms, shade + film %.3f ms)" % (name, leg["ms_per_step"], leg["mpaths_per_s"], leg["trace_ms"], leg["shade_ms"]))
    print(json.dumps({"scene": a.scene, "size": a.size, "spp": a.spp, "depth": a.depth, "steps": a.steps, "warmup": a.warmup, "layers": a.layers,
                      "device_table": bool(a.device_table), "legs": legs}))


if __name__ == "__main__":
    main()
