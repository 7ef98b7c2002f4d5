#!/usr/bin/env python3
"""What the pixels that cannot see the scene cost: one resident context over the whole frame against one whose tile is the live
window (drt_live_window_of, or --window x_lo,x_hi,y_lo,y_hi), same scene, samples and depth. One context per process (a fresh
process per measurement, alternated by the caller); prints one JSON line with trace_ms and shade_ms per frame.

  python tools/live_window_probe.py --tile full
  python tools/live_window_probe.py --tile live [--window 185,839,185,839]
  python tools/live_window_probe.py --share --roll 30      (no GPU: the window's share of the frame for a rolled camera)
"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))


def window_of(pydrt, bundle, params):
    out = (C.c_uint32 * 4)()
    rc = pydrt.hip_lib().drt_live_window_of(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(params), out)
    if rc != 0:
        raise SystemExit("drt_live_window_of failed: " + pydrt.hip_lib().drt_last_error().decode())
    return [int(v) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell_plane_light.scn")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--tile", choices=["full", "live"], default="full")
    ap.add_argument("--window", default="", help="x_lo,x_hi,y_lo,y_hi instead of the library's rule")
    ap.add_argument("--share", action="store_true", help="print the window and its share of the frame, render nothing")
    ap.add_argument("--roll", type=float, default=0.0, help="camera roll in degrees (--share)")
    args = ap.parse_args()
    import pydrt

    W = H = args.size
    bundle = pydrt.load_scene(os.path.join(REPO, "scenes", args.scene), W, H)
    if args.roll:
        import math
        import numpy as np
        cam = bundle.camera
        f, r, u = (np.array(list(v)) for v in (cam.forward, cam.right, cam.up))
        a = math.radians(args.roll)
        r2, u2 = math.cos(a) * r + math.sin(a) * u, math.cos(a) * u - math.sin(a) * r
        ap_ = np.array(list(cam.aperture_position))
        centre = np.array(list(cam.film_bottom_left)) + 0.5 * W * cam.pixel_width * r + 0.5 * H * cam.pixel_height * u
        bl = centre - 0.5 * W * cam.pixel_width * r2 - 0.5 * H * cam.pixel_height * u2
        for k in range(3):
            cam.right[k], cam.up[k], cam.film_bottom_left[k] = r2[k], u2[k], bl[k]
        del f, ap_
    whole = pydrt.make_params(W, H, spp=args.spp, max_depth=args.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    if args.window:
        win = [int(v) for v in args.window.split(",")]
    elif args.tile == "live" or args.share:
        win = window_of(pydrt, bundle, whole)
    else:
        win = [0, W, 0, H]
    if args.share:
        print(json.dumps({"window": win, "share": (win[1] - win[0]) * (win[3] - win[2]) / float(W * H), "roll": args.roll}))
        return
    if args.tile == "full":
        win = [0, W, 0, H]
    params = pydrt.make_params(W, H, spp=args.spp, max_depth=args.depth, seed=1, x0=win[0], y0=win[2], tile_w=win[1] - win[0],
                               tile_h=win[3] - win[2], batch_spp=pydrt.BATCH_RESIDENT)
    os.environ.setdefault("DRT_NO_LIVE_WINDOW", "1")  # the tile itself is what is being compared
    r = pydrt.Renderer(bundle, params)
    r.render(0, args.spp)  # warm-up
    r.synchronize()
    frames = []
    for _ in range(args.frames):
        r.reset_film()
        r.render(0, args.spp)
        r.synchronize()
        st = r.stats()
        frames.append({"trace_ms": round(st.trace_ms, 3), "shade_ms": round(st.shade_ms, 3), "paths": int(st.paths),
                       "redone": int(st.redone_launches)})
    best = min(frames, key=lambda f: f["trace_ms"] + f["shade_ms"])
    print(json.dumps({"tile": args.tile, "window": win, "batch_spp": r.batch_spp(), "frames": frames, "best_sum_ms": round(best["trace_ms"] + best["shade_ms"], 3)}),
          flush=True)
    r.close()


if __name__ == "__main__":
    main()
