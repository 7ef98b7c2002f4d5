#!/usr/bin/env python3
"""What a scene update costs (drt_update_surfaces, drt_set_camera, drt_rebuild_hierarchy), beside the only thing there was before it:
drt_destroy + drt_create. One process, one MI355X.

    python3 tools/scene_update_probe.py cost  [--scene headline | spheres:N] [--size 1024] [--spp 256] [--depth 8] [--reps 5]
    python3 tools/scene_update_probe.py refit [--spheres 10000] [--size 1024] [--spp 4] [--depth 8] [--frac 0.01]
    python3 tools/scene_update_probe.py build [--spheres 10000] [--size 4096] [--spp 64] [--reps 5]
    python3 tools/scene_update_probe.py drift [--spheres 10000] [--size 1024] [--spp 4] [--frames 8] [--frac 0.05] [--every 0]

cost:  on a resident context (DRT_BATCH_RESIDENT) the medians over --reps of: destroy + create (wall), the host build of the tree by
       itself (drt_bvh_stats, which runs the builder and nothing else; 0 for a scene that fits the LDS), a whole-scene host-mode
       update (wall until the stream is idle, and the kernels' HIP-event time), the same in device mode, the same with
       DRT_SURFACES_REBUILD, and a drt_set_camera.
refit: the trace-stage time of the frame after a refit of spheres displaced by --frac of the scene's size (40), against the same
       scene in a fresh context, against the refit context after DRT_SURFACES_REBUILD, and against it after a device build
       (drt_rebuild_hierarchy).
build: what a device build costs beside DRT_SURFACES_REBUILD of the same scene on the same context: medians over --reps of the
       kernels' HIP-event time and of the wall time of the call plus drt_synchronize, and the device-mode update a build follows.
drift: what a device-mode caller sees: --frames device-mode updates, each displacing every sphere by --frac of the scene's size from
       where it began, the trace stage of every frame, with a device build after every --every updates (0: never).
Each prints its lines and one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))

import pydrt  # noqa: E402


def load(scene, size):
    if scene.startswith("spheres:"):
        return pydrt.synthetic_sphere_scene(int(scene.split(":")[1]), size, size)
    return pydrt.load_scene(os.path.join(REPO, "scenes", "cornell_plane_light.scn"), size, size)


def with_rows(bundle, rows):
    """the bundle's scene with other surfaces (its materials and spectra shared)"""
    sa = pydrt.surfaces_from_rows(rows)
    sc = pydrt.Scene()
    C.memmove(C.byref(sc), C.byref(bundle.scene), C.sizeof(pydrt.Scene))
    sc.surfaces = C.cast(sa, C.POINTER(pydrt.Surface))
    return pydrt.SceneBundle(sc, bundle.camera, keep=(sa, bundle))


def wall_ms(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return statistics.median(xs) if xs else 0.0


def cost(a):
    bundle = load(a.scene, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    rows = pydrt.surface_rows(bundle)
    moved = rows.copy()
    moved[:, 1:4] += 0.01  # every surface a little: a whole-scene update
    out = {"scene": a.scene, "surfaces": int(rows.shape[0]), "size": a.size, "reps": a.reps}
    first_ms, r = wall_ms(lambda: pydrt.Renderer(bundle, params))
    out["first_create_ms"] = first_ms
    bvh = bool(r.stats().path_flags & pydrt.PATH_BVH)
    out["hierarchy"] = bvh
    recreate = []
    for _ in range(a.reps):
        def again():
            r.close()
            return pydrt.Renderer(bundle, params)
        ms, r = wall_ms(again)
        recreate.append(ms)
    out["destroy_create_ms"] = median(recreate)
    out["tree_build_ms"] = median([wall_ms(lambda: pydrt.bvh_stats(bundle))[0] for _ in range(a.reps)]) if bvh else 0.0

    def update(surfaces, **kw):
        r.update_surfaces(surfaces, **kw)
        r.synchronize()

    legs = {"host": lambda k: update(moved if k % 2 == 0 else rows), "camera": lambda k: (r.set_camera(bundle), r.synchronize())}
    if bvh:
        legs["rebuild"] = lambda k: update(moved if k % 2 == 0 else rows, rebuild=True)
    try:
        import torch
        dev = [torch.from_numpy(moved).to("cuda:0"), torch.from_numpy(rows).to("cuda:0")]
        torch.cuda.synchronize()
        legs["device"] = lambda k: update(dev[k % 2])
    except ImportError:
        pass
    r.render(0, 1)  # a context that has rendered, as a live one has
    r.reset_film()
    for name, leg in legs.items():
        leg(0)
        leg(1)  # the first update makes the device copies: not what a frame pays
        walls, kernels = [], []
        for k in range(a.reps):
            walls.append(wall_ms(lambda: leg(k))[0])
            kernels.append(r.update_report()["kernel_ms"])
        out["update_%s_wall_ms" % name] = median(walls)
        out["update_%s_kernel_ms" % name] = median(kernels)
    out["cheaper_than_recreation"] = all(out["update_%s_wall_ms" % n] < out["destroy_create_ms"] for n in legs)
    r.close()
    for k, v in out.items():
        print("%-28s %s" % (k, ("%.3f" % v) if isinstance(v, float) else v))
    print(json.dumps(out))


def refit(a):
    bundle = pydrt.synthetic_sphere_scene(a.spheres, a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    rows = pydrt.surface_rows(bundle)
    rng = np.random.default_rng(1)
    moved = rows.copy()
    moved[:a.spheres, 1:4] += rng.uniform(-1.0, 1.0, (a.spheres, 3)) * (a.frac * 40.0)
    moved_bundle = with_rows(bundle, moved)

    def frame(r):
        r.reset_film()
        r.render(0, a.spp)
        r.synchronize()  # (a warm-up: the first launch of a process pays for loading the code)
        r.reset_film()
        r.render(0, a.spp)
        st = r.stats()
        return {"trace_ms": st.trace_ms, "shade_ms": st.shade_ms, "redone_launches": st.redone_launches}

    out = {"spheres": a.spheres, "size": a.size, "spp": a.spp, "frac": a.frac}
    r = pydrt.Renderer(moved_bundle, params)
    out["fresh"] = frame(r)
    r.close()
    r = pydrt.Renderer(bundle, params)
    r.update_surfaces(moved)
    out["refit"] = frame(r)
    r.reset_film()
    r.update_surfaces(moved, rebuild=True)
    out["rebuilt"] = frame(r)
    r.close()
    r = pydrt.Renderer(bundle, params)
    r.update_surfaces(moved)
    r.rebuild_hierarchy()
    out["device_built"] = frame(r)
    out["device_built"]["depth"] = r.hierarchy_report()["depth"]
    r.close()
    out["device_over_host_trace"] = out["device_built"]["trace_ms"] / out["rebuilt"]["trace_ms"] if out["rebuilt"]["trace_ms"] > 0.0 else 0.0
    for k in ("fresh", "refit", "rebuilt", "device_built"):
        print("%-8s trace %.3f ms, shade + film %.3f ms, %d launches redone" % (k, out[k]["trace_ms"], out[k]["shade_ms"], out[k]["redone_launches"]))
    print(json.dumps(out))


def build(a):
    bundle = pydrt.synthetic_sphere_scene(a.spheres, a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    rows = pydrt.surface_rows(bundle)
    moved = rows.copy()
    moved[:, 1:4] += 0.01
    import torch
    dev = [torch.from_numpy(moved).to("cuda:0"), torch.from_numpy(rows).to("cuda:0")]
    torch.cuda.synchronize()
    r = pydrt.Renderer(bundle, params)
    r.render(0, 1)  # a context that has rendered, as a live one has
    r.reset_film()
    out = {"spheres": a.spheres, "size": a.size, "spp": a.spp, "reps": a.reps}

    def device_build(k):
        r.rebuild_hierarchy()
        r.synchronize()

    def device_update(k):
        r.update_surfaces(dev[k % 2])
        r.synchronize()

    def host_rebuild(k):
        r.update_surfaces(moved if k % 2 == 0 else rows, rebuild=True)
        r.synchronize()

    def call_only(k):
        r.rebuild_hierarchy()

    for name, leg, kernel in (("device_update", device_update, lambda: r.update_report()["kernel_ms"]),
                              ("device_build", device_build, lambda: r.hierarchy_report()["kernel_ms"]),
                              ("host_rebuild", host_rebuild, lambda: r.update_report()["kernel_ms"])):
        leg(0)
        leg(1)  # the first call makes the temporaries: not what a frame pays
        walls, kernels = [], []
        for k in range(a.reps):
            walls.append(wall_ms(lambda: leg(k))[0])
            kernels.append(kernel())
        out[name + "_wall_ms"], out[name + "_kernel_ms"] = median(walls), median(kernels)
    calls = []
    for k in range(a.reps):  # the call by itself: it enqueues and returns
        calls.append(wall_ms(lambda: call_only(k))[0])
        r.synchronize()
    out["device_build_call_ms"] = median(calls)
    rep = r.hierarchy_report()
    out["nodes"], out["depth"] = rep["nodes"], rep["depth"]
    out["device_below_host"] = out["device_build_wall_ms"] < out["host_rebuild_wall_ms"]
    r.close()
    for k, v in out.items():
        print("%-28s %s" % (k, ("%.3f" % v) if isinstance(v, float) else v))
    print(json.dumps(out))


def drift(a):
    import torch
    bundle = pydrt.synthetic_sphere_scene(a.spheres, a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    rows = pydrt.surface_rows(bundle)
    rng = np.random.default_rng(1)
    step = rng.uniform(-1.0, 1.0, (a.spheres, 3)) * (a.frac * 40.0)
    r = pydrt.Renderer(bundle, params)
    r.render(0, a.spp)
    r.synchronize()
    out = {"spheres": a.spheres, "size": a.size, "spp": a.spp, "frac": a.frac, "every": a.every, "frames": []}
    for k in range(1, a.frames + 1):
        moved = rows.copy()
        moved[:a.spheres, 1:4] += step * k
        r.reset_film()
        r.update_surfaces(torch.from_numpy(moved).to("cuda:0"))
        built = a.every > 0 and r.update_report()["refits_since_build"] >= a.every
        if built:
            r.rebuild_hierarchy()
        r.render(0, a.spp)
        st = r.stats()
        out["frames"].append({"frame": k, "built": built, "trace_ms": st.trace_ms})
        print("frame %2d  %s  trace %.3f ms" % (k, "build" if built else "refit", st.trace_ms))
    r.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="what", required=True)
    c = sub.add_parser("cost")
    c.add_argument("--scene", default="headline")
    c.add_argument("--size", type=int, default=1024)
    c.add_argument("--spp", type=int, default=256)
    c.add_argument("--depth", type=int, default=8)
    c.add_argument("--reps", type=int, default=5)
    f = sub.add_parser("refit")
    f.add_argument("--spheres", type=int, default=10000)
    f.add_argument("--size", type=int, default=1024)
    f.add_argument("--spp", type=int, default=4)
    f.add_argument("--depth", type=int, default=8)
    f.add_argument("--frac", type=float, default=0.01)
    b = sub.add_parser("build")
    b.add_argument("--spheres", type=int, default=10000)
    b.add_argument("--size", type=int, default=4096)
    b.add_argument("--spp", type=int, default=64)
    b.add_argument("--depth", type=int, default=8)
    b.add_argument("--reps", type=int, default=5)
    d = sub.add_parser("drift")
    d.add_argument("--spheres", type=int, default=10000)
    d.add_argument("--size", type=int, default=1024)
    d.add_argument("--spp", type=int, default=4)
    d.add_argument("--depth", type=int, default=8)
    d.add_argument("--frames", type=int, default=8)
    d.add_argument("--frac", type=float, default=0.05)
    d.add_argument("--every", type=int, default=0)
    a = ap.parse_args()
    {"cost": cost, "refit": refit, "build": build, "drift": drift}[a.what](a)


if __name__ == "__main__":
    main()
