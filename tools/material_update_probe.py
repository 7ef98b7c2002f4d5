#!/usr/bin/env python3
"""What a material update costs (drt_update_spectra, drt_update_materials), beside the only thing there was before it:
drt_destroy + drt_create. One process, one MI355X.

    python3 tools/material_update_probe.py [--scene headline | spheres:N] [--size 1024] [--spp 256] [--depth 8] [--reps 5]

On a resident context (DRT_BATCH_RESIDENT) the medians over --reps of: destroy + create (wall); a one-row and an all-rows
drt_update_spectra in host mode and in device mode; a drt_update_materials of every material. Per update the wall time until the stream
is idle, the wall time of the call by itself (device mode enqueues and returns), and the HIP-event time of what the call put on the
context's stream (host mode: the copy of the rows and the two kernels; device mode: the two kernels; materials: the copy of the records).
The context runs on a torch stream for this (drt_set_stream), so that torch's events bracket the work. "All rows" is every row from the
first after the observer's to the last. Prints its lines and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))

import pydrt  # noqa: E402


def load(scene, size):
    if scene.startswith("spheres:"):
        return pydrt.synthetic_sphere_scene(int(scene.split(":")[1]), size, size)
    return pydrt.load_scene(os.path.join(REPO, "scenes", "cornell_plane_light.scn"), size, size)


def wall_ms(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", default="headline")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    bundle = load(a.scene, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    sc = bundle.scene
    spds = bundle.spds()
    lo = max(int(sc.cmf_rw), int(sc.cmf_x), int(sc.cmf_y), int(sc.cmf_z)) + 1
    one = next(int(sc.materials[i].diffuse_spd) for i in range(int(sc.num_materials)) if int(sc.materials[i].diffuse_spd) >= lo)
    out = {"scene": a.scene, "surfaces": int(sc.num_surfaces), "materials": int(sc.num_materials), "rows": int(sc.num_spds), "S": bundle.S,
           "size": a.size, "reps": a.reps}
    first_ms, r = wall_ms(lambda: pydrt.Renderer(bundle, params))
    out["first_create_ms"] = first_ms
    recreate = []
    for _ in range(a.reps):
        def again():
            r.close()
            return pydrt.Renderer(bundle, params)
        ms, r = wall_ms(again)
        recreate.append(ms)
    out["destroy_create_ms"] = statistics.median(recreate)
    stream = torch.cuda.Stream(device="cuda:0")
    r.set_stream(stream.cuda_stream)
    r.render(0, 1)  # a context that has rendered, as a live one has
    r.reset_film()
    r.synchronize()
    values = [spds, spds * 0.5]
    dev = [torch.from_numpy(v.copy()).to("cuda:0") for v in values]
    mats = [bundle.materials(), bundle.materials()]
    for m in mats[1]:
        m.shininess, m.roughness = m.shininess * 0.5, m.roughness * 0.5
    torch.cuda.synchronize()
    legs = {
        "spectra_host_one": lambda k: r.update_spectra(values[k % 2][one:one + 1], first=one),
        "spectra_host_all": lambda k: r.update_spectra(values[k % 2][lo:], first=lo),
        "spectra_device_one": lambda k: r.update_spectra(dev[k % 2][one:one + 1], first=one),
        "spectra_device_all": lambda k: r.update_spectra(dev[k % 2][lo:], first=lo),
        "materials_all": lambda k: r.update_materials(mats[k % 2]),
    }
    for name, leg in legs.items():
        leg(0)
        r.synchronize()
        leg(1)  # the first update makes the device copies: not what a frame pays
        r.synchronize()
        walls, calls, events = [], [], []
        for k in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            leg(k)
            t1 = time.perf_counter()
            e1.record(stream)
            r.synchronize()
            t2 = time.perf_counter()
            e1.synchronize()
            walls.append((t2 - t0) * 1e3)
            calls.append((t1 - t0) * 1e3)
            events.append(e0.elapsed_time(e1))
        out[name + "_wall_ms"], out[name + "_call_ms"], out[name + "_event_ms"] = (statistics.median(x) for x in (walls, calls, events))
    out["cheaper_than_recreation"] = all(out[n + "_wall_ms"] < out["destroy_create_ms"] for n in legs)
    r.close()
    for k, v in out.items():
        print("%-30s %s" % (k, ("%.4f" % v) if isinstance(v, float) else v))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
