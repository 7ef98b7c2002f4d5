#!/usr/bin/env python3
"""What a sensor film costs (drt_bind_sensor), beside its yardstick: the depth-cut pass for the one cut {max_depth},
which does the same replay with a per-wavelength sink.

    python3 tools/sensor_probe.py [--size 1024] [--spp 256] [--depth 8] [--reps 3] [--out FILE]

One process per configuration and run, as tools/depth_cut_probe.py: the parent opens no device and starts the configurations one
after the other, --reps rounds over all of them, so the runs of the configurations alternate. A child creates its context
(DRT_BATCH_RESIDENT), binds what its configuration names, renders the frame once to warm up, resets the film and renders it once more,
timed: the wall time from the call to the end of drt_synchronize, and the trace and shade + pass times of its kernel pairs by HIP
events (drt_stats).

The configurations, on cornell_plane_light.scn at --size^2 x --spp and --depth:
    plain             nothing bound
    cut               depth cuts {--depth}
    observer          a sensor of pydrt.observer_curves (3 channels)
    eight             a sensor of 8 seeded curves
and from their medians the pass per frame: shade_ms with it bound minus shade_ms of `plain`. Prints its lines and one JSON line (also
written to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))

CONFIGS = ("plain", "cut", "observer", "eight")


def child(a):
    import numpy as np
    import pydrt
    bundle = pydrt.load_scene(os.path.join(REPO, "scenes", "cornell_plane_light.scn"), a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    r = pydrt.Renderer(bundle, params)
    try:
        if a.config == "cut":
            r.bind_depth_cuts([a.depth])
        elif a.config == "observer":
            r.bind_sensor(pydrt.observer_curves(bundle))
        elif a.config == "eight":
            r.bind_sensor(np.random.default_rng(8).uniform(-0.5, 1.0, size=(8, bundle.S)))
        r.render()
        r.synchronize()
        r.reset_film()
        t0 = time.perf_counter()
        r.render()
        r.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        st = r.stats()
        assert st.paths == a.size * a.size * a.spp and st.redone_launches == 0
        print(json.dumps({"config": a.config, "wall_ms": wall, "trace_ms": st.trace_ms, "shade_ms": st.shade_ms, "launches": st.launches}))
    finally:
        r.close()


def run_child(a, config):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--spp", str(a.spp), "--depth", str(a.depth), "--config", config]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("sensor_probe: the run of `%s` failed (%d)" % (config, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--config", default="plain", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {c: [] for c in CONFIGS}
    for rep in range(a.reps):
        for c in CONFIGS:
            runs[c].append(run_child(a, c))
            print("rep %d %-9s wall %8.2f ms  trace %8.2f  shade(+pass) %8.2f" % (rep, c, runs[c][-1]["wall_ms"], runs[c][-1]["trace_ms"], runs[c][-1]["shade_ms"]),
                  flush=True)
    med = {c: {k: statistics.median(x[k] for x in runs[c]) for k in ("wall_ms", "trace_ms", "shade_ms")} for c in CONFIGS}
    out = {"size": a.size, "spp": a.spp, "depth": a.depth, "reps": a.reps,
           "runs": [{"config": c, **med[c], "wall_all_ms": [x["wall_ms"] for x in runs[c]], "shade_all_ms": [x["shade_ms"] for x in runs[c]]} for c in CONFIGS],
           "pass_ms": {c: med[c]["shade_ms"] - med["plain"]["shade_ms"] for c in CONFIGS if c != "plain"},
           "wall_over_plain_ms": {c: med[c]["wall_ms"] - med["plain"]["wall_ms"] for c in CONFIGS if c != "plain"}}
    print("shade kernel %.2f ms per frame; the pass on top of it: %s; wall on top of plain: %s" %
          (med["plain"]["shade_ms"], {k: round(v, 2) for k, v in out["pass_ms"].items()}, {k: round(v, 2) for k, v in out["wall_over_plain_ms"].items()}))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
