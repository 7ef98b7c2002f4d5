#!/usr/bin/env python3
"""What bucket films cost (drt_bind_buckets), beside their yardstick: the depth-cut pass for the one cut {max_depth},
which does the same replay with one film update per sample into one film.

    python3 tools/bucket_probe.py [--size 1024] [--spp 256] [--depth 8] [--reps 3] [--out FILE]

One process per configuration and run, as tools/sensor_probe.py: the parent opens no device and starts the configurations one after
the other, --reps rounds over all of them, so the runs of the configurations alternate. A child creates its context
(DRT_BATCH_RESIDENT), binds what its configuration names, renders the frame once to warm up, resets the film and renders it once more,
timed: the wall time from the call to the end of drt_synchronize, and the trace and shade + pass times of its kernel pairs by HIP
events (drt_stats). A child with two buckets or more then resolves twice (the median's trim) and times the second: wall time from
drt_resolve_buckets to the end of drt_synchronize, one kernel over films that are in place.

The configurations, on cornell_plane_light.scn at --size^2 x --spp and --depth:
    plain             nothing bound
    cut               depth cuts {--depth}
    b1, b2, b4, b8    1, 2, 4, 8 buckets
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

CONFIGS = ("plain", "cut", "b1", "b2", "b4", "b8")


def child(a):
    import pydrt
    bundle = pydrt.load_scene(os.path.join(REPO, "scenes", "cornell_plane_light.scn"), a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    r = pydrt.Renderer(bundle, params)
    try:
        n = int(a.config[1:]) if a.config[0] == "b" else 0
        if a.config == "cut":
            r.bind_depth_cuts([a.depth])
        elif n:
            r.bind_buckets(n)
        r.render()
        r.synchronize()
        r.reset_film()
        t0 = time.perf_counter()
        r.render()
        r.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        st = r.stats()
        assert st.paths == a.size * a.size * a.spp and st.redone_launches == 0
        out = {"config": a.config, "wall_ms": wall, "trace_ms": st.trace_ms, "shade_ms": st.shade_ms, "launches": st.launches}
        if n >= 2 and a.spp >= n:
            r.resolve_buckets()
            r.synchronize()
            t0 = time.perf_counter()
            r.resolve_buckets()
            r.synchronize()
            out["resolve_ms"] = (time.perf_counter() - t0) * 1e3
        print(json.dumps(out))
    finally:
        r.close()


def run_child(a, config):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--spp", str(a.spp), "--depth", str(a.depth), "--config", config]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("bucket_probe: the run of `%s` failed (%d)" % (config, out.returncode))
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
            x = runs[c][-1]
            print("rep %d %-6s wall %8.2f ms  trace %8.2f  shade(+pass) %8.2f%s" % (rep, c, x["wall_ms"], x["trace_ms"], x["shade_ms"],
                                                                                  "  resolve %.3f" % x["resolve_ms"] if "resolve_ms" in x else ""), flush=True)
    med = {c: {k: statistics.median(x[k] for x in runs[c]) for k in ("wall_ms", "trace_ms", "shade_ms")} for c in CONFIGS}
    resolve = {c: statistics.median(x["resolve_ms"] for x in runs[c]) for c in CONFIGS if all("resolve_ms" in x for x in runs[c])}
    cut_all = [x["shade_ms"] for x in runs["cut"]]
    out = {"size": a.size, "spp": a.spp, "depth": a.depth, "reps": a.reps,
           "runs": [{"config": c, **med[c], "wall_all_ms": [x["wall_ms"] for x in runs[c]], "shade_all_ms": [x["shade_ms"] for x in runs[c]]} for c in CONFIGS],
           "pass_ms": {c: med[c]["shade_ms"] - med["plain"]["shade_ms"] for c in CONFIGS if c != "plain"},
           "yardstick_spread_ms": max(cut_all) - min(cut_all),
           "wall_over_plain_ms": {c: med[c]["wall_ms"] - med["plain"]["wall_ms"] for c in CONFIGS if c != "plain"},
           "resolve_ms": resolve, "resolve_all_ms": {c: [x["resolve_ms"] for x in runs[c]] for c in resolve}}
    print("shade kernel %.2f ms per frame; the pass on top of it: %s (the yardstick `cut` spreads over %.2f ms); resolve: %s" %
          (med["plain"]["shade_ms"], {k: round(v, 2) for k, v in out["pass_ms"].items()}, out["yardstick_spread_ms"], {k: round(v, 3) for k, v in resolve.items()}))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
