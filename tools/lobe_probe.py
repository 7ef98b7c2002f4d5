#!/usr/bin/env python3
"""What lobe films cost (drt_bind_lobes), beside their yardstick: the bucket pass at the same film count, which does the
same replay with one film update per sample where the lobe pass runs one per film and sample.

    python3 tools/lobe_probe.py [--size 1024] [--spp 256] [--depth 8] [--reps 3] [--configs plain,l7,l8] [--out FILE]

One process per configuration and run, as tools/sensor_probe.py: the parent opens no device and starts the configurations one after
the other, --reps rounds over all of them, so the runs of the configurations alternate. A child creates its context
(DRT_BATCH_RESIDENT), binds what its configuration names, renders the frame once to warm up, resets the film and renders it once more,
timed: the wall time from the call to the end of drt_synchronize, and the trace and shade + pass times of its kernel pairs by HIP
events (drt_stats).

The configurations, on cornell_plane_light.scn at --size^2 x --spp and --depth:
    plain                  nothing bound
    b1, b2, b4, b7, b8     1, 2, 4, 7, 8 buckets
    l1, l2, l4, l7, l8     1, 2, 4, 7, 8 lobe films: l1 everything on film 0; l2 emission and direct light on film 0, indirect on film 1;
                           l4 emission, the diffuse direct light, the other direct light, all indirect light; l7 the preset "standard";
                           l8 the preset "functions"
(--configs: a subset of them, `plain` always included; DRT_HIP_LIB names another build of the library, for an A/B of one change)
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

COUNTS = (1, 2, 4, 7, 8)
CONFIGS = ("plain",) + tuple("b%d" % n for n in COUNTS) + tuple("l%d" % n for n in COUNTS)


def lobe_binding(pydrt, n):
    """what configuration l<n> binds"""
    names = pydrt.BDSF_NAMES
    if n == 1:
        return pydrt.lobe_map(default=0), 1
    if n == 2:
        return pydrt.lobe_map(emission=0, direct={f: 0 for f in names}, indirect={f: 1 for f in names}), 2
    if n == 4:
        direct = {f: 2 for f in names}
        direct["bp_diffuse_bdsf"] = 1
        return pydrt.lobe_map(emission=0, direct=direct, indirect={f: 3 for f in names}), 4
    return {7: "standard", 8: "functions"}[n], None


def child(a):
    import pydrt
    bundle = pydrt.load_scene(os.path.join(REPO, "scenes", "cornell_plane_light.scn"), a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    r = pydrt.Renderer(bundle, params)
    try:
        n = int(a.config[1:]) if a.config[0] in "bl" else 0
        if a.config[0] == "b":
            r.bind_buckets(n)
        elif a.config[0] == "l":
            r.bind_lobes(*lobe_binding(pydrt, n))
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
        print(json.dumps(out))
    finally:
        r.close()


def run_child(a, config):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--spp", str(a.spp), "--depth", str(a.depth), "--config", config]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("lobe_probe: the run of `%s` failed (%d)" % (config, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default="")
    ap.add_argument("--config", default="plain", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    configs = ["plain"] + [c for c in a.configs.split(",") if c != "plain"]
    if any(c not in CONFIGS for c in configs):
        raise SystemExit("lobe_probe: --configs takes %s" % ", ".join(CONFIGS))
    runs = {c: [] for c in configs}
    for rep in range(a.reps):
        for c in configs:
            runs[c].append(run_child(a, c))
            x = runs[c][-1]
            print("rep %d %-6s wall %8.2f ms  trace %8.2f  shade(+pass) %8.2f" % (rep, c, x["wall_ms"], x["trace_ms"], x["shade_ms"]), flush=True)
    med = {c: {k: statistics.median(x[k] for x in runs[c]) for k in ("wall_ms", "trace_ms", "shade_ms")} for c in configs}
    pass_ms = {c: med[c]["shade_ms"] - med["plain"]["shade_ms"] for c in configs if c != "plain"}
    out = {"size": a.size, "spp": a.spp, "depth": a.depth, "reps": a.reps,
           "runs": [{"config": c, **med[c], "wall_all_ms": [x["wall_ms"] for x in runs[c]], "shade_all_ms": [x["shade_ms"] for x in runs[c]]} for c in configs],
           "pass_ms": pass_ms,
           "lobes_over_buckets_ms": {str(n): pass_ms["l%d" % n] - pass_ms["b%d" % n] for n in COUNTS if "l%d" % n in pass_ms and "b%d" % n in pass_ms},
           "spread_ms": {c: max(x["shade_ms"] for x in runs[c]) - min(x["shade_ms"] for x in runs[c]) for c in configs},
           "wall_over_plain_ms": {c: med[c]["wall_ms"] - med["plain"]["wall_ms"] for c in configs if c != "plain"}}
    print("shade kernel %.2f ms per frame; the pass on top of it: %s; lobes minus buckets at the same count: %s" %
          (med["plain"]["shade_ms"], {k: round(v, 2) for k, v in pass_ms.items()}, {k: round(v, 2) for k, v in out["lobes_over_buckets_ms"].items()}))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
