#!/usr/bin/env python3
"""What depth-cut films cost (drt_bind_depth_cuts), beside the only thing there was before them: one render per depth.

    python3 tools/depth_cut_probe.py [--size 1024] [--spp 256] [--depth 8] [--reps 3] [--out FILE]

One process per configuration and run: the parent opens no device and starts the configurations one after the other, --reps rounds
over all of them, so the runs of two configurations alternate. A child creates its context (DRT_BATCH_RESIDENT), binds its cuts,
renders the frame once to warm up (code objects, the pool measurement), resets the film and renders it once more, timed: the wall time
from the call to the end of drt_synchronize, and the trace and shade + cut-pass times of its kernel pairs by HIP events (drt_stats).

The configurations, on cornell_plane_light.scn at --size^2 x --spp:
    depth d, no cuts, for d = 1 .. --depth    (the frame a caller renders once per depth today)
    depth --depth with cuts 1 .. min(--depth, 8); with cuts {1, --depth}; with cuts {1}; with cuts {1, 2, 3}
and from their medians:
    (b) one render with cuts 1..8 against the sum of the renders at depths 1..8
    (c) one render with cuts {1, D} against the renders at depths 1 and D
    (d) the cut pass per frame for 1, 3 and 8 cuts: shade_ms with the cuts bound minus shade_ms without, beside the shade kernel's
Prints its lines and one JSON line (also written to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "daily-ray-trace_amd"))


def child(a):
    import pydrt
    cuts = [int(c) for c in a.cuts.split(",")] if a.cuts else []
    bundle = pydrt.load_scene(os.path.join(REPO, "scenes", "cornell_plane_light.scn"), a.size, a.size)
    params = pydrt.make_params(a.size, a.size, spp=a.spp, max_depth=a.depth, seed=1, batch_spp=pydrt.BATCH_RESIDENT)
    r = pydrt.Renderer(bundle, params)
    try:
        if cuts:
            r.bind_depth_cuts(cuts)
        r.render()
        r.synchronize()
        r.reset_film()
        t0 = time.perf_counter()
        r.render()
        r.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        st = r.stats()
        assert st.paths == a.size * a.size * a.spp and st.redone_launches == 0
        print(json.dumps({"depth": a.depth, "cuts": cuts, "wall_ms": wall, "trace_ms": st.trace_ms, "shade_ms": st.shade_ms, "launches": st.launches}))
    finally:
        r.close()


def run_child(a, depth, cuts):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--spp", str(a.spp), "--depth", str(depth),
           "--cuts", ",".join(str(c) for c in cuts)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("depth_cut_probe: the run at depth %d with cuts %s failed (%d)" % (depth, cuts, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--cuts", default="", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    D = a.depth
    all_cuts = tuple(range(1, min(D, 8) + 1))
    configs = [(d, ()) for d in range(1, D + 1)] + [(D, all_cuts), (D, tuple(sorted({1, D}))), (D, (1,)), (D, tuple(c for c in (1, 2, 3) if c <= D))]
    configs = list(dict.fromkeys(configs))
    runs = {c: [] for c in configs}
    for rep in range(a.reps):
        for c in configs:
            runs[c].append(run_child(a, *c))
            print("rep %d depth %d cuts %-22s wall %8.2f ms  trace %8.2f  shade(+cuts) %8.2f" % (rep, c[0], list(c[1]), runs[c][-1]["wall_ms"], runs[c][-1]["trace_ms"],
                                                                                         runs[c][-1]["shade_ms"]), flush=True)
    med = {c: {k: statistics.median(x[k] for x in runs[c]) for k in ("wall_ms", "trace_ms", "shade_ms")} for c in configs}
    spread = {c: [min(x["wall_ms"] for x in runs[c]), max(x["wall_ms"] for x in runs[c])] for c in configs}
    plain = med[(D, ())]
    out = {"size": a.size, "spp": a.spp, "depth": D, "reps": a.reps,
           "runs": [{"depth": c[0], "cuts": list(c[1]), **med[c], "wall_min_max_ms": spread[c]} for c in configs],
           "b_cuts_all_wall_ms": med[(D, all_cuts)]["wall_ms"], "b_renders_sum_wall_ms": sum(med[(d, ())]["wall_ms"] for d in all_cuts),
           "c_cuts_1_D_wall_ms": med[(D, tuple(sorted({1, D})))]["wall_ms"], "c_renders_1_D_wall_ms": sum(med[(d, ())]["wall_ms"] for d in sorted({1, D})),
           "d_shade_ms": plain["shade_ms"],
           "d_cut_pass_ms": {str(len(c[1])): med[c]["shade_ms"] - plain["shade_ms"] for c in configs if c[1] and c[1] != tuple(sorted({1, D}))}}
    print("(b) cuts %s in one render: %.2f ms wall; the renders at those depths one by one: %.2f ms" % (list(all_cuts), out["b_cuts_all_wall_ms"], out["b_renders_sum_wall_ms"]))
    print("(c) cuts [1, %d] in one render: %.2f ms wall; the renders at depths 1 and %d: %.2f ms" % (D, out["c_cuts_1_D_wall_ms"], D, out["c_renders_1_D_wall_ms"]))
    print("(d) shade kernel %.2f ms per frame; the cut pass by number of cuts: %s" % (out["d_shade_ms"], {k: round(v, 2) for k, v in out["d_cut_pass_ms"].items()}))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
