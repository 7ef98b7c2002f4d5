#!/usr/bin/env python3
"""Per-kernel register / spill / scratch / occupancy figures of libdrt_hip.so's kernels, from the compiler's own output: the device
assembly of csrc/drt_launcher.hip (the Makefile's flags plus -S -gline-tables-only) and the kernel metadata at its end. Extra
arguments are passed on (e.g. -DSHADE_PREFETCH_DEPTH=3).   python3 tools/kernel_resources.py [filter substring | group] [--loops] [--waits] [--asm=FILE] [-D...]
A filter that names a group (GROUPS below: `features`, `mattes`, `rays`, `rayfilm`, `closed`, `trace`, `update`, `build`, `material`) stands for the group's kernels.

Columns: VGPRs, SGPRs, `sspill` / `vspill` = the metadata's .sgpr_spill_count / .vgpr_spill_count, scratch bytes per lane, static
LDS, occupancy (waves per SIMD, from the VGPR count), `valu` = vector ALU instructions in the kernel's text, `lanemv` = how many of
them are SPILL LANE MOVES. On gfx9 a spilled scalar register is parked in a lane of a reserved vector register: v_writelane_b32
stores it, v_readlane_b32 with a constant lane brings it back, and both issue in the vector pipe. Counted are every v_writelane_b32,
and every v_readlane_b32 with a constant lane whose source is a register some v_writelane_b32 of the kernel writes (a kernel's own
v_readlane with a variable lane, or on a register it never writes lanes of, is its algorithm and not a spill).
--loops adds, per kernel, both counts by loop depth as the assembly's loop annotations nest the basic blocks.

--waits adds, per kernel and per OUTERMOST loop (named by its header's label; `main` marks the one with the most instructions, a
persistent kernel's path loop), what the loop waits for on the vector-memory counter: its vector-memory loads by kind (global_load,
scratch_load, ...; atomics that return a value are listed apart), and every s_waitcnt with a vmcnt field, with the kind of the
vector-memory instruction that stands before it in the text and the source line the wait belongs to. gfx9 has ONE vmcnt, counted in
order for loads and stores alike, so a wait for a loaded value also waits for every store issued before the load: a reload behind a
burst of record stores costs the stores' round trip. --asm=FILE reads a saved listing instead of compiling."""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "daily-ray-trace_amd")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
# the Makefile's HIPFLAGS (warnings aside)
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=c++17", "-I" + os.path.join(REPO, "include")]

# a filter word that is a key here selects the kernels whose names hold one of the substrings
GROUPS = {"features": ("drt_feature_kernel", "drt_feature_bvh_kernel", "drt_feature_counts_kernel", "drt_feature_bgra_kernel"),
          "mattes": ("drt_matte_kernel", "drt_matte_bvh_kernel", "drt_matte_select_kernel", "drt_matte_bgra_kernel"),
          "rays": ("drt_ray_closest_kernel", "drt_ray_visible_kernel", "drt_ray_closest_bvh_kernel", "drt_ray_visible_bvh_kernel"),
          # the ray-mode entry points of the render path (drt_bind_rays) and the camera twins they share their bodies with
          "rayfilm": ("drt_trace_rays_kernel", "drt_primary_rays_kernel", "drt_bounce_rays_kernel", "drt_trace_kernel", "drt_primary_kernel",
                      "drt_bounce_kernel"),
          # the closed shade kernel's three forms: four waves, five (headers in LDS), six (512-lane workgroups)
          "closed": ("drt_shade_kernel_closed<", "drt_shade_kernel_closed_lds<", "drt_shade_kernel_closed_lds6<"),
          # the trace kernel's two forms: drt_trace_kernel starts paths from its ray stash, drt_trace_direct_kernel in the idle lane
          "trace": ("drt_trace_kernel", "drt_trace_direct_kernel"),
          # scene updates (drt_update_surfaces, drt_set_camera)
          "update": ("drt_surface_derive_kernel", "drt_bvh_leaf_kernel", "drt_bvh_refit_kernel"),
          # device hierarchy builds (drt_rebuild_hierarchy)
          "build": ("drt_build_init_kernel", "drt_build_bounds_kernel", "drt_build_keys_kernel", "drt_build_count_kernel", "drt_build_scan_kernel",
                    "drt_build_scatter_kernel", "drt_build_topology_kernel", "drt_build_refit_kernel"),
          # material updates (drt_update_spectra, drt_update_materials)
          "material": ("drt_spectra_derive_kernel", "drt_spectra_finish_kernel")}

# vector ALU mnemonics: v_* except the few that are not issued to the VALU
_NOT_VALU = ("v_nop", "v_interp")


def device_asm(extra=(), source=None):
    """The gfx950 assembly of csrc/drt_launcher.hip as text; `source`: of that file instead (one that includes the kernels' headers and
    instantiates a few of them compiles in seconds where the whole library takes minutes)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "drt.s")
        src = source or os.path.join(PKG, "csrc", "drt_launcher.hip")
        cmd = [HIPCC] + FLAGS + ["-I" + os.path.join(PKG, "csrc"), "--cuda-device-only", "-S", "-gline-tables-only", src, "-o", out] + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + r.stderr[-4000:])
        return open(out, encoding="utf-8", errors="replace").read()


def _demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    plain = r.stdout.splitlines() if r.returncode == 0 else list(names)
    return {m: p.split("(")[0].replace("void ", "") for m, p in zip(names, plain)}


def _metadata(asm):
    """{mangled name: {field: value}} from the .amdhsa.kernels list of the amdgpu_metadata block."""
    kernels, cur = {}, None
    start = asm.find("amdhsa.kernels:")
    if start < 0:
        return kernels
    fields = {}
    for line in asm[start:].splitlines()[1:]:
        if line.startswith("amdhsa.") or line.startswith("..."):
            break
        m = re.match(r"^  - (\.\w+):\s*(.*)$", line)  # first key of a kernel's map
        if m:
            if fields.get(".name"):
                kernels[fields[".name"]] = fields
            fields = {m.group(1): m.group(2).strip()}
            continue
        m = re.match(r"^    (\.\w+):\s*(.*)$", line)
        if m:
            fields[m.group(1)] = m.group(2).strip().strip("'")
    if fields.get(".name"):
        kernels[fields[".name"]] = fields
    return kernels


def _body_stats(body):
    """Vector-ALU instructions and spill lane moves of one kernel's text, in all and by loop depth."""
    depth, hdr = 0, None
    rows = []  # (depth, mnemonic, operands)
    for line in body:
        t = line.strip()
        if re.match(r"^\.?LBB\d+_\d+:", t) or re.match(r"^; %bb\.\d+", t):
            depth, hdr = 0, None  # a basic block: its loop annotations are on the label's line and the comment lines after it
        if t.startswith(";") or t.startswith(".LBB"):
            m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", t)
            if m:
                hdr = int(m.group(1))
                depth = hdr
            elif hdr is None:
                m = re.search(r"in Loop: Header=\S+ Depth=(\d+)", t)
                if m:
                    depth = int(m.group(1))
            continue
        m = re.match(r"^(v_\w+)\s*(.*?)(?:\s*;.*)?$", t)
        if m and not m.group(1).startswith(_NOT_VALU):
            rows.append((depth, m.group(1), m.group(2)))
    parked = set()
    for _, op, args in rows:
        if op == "v_writelane_b32":
            parked.add(args.split(",")[0].strip())
    valu, moves, writes, reads = {}, {}, 0, 0
    for d, op, args in rows:
        valu[d] = valu.get(d, 0) + 1
        a = [x.strip() for x in args.split(",")]
        spill = False
        if op == "v_writelane_b32":
            spill = True
            writes += 1
        elif op == "v_readlane_b32" and len(a) == 3 and a[1] in parked and re.fullmatch(r"\d+|0x[0-9a-fA-F]+", a[2]):
            spill = True
            reads += 1
        if spill:
            moves[d] = moves.get(d, 0) + 1
    return {"valu": sum(valu.values()), "lane_moves": writes + reads, "lane_writes": writes, "lane_reads": reads,
            "parked_in": sorted(parked, key=lambda r: int(r[1:]) if r[1:].isdigit() else 0),
            "by_depth": {d: (valu[d], moves.get(d, 0)) for d in sorted(valu)}}


_VMEM = re.compile(r"^(global|scratch|buffer|flat)_(load|store|atomic)")


def _wait_stats(body):
    """{outermost loop's header label: figures} for one kernel's text, and the label of the loop with the most instructions."""
    outer, src, last = None, "", None
    loops = {}
    for line in body:
        t = line.strip()
        m = re.match(r"^\.?L?(BB\d+_\d+):", t)
        if m or re.match(r"^; %bb\.\d+", t):
            outer = None  # a basic block: which loop it is in follows on the label's line and the comment lines after it
            label = m.group(1) if m else None
        if t.startswith(";") or t.startswith(".LBB"):
            if outer is None:  # the first annotation names the outermost loop: a parent of depth 1, else the block's own loop
                m = re.search(r"Parent Loop (BB\d+_\d+) Depth=1\b", t) or re.search(r"in Loop: Header=(BB\d+_\d+) Depth=1\b", t)
                if m:
                    outer = m.group(1)
                elif re.search(r"This (?:Inner )?Loop Header: Depth=1\b", t):
                    outer = label
            continue
        if t.startswith(".loc"):
            m = re.search(r";\s*(\S+?):(\d+):\d+", t)
            if m:
                src = "%s:%s" % (os.path.basename(m.group(1)), m.group(2))
            continue
        if not t or t.startswith("."):
            continue
        op = t.split()[0]
        m = _VMEM.match(op)
        kind = m.group(0) if m else None
        if kind and kind.endswith("atomic"):
            kind += "_ret" if re.search(r"\bsc0\b|\bglc\b", t) else ""
        if outer is not None:
            lp = loops.setdefault(outer, {"insts": 0, "loads": {}, "vmcnt_waits": 0, "waits": []})
            lp["insts"] += 1
            if kind and (kind.endswith("_load") or kind.endswith("_ret")):
                lp["loads"][kind] = lp["loads"].get(kind, 0) + 1
            m = re.match(r"^s_waitcnt\b.*\bvmcnt\((\d+)\)", t)
            if m:
                lp["vmcnt_waits"] += 1
                lp["waits"].append((int(m.group(1)), last or "-", src))
        if kind:
            last = kind
    main = max(loops, key=lambda k: loops[k]["insts"]) if loops else None
    return loops, main


def kernel_stats(extra=(), asm=None, source=None):
    """{demangled kernel name: figures}; see the module's docstring for what they are."""
    asm = asm if asm is not None else device_asm(extra, source)
    meta = _metadata(asm)
    lines = asm.splitlines()
    names = _demangle(list(meta))
    out = {}
    label = {}
    for n, l in enumerate(lines):
        if l.startswith("_Z") or l.startswith("drt_"):
            label.setdefault(l.split(":")[0], n)
    for mangled, md in meta.items():
        a = label.get(mangled)
        if a is None:
            continue
        b = a
        while b < len(lines) and not lines[b].startswith(".Lfunc_end") and ".amdhsa_kernel" not in lines[b]:
            b += 1
        body = lines[a + 1:b]
        st = _body_stats(body)
        st["loops"], st["main_loop"] = _wait_stats(body)
        occ = None
        for l in lines[b:b + 400]:
            m = re.search(r";\s*Occupancy:\s*(\d+)", l)
            if m:
                occ = int(m.group(1))
                break
        st.update({"vgprs": int(md.get(".vgpr_count", 0)), "sgprs": int(md.get(".sgpr_count", 0)),
                   "sgpr_spill_count": int(md.get(".sgpr_spill_count", 0)), "vgpr_spill_count": int(md.get(".vgpr_spill_count", 0)),
                   "scratch": int(md.get(".private_segment_fixed_size", 0)), "lds": int(md.get(".group_segment_fixed_size", 0)), "occupancy": occ})
        out[names[mangled]] = st
    return out


def main(argv):
    loops, waits = "--loops" in argv, "--waits" in argv
    saved = [a[len("--asm="):] for a in argv if a.startswith("--asm=")]
    argv = [a for a in argv if a not in ("--loops", "--waits") and not a.startswith("--asm=")]
    args = [a for a in argv if a.startswith("-")]
    flt = [s for a in argv if not a.startswith("-") for s in GROUPS.get(a, (a,))]
    rows = kernel_stats(args, asm=open(saved[0], encoding="utf-8", errors="replace").read() if saved else None)
    print("%-60s %5s %5s %6s %6s %7s %6s %4s %6s %6s" % ("kernel", "VGPRs", "SGPRs", "sspill", "vspill", "scratch", "LDS", "occ", "valu", "lanemv"))
    for name, r in rows.items():
        if flt and not any(f in name for f in flt):
            continue
        print("%-60s %5d %5d %6d %6d %7d %6d %4s %6d %6d" % (name[:60], r["vgprs"], r["sgprs"], r["sgpr_spill_count"], r["vgpr_spill_count"], r["scratch"],
                                                          r["lds"], r["occupancy"], r["valu"], r["lane_moves"]))
        if loops:
            print("    lane moves: %d v_writelane, %d v_readlane, parked in %s" % (r["lane_writes"], r["lane_reads"], " ".join(r["parked_in"]) or "-"))
            for d, (v, m) in r["by_depth"].items():
                print("    loop depth %d: %5d vector instructions, %4d spill lane moves" % (d, v, m))
        if waits:
            for hdr, lp in r["loops"].items():
                if not lp["loads"] and not lp["vmcnt_waits"]:
                    continue
                print("    loop %s%s: %d instructions; loads: %s; %d vmcnt waits" % (
                    hdr, " (main)" if hdr == r["main_loop"] else "", lp["insts"],
                    ", ".join("%d %s" % (n, k) for k, n in sorted(lp["loads"].items())) or "none", lp["vmcnt_waits"]))
                for n, before, src in lp["waits"]:
                    print("        vmcnt(%d) behind %-18s %s" % (n, before, src))


if __name__ == "__main__":
    main(sys.argv[1:])
