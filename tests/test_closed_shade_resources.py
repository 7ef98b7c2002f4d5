"""CPU: what the closed shade kernel's form with headers in LDS needs to keep five waves on a SIMD -- registers, from the compiler's own metadata, and LDS, from
the launcher's rule (csrc/drt_shade_lds_rule.h).

Registers (needs hipcc, which cross-compiles without a GPU; skipped where it is absent): both instantiations of
drt_shade_kernel_closed_lds are allocated at most 96 vector registers (the 88-96 step of gfx950's register file: five waves per SIMD),
spill no vector register and use no scratch. tools/kernel_resources.py reads the figures; it compiles a file that includes the
kernels' header and instantiates these two kernels alone, with the library's flags -- seconds where the whole library takes minutes,
and the same figures (the kernels are templates of that header).

LDS: a wave per SIMD more is a workgroup per compute unit more, and every workgroup holds the SPD table. tests/host/
shade_lds_rule_main.cpp runs the rule as the launcher does; for the table of the headline scene and of config 4's (38 rows of 69:
the scene's 28 spectra, a diffuse / pi row per distinct diffuse spectrum, two rows per material with Fresnel functions, the zero row)
the closed form's region must leave room for five workgroups, the general form's must not be claimed to, and no table may ever be
given more workgroups than fit."""
import importlib.util
import os
import re
import subprocess

import pytest

import cases
import pydrt

CSRC = os.path.join(cases.REPO, "daily-ray-trace_amd", "csrc")
KERNELS = open(os.path.join(CSRC, "drt_kernels.h")).read()
CLOSED = ("drt_shade_kernel_closed_lds<true>", "drt_shade_kernel_closed_lds<false>")
ARGS = "DevScene, ShadeParams, const uint64_t *__restrict__, const uint64_t *__restrict__, double *__restrict__, double *__restrict__, double *__restrict__, unsigned long long *__restrict__"
LDS_PER_CU, SHADE_WAVES = 160 * 1024, 4


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(cases.REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def stats(tmp_path_factory):
    tool = _tool()
    if not os.path.exists(tool.HIPCC):
        pytest.skip("no hipcc on this machine")
    src = tmp_path_factory.mktemp("closed") / "closed_only.hip"
    src.write_text('#include "drt_kernels.h"\n' + "".join("template __global__ void %s(%s);\n" % (k, ARGS) for k in CLOSED))
    return tool.kernel_stats(source=str(src))


@pytest.mark.parametrize("kernel", CLOSED)
def test_five_waves_without_a_spill(stats, kernel):
    assert kernel in stats, sorted(stats)
    r = stats[kernel]
    print("%s: %d VGPRs, %d SGPR spills, %d VGPR spills, %d B scratch, occupancy %s" % (
        kernel, r["vgprs"], r["sgpr_spill_count"], r["vgpr_spill_count"], r["scratch"], r["occupancy"]))
    allocated = (r["vgprs"] + 7) // 8 * 8  # the hardware's granule is eight registers
    assert allocated <= 96, "%s: %d vector registers allocated" % (kernel, allocated)
    assert r["vgpr_spill_count"] == 0 and r["scratch"] == 0, "%s spills %d vector registers, %d bytes of scratch" % (kernel, r["vgpr_spill_count"], r["scratch"])
    assert r["occupancy"] == 5


def test_the_bound_asks_for_five_waves():
    assert re.search(r"#define DRT_SHADE_CLOSED_LDS_HEADERS 1\n", KERNELS)
    assert re.search(r"#ifndef DRT_SHADE_WAVES_CLOSED_LDS\n#define DRT_SHADE_WAVES_CLOSED_LDS 5\n", KERNELS)
    assert "__launch_bounds__(SHADE_BLOCK, DRT_SHADE_WAVES_CLOSED_LDS) void drt_shade_kernel_closed_lds(" in KERNELS


# ---- the LDS rule ----

def macro(name):
    return int(re.search(r"#define %s (\d+)u" % name, KERNELS).group(1))


def closed_wave_words():
    """SHADE_CLOSED_WAVE_LDS_WORDS, from the header's own defines (SHADE_PREFETCH_REGS is 2)"""
    regs = int(re.search(r"#define SHADE_PREFETCH_REGS (\d+)", KERNELS).group(1))
    assert "#define SHADE_CLOSED_SLOT_WORDS (64u * SHADE_PREFETCH_REGS)" in KERNELS
    assert "#define SHADE_CLOSED_HDR01_AT SHADE_CLOSED_SLOT_WORDS" in KERNELS
    assert "#define SHADE_CLOSED_HDR2_AT (SHADE_CLOSED_HDR01_AT + 128u)" in KERNELS
    assert "#define SHADE_CLOSED_WAVE_LDS_WORDS (SHADE_CLOSED_HDR2_AT + 64u)" in KERNELS
    return 64 * regs + 128 + 64


def general_wave_words():
    """SHADE_WAVE_LDS_WORDS: the larger of two record slots and the tail pass's window"""
    entries = macro("TAIL_WINDOW_ENTRIES")
    regs = int(re.search(r"#define SHADE_PREFETCH_REGS (\d+)", KERNELS).group(1))
    return max(2 * 64 * regs, 3 * entries + entries // 4)


def device_spd_rows(bundle):
    """rows of the table the launcher uploads (build_device_scene): the scene's, a diffuse / pi row per distinct diffuse spectrum, two
    rows per material whose list holds dielectric or conductor Fresnel functions (not both), the all-zero row"""
    dielectric = ("fs_dielectric_reflectance_bdsf", "fs_dielectric_transmittance_bdsf")
    conductor = ("fs_conductor_bdsf", "ct_conductor_bdsf")
    mats = bundle.materials()
    rows = bundle.spds().shape[0] + len({m.diffuse_spd for m in mats if m.diffuse_spd >= 0}) + 1
    for m in mats:
        names = [pydrt.BDSF_NAMES[m.bdsfs[j]] for j in range(int(m.num_bdsfs))]
        d, c = any(n in dielectric for n in names), any(n in conductor for n in names)
        rows += 2 * int(d != c)
    return rows


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ldsrule") / "shade_lds_rule_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + CSRC, os.path.join(cases.REPO, "tests", "host", "shade_lds_rule_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def plans(rule_program, lines):
    text = "".join(" ".join(str(int(v)) for v in line) + "\n" for line in lines)
    r = subprocess.run([rule_program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    names = ("table_bytes", "wave_bytes", "group_bytes", "granted_bytes", "groups_by_lds", "groups", "waves_per_simd")
    out = [dict(zip(names, (int(v) for v in row.split()))) for row in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("scene", ["cornell_plane_light.scn", "cornell_gold_mirror.scn"])  # the headline's and config 4's
def test_five_workgroups_fit_beside_the_benchmark_scenes_table(rule_program, scene):
    bundle = pydrt.load_scene(cases.scene_path(scene), 64, 64)
    n_spd, S = device_spd_rows(bundle), bundle.S
    closed, general = plans(rule_program, [(n_spd, S, 1, SHADE_WAVES, closed_wave_words(), 5), (n_spd, S, 1, SHADE_WAVES, general_wave_words(), 5)])
    print("%s: table %d x %d; closed region: %s; general region at the same register bound: %s" % (scene, n_spd, S, closed, general))
    assert closed["table_bytes"] == n_spd * S * 8 and closed["group_bytes"] == closed["table_bytes"] + SHADE_WAVES * closed_wave_words() * 8
    assert closed["groups"] == 5 and closed["waves_per_simd"] == 5
    # what step 0 found: with the general form's regions a fifth workgroup does not fit, whatever the registers allow
    assert general["groups_by_lds"] == 4 and general["waves_per_simd"] == 4


def test_never_more_workgroups_than_lds_holds(rule_program):
    S = 69
    rows = list(range(1, 120)) + [200, 296]
    for words in (closed_wave_words(), general_wave_words()):
        got = plans(rule_program, [(n, S, 1, SHADE_WAVES, words, 5) for n in rows])
        for n, p in zip(rows, got):
            assert p["group_bytes"] == n * S * 8 + SHADE_WAVES * words * 8 and p["granted_bytes"] >= p["group_bytes"]
            assert p["groups"] <= 5 and p["groups"] * p["granted_bytes"] <= LDS_PER_CU, (n, p)
            assert p["groups"] == min(5, LDS_PER_CU // p["granted_bytes"]) and p["waves_per_simd"] == p["groups"]
        assert got[0]["groups"] == 5 and got[-1]["groups"] == 0  # a table of 296 rows does not fit at all
        fits = [n for n, p in zip(rows, got) if p["groups"] == 5]
        assert fits == list(range(1, fits[-1] + 1)), "fewer workgroups from some table size on, never more again"
    # the table read from memory: only the waves' regions count
    (p,) = plans(rule_program, [(38, S, 0, SHADE_WAVES, closed_wave_words(), 4)])
    assert p["table_bytes"] == 0 and p["groups"] == 4 and p["groups_by_lds"] >= 5
