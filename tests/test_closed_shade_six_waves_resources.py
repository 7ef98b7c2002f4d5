"""CPU: what the closed shade kernel's six-wave form (drt_shade_kernel_closed_lds6) needs to keep six waves on a SIMD -- registers,
from the compiler's own metadata, and LDS, from the launcher's rule (csrc/drt_shade_lds_rule.h, shade_lds_plan_six) -- and that the
five-wave and four-wave closed kernels, its fallbacks, keep the figures they had.

Registers (needs hipcc, which cross-compiles without a GPU; skipped where it is absent): both instantiations of the new kernel are
allocated at most 80 vector registers (512 / 6 in the granule of eight), spill none and use no scratch. tools/kernel_resources.py
reads the figures from a file that instantiates the six closed kernels alone, with the library's flags.

LDS: three workgroups of eight waves, each with one copy of the table, must fit a compute unit beside the table of the headline scene
and of config 4 (38 rows of 69); tests/host/shade_lds_six_main.cpp runs the rule as the launcher does."""
import os
import re
import subprocess

import pytest

import cases
import pydrt
import test_closed_shade_resources as FIVE

SIX = ("drt_shade_kernel_closed_lds6<true>", "drt_shade_kernel_closed_lds6<false>")
# (VGPRs, scalar registers parked in vector lanes, spilled vector registers, scratch bytes, waves per SIMD): the fallbacks' figures
KEPT = {"drt_shade_kernel_closed_lds<true>": (92, 62, 0, 0, 5), "drt_shade_kernel_closed_lds<false>": (93, 54, 0, 0, 5),
        "drt_shade_kernel_closed<true>": (108, 65, 0, 0, 4), "drt_shade_kernel_closed<false>": (109, 61, 0, 0, 4)}
LDS_PER_CU, GRANULE, BLOCK_WAVES = 160 * 1024, 1280, 8


@pytest.fixture(scope="module")
def stats(tmp_path_factory):
    tool = FIVE._tool()
    if not os.path.exists(tool.HIPCC):
        pytest.skip("no hipcc on this machine")
    src = tmp_path_factory.mktemp("six") / "closed_six.hip"
    src.write_text('#include "drt_kernels.h"\n' + "".join("template __global__ void %s(%s);\n" % (k, FIVE.ARGS) for k in SIX + tuple(KEPT)))
    return tool.kernel_stats(source=str(src))


@pytest.mark.parametrize("kernel", SIX)
def test_six_waves_without_a_spill(stats, kernel):
    assert kernel in stats, sorted(stats)
    r = stats[kernel]
    print("%s: %d VGPRs, %d SGPR spills, %d VGPR spills, %d B scratch, occupancy %s" % (
        kernel, r["vgprs"], r["sgpr_spill_count"], r["vgpr_spill_count"], r["scratch"], r["occupancy"]))
    assert r["vgprs"] <= 80, "%s: %d vector registers" % (kernel, r["vgprs"])
    assert r["vgpr_spill_count"] == 0 and r["scratch"] == 0, "%s spills %d vector registers, %d bytes of scratch" % (kernel, r["vgpr_spill_count"], r["scratch"])
    assert r["occupancy"] == 6


@pytest.mark.parametrize("kernel", sorted(KEPT))
def test_the_fallbacks_keep_their_figures(stats, kernel):
    r = stats[kernel]
    got = (r["vgprs"], r["sgpr_spill_count"], r["vgpr_spill_count"], r["scratch"], r["occupancy"])
    assert got == KEPT[kernel], "%s: (VGPRs, scalar spills, vector spills, scratch, waves) = %s, were %s" % (kernel, got, KEPT[kernel])


def test_the_bound_asks_for_six_waves_of_512_lanes():
    k = FIVE.KERNELS
    assert re.search(r"#define SHADE_BLOCK_CLOSED_LDS6 512\n", k)
    assert re.search(r"#ifndef DRT_SHADE_WAVES_CLOSED_LDS6\n#define DRT_SHADE_WAVES_CLOSED_LDS6 6\n", k)
    assert "__launch_bounds__(SHADE_BLOCK_CLOSED_LDS6, DRT_SHADE_WAVES_CLOSED_LDS6) void drt_shade_kernel_closed_lds6(" in k
    rule = open(os.path.join(FIVE.CSRC, "drt_shade_lds_rule.h")).read()
    assert "#define SHADE_LDS_SIX_BLOCK_WAVES 8u" in rule and "#define SHADE_LDS_SIX_WAVES_PER_SIMD 6u" in rule


# ---- the LDS rule ----

rule_program = FIVE.rule_program  # (the five-wave test's host program, for the comparison with four-wave workgroups)

@pytest.fixture(scope="module")
def six_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ldssix") / "shade_lds_six_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + FIVE.CSRC, os.path.join(cases.REPO, "tests", "host", "shade_lds_six_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def six_plans(program, lines):
    text = "".join(" ".join(str(int(v)) for v in line) + "\n" for line in lines)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    names = ("table_bytes", "wave_bytes", "group_bytes", "granted_bytes", "groups_by_lds", "groups", "waves_per_simd", "fits")
    out = [dict(zip(names, (int(v) for v in row.split()))) for row in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("scene", ["cornell_plane_light.scn", "cornell_gold_mirror.scn"])  # the headline's and config 4's
def test_three_workgroups_fit_beside_the_benchmark_scenes_table(six_program, rule_program, scene):
    bundle = pydrt.load_scene(cases.scene_path(scene), 64, 64)
    n_spd, S, words = FIVE.device_spd_rows(bundle), bundle.S, FIVE.closed_wave_words()
    (p,) = six_plans(six_program, [(n_spd, S, 1, words)])
    print("%s: table %d x %d; six-wave shape: %s" % (scene, n_spd, S, p))
    assert (n_spd, S) == (38, 69)
    assert p["table_bytes"] == 20976 and p["group_bytes"] == 20976 + BLOCK_WAVES * 2560 == 41456
    assert p["granted_bytes"] == 33 * GRANULE and 3 * p["granted_bytes"] <= LDS_PER_CU
    assert p["groups"] == 3 and p["waves_per_simd"] == 6 and p["fits"] == 1
    # ... where a sixth workgroup of four waves, each with a table of its own, does not
    (q,) = FIVE.plans(rule_program, [(n_spd, S, 1, FIVE.SHADE_WAVES, words, 6)])
    assert q["groups_by_lds"] == 5 and q["waves_per_simd"] == 5



def test_never_more_workgroups_than_lds_holds(six_program):
    S, words = 69, FIVE.closed_wave_words()
    rows = list(range(1, 120)) + [200, 296]
    got = six_plans(six_program, [(n, S, 1, words) for n in rows])
    for n, p in zip(rows, got):
        assert p["group_bytes"] == n * S * 8 + BLOCK_WAVES * words * 8 and p["granted_bytes"] >= p["group_bytes"] and p["granted_bytes"] % GRANULE == 0
        assert p["groups"] == min(3, LDS_PER_CU // p["granted_bytes"]) and p["groups"] * p["granted_bytes"] <= LDS_PER_CU, (n, p)
        assert p["waves_per_simd"] == 2 * p["groups"] and p["fits"] == int(p["groups"] == 3)
    assert got[0]["fits"] == 1 and got[-1]["groups"] == 0
    fits = [n for n, p in zip(rows, got) if p["fits"]]
    assert fits == list(range(1, fits[-1] + 1)) and fits[-1] >= 38, "fewer workgroups from some table size on, never more again"
    # the table read from memory: only the waves' regions count
    (p,) = six_plans(six_program, [(38, S, 0, words)])
    assert p["table_bytes"] == 0 and p["groups"] == 3 and p["groups_by_lds"] >= 3
