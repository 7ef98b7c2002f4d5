"""The shade kernel's closed instantiations, from the compiler's own metadata (tools/kernel_resources.py) and the launcher's text.

drt_shade_kernel_closed (csrc/drt_kernels.h) is the shade kernel without the general BDSF list, for scenes whose every list has
straight-line code. It ships at DRT_SHADE_WAVES_CLOSED waves per SIMD; at four waves that means no spilled vector register and no
scratch, like the dense general instantiations (tests/test_shade_fixed_lists_cpu.py). DRT_NO_CLOSED_SHADE is read once, where the
context is created.

Needs hipcc (cross-compiles without a GPU); skipped where it is absent.
"""
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLOSED = ("drt_shade_kernel_closed<true>", "drt_shade_kernel_closed<false>")  # <DARK>; the headline and config 4 run the first
WAVES = 4  # DRT_SHADE_WAVES_CLOSED as committed


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def stats():
    tool = _tool()
    if not os.path.exists(tool.HIPCC):
        pytest.skip("no hipcc on this machine")
    return tool.kernel_stats()


def _source(name):
    return open(os.path.join(REPO, "daily-ray-trace_amd", "csrc", name)).read()


def test_the_committed_bound():
    m = re.search(r"#ifndef DRT_SHADE_WAVES_CLOSED\n#define DRT_SHADE_WAVES_CLOSED (\d+)", _source("drt_kernels.h"))
    assert m and int(m.group(1)) == WAVES


@pytest.mark.parametrize("kernel", CLOSED)
def test_closed_instantiations_exist_at_the_committed_waves_without_a_vector_spill(stats, kernel):
    assert kernel in stats, "no such kernel in the build: %s" % kernel
    r = stats[kernel]
    print("%s: occupancy %s, %d VGPRs, %d VGPR spills, %d SGPR spills, %d B scratch" % (
        kernel, r["occupancy"], r["vgprs"], r["vgpr_spill_count"], r["sgpr_spill_count"], r["scratch"]))
    assert r["occupancy"] == WAVES, "%s runs %s waves per SIMD, not %d" % (kernel, r["occupancy"], WAVES)
    assert r["vgpr_spill_count"] == 0, "%s spills %d vector registers" % (kernel, r["vgpr_spill_count"])
    assert r["scratch"] == 0, "%s uses %d bytes of scratch per lane" % (kernel, r["scratch"])


def test_the_closed_text_is_leaner_than_the_general_one(stats):
    """what the instantiation is for: fewer registers and less text than the headline's general instantiation"""
    general = stats["drt_shade_kernel<1, true, false, true, false, false>"]
    closed = stats[CLOSED[0]]
    assert closed["vgprs"] < general["vgprs"] and closed["valu"] < general["valu"]
    assert closed["sgpr_spill_count"] <= general["sgpr_spill_count"]


def test_the_switch_is_read_once_at_context_creation():
    """DRT_NO_CLOSED_SHADE is read once, inside build_device_scene (which drt_create calls and nothing else), into the context; what
    decides the launch reads the context: no getenv per launch"""
    launcher = _source("drt_launcher.hip")
    assert launcher.count('getenv("DRT_NO_CLOSED_SHADE")') == 1
    start = launcher.index("static int build_device_scene(drt_context *ctx")
    end = launcher.index("\n}\n", start)  # the function's closing brace: the first one in column 0 after its head
    body = launcher[start:end]
    assert 'ctx->no_closed_shade = getenv("DRT_NO_CLOSED_SHADE")' in body and "ctx->closed_lists = closed_lists(" in body
    assert len(re.findall(r"\bbuild_device_scene\(ctx\b", launcher)) == 1, "called once (where the context is created)"
    decide = launcher[launcher.index("static bool shade_closed"):launcher.index("static int launch_shade_mode")]
    assert "no_closed_shade" in decide and "closed_lists" in decide and "getenv" not in decide


def test_a_shaded_material_without_a_list_is_refused_where_the_lists_are_checked():
    """closed_lists() looks at every surface's material: one that is no black body and lists nothing keeps the general instantiation
    (tests/test_gpu_closed_lists.py renders such a scene)"""
    launcher = _source("drt_launcher.hip")
    fn = launcher[launcher.index("static bool closed_lists("):launcher.index("static int build_device_scene(")]
    assert re.search(r"!mats\[smat\[i\]\]\.is_black_body\s*&&\s*mats\[smat\[i\]\]\.num_bdsfs\s*==\s*0u\)\s*return false", fn)
