"""Occupancy of the dense shade instantiations, from the compiler's own metadata (tools/kernel_resources.py).

The shade kernel's main pass has straight-line bodies for mirror, glass and smooth-conductor vertices (csrc/drt_kernels.h,
fixed_vertex). The kernel lives on its waves per SIMD -- it is bound by what a wave issues, and the other waves are what hides a
wave's waits -- so code added to it must not cost a wave, and must not push a vector register into scratch memory: a build that
looks faster in one run with a wave less is wrong. tests/test_kernel_spill_budget.py holds the scalar spills and the scratch bytes of
the same three kernels; this file holds their waves per SIMD and their vector spills.

Needs hipcc (cross-compiles without a GPU); skipped where it is absent.
"""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel (dense instantiation): waves per SIMD
WAVES = {
    "drt_shade_kernel<1, true, false, true, false, false>": 4,   # headline
    "drt_shade_kernel<1, true, false, false, false, false>": 4,
    "drt_shade_kernel<1, true, false, true, true, false>": 5,    # SIMPLE, config 3
}


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


@pytest.mark.parametrize("kernel", sorted(WAVES))
def test_waves_per_simd_and_no_vector_spill(stats, kernel):
    assert kernel in stats, "no such kernel in the build: %s" % kernel
    r = stats[kernel]
    print("%s: occupancy %s, %d VGPRs, %d VGPR spills, %d SGPR spills, %d B scratch" % (
        kernel, r["occupancy"], r["vgprs"], r["vgpr_spill_count"], r["sgpr_spill_count"], r["scratch"]))
    assert r["occupancy"] == WAVES[kernel], "%s runs %s waves per SIMD, not %d" % (kernel, r["occupancy"], WAVES[kernel])
    assert r["vgpr_spill_count"] == 0, "%s spills %d vector registers" % (kernel, r["vgpr_spill_count"])


def test_the_switch_is_one_scalar_of_the_launch_parameters():
    """DRT_NO_FIXED_LISTS is read once, where the context is created, and travels in ShadeParams: no getenv per launch, no second
    set of shade instantiations"""
    launcher = open(os.path.join(REPO, "daily-ray-trace_amd", "csrc", "drt_launcher.hip")).read()
    kernels = open(os.path.join(REPO, "daily-ray-trace_amd", "csrc", "drt_kernels.h")).read()
    assert launcher.count('getenv("DRT_NO_FIXED_LISTS")') == 1
    create = launcher.index('getenv("DRT_NO_SIMPLE_SHADE")')
    assert abs(launcher.index('getenv("DRT_NO_FIXED_LISTS")') - create) < 400, "read beside DRT_NO_SIMPLE_SHADE, at context creation"
    assert "no_fixed_lists" in kernels[kernels.index("struct ShadeParams"):kernels.index("word_as_double")]
