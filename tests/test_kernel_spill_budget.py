"""Register-spill budget of the kernels the benchmark runs, from the compiler's own metadata (tools/kernel_resources.py).

A spilled SCALAR register costs vector instructions on gfx9 -- it is parked in a lane of a reserved vector register, written by
v_writelane_b32 and read back by v_readlane_b32 -- and both headline kernels are bound by vector issue. The trace kernels read their
launch constants where they use them instead of holding them in scalar registers across the path loop (csrc/drt_kernels.h,
TraceConst); this test keeps the spill counts and the scratch sizes from creeping back. The ceilings are what the tree compiles to.
For the trace kernels they are below what the kernels had while every argument was held in registers (159 / 119 scalar spills,
244 / 204 bytes of scratch); the shade and hierarchy kernels have not been put on that diet yet and carry their counts as they are.

Needs hipcc (cross-compiles without a GPU); skipped where it is absent.
"""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel (dense instantiation): (SGPR spills, scratch bytes per lane) -- ceilings
BUDGET = {
    "drt_trace_kernel<true, true, false>": (54, 128),   # headline, configs 3 and 4
    "drt_trace_kernel<true, false, false>": (49, 96),
    "drt_shade_kernel<1, true, false, true, false, false>": (96, 0),   # headline
    "drt_shade_kernel<1, true, false, false, false, false>": (88, 0),
    "drt_shade_kernel<1, true, false, true, true, false>": (78, 0),    # SIMPLE, config 3
    "drt_primary_kernel<false>": (66, 76),   # config 5
    "drt_bounce_kernel<false>": (130, 320),  # config 5
}
# what the trace kernels had with every launch constant held in scalar registers: the ceilings above must stay below / not above these
TRACE_BEFORE = {
    "drt_trace_kernel<true, true, false>": (159, 244),
    "drt_trace_kernel<true, false, false>": (119, 204),
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


def test_ceilings_are_below_the_register_held_form():
    for name, (sgpr_before, scratch_before) in TRACE_BEFORE.items():
        assert BUDGET[name][0] < sgpr_before and BUDGET[name][1] <= scratch_before, name


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_spills_within_budget(stats, kernel):
    assert kernel in stats, "no such kernel in the build: %s (has: %s)" % (kernel, ", ".join(sorted(k for k in stats if k.split("<")[0] == kernel.split("<")[0])))
    r = stats[kernel]
    sgpr_max, scratch_max = BUDGET[kernel]
    print("%s: %d SGPR spills (ceiling %d), %d B scratch (ceiling %d), %d spill lane moves of %d vector instructions" % (
        kernel, r["sgpr_spill_count"], sgpr_max, r["scratch"], scratch_max, r["lane_moves"], r["valu"]))
    assert r["sgpr_spill_count"] <= sgpr_max, "%s spills %d scalar registers, budget %d" % (kernel, r["sgpr_spill_count"], sgpr_max)
    assert r["scratch"] <= scratch_max, "%s uses %d bytes of scratch per lane, budget %d" % (kernel, r["scratch"], scratch_max)


def test_lane_moves_are_counted(stats):
    """the tool's count of spill lane moves agrees with the metadata: a kernel writes at least one lane per spilled scalar register
    and none when nothing is spilled"""
    for name in BUDGET:
        r = stats[name]
        if r["sgpr_spill_count"] == 0:
            assert r["lane_writes"] == 0, name
        else:
            assert r["lane_writes"] > 0 and r["lane_reads"] > 0, name
