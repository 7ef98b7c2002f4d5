"""What the trace kernel's path loop waits for on the vector-memory counter, from the compiler's own output
(tools/kernel_resources.py --waits).

gfx9 has one vmcnt, counted in order for loads and stores alike: an `s_waitcnt vmcnt(0)` in front of a loaded value also waits for
every record store issued before the load. The path loop stores a light record, a vertex record, a header and the tail stage per
iteration, every lane to lines of its own, so a load behind them -- of a word the lane stored itself, or of a spilled register -- costs
the stores' round trip. The loop therefore loads nothing from global memory (the vignette stays in LDS, csrc/drt_kernels.h), and what
it keeps per lane beyond its registers it keeps in LDS lane rows (TRACE_LW_*), which have a counter of their own. This test holds
that: no global load in the loop, and the loop's spill reloads and vmcnt waits at what the tree compiles to, below the figures of the
tree before (TRACE_BEFORE, taken with the same tool). What is left is the three atomics of the work and pool queues, whose values
the wave needs, and reloads in branches the shipped scenes do not take (the table block of paths beyond 12 vertices, pow()'s
constants for a shininess that is no integer).

Needs hipcc (cross-compiles without a GPU); skipped where it is absent.
"""
import importlib.util
import os

import pytest

import test_kernel_spill_budget as SB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TTF = "drt_trace_kernel<true, true, false>"    # headline, configs 3 and 4
TFF = "drt_trace_kernel<true, false, false>"
# inside the path loop: (global loads, scratch loads, s_waitcnt with a vmcnt field)
TRACE_BEFORE = {TTF: (1, 21, 26), TFF: (0, 17, 20)}  # the tree before: the hdr[1] reload, the media indices, blk, the power's exponent
CEILING = {TTF: (0, 10, 13), TFF: (0, 6, 9)}
REGISTERS, WAVES_PER_SIMD = 168, 3


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


def path_loop(r):
    """(global loads, scratch loads, vmcnt waits) of the kernel's persistent loop: the outermost loop with the most instructions"""
    lp = r["loops"][r["main_loop"]]
    other = sum(n for k, n in lp["loads"].items() if k.endswith("_load") and k != "scratch_load")
    return other, lp["loads"].get("scratch_load", 0), lp["vmcnt_waits"]


def test_ceilings_are_below_the_tree_before():
    for name, before in TRACE_BEFORE.items():
        g, s, w = CEILING[name]
        assert g == 0 and s < before[1] and w < before[2], name


@pytest.mark.parametrize("kernel", sorted(CEILING))
def test_the_path_loop_loads_nothing_back(stats, kernel):
    r = stats[kernel]
    lp = r["loops"][r["main_loop"]]
    assert lp["insts"] > 2000, "%s: the loop found is not the path loop (%d instructions)" % (kernel, lp["insts"])
    g, s, w = path_loop(r)
    print("%s: loop %s, %d instructions: %d global loads, %d scratch loads (ceiling %d), %d vmcnt waits (ceiling %d)" % (
        kernel, r["main_loop"], lp["insts"], g, s, CEILING[kernel][1], w, CEILING[kernel][2]))
    for n, before, src in lp["waits"]:
        print("    vmcnt(%d) behind %-18s %s" % (n, before, src))
    assert g == 0, "%s: %d loads from global memory inside the path loop: %s" % (kernel, g, lp["loads"])
    assert s <= CEILING[kernel][1], "%s: %d spill reloads inside the path loop, ceiling %d" % (kernel, s, CEILING[kernel][1])
    assert w <= CEILING[kernel][2], "%s: %d vmcnt waits inside the path loop, ceiling %d" % (kernel, w, CEILING[kernel][2])
    assert lp["loads"].get("global_atomic_ret", 0) == 3  # the work queue's chunk and the pool's two chunks: values the wave needs


@pytest.mark.parametrize("kernel", sorted(CEILING))
def test_budgets(stats, kernel):
    r = stats[kernel]
    sgpr_max, scratch_max = SB.BUDGET[kernel]
    assert r["vgprs"] <= REGISTERS and r["occupancy"] >= WAVES_PER_SIMD, "%s: %d registers, %s waves per SIMD" % (kernel, r["vgprs"], r["occupancy"])
    assert r["sgpr_spill_count"] <= sgpr_max and r["scratch"] <= scratch_max, (kernel, r["sgpr_spill_count"], r["scratch"])


LISTING = """
_Z1kv:
; %bb.0:
	global_load_dword v1, v0, s[0:1]
	s_waitcnt vmcnt(0)
.LBB0_1:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_2 Depth 2
	.loc	2 10 5                          ; csrc/a.h:10:5
	global_store_dwordx2 v[2:3], v[4:5], off
	scratch_load_dword v6, off, off offset:4 ; 4-byte Folded Reload
	s_waitcnt vmcnt(0) lgkmcnt(0)
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
	.loc	2 12 9                          ; csrc/a.h:12:9
	global_atomic_add_x2 v[8:9], v1, v[8:9], s[2:3] sc0
	s_waitcnt vmcnt(0)
	s_waitcnt lgkmcnt(0)
	s_cbranch_execnz .LBB0_2
; %bb.3:                                ;   in Loop: Header=BB0_1 Depth=1
	global_store_dword v[2:3], v6, off
	s_waitcnt vmcnt(1)
	s_cbranch_execnz .LBB0_1
.LBB0_4:                                ; =>This Inner Loop Header: Depth=1
	global_load_dword v1, v0, s[0:1]
	s_waitcnt vmcnt(0)
	s_cbranch_execnz .LBB0_4
; %bb.5:
	scratch_load_dword v6, off, off offset:4 ; 4-byte Folded Reload
	s_waitcnt vmcnt(0)
	s_endpgm
"""


def test_the_listing_is_read_per_outermost_loop():
    """a hand-written listing: blocks of an inner loop belong to their depth-1 parent, code outside every loop is not counted, a wait
    names the kind of the vector-memory instruction before it and its source line, a wait without a vmcnt field is none"""
    loops, main = _tool()._wait_stats(LISTING.splitlines())
    assert sorted(loops) == ["BB0_1", "BB0_4"] and main == "BB0_1"
    a, b = loops["BB0_1"], loops["BB0_4"]
    assert a["loads"] == {"scratch_load": 1, "global_atomic_ret": 1} and a["vmcnt_waits"] == 3
    assert a["waits"] == [(0, "scratch_load", "a.h:10"), (0, "global_atomic_ret", "a.h:12"), (1, "global_store", "a.h:12")]
    assert b["loads"] == {"global_load": 1} and b["waits"] == [(0, "global_load", "a.h:12")]
