"""No GPU: the rule of device hierarchy builds (drt_rebuild_hierarchy; csrc/drt_build_rule.h). The numpy
restatement (tests/hierarchy_rule.py) gives valid trees on every kind of input, at most 32 levels deep -- by the depth budget, which the
deep case shows by building without it; the C++ text the kernels compile gives the same trees on the host, under the address and
undefined-behaviour sanitizers (a stand-alone program: nothing is loaded into Python); and the header, the compiler and pydrt agree on
the new calls and the report."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import build_pass_cases as B
import cases
import hierarchy_cases as HC
import hierarchy_rule as R
import pydrt
import scene_update_cases as U


def _line(n):
    return [("sphere", (0.37 * k - 3.0, 1.0, -2.0), 0.2 + 0.001 * k) for k in range(n)]


def _rows(name):
    if name.startswith("m"):
        rng = np.random.default_rng(int(name[1:]) + 5)
        return HC.sphere_rows([("sphere", tuple(rng.uniform(-4.0, 4.0, 3)), 0.5) for _ in range(int(name[1:]))])
    if name == "coincident_300":
        return HC.sphere_rows(HC.coincident_spheres())
    if name == "line_40":
        return HC.sphere_rows(_line(40))
    if name == "deep_64":
        return HC.sphere_rows(HC.deep_spheres())
    if name == "unbounded_plane":  # parallel_edges' scene before its update: the last plane's edge vectors are parallel
        return pydrt.surface_rows(U.load("parallel_edges")["after"])
    if name in SCENE_INPUTS:
        return pydrt.surface_rows(HC.load(name)["after"])
    return pydrt.surface_rows(U.load(name)["before"])


# the scenes tests/test_gpu_hierarchy.py builds past one tile, one block and one wave, and the key sets of tests/test_gpu_build_passes.py
SCENE_INPUTS = [n for n in HC.OWN if n not in ("coincident_300", "deep_64")]
KEY_INPUTS = B.TOPOLOGY_NAMES
SIZES = {"m0": 0, "m1": 1, "m2": 2, "m3": 3, "coincident_300": 300, "line_40": 40, "deep_64": 64, "three_spheres": 3, "four_spheres": 4, "five_spheres": 5,
         "spheres_1024": 1025, "spheres_2049": 2050, "spheres_4097": 4098, "lattice_5000": 5001, "planes_first": 270, "planes_last_only_bounded": 133,
         "spheres_20000": 20001, "comb": 129, "deep_blob": 4096 + 18, "deep_blob_19": 4096 + 19}  # (the sphere scenes have their plane light)
INPUTS = ["m0", "m1", "m2", "m3", "coincident_300", "line_40", "unbounded_plane", "deep_64", "spheres_96", "lights_all_bvh"] + SCENE_INPUTS + KEY_INPUTS
_trees = {}


def _tree(name):
    """(rows or None, the rule's tree) of an input: a key set has no rows, its tree is made of the keys as they stand"""
    if name not in _trees:
        if name in KEY_INPUTS:
            key = B.topology_keys(name)
            order = np.argsort(key, kind="stable").astype(np.uint32)
            child, count, depth = R.topology(key[order])
            _trees[name] = None, {"key": key, "order": order, "child": child, "count": count, "depth": depth}
        else:
            rows = _rows(name)
            _trees[name] = rows, R.build_rows(rows)
    return _trees[name]


@pytest.mark.parametrize("name", INPUTS)
def test_the_rule_gives_a_valid_tree(name):
    rows, t = _tree(name)
    m = len(t["order"])
    assert m == (SIZES[name] if name in SIZES else int(name.rsplit("-", 1)[1]) if name in KEY_INPUTS else m)
    assert sorted(t["order"].tolist()) == list(range(m))  # every tree surface in exactly one leaf slot
    levels, ranges = R.check_tree(t["child"], t["count"], m)
    assert levels == t["depth"] <= R.BVH_STACK
    assert len(t["child"]) == max(m - 1, 1)
    key = t["key"][t["order"]]
    for j in range(1, m):  # (key, position) ascending
        assert key[j - 1] < key[j] or t["order"][j - 1] < t["order"][j]
    if rows is not None:
        again = R.build_rows(rows.copy())
        for f in ("key", "order", "child", "count"):
            assert again[f].tobytes() == t[f].tobytes(), f
    else:
        assert t["order"].tolist() == list(range(m))  # a key set is handed over sorted
    if name == "coincident_300":
        assert len(np.unique(t["key"])) == 1 and t["depth"] == 9  # medians all the way: ceil(log2 300) levels
        assert t["order"].tolist() == list(range(300))
    if name == "unbounded_plane":
        assert (t["key"] == R.UNBOUNDED).sum() == 1 and t["key"][t["order"][-1]] == R.UNBOUNDED  # sorts last
        assert not (np.abs(t["lo"]) < 1e299).all()
    if name == "line_40":
        assert len(np.unique(t["key"])) == 40
    if name in ("three_spheres", "m3"):  # a root with one leaf and one inner child
        assert sorted(t["count"][0].tolist()) == [0, 1] and t["depth"] == 2
    if name == "lattice_5000":  # 1000 sites of five spheres with one key each (and the plane light): the five lie a thousand positions apart
        values, n = np.unique(t["key"][:5000], return_counts=True)
        assert len(values) == 1000 and (n == 5).all() and np.array_equal(t["key"][:1000], t["key"][4000:5000])
        assert t["key"][5000] not in values
    if name == "planes_first":  # the first wave of the bounds pass holds no bounded surface
        assert (t["key"][:70] == R.UNBOUNDED).all() and (t["key"][70:] != R.UNBOUNDED).all() and t["order"][-70:].tolist() == list(range(70))
    if name == "planes_last_only_bounded":  # the bounded ones sit in the last, partial wave alone
        assert np.flatnonzero(t["key"] != R.UNBOUNDED).tolist() == [130, 131, 132] and 128 <= 130 and m < 192
    if name in ("spheres_1024", "spheres_2049", "spheres_4097", "spheres_20000"):
        assert len(np.unique(t["key"])) == m
    if name == "comb":
        assert len(np.unique(t["key"])) == 64 and t["depth"] == 30


def test_the_depth_budget_is_what_bounds_the_deep_case():
    rows = _rows("deep_64")
    free = R.build_rows(rows, budget=False)
    levels, _ = R.check_tree(free["child"], free["count"], 64)
    assert levels == free["depth"] == 63 > R.BVH_STACK  # a chain: every split by the highest differing bit peels one sphere off
    top = [int(k).bit_length() - 1 for k in free["key"]]
    assert sorted(top) == [-1] + list(range(63))  # every key has a highest set bit of its own (the sphere at the origin has none)
    held = R.build_rows(rows)
    levels, _ = R.check_tree(held["child"], held["count"], 64)
    assert levels == held["depth"] <= R.BVH_STACK
    assert held["order"].tobytes() == free["order"].tobytes() and held["child"].tobytes() != free["child"].tobytes()
    # the chain's node at depth d holds 64 - d spheres; the budget lets it peel while d + 2 + ceil(log2(64 - d)) < 32, that is down to
    # d = 23 (41 spheres). The node at depth 24 holds 40: medians from there, 40 -> 20 -> 10 -> 5 -> 3 -> 2, inner nodes down to depth
    # 29, leaves on level 30
    assert held["depth"] == 30


def test_the_deep_blob_is_as_deep_as_the_rule_allows():
    """18 keys with one high bit each above 4096 keys 0 .. 4095. The chain's node at depth d holds 4114 - d keys, ceil(log2) = 13, and the
    budget lets it peel its last key off while d + 2 + 13 < 32: down to d = 16. The node at depth 17 holds 4097 and is split at the
    middle, and so is everything below: 2048 | 2049 at depth 18, and the odd halves 2049 -> 1025 -> 513 -> ... -> 3 -> 2 reach an inner
    node at depth 29, the deepest the rule allows (d + 2 + 1 < 32 fails from d = 29 on, and a range of 2 splits no further). Levels 0 to
    17 hold one inner node each, level 18 + j holds 2^(j + 1) up to 2048 on level 28, level 29 holds the one node over the last two keys
    of the odd chain. With 19 keys the node at depth 17 holds 4098 and both halves are odd chains: 1537 nodes on level 28 and 1015 on
    level 29. Without the budget the chain peels every one of its keys and the blob's 12 levels follow: 18 + 12 = 30 and 19 + 12 = 31
    levels, other trees both."""
    for name, deepest in (("deep_blob", [512, 1024, 2048, 1]), ("deep_blob_19", [385, 769, 1537, 1015])):
        key = B.topology_keys(name)
        child, count, depth = R.topology(key)
        levels, _ = R.check_tree(child, count, len(key))
        assert levels == depth == 30 <= R.BVH_STACK
        per_level = [len(e) for e in R.level_entries(child, count)]
        assert per_level[1:18] == [1] * 17 and per_level[18:20] == [2, 4] and per_level[26:] == deepest and sum(per_level) == len(key) - 2
        free = R.topology(key, budget=False)
        assert free[2] == len(key) - 4096 + 12 and free[0].tobytes() != child.tobytes()


def test_the_level_walk_counts_every_inner_node_once():
    for name in ("comb", "random-257", "one_value-5", "unbounded_tail-1025"):
        key = B.topology_keys(name)
        child, count, depth = R.topology(key)
        entries = R.level_entries(child, count)
        assert len(entries) == depth and entries[0] == []
        nodes = [n for e in entries for n, _ in e]
        assert sorted(nodes) == list(range(1, len(key) - 1))
        for e in entries[1:]:
            for node, link in e:
                assert child[link // 2, link % 2] == node and count[link // 2, link % 2] == 0


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rule") / "hierarchy_rule_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(cases.REPO, "daily-ray-trace_amd", "csrc"), os.path.join(cases.REPO, "tests", "host", "hierarchy_rule_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("name", INPUTS)
def test_one_text_on_host_and_device(rule_program, name):
    rows, t = _tree(name)
    if rows is None:  # a key set: the program's key mode
        text = "keys %d\n" % len(t["key"]) + "".join("%d\n" % int(k) for k in t["key"])
    else:
        lo, hi = t["lo"], t["hi"]
        with np.errstate(all="ignore"):
            bounded = (np.abs(lo) < 1e299).all(axis=1) & (np.abs(hi) < 1e299).all(axis=1) if len(lo) else np.zeros(0, dtype=bool)
            c = 0.5 * (lo + hi)
        text = "%d\n" % len(lo) + "".join("%d %s %s %s\n" % ((int(bounded[k]),) + tuple(float(x).hex() if bounded[k] else "0x0p+0" for x in c[k])) for k in range(len(lo)))
    r = subprocess.run([rule_program], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]  # ends clean: no sanitizer report
    lines = [line.split() for line in r.stdout.splitlines()]
    assert int(lines[0][1]) == t["depth"]
    assert [int(x[1]) for x in lines if x[0] == "key"] == [int(k) for k in t["key"]]
    assert [int(x[1]) for x in lines if x[0] == "slot"] == t["order"].tolist()
    nodes = np.array([[int(v) for v in x[1:]] for x in lines if x[0] == "node"], dtype=np.int32)
    assert np.array_equal(nodes[:, 0:2], t["child"]) and np.array_equal(nodes[:, 2:4], t["count"])


def test_the_kernels_compile_the_rules_text():
    csrc = os.path.join(cases.REPO, "daily-ray-trace_amd", "csrc")
    rule = open(os.path.join(csrc, "drt_build_rule.h")).read()
    assert re.findall(r"#include\s+(\S+)", rule) == ["<stdint.h>"]  # no HIP include
    kernels = open(os.path.join(csrc, "drt_build_kernels.h")).read()
    assert '#include "drt_build_rule.h"' in kernels
    for f in ("build_quantise", "build_key", "build_split", "build_child_node", "build_leaf_ref"):
        assert re.search(r"DRT_RULE_FN \w+ %s\(" % f, rule) and re.search(r"\b%s\(" % f, kernels), f
    # the selftests of tests/test_gpu_build_passes.py run the enqueue code a build runs: the launch loops of the sort and of the topology
    # are in one helper each, both sites call it, and nothing else launches those kernels
    launcher = open(os.path.join(csrc, "drt_launcher.hip")).read()

    def body(signature):
        start = launcher.index(signature)
        return launcher[start:launcher.index("\n}\n", start)]

    build = body("static int hierarchy_enqueue(drt_context *ctx)")
    sort, topology = body('extern "C" int drt_selftest_build_sort('), body('extern "C" int drt_selftest_build_topology(')
    helpers = {"hierarchy_enqueue_init": ["drt_build_init_kernel"],
               "hierarchy_enqueue_sort": ["drt_build_count_kernel", "drt_build_scan_kernel", "drt_build_scatter_kernel"],
               "hierarchy_enqueue_topology": ["drt_build_topology_kernel"]}
    for helper, launched in helpers.items():
        text = body("static int %s(" % helper)
        for kernel in launched:
            assert len(re.findall(r"hipLaunchKernelGGL\(%s\b" % kernel, launcher)) == 1 and "hipLaunchKernelGGL(%s," % kernel in text, kernel
        assert len(re.findall(r"\b%s\(" % helper, build)) == 1, helper
    calls = lambda text: sorted(set(re.findall(r"\b(hierarchy_enqueue_\w+)\(", text)))
    assert calls(sort) == ["hierarchy_enqueue_sort"] and calls(topology) == ["hierarchy_enqueue_init", "hierarchy_enqueue_topology"]
    assert calls(build) == sorted(helpers)
    assert "hipLaunchKernelGGL" not in sort + topology  # no loop of their own
    assert "hierarchy_level_grid(" in body("static int hierarchy_enqueue_topology(") and "hierarchy_level_grid(" in build  # one grid rule for the levels


# ------------------------------------------------------------------------------------------------
REPORT_FIELDS = [("nodes", 0), ("leaf_surfaces", 4), ("depth", 8), ("device_builds", 12), ("built_by", 16), ("pad", 20), ("kernel_ms", 24)]
CALLS = ("drt_rebuild_hierarchy", "drt_group_rebuild_hierarchy", "drt_get_hierarchy_report", "drt_read_hierarchy", "drt_selftest_build_sort",
         "drt_selftest_build_topology")


def test_the_header_the_compiler_and_pydrt_agree_on_the_calls_and_the_report(tmp_path):
    header = open(os.path.join(cases.REPO, "include", "drt_hip.h")).read()
    for call in CALLS:
        assert re.search(r"\bint %s\(" % call, header) and call in pydrt.HIP_SYMBOLS, call
    src = tmp_path / "report.c"
    lines = ['printf("%s %%zu\\n", offsetof(drt_hierarchy_report, %s));' % (n, n) for n, _ in REPORT_FIELDS]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "drt_hip.h"\nint main(void) {\n%s\n'
                   'printf("sizeof %%zu\\nupdate %%zu\\n", sizeof(drt_hierarchy_report), sizeof(drt_update_report));\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "report"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(cases.REPO, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(pydrt.HierarchyReport) == 32 and int(out["update"]) == 24  # drt_update_report stays
    assert [(n, int(out[n])) for n, _ in REPORT_FIELDS] == REPORT_FIELDS
    assert [(n, getattr(pydrt.HierarchyReport, n).offset) for n, _ in pydrt.HierarchyReport._fields_] == REPORT_FIELDS
    assert pydrt.BVH_NODE.itemsize == R.NODE_DTYPE.itemsize == 64 and pydrt.BVH_NODE == R.NODE_DTYPE
    for method in ("rebuild_hierarchy", "hierarchy_report", "read_hierarchy"):
        assert callable(getattr(pydrt.Renderer, method))
    assert callable(pydrt.Group.rebuild_hierarchy)
