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
    return pydrt.surface_rows(U.load(name)["before"])


INPUTS = ["m0", "m1", "m2", "m3", "coincident_300", "line_40", "unbounded_plane", "deep_64", "spheres_96", "lights_all_bvh"]


@pytest.mark.parametrize("name", INPUTS)
def test_the_rule_gives_a_valid_tree(name):
    rows = _rows(name)
    t = R.build_rows(rows)
    m = len(t["order"])
    assert m == {"m0": 0, "m1": 1, "m2": 2, "m3": 3, "coincident_300": 300, "line_40": 40, "deep_64": 64}.get(name, m)
    assert sorted(t["order"].tolist()) == list(range(m))  # every tree surface in exactly one leaf slot
    levels, ranges = R.check_tree(t["child"], t["count"], m)
    assert levels == t["depth"] <= R.BVH_STACK
    assert len(t["child"]) == max(m - 1, 1)
    key = t["key"][t["order"]]
    for j in range(1, m):  # (key, position) ascending
        assert key[j - 1] < key[j] or t["order"][j - 1] < t["order"][j]
    again = R.build_rows(rows.copy())
    for f in ("key", "order", "child", "count"):
        assert again[f].tobytes() == t[f].tobytes(), f
    if name == "coincident_300":
        assert len(np.unique(t["key"])) == 1 and t["depth"] == 9  # medians all the way: ceil(log2 300) levels
        assert t["order"].tolist() == list(range(300))
    if name == "unbounded_plane":
        assert (t["key"] == R.UNBOUNDED).sum() == 1 and t["key"][t["order"][-1]] == R.UNBOUNDED  # sorts last
        assert not (np.abs(t["lo"]) < 1e299).all()
    if name == "line_40":
        assert len(np.unique(t["key"])) == 40


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
    t = R.build_rows(_rows(name))
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


# ------------------------------------------------------------------------------------------------
REPORT_FIELDS = [("nodes", 0), ("leaf_surfaces", 4), ("depth", 8), ("device_builds", 12), ("built_by", 16), ("pad", 20), ("kernel_ms", 24)]
CALLS = ("drt_rebuild_hierarchy", "drt_group_rebuild_hierarchy", "drt_get_hierarchy_report", "drt_read_hierarchy")


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
