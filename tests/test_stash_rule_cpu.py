"""CPU: the ray stash's hand-out rule (csrc/drt_stash_rule.h), run on the host as the trace kernel runs it.

tests/host/stash_rule_main.cpp drives one wave through the header with a stash that holds path ids instead of rays; it is built with
the address and undefined-behaviour sanitizers as a program of its own. `direct` below is the direct form's hand-out
(trace_paths, "refill idle lanes") written out again: for every sequence of idle-lane counts the stash must give every rank the id
the direct form gives it, draw from the work counter when the direct form draws, hand every id out exactly once in ascending order
and never make an entry at or beyond chunk_end."""
import os
import re
import subprocess

import pytest

import cases

CSRC = os.path.join(cases.REPO, "daily-ray-trace_amd", "csrc")
STEPS = [64, 1, 37, 64, 5, 63, 2, 64, 20] * 3 + [64]  # tests/test_gpu_path_ids.py's
CHUNKS = (64, 256, 1024)
ENDS = (0, 1, 63, 64)  # ids a launch's last chunk holds (0: the launch ends on a chunk boundary)
SEQUENCES = {"all 64": [64], "single lanes": [1], "1 to 64 in turn": list(range(1, 65)), "path id steps": STEPS,
             "a few per iteration": [13, 12, 14, 11, 13, 15, 9]}


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stash") / "stash_rule_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + CSRC, os.path.join(cases.REPO, "tests", "host", "stash_rule_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def direct(chunk, n_paths, wants):
    """(ids per step, bases drawn) of the direct form's hand-out"""
    counter = nxt = end = 0
    exhausted = False
    out, draws = [], []
    for want in wants:
        ids = [-1] * want
        if not exhausted:
            avail = end - nxt
            if avail < want:
                for r in range(avail):
                    ids[r] = nxt + r
                base, counter = counter, counter + chunk
                draws.append(base)
                if base >= n_paths:
                    exhausted, nxt, end = True, 0, 0
                else:
                    nxt, end = base, min(base + chunk, n_paths)
                    used = min(want - avail, end - nxt)
                    for r in range(used):
                        ids[avail + r] = nxt + r
                    nxt += used
            else:
                ids = [nxt + r for r in range(want)]
                nxt += want
        out.append(ids)
    return out, draws


def run(rule_program, chunk, n_paths, wants):
    text = "%d %d %d\n" % (chunk, n_paths, len(wants)) + " ".join(str(w) for w in wants) + "\n"
    r = subprocess.run([rule_program], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]  # ends clean: no report of the program's or a sanitizer's
    lines = [line.split() for line in r.stdout.splitlines()]
    steps = [[int(v) for v in x[2:]] for x in lines if x[0] == "step"]
    fills = [tuple(int(v) for v in x[1:]) for x in lines if x[0] == "fill"]
    draws = [int(x[1]) for x in lines if x[0] == "draw"]
    left = [tuple(int(v) for v in x[1:]) for x in lines if x[0] == "left"][0]
    return steps, fills, draws, left


@pytest.mark.parametrize("end", ENDS)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_the_stash_hands_out_what_the_direct_form_hands_out(rule_program, name, chunk, end):
    n_paths = 2 * chunk + end
    seq = SEQUENCES[name]
    wants = []
    while sum(wants) < n_paths + 3 * 64:  # past the launch's end: the waves find the counter used up, more than once
        wants += seq
    steps, fills, draws, left = run(rule_program, chunk, n_paths, wants)
    want_steps, want_draws = direct(chunk, n_paths, wants)
    assert steps == want_steps, next((k, a, b) for k, (a, b) in enumerate(zip(steps, want_steps)) if a != b)
    assert draws == want_draws
    handed = [i for s in steps for i in s if i >= 0]
    assert handed == list(range(n_paths))  # every id once, ascending
    for first, n, chunk_end in fills:
        assert 1 <= n <= 64 and first + n <= chunk_end <= n_paths and first % 64 == 0
        assert n == 64 or first + n == n_paths  # only a launch's last fill is short
    assert sum(n for _, n, _ in fills) == n_paths and left == (0, 0)


def test_a_launch_that_stops_in_the_middle_leaves_its_entries_counted(rule_program):
    """the state after a few iterations: what the stash still holds and what the chunk still holds add up to the ids not handed out"""
    steps, fills, draws, left = run(rule_program, 256, 10 * 256, [13] * 7)
    assert sum(len(s) for s in steps) == 91 and draws == [0]
    assert fills == [(0, 64, 256), (64, 64, 256)] and left == (128 - 91, 256 - 128)


def test_the_kernel_compiles_the_rules_text():
    rule = open(os.path.join(CSRC, "drt_stash_rule.h")).read()
    assert re.findall(r"#include\s+(\S+)", rule) == ["<cstdint>"]  # no HIP include
    kernels = open(os.path.join(CSRC, "drt_kernels.h")).read()
    assert '#include "drt_stash_rule.h"' in kernels
    for name in ("stash_first_entry", "stash_after_first", "stash_fill_size", "stash_second_entry", "stash_after_fill"):
        assert re.search(r"\b%s\(" % name, kernels), name
        assert len(re.findall(r"\b%s\(" % name, rule)) == 1, name  # defined once, and not restated in the kernel
        assert not re.search(r"uint32_t\s+%s\(|void\s+%s\(" % (name, name), kernels)
