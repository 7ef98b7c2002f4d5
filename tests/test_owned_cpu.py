"""csrc/drt_owned.h on the host: Owned<T, Mem> with a malloc-backed counting policy, in a stand-alone program under the address and
undefined-behaviour sanitizers (tests/host/owned_main.cpp). The header must compile without HIP when the policy needs none."""
import os
import subprocess

import cases


def test_owned_frees_each_block_once_under_the_sanitizers(tmp_path):
    exe = tmp_path / "owned_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(cases.REPO, "daily-ray-trace_amd", "csrc"), os.path.join(cases.REPO, "tests", "host", "owned_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.stdout + r.stderr)[-4000:]  # ends clean: no count off, no sanitizer report
    assert r.stdout.strip() == "owned ok"
