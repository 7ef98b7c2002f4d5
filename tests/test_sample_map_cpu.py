"""Sample maps without a GPU (-m "not gpu"): the plan's invariants (tests/sample_map_rule.py), the C-ABI as the header, the compiler and
pydrt see it, the argument checks and the map helpers of pydrt, the host program's DRT_REGIONS refusals, and -- on the oracle alone --
that the counts the GPU tests use have different films, so that a wrong count cannot pass their comparison by accident."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import pydrt
import sample_map_rule as SM

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")
VALUES = (0, 1, 2, 3, 5, 8, 13, 21, 40)


def hand_made():
    """(counts, targets, add) by hand: the example of the rule, empty and zero maps, pixels above their target, the largest counts"""
    top = 2 ** 32 - 1
    return [(np.zeros(4), [5, 0, 1, 4], False),                      # 5 = round 0 + round 2
            (np.zeros(0), np.zeros(0), False), (np.zeros(3), np.zeros(3), False), (np.zeros(3), np.zeros(3), True),
            ([4, 4, 9, 0], [2, 4, 40, 1], False),                    # above, equal, below, fresh
            ([4, 4, 9, 0], [2, 4, 40, 1], True),
            ([0, 1, top, top - 1], [top, top, top, top], False),     # every bit set; nothing left; one sample left
            ([0, 1, top], [top, top - 1, 0], True),
            ([7] * 300, [7 + (k % 9) for k in range(300)], False)]


def seeded(k):
    rng = np.random.default_rng(100 + k)
    P = int(rng.integers(1, 700))
    counts = rng.choice(np.array(VALUES), size=P)
    hi = [4, 50, 2 ** 16, 2 ** 31][k % 4]
    return counts, rng.integers(0, hi, size=P), bool(k & 1)


@pytest.mark.parametrize("counts, targets, add", hand_made() + [seeded(k) for k in range(24)])
def test_the_plan_renders_every_remainder_in_ascending_ranges_without_a_gap(counts, targets, add):
    n, t = np.asarray(counts, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    plan = SM.plan(n, t, add)
    R = plan["remainders"].astype(np.int64)
    assert np.array_equal(R, t if add else np.maximum(t - n, 0))
    assert len(plan["rounds"]) == plan["report"]["rounds"] <= 32
    bits = [b for b, _, _ in plan["rounds"]]
    assert bits == sorted(set(bits)) and sum(1 << b for b in bits) == plan["B"]
    got, at = np.zeros_like(n), n.copy()
    for (b, pixels, k), starts in zip(plan["rounds"], plan["starts"]):
        assert k == 1 << b and pixels.size > 0 and np.array_equal(pixels, np.sort(pixels)) and np.unique(pixels).size == pixels.size
        assert np.array_equal(starts, at[pixels])  # every sample range begins where the pixel's last one ended
        at[pixels] += k
        got[pixels] += k
    assert np.array_equal(got, R) and np.array_equal(at, n + R) and np.array_equal(plan["final"], (n + R).astype(np.uint32))
    rep = plan["report"]
    assert rep["paths"] == int(R.sum()) and rep["pixels_rendered"] == int((R > 0).sum())
    assert rep["pixels_above"] == (0 if add else int((n > t).sum())) and rep["max_count"] == (int((n + R).max()) if n.size else 0)


def test_the_plan_of_the_example_and_the_add_overflow():
    plan = SM.plan([0], [5])
    assert [(b, list(p), k) for b, p, k in plan["rounds"]] == [(0, [0], 1), (2, [0], 4)] and [list(s) for s in plan["starts"]] == [[0], [1]]
    with pytest.raises(OverflowError, match="^2$"):
        SM.plan([0, 1, 4, 4], [2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32 - 4, 2 ** 32 - 1], add=True)


def test_the_header_the_compiler_and_pydrt_agree_on_the_calls(tmp_path):
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for call in ("drt_render_sample_map", "drt_group_render_sample_map"):
        assert re.search(r"\bint %s\(" % call, plain) and call in pydrt.HIP_SYMBOLS, call
    assert re.search(r"#define DRT_MAP_DEVICE\s+1u", header) and pydrt.MAP_DEVICE == 1
    assert re.search(r"#define DRT_MAP_ADD\s+2u", header) and pydrt.MAP_ADD == 2
    src = tmp_path / "map.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "drt_hip.h"\n'
                   'int (*a)(drt_context *, drt_sample_map *) = drt_render_sample_map;\n'
                   'int (*b)(drt_group *, drt_sample_map *) = drt_group_render_sample_map;\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(drt_sample_map), offsetof(drt_sample_map, flags),\n'
                   '    offsetof(drt_sample_map, rounds), offsetof(drt_sample_map, max_count), offsetof(drt_sample_map, paths)); return 0; }\n')
    obj, exe = str(tmp_path / "map.o"), str(tmp_path / "map")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I" + os.path.join(REPO, "include"), str(src), "-o", obj],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the layout, from a program that takes no address of the library's
    src.write_text(src.read_text().replace("int (*a)", "//").replace("int (*b)", "//"))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes = subprocess.run([exe], capture_output=True, text=True).stdout.split()
    M = pydrt.SampleMap
    assert sizes == [str(v) for v in (40, M.flags.offset, M.rounds.offset, M.max_count.offset, M.paths.offset)]
    assert C.sizeof(M) == 40 and (M.flags.offset, M.paths.offset) == (8, 32)
    if os.path.exists(os.path.join(REPO, "daily-ray-trace_amd", "libdrt_hip.so")):
        L = pydrt.hip_lib()
        assert L.drt_render_sample_map.argtypes == [C.c_void_p, C.POINTER(M)]
        assert L.drt_group_render_sample_map.argtypes == [C.c_void_p, C.POINTER(M)]
        # null arguments are refused with a message, without a device
        assert L.drt_render_sample_map(None, None) != 0 and b"null" in L.drt_last_error()
        assert L.drt_group_render_sample_map(None, C.byref(M())) != 0 and b"null" in L.drt_last_error()


def test_pydrt_signatures_and_argument_checks():
    for cls in (pydrt.Renderer, pydrt.Group):
        sig = inspect.signature(cls.render_sample_map)
        assert list(sig.parameters) == ["self", "targets", "add"] and sig.parameters["add"].default is False
    assert list(inspect.signature(pydrt.region_map).parameters) == ["tile_w", "tile_h", "base", "regions"]
    assert list(inspect.signature(pydrt.coverage_map).parameters) == ["coverage", "base", "extra"]
    u = pydrt._map_u32
    for good in (np.arange(12).reshape(3, 4), np.arange(12), np.arange(12, dtype=np.int8), np.full((3, 4), 2 ** 32 - 1, dtype=np.uint64),
                 np.full(12, 2 ** 32 - 1, dtype=np.int64), np.zeros((3, 4), dtype=np.uint32)):
        out = u(good, 4, 3, "t")
        assert out.dtype == np.uint32 and out.shape == (12,) and out.flags["C_CONTIGUOUS"]
        assert np.array_equal(out.astype(np.uint64), np.asarray(good).reshape(-1).astype(np.uint64))
    strided = np.arange(24, dtype=np.uint32)[::2]
    assert np.array_equal(u(strided, 4, 3, "t"), np.arange(0, 24, 2))
    with pytest.raises(ValueError, match="shape"):
        u(np.zeros((4, 3), dtype=np.int64), 4, 3, "t")  # (tile_w, tile_h): transposed
    with pytest.raises(ValueError, match="shape"):
        u(np.zeros(11, dtype=np.int64), 4, 3, "t")
    with pytest.raises(ValueError, match="shape"):
        u(np.zeros((1, 3, 4), dtype=np.int64), 4, 3, "t")
    with pytest.raises(ValueError, match="negative"):
        u(np.array([0] * 11 + [-1]), 4, 3, "t")
    with pytest.raises(ValueError, match=r"above 2\^32 - 1"):
        u(np.array([0] * 11 + [2 ** 32]), 4, 3, "t")
    with pytest.raises(ValueError, match="integers"):
        u(np.zeros(12), 4, 3, "t")
    with pytest.raises(ValueError, match="integers"):
        u(np.zeros(12, dtype=bool), 4, 3, "t")


def test_region_map_clips_and_takes_the_maximum():
    regions = [(-2, -1, 5, 3, 9), (1, 1, 100, 2, 6), (2, 0, 2, 4, 7), (0, 3, 1, 1, 1), (5, 5, 0, 3, 99), (6, 0, 3, 3, 99), (0, 4, 3, 3, 99)]
    got = pydrt.region_map(6, 4, 2, regions)
    assert got.dtype == np.uint32 and got.shape == (4, 6)
    assert np.array_equal(got, SM.region_map(6, 4, 2, regions))
    assert np.array_equal(got, [[9, 9, 9, 7, 2, 2], [9, 9, 9, 7, 6, 6], [2, 6, 7, 7, 6, 6], [2, 2, 7, 7, 2, 2]])  # (0, 3) keeps the base: 1 < 2
    assert np.array_equal(pydrt.region_map(3, 2, 4, []), np.full((2, 3), 4))
    rng = np.random.default_rng(3)
    for _ in range(20):
        w, h = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        regs = [tuple(int(v) for v in (rng.integers(-4, 12), rng.integers(-4, 12), rng.integers(0, 9), rng.integers(0, 9), rng.integers(0, 50)))
                for _ in range(int(rng.integers(0, 5)))]
        assert np.array_equal(pydrt.region_map(w, h, 3, regs), SM.region_map(w, h, 3, regs))
    with pytest.raises(ValueError):
        pydrt.region_map(4, 4, 1, [(0, 0, -1, 2, 3)])
    with pytest.raises(ValueError):
        pydrt.region_map(4, 4, 2 ** 32, [])


def test_coverage_map_rounds_up():
    cov = np.array([[0.0, 1e-12, 0.25], [0.5, 0.999, 1.0]])
    got = pydrt.coverage_map(cov, 3, 8)
    assert got.dtype == np.uint32 and np.array_equal(got, [[3, 4, 5], [7, 11, 11]]) and np.array_equal(got, SM.coverage_map(cov, 3, 8))
    assert np.array_equal(pydrt.coverage_map(cov, 0, 0), np.zeros((2, 3)))
    assert np.array_equal(pydrt.coverage_map(np.array([1.0 / 3.0]), 1, 3), [2])
    for bad in (np.array([1.5]), np.array([-0.1]), np.array([np.nan])):
        with pytest.raises(ValueError):
            pydrt.coverage_map(bad, 0, 4)
    with pytest.raises(ValueError):
        pydrt.coverage_map(np.array([1.0]), 2 ** 32 - 1, 1)


# the configuration of these runs: config.cfg as shipped (800 x 600, num_pixel_samples 4)
@pytest.mark.parametrize("env, message", [
    ({"DRT_REGIONS": ""}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": "1,2,3,4"}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": "1,2,3:8"}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": "1,2,3,4,8"}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": "1,2,3,4:8;"}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": "1,2,3,4:8,5,6,7,8:9"}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": "-1,2,3,4:8"}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": "1,2,3,4:8.5"}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": " 1,2,3,4:8"}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": "1,2,3,4:4294967296"}, "regions x,y,w,h:spp of whole numbers"),
    ({"DRT_REGIONS": "1,2,0,4:8"}, "region 0 (1,2,0,4) has no size"),
    ({"DRT_REGIONS": "1,2,3,4:8;5,6,7,0:8"}, "region 1 (5,6,7,0) has no size"),
    ({"DRT_REGIONS": "800,0,3,4:8"}, "region 0 (800,0,3,4) lies outside the 800 x 600 image"),
    ({"DRT_REGIONS": "0,600,3,4:8"}, "region 0 (0,600,3,4) lies outside the 800 x 600 image"),
    ({"DRT_REGIONS": "1,2,3,4:0"}, "asks for 0 samples: num_pixel_samples (4) or more"),
    ({"DRT_REGIONS": "1,2,3,4:3"}, "asks for 3 samples: num_pixel_samples (4) or more"),
    ({"DRT_REGIONS": ";".join(["1,2,3,4:8"] * 65)}, "64 regions at most"),
    ({"DRT_REGIONS": "1,2,3,4:8", "DRT_ADAPTIVE_ERROR": "0.1"}, "DRT_REGIONS cannot be combined with DRT_ADAPTIVE_ERROR"),
    ({"DRT_REGIONS": "1,2,3,4:8", "DRT_CHECKPOINT_SPP": "1"}, "DRT_REGIONS cannot be combined with DRT_CHECKPOINT_SPP"),
    ({"DRT_REGIONS": "1,2,3,4:8", "DRT_RESUME": "1"}, "DRT_REGIONS cannot be combined with DRT_RESUME"),
    ({"DRT_REGIONS": "1,2,3,4:8", "DRT_TURNTABLE": "2"}, "DRT_REGIONS cannot be combined with DRT_TURNTABLE"),
    ({"DRT_REGIONS": "1,2,3,4:8", "DRT_LIGHT_LEVELS": "1,2"}, "DRT_REGIONS cannot be combined with DRT_LIGHT_LEVELS"),
    ({"DRT_REGIONS": "1,2,3,4:8", "DRT_DEPTH_CUTS": "1,2"}, "DRT_REGIONS cannot be combined with DRT_DEPTH_CUTS"),
    ({"DRT_REGIONS": "1,2,3,4:8", "DRT_PROJECTION": "equirect"}, "DRT_REGIONS cannot be combined with DRT_PROJECTION"),
    ({"DRT_REGIONS": "1,2,3,4:8", "output_spd": "output/" + "o" * 42 + ".spd"}, "with .counts.bmp behind it is longer than 63 characters"),
])
def test_the_host_refuses_bad_regions_before_any_device_call(tmp_path, env, message):
    """Exit status nonzero, the reason on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run that got as
    far as the launcher would fail there with the launcher's message instead."""
    cfg = open(os.path.join(REPO, "config.cfg")).read()
    env = dict(env)
    if "output_spd" in env:
        cfg, n = re.subn(r"(?m)^output_spd\s+\S+", "output_spd        " + env.pop("output_spd"), cfg)
        assert n == 1
    (tmp_path / "config.cfg").write_text(cfg)
    os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
    os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout


def test_neighbouring_counts_have_different_films():
    """plane_light_48 in DEVICE arithmetic, snapshots at the counts the GPU tests' map holds: film_at_counts of two neighbouring counts
    differs in all three buffers, so a pixel rendered to the wrong count cannot pass the comparison"""
    import oracle_py as O
    bundle, p = cases.load_case("plane_light_48")
    counts = [v for v in VALUES if v]
    snaps, film, prev = {}, None, 0
    for n in counts:
        q = pydrt.make_params(int(p.width), int(p.height), spp=n - prev, max_depth=int(p.max_depth), seed=int(p.seed),
                              pixel_scheme=int(p.pixel_scheme), first_sample=prev)
        px, av, va, _, _ = O.oracle_render_tile(bundle, q, num_threads=8, math_mode=O.MATH_DEVICE, film=film)
        film = (px, av, va)
        snaps[n] = film
        prev = n
    import test_gpu_adaptive as A
    P = int(p.width) * int(p.height)
    for a, b in zip(counts, counts[1:]):
        fa, fb = A.film_at_counts(snaps, np.full(P, a)), A.film_at_counts(snaps, np.full(P, b))
        for k, buf in enumerate(("pixels", "means", "variances")):
            if a == 1 and k == 2:
                assert not fa[k].any()  # one sample has no variance yet
            assert not cases.same_bits(fa[k], fb[k]), "the %s at %d and %d samples are the same" % (buf, a, b)
