"""Depth-cut films without a GPU (-m "not gpu"): the premise of the rule on the oracle alone, that the cases tell depths apart, the
C-ABI as the header, the compiler and pydrt see it, depth_layers, and the host program's refusals.

The rule: cut d of a render at max_depth D is the oracle's render at max_depth = d. It holds only because the
path generator is keyed by (seed, pixel, sample): a render at max_depth = d walks the first d loop iterations of the render at D. That
is checked here on the hit log -- the log at depth d is the first d columns of the full one -- for every case and every cut the GPU
tests use (depth_cut_cases.ALL_CUTS)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import depth_cut_cases as DC
import pydrt

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")


def full_depth(name):
    return int(DC.load(name)[1].max_depth)


@pytest.mark.parametrize("name", sorted(DC.ALL_CUTS))
def test_a_shorter_render_walks_the_first_vertices_of_the_full_one(name):
    D = full_depth(name)
    cuts = DC.ALL_CUTS[name]
    assert list(cuts) == sorted(set(cuts)) and 1 <= cuts[0] and cuts[-1] <= D and len(cuts) <= pydrt.MAX_DEPTH_CUTS
    full = DC.oracle_at_cpu(name, D)
    assert full[3].shape[1] == D
    for d in cuts:
        short = DC.oracle_at_cpu(name, d)
        assert short[3].shape == (full[3].shape[0], d)
        assert np.array_equal(short[3], full[3][:, :d]), "%s: the hit log at max_depth %d is not the first %d columns of the full one" % (name, d, d)
    # the same call twice gives the same film: cut D is the full film's bits
    bundle, params = DC.load(name)
    import oracle_py as O
    again = O.oracle_render_tile(bundle, DC.params_at(params, D), want_hits=True, num_threads=3, math_mode=O.MATH_DEVICE)
    DC.assert_film(again[:3], full[:3], "%s at full depth, rendered twice" % name)


@pytest.mark.parametrize("name", sorted(DC.CUTS))
def test_neighbouring_cuts_have_different_films(name):
    """so a kernel that ignores the depth cannot pass: every pair of neighbouring cuts (many_lights and spheres_1500 are constant
    from depth 3 on, which is where their lists end)"""
    depths = DC.CUTS[name]
    for a, b in zip(depths, depths[1:]):
        fa, fb = DC.oracle_at_cpu(name, a), DC.oracle_at_cpu(name, b)
        for k, buf in enumerate(("pixels", "means", "variances")):
            assert not cases.same_bits(fa[k], fb[k]), "%s: the %s at depths %d and %d are the same" % (name, buf, a, b)


@pytest.mark.parametrize("name", sorted(DC.FLAT_CUTS))
def test_the_flat_cases_are_flat(name):
    """first_scene: nothing beyond the first hit; example_scene: every ray NaN. All cuts are one film, NaN for NaN"""
    a, b = (DC.oracle_at_cpu(name, d) for d in DC.FLAT_CUTS[name])
    DC.assert_film(a[:3], b[:3], name)
    if name == "example_scene":
        assert np.isnan(a[0][:, :-1]).all()


def test_deep_paths_reach_the_third_block_and_the_table_block():
    """paths with 13 vertices and more read the header's table block, with 9 to 12 its third block"""
    bundle, params = DC.load("deep_paths")
    hits = DC.oracle_at_cpu("deep_paths", full_depth("deep_paths"))[3]
    surf_mat = np.array([bundle.scene.surfaces[i].material for i in range(int(bundle.scene.num_surfaces))])
    black = np.array([bool(m.is_black_body) for m in bundle.materials()])
    hit = hits >= 0
    shaded = np.cumprod(hit & ~black[np.where(hit, surf_mat[np.where(hit, hits, 0)], 0)], axis=1).sum(axis=1)
    assert int((shaded >= 13).sum()) >= 40 and int((shaded >= 17).sum()) >= 15 and int(((shaded >= 9) & (shaded <= 12)).sum()) >= 10


def test_the_header_the_compiler_and_pydrt_agree_on_the_calls(tmp_path):
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    calls = ("drt_bind_depth_cuts", "drt_read_depth_film", "drt_depth_film_device_ptrs", "drt_read_depth_xyz", "drt_read_depth_bgra",
             "drt_group_bind_depth_cuts", "drt_group_read_depth_film")
    for call in calls:
        assert re.search(r"\bint %s\(" % call, plain) and call in pydrt.HIP_SYMBOLS, call
    assert re.search(r"#define DRT_MAX_DEPTH_CUTS\s+8\b", header) and pydrt.MAX_DEPTH_CUTS == 8
    # the declarations, called with the argument types pydrt gives them
    src = tmp_path / "depth.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "drt_hip.h"\n'
                   'int (*a)(drt_context *, const uint32_t *, uint32_t) = drt_bind_depth_cuts;\n'
                   'int (*b)(drt_context *, uint32_t, double *, double *, double *) = drt_read_depth_film;\n'
                   'int (*c)(drt_context *, uint32_t, void **, void **, void **) = drt_depth_film_device_ptrs;\n'
                   'int (*d)(drt_context *, uint32_t, double *) = drt_read_depth_xyz;\n'
                   'int (*e)(drt_context *, uint32_t, int, uint8_t *) = drt_read_depth_bgra;\n'
                   'int (*f)(drt_group *, const uint32_t *, uint32_t) = drt_group_bind_depth_cuts;\n'
                   'int (*g)(drt_group *, uint32_t, double *, double *, double *) = drt_group_read_depth_film;\n'
                   'int main(void) { printf("%d\\n", DRT_MAX_DEPTH_CUTS); return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "depth.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if os.path.exists(os.path.join(REPO, "daily-ray-trace_amd", "libdrt_hip.so")):
        L = pydrt.hip_lib()
        u32p, f64p, vpp = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_void_p)
        assert L.drt_bind_depth_cuts.argtypes == [C.c_void_p, u32p, C.c_uint32]
        assert L.drt_read_depth_film.argtypes == [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
        assert L.drt_depth_film_device_ptrs.argtypes == [C.c_void_p, C.c_uint32, vpp, vpp, vpp]
        assert L.drt_read_depth_xyz.argtypes == [C.c_void_p, C.c_uint32, f64p]
        assert L.drt_read_depth_bgra.argtypes == [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint8)]
        assert L.drt_group_bind_depth_cuts.argtypes == [C.c_void_p, u32p, C.c_uint32]
        assert L.drt_group_read_depth_film.argtypes == [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
        # a null context is refused with a message, without a device
        assert L.drt_bind_depth_cuts(None, None, 0) != 0 and b"null context" in L.drt_last_error()
        assert L.drt_read_depth_film(None, 0, None, None, None) != 0 and b"null context" in L.drt_last_error()


def test_depth_layers_are_the_differences_of_the_cumulative_means():
    means = np.array([[[1.0, 2.0], [0.0, 0.5]], [[1.5, 2.0], [0.25, 0.5]], [[4.0, 2.0], [0.25, 8.5]]])
    layers = pydrt.depth_layers(means)
    assert layers.shape == means.shape and layers.dtype == np.float64
    assert np.array_equal(layers[0], means[0])
    assert np.array_equal(layers[1], [[0.5, 0.0], [0.25, 0.0]])
    assert np.array_equal(layers[2], [[2.5, 0.0], [0.0, 8.0]])
    assert np.array_equal(layers.sum(axis=0), means[-1])
    assert np.array_equal(means, np.array([[[1.0, 2.0], [0.0, 0.5]], [[1.5, 2.0], [0.25, 0.5]], [[4.0, 2.0], [0.25, 8.5]]]))  # the input is left alone
    one = pydrt.depth_layers([[3.0, 4.0]])
    assert np.array_equal(one, [[3.0, 4.0]])
    nan = pydrt.depth_layers(np.array([[np.nan, 1.0], [np.nan, 3.0]]))
    assert np.isnan(nan[:, 0]).all() and np.array_equal(nan[:, 1], [1.0, 2.0])
    with pytest.raises(ValueError):
        pydrt.depth_layers(np.zeros((0, 4)))


# the configuration of these runs: config.cfg with max_cast_depth 12
@pytest.mark.parametrize("env, message", [
    ({"DRT_DEPTH_CUTS": ""}, "whole numbers separated by commas"),
    ({"DRT_DEPTH_CUTS": "1,,2"}, "whole numbers separated by commas"),
    ({"DRT_DEPTH_CUTS": "1,2,"}, "whole numbers separated by commas"),
    ({"DRT_DEPTH_CUTS": "1;2"}, "whole numbers separated by commas"),
    ({"DRT_DEPTH_CUTS": "1,two"}, "whole numbers separated by commas"),
    ({"DRT_DEPTH_CUTS": "-1"}, "whole numbers separated by commas"),
    ({"DRT_DEPTH_CUTS": "1.5"}, "whole numbers separated by commas"),
    ({"DRT_DEPTH_CUTS": " 1"}, "whole numbers separated by commas"),
    ({"DRT_DEPTH_CUTS": "0,1"}, "depth 0 is not in 1..max_cast_depth (12)"),
    ({"DRT_DEPTH_CUTS": "1,13"}, "depth 13 is not in 1..max_cast_depth (12)"),
    ({"DRT_DEPTH_CUTS": "4294967297"}, "is not in 1..max_cast_depth (12)"),
    ({"DRT_DEPTH_CUTS": "2,1"}, "not strictly ascending"),
    ({"DRT_DEPTH_CUTS": "1,2,2"}, "not strictly ascending"),
    ({"DRT_DEPTH_CUTS": "1,2,3,4,5,6,7,8,9"}, "8 depths at most"),
    ({"DRT_DEPTH_CUTS": "1,2", "DRT_ADAPTIVE_ERROR": "0.1"}, "DRT_DEPTH_CUTS cannot be combined with DRT_ADAPTIVE_ERROR"),
    ({"DRT_DEPTH_CUTS": "1,2", "DRT_CHECKPOINT_SPP": "1"}, "DRT_DEPTH_CUTS cannot be combined with DRT_CHECKPOINT_SPP"),
    ({"DRT_DEPTH_CUTS": "1,2", "DRT_RESUME": "1"}, "DRT_DEPTH_CUTS cannot be combined with DRT_RESUME"),
    ({"DRT_DEPTH_CUTS": "1,2", "DRT_TURNTABLE": "2"}, "DRT_DEPTH_CUTS cannot be combined with DRT_TURNTABLE"),
    ({"DRT_DEPTH_CUTS": "1,2", "DRT_LIGHT_LEVELS": "1,2"}, "DRT_DEPTH_CUTS cannot be combined with DRT_LIGHT_LEVELS"),
])
def test_the_host_refuses_bad_depth_cuts_before_any_device_call(tmp_path, env, message):
    """Exit status nonzero, the reason on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run that got as
    far as the launcher would fail there with the launcher's message instead (tests/test_features_cpu.py's last test)."""
    cfg, n = re.subn(r"(?m)^max_cast_depth\s+\d+", "max_cast_depth    12", open(os.path.join(REPO, "config.cfg")).read())
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
