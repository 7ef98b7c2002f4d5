"""Sensor films without a GPU (-m "not gpu"): the premise of the rule on the oracle alone, the summation tree, the C-ABI as the header,
the compiler and pydrt see it, observer_curves, and the host program's refusals.

The rule (tests/sensor_rule.py): the channel value of a sample is its spectrum times the curve, summed by
pairs inside every set of 64 wavelengths and then over the sets in order, and goes through the reference's film update. Its input is
the existing oracle's one-sample render; the premise checked here is that a curve which is 1.0 at one wavelength and 0 elsewhere turns
the rule into the oracle's own film update of that wavelength: all three buffers of its multi-sample film, bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import pydrt
import sensor_cases as SC
import sensor_rule

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")


@pytest.mark.parametrize("name", SC.CPU_CASES)
def test_delta_curves_give_the_oracles_own_film_columns(name):
    bundle, params = SC.load(name)
    S = bundle.S
    w = SC.delta_wavelengths(S)
    samples = SC.samples_cpu(name)
    assert samples.shape == (int(params.spp), int(params.tile_w) * int(params.tile_h), S)
    px, av, va = SC.film_cpu(name)
    got = sensor_rule.sensor_film(SC.delta_curves(S, w), samples)
    want = (np.concatenate([px[:, w], px[:, S:]], axis=1), av[:, w], va[:, w])
    SC.assert_film(got, want, "%s: the rule on delta curves against the oracle's film at wavelengths %s" % (name, list(w)))
    assert np.array_equal(got[0][:, -1], np.full(px.shape[0], float(params.spp)))
    if name != "first_scene":
        assert (va[:, w] != 0).any(), "a film without variance tells nothing about the running mean"


def test_the_tree_is_not_a_left_to_right_sum():
    # 1 + 2^-53 + 2^-53: left to right both halves are rounded away; the pair (2^-53 + 2^-53) = 2^-52 is not
    c = np.zeros((1, 64))
    c[0, 1], c[0, 2], c[0, 3] = 1.0, 2.0 ** -53, 2.0 ** -53
    ones = np.ones((1, 64))
    left = 0.0
    for x in c[0]:
        left = left + x
    assert left == 1.0
    assert sensor_rule.channel_values(ones, c)[0, 0] == 1.0 + 2.0 ** -52
    # the same three values one place to the left pair differently: (0 + 1) + (2^-53 + 2^-53) against (1 + 2^-53) + (2^-53 + 0)
    c2 = np.zeros((1, 64))
    c2[0, 0], c2[0, 1], c2[0, 2] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert sensor_rule.channel_values(ones, c2)[0, 0] == 1.0
    # the curve multiplies before anything is added, and a negative curve value subtracts
    r = np.zeros((1, 64))
    r[0, 4], r[0, 5] = 3.0, -2.0
    c3 = np.zeros((1, 64))
    c3[0, 4], c3[0, 5], c3[0, 6] = 0.5, 0.25, 100.0
    assert sensor_rule.channel_values(r, c3)[0, 0] == 1.0
    # the sets are added in order, after their own trees: (big + -big) + small keeps small, big + (-big + small) would not
    S = 192
    c4 = np.zeros((1, S))
    c4[0, 0], c4[0, 64], c4[0, 128] = 2.0 ** 60, -2.0 ** 60, 1.0
    assert sensor_rule.channel_values(np.ones((1, S)), c4)[0, 0] == 1.0
    c5 = np.zeros((1, S))
    c5[0, 0], c5[0, 64], c5[0, 128] = 1.0, 2.0 ** 60, -2.0 ** 60
    assert sensor_rule.channel_values(np.ones((1, S)), c5)[0, 0] == 0.0


def manual(curve, c):
    """the rule by hand for one pixel and one curve, python floats"""
    S = len(c)
    v = None
    for j in range((S + 63) // 64):
        q = [curve[64 * j + i] * c[64 * j + i] if 64 * j + i < S else 0.0 for i in range(64)]
        while len(q) > 1:
            q = [q[2 * i] + q[2 * i + 1] for i in range(len(q) // 2)]
        v = q[0] if v is None else v + q[0]
    return v


@pytest.mark.parametrize("S", [64, 65, 69, 128])
def test_partial_sets_are_padded_with_positive_zeros(S):
    rng = np.random.default_rng(S)
    curves = rng.uniform(-1.0, 1.0, size=(3, S))
    c = rng.uniform(0.0, 4.0, size=(5, S)) * 10.0 ** rng.integers(-8, 8, size=(5, S))
    v = sensor_rule.channel_values(curves, c)
    assert v.shape == (5, 3)
    for p in range(5):
        for k in range(3):
            assert v[p, k] == manual(list(curves[k]), list(c[p]))
    # the padding is +0.0: a spectrum of -0.0 products sums to -0.0 in a full set, and to +0.0 as soon as one padded zero joins it
    neg = sensor_rule.channel_values(-np.ones((1, S)), np.zeros((1, S)))
    assert neg[0, 0] == 0.0 and bool(np.signbit(neg[0, 0])) == (S % 64 == 0)
    # a wavelength in the last set counts, and one set more than S has would not be looked at
    last = np.zeros((1, S))
    last[0, S - 1] = 7.0
    assert sensor_rule.channel_values(np.ones((1, S)), last)[0, 0] == 7.0


def test_the_film_update_is_the_references():
    v = np.array([[3.0, -1.0]])
    film = sensor_rule.empty_film(1, 2)
    sensor_rule.film_update(film, v, 0)
    sensor_rule.film_update(film, np.array([[1.0, 0.5]]), 1)
    px, av, va = film
    assert np.array_equal(px, [[4.0, -0.5, 2.0]]) and np.array_equal(av, [[2.0, -0.25]]) and np.array_equal(va, [[2.0, 1.125]])
    # sample numbers are absolute: a film continued at sample 2 divides by 3
    sensor_rule.film_update(film, np.array([[2.0, -0.25]]), 2)
    assert np.array_equal(av, [[2.0, -0.25]]) and px[0, 2] == 3.0
    # bytes: clamp, x 255, truncate, NaN to 0, B G R 255
    film = (np.array([[0.5, 2.0, -1.0, 2.0], [np.nan, 0.0, 1.0, 1.0]]), np.array([[0.999, 0.5, 0.25], [0.0, np.nan, 1.0]]), np.zeros((2, 3)))
    # (0 * NaN is NaN: a pixel with one NaN channel is black in every byte, through any matrix)
    assert np.array_equal(sensor_rule.bgra(film, 0, np.eye(3)), [[0, 255, 63, 255], [0, 0, 0, 255]])
    assert np.array_equal(sensor_rule.bgra(film, 1, np.eye(3)), [[63, 127, 254, 255], [0, 0, 0, 255]])
    assert np.array_equal(sensor_rule.bgra(film, 1, [[0, 0, 4], [0, 1, 0], [1, 0, 0]])[0], [254, 127, 255, 255])


def test_the_header_the_compiler_and_pydrt_agree_on_the_calls(tmp_path):
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    calls = ("drt_bind_sensor", "drt_read_sensor_film", "drt_sensor_film_device_ptrs", "drt_read_sensor_bgra", "drt_group_bind_sensor",
             "drt_group_read_sensor_film")
    for call in calls:
        assert re.search(r"\bint %s\(" % call, plain) and call in pydrt.HIP_SYMBOLS, call
    assert re.search(r"#define DRT_MAX_SENSOR_CHANNELS\s+8\b", header) and pydrt.MAX_SENSOR_CHANNELS == 8
    src = tmp_path / "sensor.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "drt_hip.h"\n'
                   'int (*a)(drt_context *, const double *, uint32_t) = drt_bind_sensor;\n'
                   'int (*b)(drt_context *, double *, double *, double *) = drt_read_sensor_film;\n'
                   'int (*c)(drt_context *, void **, void **, void **) = drt_sensor_film_device_ptrs;\n'
                   'int (*d)(drt_context *, int, const double *, uint8_t *) = drt_read_sensor_bgra;\n'
                   'int (*e)(drt_group *, const double *, uint32_t) = drt_group_bind_sensor;\n'
                   'int (*f)(drt_group *, double *, double *, double *) = drt_group_read_sensor_film;\n'
                   'int main(void) { printf("%d\\n", DRT_MAX_SENSOR_CHANNELS); return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "sensor.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = pydrt.hip_lib()
    f64p, vpp = C.POINTER(C.c_double), C.POINTER(C.c_void_p)
    assert L.drt_bind_sensor.argtypes == [C.c_void_p, f64p, C.c_uint32]
    assert L.drt_read_sensor_film.argtypes == [C.c_void_p, f64p, f64p, f64p]
    assert L.drt_sensor_film_device_ptrs.argtypes == [C.c_void_p, vpp, vpp, vpp]
    assert L.drt_read_sensor_bgra.argtypes == [C.c_void_p, C.c_int, f64p, C.POINTER(C.c_uint8)]
    assert L.drt_group_bind_sensor.argtypes == [C.c_void_p, f64p, C.c_uint32]
    assert L.drt_group_read_sensor_film.argtypes == [C.c_void_p, f64p, f64p, f64p]
    # a null context or group is refused with a message, without a device
    assert L.drt_bind_sensor(None, None, 0) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_read_sensor_film(None, None, None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_sensor_film_device_ptrs(None, None, None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_read_sensor_bgra(None, 0, None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_group_bind_sensor(None, None, 0) != 0 and b"null group" in L.drt_last_error()
    assert L.drt_group_read_sensor_film(None, None, None, None) != 0 and b"null group" in L.drt_last_error()


def test_pydrt_checks_the_shapes_it_alone_can_see():
    import inspect
    for cls in (pydrt.Renderer, pydrt.Group):
        assert list(inspect.signature(cls.bind_sensor).parameters) == ["self", "curves"]
        assert list(inspect.signature(cls.read_sensor_film).parameters) == ["self"]
    assert list(inspect.signature(pydrt.Renderer.sensor_film_device_ptrs).parameters) == ["self"]
    assert list(inspect.signature(pydrt.Renderer.read_sensor_bgra).parameters) == ["self", "which", "matrix"]
    assert pydrt._sensor_curves(None, 69) == (None, 0) and pydrt._sensor_curves([], 69) == (None, 0)
    assert pydrt._sensor_curves(np.zeros((0, 69)), 69) == (None, 0)
    a, n = pydrt._sensor_curves([[1] * 69, [2] * 69], 69)
    assert n == 2 and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.shape == (2, 69)
    a, n = pydrt._sensor_curves(np.ones((69, 9)).T, 69)  # nine rows pass here: the count is the library's to refuse, with its reason
    assert n == 9 and a.flags["C_CONTIGUOUS"]
    for bad in (np.zeros(69), np.zeros((2, 68)), np.zeros((2, 3, 69))):
        with pytest.raises(ValueError, match="bind_sensor"):
            pydrt._sensor_curves(bad, 69)
    assert pydrt._sensor_matrix(np.eye(3), 3).dtype == np.float64
    for bad in (np.eye(3), np.zeros((8, 3)), np.zeros(24)):
        with pytest.raises(ValueError, match="read_sensor_bgra"):
            pydrt._sensor_matrix(bad, 8)


def test_observer_curves_are_the_colour_matching_functions_times_the_white():
    bundle, _ = SC.load(SC.BASE)
    spds, sc = bundle.spds(), bundle.scene
    curves = pydrt.observer_curves(bundle)
    assert curves.shape == (3, bundle.S) and curves.dtype == np.float64
    for k, row in enumerate((sc.cmf_x, sc.cmf_y, sc.cmf_z)):
        for s in range(bundle.S):
            assert curves[k, s] == spds[int(row), s] * spds[int(sc.cmf_rw), s]
    # non-negative, but for what the CSV resampling leaves where cmf_z reaches zero (-1.7e-21 at one wavelength): 1e-20 of a row's sum,
    # far below the 2^-53 per term that the comparison of two orders of summation (tests/test_gpu_sensor.py) allows for
    assert (curves > -1e-20).all() and (curves.sum(axis=1) > 1.0).all()
    assert np.array_equal(spds, bundle.spds())


def _curve_csv(path, values):
    path.write_text("wavelength,value\n" + "".join("%d,%g\n" % (wl, v) for wl, v in values))


@pytest.mark.parametrize("env, message", [
    ({"DRT_SENSOR": ""}, "an empty entry"),
    ({"DRT_SENSOR": "r.csv,,b.csv"}, "an empty entry"),
    ({"DRT_SENSOR": "r.csv,g.csv,"}, "an empty entry"),
    ({"DRT_SENSOR": "r.csv,missing.csv"}, "DRT_SENSOR: cannot read missing.csv"),
    ({"DRT_SENSOR": "r.csv,a_directory"}, "DRT_SENSOR: cannot read a_directory"),
    ({"DRT_SENSOR": ",".join(["r.csv"] * 9)}, "DRT_SENSOR: 8 curves at most"),
    ({"DRT_SENSOR": "r.csv", "LONG_NAME": "1"}, "an output name with .sensor.spd behind it is longer than 63 characters"),
    ({"DRT_SENSOR": "r.csv", "DRT_ADAPTIVE_ERROR": "0.1"}, "DRT_SENSOR cannot be combined with DRT_ADAPTIVE_ERROR"),
    ({"DRT_SENSOR": "r.csv", "DRT_CHECKPOINT_SPP": "1"}, "DRT_SENSOR cannot be combined with DRT_CHECKPOINT_SPP"),
    ({"DRT_SENSOR": "r.csv", "DRT_RESUME": "1"}, "DRT_SENSOR cannot be combined with DRT_RESUME"),
    ({"DRT_SENSOR": "r.csv", "DRT_TURNTABLE": "2"}, "DRT_SENSOR cannot be combined with DRT_TURNTABLE"),
    ({"DRT_SENSOR": "r.csv", "DRT_LIGHT_LEVELS": "1,2"}, "DRT_SENSOR cannot be combined with DRT_LIGHT_LEVELS"),
    ({"DRT_SENSOR": "r.csv", "DRT_DEPTH_CUTS": "1,2"}, "DRT_SENSOR cannot be combined with DRT_DEPTH_CUTS"),
    ({"DRT_SENSOR": "r.csv", "DRT_REGIONS": "0,0,4,4:8"}, "DRT_SENSOR cannot be combined with DRT_REGIONS"),
])
def test_the_host_refuses_a_bad_sensor_before_any_device_call(tmp_path, env, message):
    """Exit status nonzero, the reason on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run that got as
    far as the launcher would fail there with the launcher's message instead."""
    cfg = open(os.path.join(REPO, "config.cfg")).read()
    env = dict(env)
    if env.pop("LONG_NAME", None):
        cfg, n = re.subn(r"(?m)^variance_spd\s+\S+", "variance_spd      output/" + "v" * 44 + ".spd", cfg)  # fits by itself, not with .sensor
        assert n == 1
    (tmp_path / "config.cfg").write_text(cfg)
    os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
    os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    _curve_csv(tmp_path / "r.csv", [(380, 0.0), (600, 1.0), (720, 0.5)])
    _curve_csv(tmp_path / "g.csv", [(380, 0.0), (550, 1.0), (720, 0.0)])
    _curve_csv(tmp_path / "b.csv", [(380, 1.0), (450, 1.0), (720, 0.0)])
    (tmp_path / "a_directory").mkdir()
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout
