"""Sensor films (drt_bind_sensor): the shared cases, curves and per-sample spectra.

The rule (tests/sensor_rule.py) needs no oracle code of its own: the contribution of sample m to pixel p is the `pixels` buffer of the
existing oracle's render with spp = 1, first_sample = m onto a zero film (0 + c is c, with -0 becoming +0, which no later step can
tell apart). samples_cpu() makes those through oracle_py.oracle_render_tile(math_mode=MATH_DEVICE) for the tests without a GPU,
samples_device() through cases.oracle_render_device_pow for the GPU tests; both once per (case, changes), shared, and nothing writes
to what they return."""
import numpy as np

import cases
import oracle_py as O
import pydrt
import sensor_rule

# every case is at most 32 x 32 pixels and 4 samples (tests/cases.py)
GPU_CASES = ("plane_light_16", "grid_10nm", "grid_2p5nm", "gold_mirror", "many_lights", "deep_paths", "lens", "first_scene", "spheres_1500",
             "example_scene")
CPU_CASES = ("plane_light_16", "grid_10nm", "grid_2p5nm", "first_scene")
BASE = "plane_light_16"

_bundles, _cpu, _device, _films = {}, {}, {}, {}


def load(name):
    if name not in _bundles:
        _bundles[name] = cases.load_case(name)
    return _bundles[name]


def params_with(params, **changes):
    p = pydrt.Params.from_buffer_copy(params)
    for k, v in changes.items():
        setattr(p, k, v)
    return p


def _key(name, changes):
    return (name, tuple(sorted(changes.items())))


def _tile_pixels(p):
    return int(p.tile_w) * int(p.tile_h)


def samples_cpu(name, **changes):
    """[spp][P][S]: the contribution of every sample of the case, oracle in DEVICE arithmetic with glibc's power"""
    key = _key(name, changes)
    if key not in _cpu:
        bundle, params = load(name)
        p = params_with(params, **changes)
        first, spp = int(p.first_sample), int(p.spp)
        out = []
        for m in range(first, first + spp):
            px = O.oracle_render_tile(bundle, params_with(p, spp=1, first_sample=m), num_threads=16, math_mode=O.MATH_DEVICE)[0]
            out.append(px[:, :-1].copy())
        _cpu[key] = np.stack(out)
    return _cpu[key]


def film_cpu(name):
    """the oracle's own multi-sample film of the case, same arithmetic as samples_cpu"""
    key = ("cpu film", name)
    if key not in _films:
        bundle, params = load(name)
        _films[key] = O.oracle_render_tile(bundle, params, num_threads=16, math_mode=O.MATH_DEVICE)[:3]
    return _films[key]


def samples_device(name, **changes):
    """[spp][P][S] as samples_cpu, with the glossy lobe's power from the device: what the HIP kernels compute bit for bit"""
    key = _key(name, changes)
    if key not in _device:
        bundle, params = load(name)
        p = params_with(params, **changes)
        first, spp = int(p.first_sample), int(p.spp)
        out = []
        for m in range(first, first + spp):
            px = cases.oracle_render_device_pow(bundle, params_with(p, spp=1, first_sample=m), num_threads=16)[0]
            out.append(px[:, :-1].copy())
        _device[key] = np.stack(out)
    return _device[key]


def film_device(name, **changes):
    """(pixels, means, variances, hits, stats) of the oracle's render of the case: what the main film must equal"""
    key = ("device film",) + _key(name, changes)
    if key not in _films:
        bundle, params = load(name)
        _films[key] = cases.oracle_render_device_pow(bundle, params_with(params, **changes), want_hits=True, num_threads=16)
    return _films[key]


def seeded_curves(n, S, seed=0):
    """n curves of S values in [-0.5, 1): negative values included, as an opponent channel has"""
    c = np.random.default_rng(1000 * n + S + seed).uniform(-0.5, 1.0, size=(n, S))
    assert (c < 0).any() and (c > 0).any()
    return c


def delta_wavelengths(S, n=8):
    """n wavelengths spread over all sets of 64, the last (partial) one included"""
    w = np.unique(np.round(np.linspace(0, S - 1, n)).astype(int))
    assert len(w) == n and w[-1] == S - 1 and set(w // 64) == set(range((S + 63) // 64))
    return w


def delta_curves(S, wavelengths):
    c = np.zeros((len(wavelengths), S))
    c[np.arange(len(wavelengths)), wavelengths] = 1.0
    return c


def expected_film(name, curves, **changes):
    """the rule's sensor film for the GPU tests"""
    bundle, params = load(name)
    p = params_with(params, **changes)
    return sensor_rule.sensor_film(curves, samples_device(name, **changes), first_sample=int(p.first_sample))


def assert_film(got, want, what):
    for g, w, buf in zip(got, want, ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s, %s: %s" % (what, buf, cases.first_difference(g, w))
