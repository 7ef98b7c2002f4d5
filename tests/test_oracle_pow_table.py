"""CPU: the oracle's table of the glossy lobe's power (drt_oracle.h, DRT_ORACLE_POW_*).

The GPU tests hold HIP films to the oracle bit for bit by rendering the oracle twice: once collecting every (x, y) the glossy
lobe's pow is called with, once looking each pair up in a table of the device's values (cases.oracle_render_device_pow). Here
the table itself is checked with glibc's own values, so no GPU is needed: it must change nothing but the power, collect the same
pairs at any thread count, be looked up by exact bit pattern, fail loudly on a miss and leave REFERENCE mode alone.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import fuzz_scenes
import oracle_py as O
import pydrt

_libm = C.CDLL("libm.so.6")
_libm.pow.restype = C.c_double
_libm.pow.argtypes = [C.c_double, C.c_double]


def glibc_table(xs, ys):
    return np.array([_libm.pow(float(x), float(y)) for x, y in zip(xs, ys)])


def films_equal(a, b):
    return all(cases.same_bits(u, v) for u, v in zip(a[:3], b[:3]))


def scenes():
    """integer shininess (100), the fuzz scenes' 32.5 and the degenerate scene's 2.5 and 10^6"""
    out = {"plane_light_16": cases.load_case("plane_light_16")}
    bundle, params = fuzz_scenes.load(3, pydrt)
    out["fuzz_3"] = (bundle, params)
    b = pydrt.load_scene_text(cases.degenerate_scenes()["roughness_0_and_odd_shininess"], 16, 16)
    out["odd_shininess"] = (b, pydrt.make_params(16, 16, spp=3, max_depth=6, seed=3))
    return out


@pytest.fixture(scope="module")
def collected():
    """per scene: the DEVICE-mode film with glibc's pow and no table, and the pairs it collected (1 thread)"""
    out = {}
    for name, (bundle, params) in scenes().items():
        plain = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_DEVICE)
        coll = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_DEVICE, pow_collect=True)
        xs, ys = O.oracle_pow_pairs()
        assert films_equal(plain, coll) and np.array_equal(plain[3], coll[3]), name
        out[name] = (bundle, params, plain, xs, ys)
    return out


@pytest.mark.parametrize("threads", [1, 8])
def test_a_table_of_glibcs_values_gives_the_same_film(collected, threads):
    for name, (bundle, params, plain, xs, ys) in collected.items():
        assert xs.size > 100, name
        got = O.oracle_render_tile(bundle, params, want_hits=True, num_threads=threads, math_mode=O.MATH_DEVICE,
                                   pow_table=(xs, ys, glibc_table(xs, ys)))
        assert films_equal(got, plain), (name, threads)
        assert np.array_equal(got[3], plain[3]) and cases.stat_counts(got[4]) == cases.stat_counts(plain[4])
    assert O.oracle_lib().drt_oracle_get_pow_mode() == O.POW_LIBM  # switched off again


def test_collected_pairs_do_not_depend_on_the_thread_count(collected):
    seen_y = set()
    for name, (bundle, params, plain, xs, ys) in collected.items():
        O.oracle_render_tile(bundle, params, num_threads=8, math_mode=O.MATH_DEVICE, pow_collect=True)
        xs8, ys8 = O.oracle_pow_pairs()
        assert np.array_equal(xs.view(np.uint64), xs8.view(np.uint64)) and np.array_equal(ys.view(np.uint64), ys8.view(np.uint64)), name
        keys = np.stack([xs.view(np.uint64), ys.view(np.uint64)], axis=1)
        assert len(np.unique(keys, axis=0)) == len(keys), name  # unique
        assert np.all((xs >= 0.0) & (xs <= 1.0)), name
        seen_y |= set(ys.tolist())
    assert {100.0, 32.5, 2.5, 1e6} <= seen_y


@pytest.mark.parametrize("scene", ["cornell_plane_light.scn", "cornell_gold_mirror.scn"])
def test_a_scene_without_a_glossy_material_collects_nothing(scene):
    """the scene with its plastics made plain diffuse (mirror, glass and gold stay): no pair, at any thread count"""
    text = open(cases.scene_path(scene)).read()
    assert "bp_glossy_bdsf" in text
    bundle = pydrt.load_scene_text(text.replace("bp_diffuse_bdsf, bp_glossy_bdsf", "bp_diffuse_bdsf"), 12, 12)
    params = pydrt.make_params(12, 12, spp=2, max_depth=6, seed=1)
    for threads in (1, 8):
        O.oracle_render_tile(bundle, params, num_threads=threads, math_mode=O.MATH_DEVICE, pow_collect=True)
        xs, ys = O.oracle_pow_pairs()
        assert xs.size == 0 and ys.size == 0
        # and an empty table is enough for it
        O.oracle_render_tile(bundle, params, num_threads=threads, math_mode=O.MATH_DEVICE, pow_table=(xs, ys, xs))


def test_one_entry_one_ulp_off_changes_the_film(collected):
    bundle, params, plain, xs, ys = collected["plane_light_16"]
    vals = glibc_table(xs, ys)
    k = int(np.argmax(vals))  # the brightest highlight's power
    for step in (np.inf, -np.inf):
        moved = vals.copy()
        moved[k] = np.nextafter(moved[k], step)
        got = O.oracle_render_tile(bundle, params, math_mode=O.MATH_DEVICE, pow_table=(xs, ys, moved))
        assert not films_equal(got, plain)
        diff = np.flatnonzero(np.any(got[0] != plain[0], axis=1))
        assert 1 <= diff.size <= 4, diff  # the pixel(s) whose path met that pair, nothing else


def test_a_missing_pair_is_an_error_not_glibcs_value(collected):
    L = O.oracle_lib()
    for name, (bundle, params, plain, xs, ys) in collected.items():
        vals = glibc_table(xs, ys)
        for drop in (0, xs.size - 1):
            keep = np.arange(xs.size) != drop
            for threads in (1, 8):
                with pytest.raises(O.PowTableMiss):
                    O.oracle_render_tile(bundle, params, num_threads=threads, math_mode=O.MATH_DEVICE,
                                         pow_table=(xs[keep], ys[keep], vals[keep]))
                assert L.drt_oracle_pow_misses() >= 1
    # the C entry point itself returns the error
    bundle, params, plain, xs, ys = collected["plane_light_16"]
    O.set_math_mode(O.MATH_DEVICE)
    assert L.drt_oracle_set_pow_table(O._ptr(xs[1:].copy()), O._ptr(ys[1:].copy()), O._ptr(xs[1:].copy()), xs.size - 1) == 0
    L.drt_oracle_set_pow_mode(O.POW_TABLE)
    n = int(params.tile_w) * int(params.tile_h)
    px, av, va = np.zeros((n, bundle.S + 1)), np.zeros((n, bundle.S)), np.zeros((n, bundle.S))
    try:
        rc = L.drt_oracle_render_tile(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(params), O._ptr(px), O._ptr(av), O._ptr(va),
                                      None, None, 4)
    finally:
        L.drt_oracle_set_pow_mode(O.POW_LIBM)
    assert rc == -3 and L.drt_oracle_pow_misses() >= 1
    # a key given twice is refused
    assert L.drt_oracle_set_pow_table(O._ptr(np.array([0.5, 0.5])), O._ptr(np.array([2.0, 2.0])), O._ptr(np.array([0.25, 0.25])), 2) == -2


def test_keys_are_bit_patterns_minus_zero_included():
    """x = -0 (f64_max keeps it) and +0 are different keys; so are the same x under two exponents"""
    bundle, params = cases.load_case("plane_light_16")
    O.oracle_render_tile(bundle, params, math_mode=O.MATH_DEVICE, pow_collect=True)
    xs, ys = O.oracle_pow_pairs()
    vals = glibc_table(xs, ys)
    extra_x, extra_y = np.array([0.0, -0.0, 0.5]), np.array([3.0, 3.0, 2.0])
    want = O.oracle_render_tile(bundle, params, math_mode=O.MATH_DEVICE, pow_table=(xs, ys, vals))
    got = O.oracle_render_tile(bundle, params, math_mode=O.MATH_DEVICE,
                               pow_table=(np.concatenate([xs, extra_x]), np.concatenate([ys, extra_y]), np.concatenate([vals, [7.0, 8.0, 9.0]])))
    assert films_equal(got, want)  # pairs the render never meets are never used


def test_reference_mode_ignores_the_table_and_collects_nothing(golden_dir):
    import os
    bundle, params = cases.load_case("plane_light_16")
    want = O.oracle_render_tile(bundle, params, math_mode=O.MATH_REFERENCE)
    g = np.load(os.path.join(golden_dir, "render_plane_light_16.npz"), allow_pickle=False)
    bogus = (np.array([0.5]), np.array([100.0]), np.array([np.nan]))
    for threads in (1, 8):
        got = O.oracle_render_tile(bundle, params, num_threads=threads, math_mode=O.MATH_REFERENCE, pow_table=bogus)
        assert films_equal(got, want) and O.oracle_lib().drt_oracle_pow_misses() == 0
        O.oracle_render_tile(bundle, params, num_threads=threads, math_mode=O.MATH_REFERENCE, pow_collect=True)
        assert O.oracle_pow_pairs()[0].size == 0
    assert np.array_equal(want[0][:, bundle.S], g["filter"]) and cases.rel_err(want[0], g["pixels"]) <= 1e-12
    if O.ref_available():  # the compiled reference, where it was built: bit for bit
        assert films_equal(got, O.ref_render_tile(bundle, params))
    O.set_math_mode(O.MATH_REFERENCE)
