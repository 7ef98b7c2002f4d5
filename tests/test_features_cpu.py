"""CPU: the first-hit feature rule (tests/feature_rule.py) against the path it restates -- the surface and the
coverage of the oracle's own hit log -- against a second, sample-by-sample implementation written here, and on the cases that pin
its corners down. Then what needs no device: the struct's layout and the drt_render host's DRT_FEATURES* refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import feature_rule as F
import oracle_py as O
import pydrt

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")
CASES = ["plane_light_16", "plane_light_center", "lights", "lens", "downward", "spheres_1500", "example_scene"]
# pixels whose samples partly hit something, counted on the oracle's hit log
PARTLY_COVERED = {"plane_light_16": 15, "plane_light_center": 0, "lights": 54, "downward": 5, "spheres_1500": 113, "example_scene": 0}

_rule = {}


def rule_of(name):
    """(bundle, params, mean, m2, ids, empty, subnormal quotients) of a case at its own spp, computed once"""
    if name not in _rule:
        bundle, params = cases.load_case(name)
        _rule[name] = (bundle, params) + F.features(bundle, params, n_samples=int(params.spp))
    return _rule[name]


def test_features_struct_matches_the_header():
    T = pydrt.Features
    assert C.sizeof(T) == 32
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [
        ("n_samples", 0), ("first_sample", 4), ("flags", 8), ("empty_pixels", 12), ("rays", 16), ("kernel_ms", 24)]
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    body = re.search(r"typedef struct drt_features\s*\{(.*?)\}\s*drt_features;", header, re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in T._fields_]
    assert int(re.search(r"#define DRT_FEATURE_CHANNELS (\d+)", header).group(1)) == F.CHANNELS == pydrt.FEATURE_CHANNELS


@pytest.mark.parametrize("name", CASES)
def test_the_rule_sees_the_surface_and_the_coverage_of_the_paths_own_hit_log(name):
    bundle, params, mean, m2, ids, empty, sub = rule_of(name)
    assert sub == 0
    spp, P = int(params.spp), int(params.tile_w) * int(params.tile_h)
    hits = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_DEVICE)[3]
    first = hits[:, 0].reshape(spp, P)  # ordered (sample, tile row, tile column)
    assert np.array_equal(ids, first[0])
    hit = (first >= 0).astype(np.float64).T.reshape(P, spp, 1)
    cov, cov_m2, _ = F.running_moments(hit, np.full(P, spp))
    assert cases.same_bits(mean[:, 4], cov[:, 0]), cases.first_difference(mean[:, 4], cov[:, 0])
    assert cases.same_bits(m2[:, 4], cov_m2[:, 0])
    n_hit = (first >= 0).sum(axis=0)
    assert np.array_equal(mean[:, 4] == 0.0, n_hit == 0) and np.array_equal(mean[:, 4] == 1.0, n_hit == spp)
    assert empty == int((n_hit == 0).sum())
    partly = int(((n_hit > 0) & (n_hit < spp)).sum())
    print("%s: %d pixels partly covered, %d empty" % (name, partly, empty))
    if name in PARTLY_COVERED:
        assert partly == PARTLY_COVERED[name]


# ------------------------------------------------------------------------------------------------
# the rule a second time: one sample at a time, numpy scalars
def scalar_features(bundle, params, counts, first_sample):
    L = O.oracle_lib()
    O.set_math_mode(O.MATH_DEVICE)
    f8 = np.float64
    sc, cam = bundle.scene, bundle.camera
    v3 = lambda a: [f8(a[0]), f8(a[1]), f8(a[2])]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    add = lambda a, b: [a[0] + b[0], a[1] + b[1], a[2] + b[2]]
    sub = lambda a, b: [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
    mul = lambda a, f: [f * a[0], f * a[1], f * a[2]]

    def norm(a):
        ln = np.sqrt(dot(a, a))
        return [a[0] / ln, a[1] / ln, a[2] / ln]

    forward, right, up, ap, bl = v3(cam.forward), v3(cam.right), v3(cam.up), v3(cam.aperture_position), v3(cam.film_bottom_left)
    table = F.colour_table(bundle)[0]
    stride = int(params.row_stride) or 1
    P = int(params.tile_w) * int(params.tile_h)
    mean, m2, ids = np.zeros((P, 8)), np.zeros((P, 8)), np.zeros(P, dtype=np.int32)
    out3, cols, pt = (C.c_double * 3)(), (C.c_double * 9)(), O.Point()
    with np.errstate(all="ignore"):
        for p in range(P):
            x = int(params.x0) + p % int(params.tile_w)
            y = int(params.y0) + (p // int(params.tile_w)) * stride
            m, M2 = [f8(0.0)] * 8, [f8(0.0)] * 8
            for k in range(int(counts[p])):
                L.drt_oracle_seed_path(L.drt_oracle_path_key(int(params.seed), int(params.width), int(params.height), x, y, first_sample + k))
                px = py = f8(0.0)
                if int(params.pixel_scheme) == pydrt.FILM_SAMPLE_CENTER:
                    px = py = f8(0.5)
                elif int(params.pixel_scheme) == pydrt.FILM_SAMPLE_RANDOM:
                    px = f8(L.drt_oracle_rng())
                    py = f8(L.drt_oracle_rng())
                film_x = (f8(x) + px) * f8(cam.pixel_width)
                film_y = (f8(y) + py) * f8(cam.pixel_height)
                pixel_point = add(add(mul(right, film_x), mul(up, film_y)), bl)
                if f8(cam.aperture_radius) > 0.0:
                    fd = norm(sub(ap, pixel_point))
                    fd = mul(fd, f8(cam.focal_depth) / dot(fd, forward))
                    focus_point = add(pixel_point, fd)
                    L.drt_oracle_rotation_between((C.c_double * 3)(0.0, 0.0, 1.0), (C.c_double * 3)(*forward), cols)
                    L.drt_oracle_uniform_sample_disc(out3)
                    dp = mul(v3(out3), f8(cam.aperture_radius))
                    lens = [dot([f8(cols[r]), f8(cols[3 + r]), f8(cols[6 + r])], dp) for r in range(3)]
                    ro = add(ap, lens)
                    rd = norm(sub(focus_point, ro))
                else:
                    ro = pixel_point
                    rd = norm(sub(ap, ro))
                idx = L.drt_oracle_find_ray_intersection(C.byref(sc), (C.c_double * 3)(*ro), (C.c_double * 3)(*rd), C.byref(pt))
                if k == 0:
                    ids[p] = idx
                if idx >= 0:
                    d = sub(v3(pt.position), ap)
                    phi = v3(pt.normal) + [d[0] * forward[0] + d[1] * forward[1] + d[2] * forward[2], f8(1.0)] + list(table[int(pt.surface_material)])
                else:
                    phi = [f8(0.0)] * 5 + list(table[int(sc.escape_material)])
                for c in range(8):
                    dd = phi[c] - m[c]
                    m[c] = m[c] + dd / f8(k + 1)
                    M2[c] = M2[c] + dd * (phi[c] - m[c])
            mean[p], m2[p] = m, M2
    return mean, m2, ids


@pytest.mark.parametrize("name", ["plane_light_16", "lens", "example_scene"])
def test_a_scalar_implementation_gives_the_same_bits(name):
    bundle, params, mean, m2, ids, empty, sub = rule_of(name)
    P = int(params.tile_w) * int(params.tile_h)
    mean2, m22, ids2 = scalar_features(bundle, params, np.full(P, int(params.spp)), 0)
    assert cases.same_bits(mean, mean2), cases.first_difference(mean, mean2)
    assert cases.same_bits(m2, m22), cases.first_difference(m2, m22)
    assert np.array_equal(ids, ids2)


def test_a_scalar_implementation_gives_the_same_bits_with_mixed_counts_a_stride_and_a_first_sample():
    bundle, _ = cases.load_case("lights")
    params = pydrt.make_params(32, 32, spp=4, max_depth=6, seed=5, x0=13, y0=3, tile_w=5, tile_h=4, row_stride=3)
    counts = 1 + (np.arange(20) * 7) % 5
    mean, m2, ids, empty, sub = F.features(bundle, params, first_sample=3, counts=counts)
    mean2, m22, ids2 = scalar_features(bundle, params, counts, 3)
    assert sub == 0
    assert cases.same_bits(mean, mean2) and cases.same_bits(m2, m22) and np.array_equal(ids, ids2)
    one = counts == 1
    assert one.any() and not m2[one].any()  # (a single sample has no deviation)


def test_centre_samples_have_no_deviation():
    _, _, mean, m2, ids, empty, sub = rule_of("plane_light_center")
    assert not m2.any()
    hit = ids >= 0
    assert hit.any() and empty == int((~hit).sum())
    assert np.all(mean[hit, 4] == 1.0) and np.all(mean[hit, 3] > 0.0) and not mean[~hit, 0:5].any()
    n = mean[hit, 0:3]
    assert np.allclose(np.sqrt((n * n).sum(axis=1)), 1.0, atol=1e-12)  # (every sample the same normal: the mean is that normal)


def test_a_camera_without_a_field_of_view_sees_nothing_and_no_nan():
    bundle, params, mean, m2, ids, empty, sub = rule_of("example_scene")
    P = int(params.tile_w) * int(params.tile_h)
    assert empty == P and np.all(ids == -1)
    assert not np.isnan(mean).any() and not np.isnan(m2).any()
    assert not mean[:, 0:5].any() and not m2.any()
    escape = F.colour_table(bundle)[0][int(bundle.scene.escape_material)]
    assert np.array_equal(mean[:, 5:8], np.tile(escape, (P, 1)))


def test_the_smallest_nonzero_mean_is_far_from_the_subnormal_range():
    for name in CASES:
        mean = np.abs(rule_of(name)[2])
        assert rule_of(name)[6] == 0
        assert not mean[mean != 0.0].size or mean[mean != 0.0].min() >= 1e-3


def test_the_colour_table_is_the_xyz_of_the_materials_spectra():
    """loosely: spectrum_to_xyz sums in another order"""
    bundle, _ = cases.load_case("plane_light_16")
    sc, spds = bundle.scene, bundle.spds()
    table, sub = F.colour_table(bundle)
    assert sub == 0
    xyz = np.zeros(3)
    zeros = np.zeros(bundle.S)
    seen = 0
    for m in range(int(sc.num_materials)):
        mat = sc.materials[m]
        row = lambda i: spds[i] if i >= 0 else zeros
        r = row(mat.emission_spd) if mat.is_emissive else row(mat.diffuse_spd) + row(mat.glossy_spd) + row(mat.mirror_spd)
        r = np.ascontiguousarray(r)
        O.oracle_lib().drt_oracle_spectrum_to_xyz(C.byref(sc), r.ctypes.data_as(C.POINTER(C.c_double)), xyz.ctypes.data_as(C.POINTER(C.c_double)))
        assert np.allclose(table[m], xyz, rtol=1e-12, atol=1e-15)
        seen += int(table[m].any())
    assert seen >= 3


def test_the_byte_rule_clamps_rounds_and_maps_nan_to_0():
    mean = np.zeros((5, 8))
    mean[:, 3] = [-1.0, 0.0, 0.5, 2.0, np.nan]
    b = F.feature_bgra(mean, 1, 0.0, 1.0)
    assert b[:, 0].tolist() == [0, 0, 128, 255, 0] and np.all(b[:, 3] == 255)
    assert np.array_equal(b[:, 0], b[:, 1]) and np.array_equal(b[:, 1], b[:, 2])
    mean[0, 0:3] = [-1.0, 0.0, 1.0]
    assert F.feature_bgra(mean, 0, -1.0, 1.0)[0].tolist() == [255, 128, 0, 255]  # B, G, R = z, y, x


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env, name", [
    ({"DRT_FEATURES": "2"}, "DRT_FEATURES"),
    ({"DRT_FEATURES": "-1"}, "DRT_FEATURES"),
    ({"DRT_FEATURES": "yes"}, "DRT_FEATURES"),
    ({"DRT_FEATURES": ""}, "DRT_FEATURES"),
    ({"DRT_FEATURES": "1x"}, "DRT_FEATURES"),
    ({"DRT_FEATURES_SPD": "a.spd"}, "DRT_FEATURES_SPD"),
    ({"DRT_FEATURES_M2_SPD": "b.spd"}, "DRT_FEATURES_M2_SPD"),
    ({"DRT_FEATURES": "0", "DRT_FEATURES_SPD": "a.spd"}, "DRT_FEATURES_SPD"),
    ({"DRT_FEATURES": "1", "DRT_FEATURES_SPD": ""}, "DRT_FEATURES_SPD"),
    ({"DRT_FEATURES": "1", "DRT_FEATURES_SPD": "a.spd", "DRT_FEATURES_M2_SPD": "a.spd"}, "DRT_FEATURES_M2_SPD"),
])
def test_the_host_refuses_bad_feature_settings_before_any_device_call(tmp_path, env, name):
    """Exit status nonzero, the variable named on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run
    that got as far as the launcher would fail there with the launcher's message instead."""
    cfg = open(os.path.join(REPO, "config.cfg")).read()
    (tmp_path / "config.cfg").write_text(cfg)
    os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
    os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0
    assert name in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout
