"""CPU: the variance-guided denoiser's rule (tests/denoise_rule.py) against the adaptive rule, against a second,
pixel-by-pixel implementation written here, on hand-made films that pin its decisions down, and on oracle films for what it is for:
a lower error. Then the refusals that need no device: drt_denoise_buffers' parameters and the drt_render host's DRT_DENOISE_*."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_rule
import cases
import denoise_rule as D
import oracle_py as O
import pydrt

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")
THREADS = max(1, min(8, os.cpu_count() or 1))


def cmf_rows(bundle):
    sc = bundle.scene
    return (int(sc.cmf_rw), int(sc.cmf_x), int(sc.cmf_y), int(sc.cmf_z))


def oracle_film(name, spp, size=None):
    """(bundle, params, pixels, avgs, vars) of a case's scene in DEVICE arithmetic, at `spp` samples and, if given, another size"""
    scene, w, h, _, depth, seed, scheme = cases.RENDER_CASES[name][:7]
    if size:
        w, h = size
    bundle = pydrt.load_scene(cases.scene_path(scene), w, h)
    params = pydrt.make_params(w, h, spp=spp, max_depth=depth, seed=seed, pixel_scheme=scheme)
    px, av, va, _, _ = O.oracle_render_tile(bundle, params, num_threads=THREADS, math_mode=O.MATH_DEVICE)
    return bundle, params, px, av, va


def test_denoise_struct_matches_the_header():
    T = pydrt.Denoise
    assert C.sizeof(T) == 40
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [
        ("radius", 0), ("patch", 4), ("flags", 8), ("unusable", 12), ("k", 16), ("alpha", 24), ("kernel_ms", 32)]
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    body = re.search(r"typedef struct drt_denoise\s*\{(.*?)\}\s*drt_denoise;", header, re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in T._fields_]


def test_the_guide_of_y_is_the_adaptive_rules_luminance_and_error():
    bundle, params, px, av, va = oracle_film("plane_light_16", 4)
    spds, cmf = bundle.spds(), cmf_rows(bundle)
    interval = float(bundle.scene.wavelength_interval)
    G, s, V, nv, ok = D.guide(spds, cmf, interval, px, av, va)
    Y, E = adaptive_rule.luminance_and_error(spds, cmf[0], cmf[2], interval, av, va, 4)
    assert cases.same_bits(G[:, 1], Y), cases.first_difference(G[:, 1], Y)
    assert cases.same_bits(s[:, 1], E), cases.first_difference(s[:, 1], E)
    assert cases.same_bits(V, s * s) and ok.all()


# ------------------------------------------------------------------------------------------------
# the rule a second time: one pixel at a time, numpy scalars (Python's own floats raise on a division by zero)

def scalar_denoise(spds, cmf, interval, w, h, px, av, va, R, F, k, alpha):
    f = np.float64
    S = spds.shape[1]
    rw, rows = spds[cmf[0]], [spds[cmf[1]], spds[cmf[2]], spds[cmf[3]]]
    P = w * h
    with np.errstate(all="ignore"):
        N = f(0.0)
        for i in range(S):
            N = N + rows[1][i] * rw[i]
        N = N * f(interval)
        scale = f(interval) / N
        G, V, nvar, usable = [], [], [], []
        for p in range(P):
            c = f(px[p][S])
            d = c * (c - f(1.0))
            nv = [f(va[p][i]) / d for i in range(S)]
            g3, v3 = [], []
            for ch in range(3):
                g = e = f(0.0)
                for i in range(S):
                    g = g + rows[ch][i] * f(av[p][i]) * rw[i]
                    e = e + rows[ch][i] * np.sqrt(nv[i]) * rw[i]
                g, e = g * scale, e * scale
                g3.append(g)
                v3.append(e * e)
            whole = bool(c >= 2.0) and bool(c < 4294967296.0) and bool(c == np.floor(c))
            usable.append(whole and all(np.isfinite(x) for x in g3 + v3))
            G.append(g3); V.append(v3); nvar.append(nv)
        k2 = f(k) * f(k)

        def at(x, y):
            return y * w + x if 0 <= x < w and 0 <= y < h and usable[y * w + x] else -1

        def e_pair(a, b):
            e = None
            for ch in range(3):
                diff = G[a][ch] - G[b][ch]
                num = diff * diff - f(alpha) * (V[a][ch] + min(V[b][ch], V[a][ch]))
                den = k2 * (V[a][ch] + V[b][ch])
                delta = num / den if den > 0.0 else (f(0.0) if num <= 0.0 else f(np.inf))
                e = delta if e is None else e + delta
            return e

        def falloff(x):
            if not x < 1.0:
                return f(0.0)
            t = f(1.0) - (x if x > 0.0 else f(0.0))
            return t * t

        mean, var = np.empty((P, S)), np.empty((P, S))
        for y in range(h):
            for x in range(w):
                p = y * w + x
                if not usable[p]:
                    mean[p], var[p] = av[p], nvar[p]
                    continue
                Wsum = f(0.0)
                am, avv = [f(0.0)] * S, [f(0.0)] * S
                for dy in range(-R, R + 1):
                    for dx in range(-R, R + 1):
                        q = at(x + dx, y + dy)
                        if q < 0:
                            continue
                        total, n = f(0.0), 0
                        for oy in range(-F, F + 1):
                            for ox in range(-F, F + 1):
                                a, b = at(x + ox, y + oy), at(x + dx + ox, y + dy + oy)
                                if a >= 0 and b >= 0:
                                    total = total + e_pair(a, b)
                                    n += 1
                        wq = min(falloff(total / f(3.0 * n)), falloff(e_pair(p, q) / f(3.0)))
                        Wsum = Wsum + wq
                        for i in range(S):
                            am[i] = am[i] + wq * f(av[q][i])
                            avv[i] = avv[i] + (wq * wq) * nvar[q][i]
                for i in range(S):
                    mean[p][i] = am[i] / Wsum
                    var[p][i] = avv[i] / (Wsum * Wsum)
    return mean, var, P - sum(usable)


def check_against_scalar(spds, cmf, interval, w, h, px, av, va, R, F, k, alpha):
    mean, var, unusable, subnormal = D.denoise(spds, cmf, interval, w, h, px, av, va, R, F, k, alpha)
    m2, v2, u2 = scalar_denoise(spds, cmf, interval, w, h, px, av, va, R, F, k, alpha)
    assert subnormal == 0
    assert unusable == u2
    assert cases.same_bits(mean, m2), cases.first_difference(mean, m2)
    assert cases.same_bits(var, v2), cases.first_difference(var, v2)
    return mean, var, unusable


def test_a_scalar_implementation_gives_the_same_bits_on_an_oracle_film():
    bundle, params, px, av, va = oracle_film("plane_light_16", 8, size=(12, 10))
    check_against_scalar(bundle.spds(), cmf_rows(bundle), float(bundle.scene.wavelength_interval), 12, 10, px, av, va, 5, 1, 1.0, 1.0)


@pytest.mark.parametrize("R, F, k, alpha", [(2, 1, 1.0, 1.0), (3, 0, 0.7, 0.5), (1, 2, 2.0, 0.0)])
def test_a_scalar_implementation_gives_the_same_bits_on_the_hand_made_film(R, F, k, alpha):
    bundle, _ = cases.load_case("grid_10nm")  # S = 35
    px, av, va, w, h = D.hand_made_film(bundle.S)
    mean, var, unusable = check_against_scalar(bundle.spds(), cmf_rows(bundle), float(bundle.scene.wavelength_interval), w, h, px, av,
                                               va, R, F, k, alpha)
    assert unusable == 9  # four counts, five rows
    assert np.isfinite(mean[[7, 8, 16, 40]]).all()  # the all-zero pixels are usable


def test_radius_0_returns_the_mean_and_the_variance_of_the_mean():
    bundle, _ = cases.load_case("grid_10nm")
    S = bundle.S
    px, av, va, w, h = D.hand_made_film(S)
    for F in (0, 2):
        mean, var, unusable, subnormal = D.denoise(bundle.spds(), cmf_rows(bundle), float(bundle.scene.wavelength_interval), w, h, px, av, va,
                                                   0, F, 1.0, 1.0)
        assert subnormal == 0 and unusable == 9
        with np.errstate(all="ignore"):
            c = px[:, S]
            nv = va / (c * (c - 1.0))[:, None]
        assert cases.same_bits(mean, av), cases.first_difference(mean, av)
        assert cases.same_bits(var, nv), cases.first_difference(var, nv)


# a 3-wavelength table for the hand-built cases: rw = 1, x = (1, 0.5, 0.25), y = (1, 2, 1), z = (0.25, 0.5, 1); interval 1 -> N = 4
SPDS = np.array([[1.0, 1.0, 1.0], [1.0, 0.5, 0.25], [1.0, 2.0, 1.0], [0.25, 0.5, 1.0]])
CMF = (0, 1, 2, 3)


def small_film(avg_levels, var_levels, count=4.0):
    """[h][w] levels -> a film whose every wavelength holds the pixel's level"""
    a = np.asarray(avg_levels, dtype=np.float64)
    h, w = a.shape
    av = np.repeat(a.reshape(-1, 1), 3, axis=1)
    va = np.repeat(np.asarray(var_levels, dtype=np.float64).reshape(-1, 1), 3, axis=1)
    px = np.empty((w * h, 4))
    px[:, :3] = av * count
    px[:, 3] = count
    return px, av, va, w, h


def test_a_noise_free_step_edge_keeps_weight_0_across_it():
    levels = np.ones((6, 8)); levels[:, 4:] = 2.0
    px, av, va, w, h = small_film(levels, np.zeros((6, 8)))
    R = 3
    mean, var, unusable, subnormal, weights = D.denoise(SPDS, CMF, 1.0, w, h, px, av, va, R, 1, 1.0, 1.0, want_weights=True)
    assert unusable == 0 and subnormal == 0
    xs = np.arange(w * h) % w
    qi = 0
    crossing = 0
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            across = ((xs < 4) != (xs + dx < 4)) & (xs + dx >= 0) & (xs + dx < w)
            assert (weights[qi][across] == 0.0).all()
            crossing += int(across.sum())
            qi += 1
    assert crossing > 0 and (weights[(2 * R + 1) * R + R] == 1.0).all()  # w(p, p) = 1
    assert cases.same_bits(mean, av) and cases.same_bits(var, np.zeros_like(va))


def test_a_noise_free_bright_pixel_does_not_leak_into_noisy_dark_neighbours():
    """The `lights` failure in miniature. The dark pixels' standard error (50) is half the step to the light (100): the centre pair's
    distance is 3 per channel, but the eight other patch offsets compare dark with dark, -1 per channel each, so the patch mean is
    (9 - 24) / 27 < 0 and, by the patch distance alone, the light would enter its neighbours at full weight."""
    levels = np.ones((7, 7)); levels[3, 3] = 101.0
    spread = np.full((7, 7), 2500.0 * 12.0); spread[3, 3] = 0.0  # var / (c (c - 1)) = 2500 at c = 4
    px, av, va, w, h = small_film(levels, spread)
    mean, var, unusable, subnormal, weights = D.denoise(SPDS, CMF, 1.0, w, h, px, av, va, 2, 1, 1.0, 1.0, want_weights=True)
    assert unusable == 0 and subnormal == 0
    dark = np.ones(w * h, dtype=bool); dark[3 * w + 3] = False
    assert (mean[dark] == 1.0).all()       # sum_q w 1 / W, exactly
    assert (mean[~dark] == 101.0).all()    # and the light keeps to itself
    leaked, _, _, _ = D.denoise(SPDS, CMF, 1.0, w, h, px, av, va, 2, 1, 1.0, 1.0, centre_gate=False)
    # without the gate it does, at full weight: one part light in a window of 25 pixels at most
    assert leaked[dark].max() >= 1.0 + 100.0 / 25.0


def test_unusable_pixels_pass_through_and_contribute_nothing():
    bundle, _ = cases.load_case("grid_10nm")
    S = bundle.S
    spds, cmf, interval = bundle.spds(), cmf_rows(bundle), float(bundle.scene.wavelength_interval)
    px, av, va, w, h = D.hand_made_film(S)
    mean, var, unusable, subnormal, weights = D.denoise(spds, cmf, interval, w, h, px, av, va, 2, 1, 1.0, 1.0, want_weights=True)
    bad = np.array([3, 10, 17, 24, 5, 12, 19, 26, 33])
    with np.errstate(all="ignore"):
        c = px[:, S]
        nv = va / (c * (c - 1.0))[:, None]
    assert cases.same_bits(mean[bad], av[bad]) and cases.same_bits(var[bad], nv[bad])
    assert (weights[:, bad] == 0.0).all()  # as p
    P = w * h
    qi = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            for b in bad:  # as q: the pixel p = q - (dy, dx), if the tile has it
                x, y = b % w - dx, b // w - dy
                if 0 <= x < w and 0 <= y < h:
                    assert weights[qi][y * w + x] == 0.0
            qi += 1
    # whatever the unusable pixels hold changes nothing elsewhere
    av2, va2 = av.copy(), va.copy()
    av2[bad] = 7.0
    va2[bad] = np.inf
    m2, v2, _, _ = D.denoise(spds, cmf, interval, w, h, px, av2, va2, 2, 1, 1.0, 1.0)
    good = np.setdiff1d(np.arange(P), bad)
    assert cases.same_bits(mean[good], m2[good]) and cases.same_bits(var[good], v2[good])


# ------------------------------------------------------------------------------------------------
QUALITY = [("plane_light_48", (64, 64)), ("gold_mirror", None), ("large_box", None), ("lens", None), ("lights", (64, 64)), ("first_scene", None)]


def rel_mse(bundle, mean, ref):
    """mean over pixels of sum_c (a - ref)^2 / (sum_c ref^2 + 1e-4), on the XYZ of the spectra (filter column 1)"""
    def xyz(m):
        return O.oracle_film_to_xyz(bundle, np.concatenate([m, np.ones((m.shape[0], 1))], axis=1))
    a, r = xyz(mean), xyz(ref)
    return float(np.mean(np.sum((a - r) ** 2, axis=1) / (np.sum(r * r, axis=1) + 1e-4)))


@pytest.mark.parametrize("name, size", QUALITY, ids=[q[0] for q in QUALITY])
def test_the_rule_lowers_the_error_of_an_8_sample_film(name, size):
    """8 samples against 512 of the same scene, R 5, F 1, k 1, alpha 1: the relative MSE of XYZ must fall (ratio < 1). Measured:
    plane_light_48 0.56, gold_mirror 0.66, large_box 0.30, lens 0.74, lights 0.61, first_scene 0.54 in the prototype; the figures of
    this test are in DESIGN.md section 5b."""
    bundle, params, px, av, va = oracle_film(name, 8, size)
    _, _, _, ref, _ = oracle_film(name, 512, size)
    mean, var, unusable, subnormal = D.denoise(bundle.spds(), cmf_rows(bundle), float(bundle.scene.wavelength_interval),
                                               int(params.tile_w), int(params.tile_h), px, av, va, 5, 1, 1.0, 1.0)
    noisy, clean = rel_mse(bundle, av, ref), rel_mse(bundle, mean, ref)
    print("%s: relative MSE %.6g noisy, %.6g denoised, ratio %.4f (unusable %d, subnormal quotients %d)"
          % (name, noisy, clean, clean / noisy, unusable, subnormal))
    assert unusable == 0
    assert clean / noisy < 1.0


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, word", [
    (dict(radius=11), "radius"), (dict(patch=4), "patch"), (dict(k=0.0), "k ="), (dict(k=-1.0), "k ="), (dict(k=float("nan")), "k ="),
    (dict(k=float("inf")), "k ="), (dict(alpha=-0.5), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"),
    (dict(mode=pydrt.MODE_XYZ), "DRT_MODE_XYZ"), (dict(row_stride=2), "row_stride"),
])
def test_denoise_buffers_refuses_before_any_device_call(kw, word):
    """no device is visible here: a call that got as far as the device would fail with HIP's message instead"""
    bundle, _ = cases.load_case("grid_10nm")
    S = bundle.S
    params = pydrt.make_params(4, 4, spp=2, max_depth=2, mode=kw.pop("mode", pydrt.MODE_SPECTRAL), row_stride=kw.pop("row_stride", 1))
    px, av, va = np.ones((16, S + 1)) * 2.0, np.ones((16, S)), np.ones((16, S))
    with pytest.raises(RuntimeError) as err:
        pydrt.denoise_buffers(bundle, params, px, av, va, **kw)
    assert "denoise: " in str(err.value) and word in str(err.value), str(err.value)
    assert "hip" not in str(err.value)


@pytest.mark.parametrize("env, name", [
    ({"DRT_DENOISE_K": "0"}, "DRT_DENOISE_K"),
    ({"DRT_DENOISE_K": "-1"}, "DRT_DENOISE_K"),
    ({"DRT_DENOISE_K": "nan"}, "DRT_DENOISE_K"),
    ({"DRT_DENOISE_K": "inf"}, "DRT_DENOISE_K"),
    ({"DRT_DENOISE_K": "1x"}, "DRT_DENOISE_K"),
    ({"DRT_DENOISE_K": ""}, "DRT_DENOISE_K"),
    ({"DRT_DENOISE_K": "1", "DRT_DENOISE_RADIUS": "11"}, "DRT_DENOISE_RADIUS"),
    ({"DRT_DENOISE_K": "1", "DRT_DENOISE_RADIUS": "-1"}, "DRT_DENOISE_RADIUS"),
    ({"DRT_DENOISE_K": "1", "DRT_DENOISE_RADIUS": "2.5"}, "DRT_DENOISE_RADIUS"),
    ({"DRT_DENOISE_K": "1", "DRT_DENOISE_PATCH": "4"}, "DRT_DENOISE_PATCH"),
    ({"DRT_DENOISE_K": "1", "DRT_DENOISE_PATCH": "one"}, "DRT_DENOISE_PATCH"),
    ({"DRT_DENOISE_K": "1", "DRT_DENOISE_ALPHA": "-0.5"}, "DRT_DENOISE_ALPHA"),
    ({"DRT_DENOISE_K": "1", "DRT_DENOISE_ALPHA": "nan"}, "DRT_DENOISE_ALPHA"),
    ({"DRT_DENOISE_K": "1", "DRT_DENOISE_SPD": ""}, "DRT_DENOISE_SPD"),
    ({"DRT_DENOISE_K": "1", "DRT_DENOISE_SPD": "a.spd", "DRT_DENOISE_VAR_SPD": "a.spd"}, "DRT_DENOISE_VAR_SPD"),
    ({"DRT_DENOISE_RADIUS": "3"}, "DRT_DENOISE_RADIUS"),
    ({"DRT_DENOISE_PATCH": "1"}, "DRT_DENOISE_PATCH"),
    ({"DRT_DENOISE_ALPHA": "1"}, "DRT_DENOISE_ALPHA"),
    ({"DRT_DENOISE_SPD": "a.spd"}, "DRT_DENOISE_SPD"),
    ({"DRT_DENOISE_VAR_SPD": "b.spd"}, "DRT_DENOISE_VAR_SPD"),
])
def test_the_host_refuses_bad_denoise_settings_before_any_device_call(tmp_path, env, name):
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
