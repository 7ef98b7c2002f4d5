"""GPU (-m gpu): the HIP path, through the C-ABI, against the CPU oracle on the same seeded inputs.

Bars: closest-hit surface indices, path statistics and RNG draw counts bit-exact; film buffers (sums, filter sums, means,
variances) and the spectral film's per-pixel XYZ BIT FOR BIT against the oracle's DEVICE arithmetic -- NaN for NaN, zeros
with their sign. The glossy lobe's power is the one operation the oracle cannot restate (drt_pow_shininess / ocml's pow
against glibc's): cases.oracle_render_device_pow renders the oracle twice and folds the device's own power in through a
table, and test_glossy_power_against_exact_arithmetic pins that power to the correctly rounded x^n on its own. Against
the golden vectors of the compiled reference (x87 long double where PI comes in) per-pixel XYZ stays within 1e-9
relative (BASELINE.json asks for <= 1e-4); DRT_MODE_XYZ, which folds the spectrum per kernel pair, within 1e-9 too."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import cases
import fuzz_scenes
import oracle_py as O
import pydrt

pytestmark = pytest.mark.gpu

REF_FILM_TOL = 1e-12  # against the compiled reference's own film: x87 arithmetic where PI comes in
REF_XYZ_TOL = 1e-9    # against the compiled reference's golden XYZ, and DRT_MODE_XYZ against the oracle (sums in another order)


def oracle(bundle, params, **kw):
    """the film the HIP path must give bit for bit: the oracle in DEVICE arithmetic with the device's power"""
    return cases.oracle_render_device_pow(bundle, params, **kw)


def assert_same_film(got, want, what=""):
    """(pixels, avgs, vars) -- or any leading part of them -- bit for bit, NaN for NaN, zeros with their sign"""
    for g, w, name in zip(got, want, ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s %s: %s" % (what, name, cases.first_difference(g, w))


def assert_same_xyz(xyz, bundle, pixels, what=""):
    """the device's drt_film_xyz_kernel against drt_oracle_film_to_xyz of the oracle's film: same operations, same order"""
    want = O.oracle_film_to_xyz(bundle, pixels)
    assert cases.same_bits(xyz, want), "%s XYZ: %s" % (what, cases.first_difference(xyz, want))


def hip_render(bundle, params, record_hits=True, batch=None):
    p = pydrt.make_params(int(params.width), int(params.height), spp=int(params.spp), max_depth=int(params.max_depth),
                          seed=int(params.seed), x0=int(params.x0), y0=int(params.y0), tile_w=int(params.tile_w),
                          tile_h=int(params.tile_h), row_stride=int(params.row_stride), first_sample=int(params.first_sample),
                          pixel_scheme=int(params.pixel_scheme), batch_spp=int(params.batch_spp) if batch is None else batch,
                          flags=pydrt.FLAG_RECORD_HITS if record_hits else 0)
    r = pydrt.Renderer(bundle, p)
    r.render()
    px, av, va = r.read_film()
    hits = r.read_hit_indices(int(p.spp)) if record_hits else None
    xyz = r.read_xyz()
    st = r.stats()
    r.close()
    return px, av, va, hits, xyz, st


def test_device_arithmetic_is_ieee_and_matches_the_oracle_spec():
    assert pydrt.hip_lib().drt_device_count() >= 1
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.uniform(0, 100, 100000), 10.0 ** rng.uniform(-300, 300, 100000), [0.0, 1e-320, 4.0]])
    b = np.concatenate([rng.uniform(-3, 3, 100000), 10.0 ** rng.uniform(-150, 150, 100000), [1.0, 3.0, 2.0]])
    assert np.array_equal(pydrt.selftest_arith(0, a), np.sqrt(a)), "f64 sqrt is not correctly rounded"
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(pydrt.selftest_arith(1, a, b), a / b), "f64 divide is not correctly rounded"
    # The one place gfx950's division is NOT the IEEE quotient: results in the SUBNORMAL range (|q| < 2^-1022), where its scaled
    # sequence rounds twice -- a few quotients per million come out one unit (2^-1074) off, never more. No radiance, mean or variance
    # of a film is anywhere near 1e-308 (and the film tolerance is relative to the frame's brightest value), so the chain of evidence
    # of DESIGN.md section 2 is not touched; it is stated and bounded here rather than left to be found.
    sub_a = (rng.integers(1 << 40, 1 << 52, 2_000_000, dtype=np.uint64) << np.uint64(0)).view(np.float64) * rng.choice([-1.0, 1.0], 2_000_000)
    sub_b = rng.integers(2, 4097, 2_000_000).astype(np.float64)
    got, want = pydrt.selftest_arith(1, sub_a, sub_b), sub_a / sub_b
    off = np.abs(got.view(np.int64) - want.view(np.int64))
    assert off.max() <= 1 and np.count_nonzero(off) <= 40, (int(off.max()), int(np.count_nonzero(off)))
    t = np.concatenate([rng.uniform(-1.0, 7.0, 20000), [0.0, np.pi / 4, np.pi / 2, np.pi, 2 * np.pi, 3 * np.pi / 4]])
    sc = pydrt.selftest_arith(2, t).reshape(-1, 2)
    L = O.oracle_lib()
    s_, c_ = C.c_double(), C.c_double()
    for i in range(t.size):
        L.drt_oracle_sincos(float(t[i]), C.byref(s_), C.byref(c_))
        assert sc[i, 0] == s_.value and sc[i, 1] == c_.value
    assert np.abs(sc[:, 0] - np.sin(t)).max() <= 2.3e-16 and np.abs(sc[:, 1] - np.cos(t)).max() <= 2.3e-16
    x = rng.uniform(0, 1, 100000)
    for y in (100.0, 32.0, 16.0, 2.5):
        got, ref = pydrt.selftest_arith(3, x, np.full_like(x, y)), np.power(x, y)
        m = ref > 1e-290
        assert np.max(np.abs(got[m] - ref[m]) / ref[m]) <= 4.5e-16  # pow: within 2 ulp of glibc
    # the glossy lobe's power (drt_pow_shininess: double-double repeated squaring for integer exponents below 1024, i.e. the correctly
    # rounded x^n but for a 2^-98 sliver): within 1 ulp of glibc's pow wherever the result is a normal number and equal to it 19 times
    # in 20 -- glibc's own error bound is 0.52 ulp, so it is glibc that misses the nearest double in the rest; other exponents go to pow()
    xs = np.concatenate([x, [0.0, 1.0, 0.5, np.nextafter(1.0, 0.0), 1e-3, 1e-200]])
    for y in (100.0, 32.0, 1.0, 0.0, 2.0, 3.0, 777.0, 1023.0, 16.0, 2.5, 1024.0, 100.5):
        got, ref = pydrt.selftest_arith(7, xs, np.full_like(xs, y)), np.power(xs, y)
        m = ref > 1e-290
        ulp = np.abs(np.spacing(ref[m]))
        err = np.abs(got[m] - ref[m]) / ulp
        assert np.max(err) <= (1.0 if y == int(y) and y < 1024 else 2.0), (y, float(np.max(err)))
        if y == int(y) and y < 1024:
            assert np.mean(err == 0.0) >= 0.93, (y, float(np.mean(err == 0.0)))
        assert np.all(got[~m] <= 1e-290) and np.all(got[~m] >= 0.0)
    keys = rng.integers(0, 2 ** 62, 5000, dtype=np.uint64)
    got = pydrt.selftest_arith(4, keys.view(np.float64))
    for i in range(0, 5000, 7):
        L.drt_oracle_seed_path(int(keys[i]))
        v = [L.drt_oracle_rng() for _ in range(4)][-1]
        assert got[i] == v


POW_EXPONENTS = (0, 1, 2, 3, 8, 12, 16, 20, 32, 50, 100, 255, 511, 1000, 1023)


def _pow_bases(n, rng):
    """bases in [0, 1] for x^n: the ends (0, -0, 1, 1 - 2^-53, the least subnormal), uniform values, values just below 1, and
    values whose n-th power lands near 2^-1022 (normal / subnormal), inside the subnormals and near 2^-1075 (subnormal / zero)"""
    one_minus = 1.0 - np.arange(1, 65) * 2.0 ** -53
    x = [np.array([0.0, -0.0, 1.0, np.nextafter(1.0, 0.0), 5e-324, 0.5, 2.0 ** -60]), rng.uniform(0.0, 1.0, 1500), one_minus,
         1.0 - rng.uniform(0.0, 1e-6, 200)]
    if n >= 1:
        for e in (1022.0, 1074.0, 1075.0):
            edge = 2.0 ** (-e / n)
            x.append(edge * (1.0 + rng.uniform(-2e-3, 2e-3, 300)))
            x.append(edge + np.arange(-20, 21) * np.spacing(edge))
        x.append(2.0 ** (-rng.uniform(1000.0, 1080.0, 300) / n))
    x = np.concatenate(x)
    return x[(x >= 0.0) & (x <= 1.0)]


def _nearest_pow(x, n):
    """x^n rounded to the nearest double (ties to even) from exact rational arithmetic, with IEEE's zeros: pow(-0, odd n) = -0"""
    if x == 0.0:
        return 1.0 if n == 0 else (x if n % 2 else 0.0)
    return float(Fraction(x) ** n)  # int / int true division: correctly rounded, subnormals included


def test_glossy_power_against_exact_arithmetic():
    """drt_pow_shininess (csrc/drt_device.h, through drt_selftest_arith op 7) -- the power the HIP films carry and the oracle now
    takes from the device -- against x^n in exact rational arithmetic rounded to the nearest double, for integer exponents up to
    1023 on thousands of bases each, clustered where the result crosses 2^-1022 and 2^-1075:
      x^n >= 2^-969:           the nearest double, every time (the double-double carries ~2^-98 relative);
      2^-1022 <= x^n < 2^-969:  within 1 ulp (the low word is subnormal there and loses bits: about one result in five is
                               the other neighbour of x^n);
      x^n < 2^-1022:           within one unit of 2^-1074 of the nearest subnormal or 0;
    and x = +-0 gives IEEE's values -- but +0 where IEEE and glibc give pow(-0, odd n) = -0: the double-double products drop the
    sign of a zero. That +0 cannot reach a film: bdsf() adds the glossy term to a reflectance that starts at +0 (src/daily_ray_trace.c:
    215-229, Q1 included), and -0 + +0 = +0, so either sign gives the same bits; the oracle now takes the device's value anyway. It
    is pinned here so that a change to it is seen. The counts are printed. Exponents it hands to ocml's pow (non-integer, >= 1024,
    and bases outside [0, 1]) give ocml's pow bit for bit."""
    rng = np.random.default_rng(1234)
    n_normal = n_exact = n_low = n_low_exact = n_sub = 0
    worst_normal = worst_sub = 0
    for n in POW_EXPONENTS:
        xs = _pow_bases(n, rng)
        got = pydrt.selftest_arith(7, xs, np.full_like(xs, float(n)))
        want = np.array([_nearest_pow(float(x), n) for x in xs])
        z = xs == 0.0
        assert np.array_equal(got[z], want[z]) and not np.signbit(got[z]).any(), "n %d, x = +-0: %s" % (n, got[z].tolist())
        assert (n % 2 == 1) == bool(np.signbit(want[z]).any())  # -0 is among the bases: for odd n IEEE's result is -0
        xs, got, want = xs[~z], got[~z], want[~z]
        off = np.abs(got.view(np.int64) - want.view(np.int64))  # both >= +0: the distance in units in the last place
        normal = want >= 2.0 ** -1022
        high = want >= 2.0 ** -969
        n_normal += int(normal.sum())
        n_exact += int((off[normal] == 0).sum())
        n_low += int((normal & ~high).sum())
        n_low_exact += int((off[normal & ~high] == 0).sum())
        n_sub += int((~normal).sum())
        worst_normal = max(worst_normal, int(off[normal].max(initial=0)))
        worst_sub = max(worst_sub, int(off[~normal].max(initial=0)))
        for m, bound, what in ((high, 0, ">= 2^-969"), (normal, 1, "normal"), (~normal, 1, "below 2^-1022")):
            k = int(np.argmax(np.where(m, off, -1)))
            assert not m.any() or off[k] <= bound, "n %d, %s: %r ^ n = %r, nearest double %r" % (n, what, xs[k], got[k], want[k])
    print("glossy power: %d normal results, %d (%.4f %%) the nearest double (%d of the %d below 2^-969), worst %d ulp; "
          "%d results below 2^-1022, worst %d units of 2^-1074" % (n_normal, n_exact, 100.0 * n_exact / n_normal, n_low_exact, n_low,
                                                                  worst_normal, n_sub, worst_sub))
    assert n_normal > 25000 and n_low > 3000 and n_sub > 12000
    # what goes to ocml's pow goes there whole
    x = np.concatenate([rng.uniform(0.0, 1.0, 2000), [0.0, -0.0, 1.0, 0.5]])
    outside = np.array([np.nextafter(1.0, 2.0), 1.5, 2.0, -0.5, -1e-300, -5e-324, np.nextafter(-1.0, -2.0), 1e300])
    for y in (2.5, 32.5, 1024.0, 1e6, 100.5, -1.0):
        ys = np.full_like(x, y)
        assert cases.same_bits(pydrt.selftest_arith(7, x, ys), pydrt.selftest_arith(3, x, ys)), y
    for y in (0.0, 1.0, 2.0, 3.0, 16.0, 100.0, 1023.0, 2.5, 1e6):
        ys = np.full_like(outside, y)
        assert cases.same_bits(pydrt.selftest_arith(7, outside, ys), pydrt.selftest_arith(3, outside, ys)), y


def _xorshift(x):
    x ^= (x << 13) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 7
    x ^= (x << 17) & 0xFFFFFFFFFFFFFFFF
    return x


def test_device_functions_on_the_reference_edge_cases(golden_dir):
    """The path's __device__ functions, called one by one through drt_selftest_unit, on the reference's own outputs
    (tests/golden/unit_*.npz: tangent, behind, parallel and on-boundary rays, total internal reflection, antiparallel
    rotation ...): bit-exact wherever the function is + - x / sqrt only, bit-exact against the oracle's DEVICE arithmetic
    and within 1e-13 of the reference where PI or sin/cos come in (x87 long double there)."""
    def g_load(name):
        return np.load(os.path.join(golden_dir, name), allow_pickle=False)

    L = O.oracle_lib()
    g = g_load("unit_geometry.npz")
    # intersectors (src/geometry.c:123-182)
    sph = pydrt.selftest_unit(pydrt.UNIT_LINE_SPHERE, np.hstack([g["sph_o"], g["sph_d"], g["sph_c"], g["sph_r"][:, None]]))[:, 0]
    assert np.array_equal(sph, g["sph_t"]) and np.isinf(sph).any() and (sph == 0.0).any()
    pl = pydrt.selftest_unit(pydrt.UNIT_LINE_PLANE, np.hstack([g["pl_o"], g["pl_d"], g["pl_p"], g["pl_n"], g["pl_u"], g["pl_v"]]))[:, 0]
    assert np.array_equal(pl, g["pl_t"]) and np.isinf(pl[910:930]).all() and np.all(pl[900:907] == 1.0)
    # hand-made edge cases against the oracle: tangent ray, origin inside / on the sphere, sphere behind; plane hit exactly on
    # its edges and corners (inclusive bounds), parallel ray, plane behind
    e_s = np.array([[0, 1, 5, 0, 0, -1, 0, 0, 0, 1], [0, 0, 0, 0, 0, -1, 0, 0, 0, 1], [0, 0, 1, 0, 0, -1, 0, 0, 0, 1],
                    [0, 0, -3, 0, 0, -1, 0, 0, 0, 1], [0, 1 + 1e-16, 5, 0, 0, -1, 0, 0, 0, 1], [0.6, 0.8, 5, 0, 0, -1, 0, 0, 0, 1]], dtype=np.float64)
    want = [L.drt_oracle_line_sphere(O._v3(r[0:3]), O._v3(r[3:6]), O._v3(r[6:9]), float(r[9])) for r in e_s]
    assert np.array_equal(pydrt.selftest_unit(pydrt.UNIT_LINE_SPHERE, e_s)[:, 0], np.array(want))
    pp, pn, pu, pv = [-0.5, -0.5, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0]
    e_p = np.array([[x, y, 1, 0, 0, dz] + pp + pn + pu + pv for (x, y, dz) in
                    ((-0.5, -0.5, -1), (0.5, 0.5, -1), (0.5, -0.5, -1), (0.5 + 1e-16, 0, -1), (0.5000001, 0, -1), (0, 0, 1), (0, -0.5, -1))]
                   + [[0, 0, 1, 1, 0, 0] + pp + pn + pu + pv], dtype=np.float64)
    want = [L.drt_oracle_line_plane(O._v3(r[0:3]), O._v3(r[3:6]), O._v3(r[6:9]), O._v3(r[9:12]), O._v3(r[12:15]), O._v3(r[15:18])) for r in e_p]
    got = pydrt.selftest_unit(pydrt.UNIT_LINE_PLANE, e_p)[:, 0]
    assert np.array_equal(got, np.array(want)) and got[0] == 1.0 and got[1] == 1.0 and np.isinf(got[4]) and np.isinf(got[5]) and np.isinf(got[7])
    # reflect / transmit (NaN on total internal reflection) / Rodrigues rotation (antiparallel -> -I)
    assert np.array_equal(pydrt.selftest_unit(pydrt.UNIT_REFLECT, np.hstack([g["rf_v"], g["rf_n"]])), g["rf_reflect"])
    tr = pydrt.selftest_unit(pydrt.UNIT_TRANSMIT, np.hstack([g["rf_v"], g["rf_n"], g["rf_ir"][:, None], g["rf_tr"][:, None]]))
    assert np.array_equal(tr, g["rf_transmit"], equal_nan=True) and np.isnan(tr).any()
    z = np.tile([0.0, 0.0, 1.0], (len(g["rot_w"]), 1))
    rot = pydrt.selftest_unit(pydrt.UNIT_ROTATION_BETWEEN, np.hstack([z, g["rot_w"]]))
    assert np.array_equal(rot, g["rot_m"]) and np.array_equal(rot[0], -np.eye(3).ravel())
    same = pydrt.selftest_unit(pydrt.UNIT_ROTATION_BETWEEN, np.array([[0, 0, 1, 0, 0, 1], [0, 0, 1, 0, 0, -1]], dtype=np.float64))
    assert np.array_equal(same[0], np.eye(3).ravel()) and np.array_equal(same[1], -np.eye(3).ravel())

    # seeding, first draw, shape samplers (src/rng.c) -- the fixture's flow: seed, rng(), sphere (2 draws), disc (2 draws)
    q = g_load("unit_sampling.npz")
    sd = pydrt.selftest_unit(pydrt.UNIT_SEED_AND_DRAW, q["keys"].view(np.float64))
    assert np.array_equal(sd[:, 0].copy().view(np.uint64), q["state"]) and np.array_equal(sd[:, 1], q["first"])
    s1 = np.array([_xorshift(int(x)) for x in q["state"]], dtype=np.uint64)
    sph = pydrt.selftest_unit(pydrt.UNIT_SAMPLE_SPHERE, s1.view(np.float64))
    s3 = sph[:, 3].copy().view(np.uint64)
    disc = pydrt.selftest_unit(pydrt.UNIT_SAMPLE_DISC, s3.view(np.float64))
    assert np.array_equal(disc[:, 3].copy().view(np.uint64), q["state_after"])
    np.testing.assert_allclose(sph[:, :3], q["sphere"], rtol=1e-13, atol=2e-15)  # unit vectors: absolute error of the f64 vs x87 sincos argument
    np.testing.assert_allclose(disc[:, :3], q["disc"], rtol=1e-13, atol=2e-15)
    O.set_math_mode(O.MATH_DEVICE)
    out = np.zeros(3)
    for i in range(0, len(s1), 5):
        L.drt_oracle_set_rng_state(int(s1[i]))
        L.drt_oracle_uniform_sample_sphere(O._ptr(out))
        assert np.array_equal(out, sph[i, :3])
        L.drt_oracle_uniform_sample_disc(O._ptr(out))
        assert np.array_equal(out, disc[i, :3])
    # GGX (src/bdsf.c:3-42) and the Fresnel loop bodies (:44-101)
    sp = g_load("unit_spectral.npz")
    d = pydrt.selftest_unit(pydrt.UNIT_GGX, np.hstack([sp["ggx_sn"], sp["ggx_mn"], sp["ggx_rough"][:, None]]))[:, 0]
    da = pydrt.selftest_unit(pydrt.UNIT_GGX_ATT, np.hstack([sp["ggx_v"], sp["ggx_sn"], sp["ggx_mn"], sp["ggx_rough"][:, None]]))[:, 0]
    np.testing.assert_allclose(d, sp["ggx"], rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(da, sp["ggx_att"], rtol=1e-13, atol=1e-300)
    for i in range(len(d)):
        a = L.drt_oracle_ggx(O._v3(sp["ggx_sn"][i]), O._v3(sp["ggx_mn"][i]), float(sp["ggx_rough"][i]))
        b = L.drt_oracle_ggx_att(O._v3(sp["ggx_v"][i]), O._v3(sp["ggx_sn"][i]), O._v3(sp["ggx_mn"][i]), float(sp["ggx_rough"][i]))
        assert a == d[i] and b == da[i]
    O.set_math_mode(O.MATH_REFERENCE)
    S = len(sp["glass"])
    cos = np.repeat(sp["cosines"], S)
    vac, glass, au_n, au_k = (np.tile(sp[k], len(sp["cosines"])) for k in ("vac", "glass", "au_n", "au_k"))
    r_out = pydrt.selftest_unit(pydrt.UNIT_FS_DIELECTRIC, np.stack([vac, glass, cos], axis=1))[:, 0].reshape(-1, S)
    r_in = pydrt.selftest_unit(pydrt.UNIT_FS_DIELECTRIC, np.stack([glass, vac, cos], axis=1))[:, 0].reshape(-1, S)
    r_c = pydrt.selftest_unit(pydrt.UNIT_FS_CONDUCTOR, np.stack([vac, au_n, au_k, cos], axis=1))[:, 0].reshape(-1, S)
    assert np.array_equal(r_out, sp["diel_r"]) and np.array_equal(r_in, sp["diel_r_inside"]) and np.array_equal(r_c, sp["cond_r"])
    assert (r_in == 1.0).any()  # the total-internal-reflection branch
    # argument checks: records narrower than the function reads are refused, not read past
    with pytest.raises(RuntimeError):
        pydrt.selftest_unit(pydrt.UNIT_LINE_PLANE, np.zeros((4, 10)))


@pytest.mark.parametrize("name", list(cases.RENDER_CASES))
def test_hip_matches_oracle_and_golden(name, golden_dir):
    bundle, params = cases.load_case(name)
    px, av, va, hits, xyz, st = hip_render(bundle, params)
    opx, oav, ova, ohits, ost = oracle(bundle, params, want_hits=True)
    assert np.array_equal(hits, ohits), "%d closest-hit indices differ" % int((hits != ohits).sum())
    assert (st.paths, st.closest_hit_scans, st.shaded_vertices, st.shadow_scans, st.rng_draws) == \
           (ost.paths, ost.closest_hit_scans, ost.shaded_vertices, ost.shadow_scans, ost.rng_draws)
    S = bundle.S
    assert_same_film((px, av, va), (opx, oav, ova), name)
    assert_same_xyz(xyz, bundle, opx, name)
    g = np.load(os.path.join(golden_dir, "render_%s.npz" % name), allow_pickle=False)
    assert cases.xyz_rel_err(xyz, g["xyz"]) <= REF_XYZ_TOL  # against the compiled reference (north star: 1e-4)
    if "hits" in g.files:
        assert np.array_equal(hits, g["hits"])  # bit-exact hit-primitive indices against the reference
    for got, key in ((px[:, :S].sum(axis=1), "pix_sum"), (av.sum(axis=1), "avg_sum"), (va.sum(axis=1), "var_sum")):
        assert cases.rel_err(got, g[key]) <= 1e-11


@pytest.mark.parametrize("seed", fuzz_scenes.FUZZ_SEEDS)
def test_random_scenes_match_the_oracle(seed):
    """Random scenes (tests/fuzz_scenes.py): hit indices, statistics and RNG draws exact, film and XYZ bit for bit, NaN for NaN
    (total internal reflection propagates NaN through a path in the reference, src/geometry.c:92-106)."""
    bundle, params = fuzz_scenes.load(seed, pydrt)
    px, av, va, hits, xyz, st = hip_render(bundle, params)
    opx, oav, ova, ohits, ost = oracle(bundle, params, want_hits=True)
    assert np.array_equal(hits, ohits), "%d closest-hit indices differ" % int((hits != ohits).sum())
    assert (st.paths, st.closest_hit_scans, st.shaded_vertices, st.shadow_scans, st.rng_draws) == \
           (ost.paths, ost.closest_hit_scans, ost.shaded_vertices, ost.shadow_scans, ost.rng_draws)
    assert_same_film((px, av, va), (opx, oav, ova), "seed %d" % seed)
    assert_same_xyz(xyz, bundle, opx, "seed %d" % seed)


@pytest.mark.parametrize("S", list(fuzz_scenes.FUZZ_GRIDS))
def test_random_scenes_on_other_wavelength_grids(S):
    """Random scenes on grids from 2 to 256 wavelengths: every lane-set count of the shade kernel (1-4), tails of 1, 6, 16
    wavelengths (packed pass) and 17 (a further set instead), in spectral and XYZ film mode."""
    grid = fuzz_scenes.FUZZ_GRIDS[S]
    for seed in (3 + S % 7, 101):
        bundle, params = fuzz_scenes.load(seed, pydrt, grid)
        assert bundle.S == S
        px, av, va, hits, xyz, st = hip_render(bundle, params)
        opx, oav, ova, ohits, ost = oracle(bundle, params, want_hits=True)
        assert np.array_equal(hits, ohits) and st.rng_draws == ost.rng_draws
        assert_same_film((px, av, va), (opx, oav, ova), "S %d seed %d" % (S, seed))
        assert_same_xyz(xyz, bundle, opx, "S %d seed %d" % (S, seed))
        p = pydrt.make_params(int(params.width), int(params.height), spp=int(params.spp), max_depth=int(params.max_depth),
                              seed=int(params.seed), mode=pydrt.MODE_XYZ)
        r = pydrt.Renderer(bundle, p)
        r.render()
        xyz2 = r.read_xyz()
        r.close()
        ok = np.isfinite(xyz).all(axis=1)
        assert np.array_equal(ok, np.isfinite(xyz2).all(axis=1))
        assert cases.xyz_rel_err(xyz2[ok], xyz[ok]) <= 1e-11


@pytest.mark.parametrize("trial", range(16))
def test_random_tiles_batches_and_sample_splits(trial):
    """Random image shapes (not square), tile rectangles, row strides, depths, pixel schemes, batch sizes and splits of the
    samples over several drt_render calls, on random scenes: always the oracle's film for exactly that tile."""
    r = np.random.default_rng(7000 + trial)
    w, h = int(r.integers(5, 40)), int(r.integers(5, 40))
    stride = int(r.integers(1, 4))
    tile_w = int(r.integers(1, w + 1)); x0 = int(r.integers(0, w - tile_w + 1))
    y0 = int(r.integers(0, h))
    tile_h = int(r.integers(1, (h - 1 - y0) // stride + 2))
    spp, first = int(r.integers(1, 9)), int(r.integers(0, 5))
    depth = int(r.choice([1, 2, 3, 8, 17]))
    scheme = int(r.choice([pydrt.FILM_SAMPLE_RANDOM, pydrt.FILM_SAMPLE_CENTER]))
    seed = int(r.integers(1, 2 ** 40))
    text = fuzz_scenes.random_scene_text(int(r.choice([4, 9, 16, 23, 103])))
    bundle = pydrt.load_scene_text(text, w, h)
    base = dict(spp=spp, max_depth=depth, seed=seed, x0=x0, y0=y0, tile_w=tile_w, tile_h=tile_h, row_stride=stride,
                first_sample=first, pixel_scheme=scheme)
    p = pydrt.make_params(w, h, batch_spp=int(r.integers(0, 6)), **base)
    ren = pydrt.Renderer(bundle, p)
    done = 0
    while done < spp:  # the samples in random pieces
        n = int(r.integers(1, spp - done + 1))
        ren.render(first + done, n)
        done += n
    px, av, va = ren.read_film()
    st = ren.stats()
    ren.close()
    opx, oav, ova, _, ost = oracle(bundle, pydrt.make_params(w, h, **base))
    assert (st.paths, st.closest_hit_scans, st.rng_draws) == (ost.paths, ost.closest_hit_scans, ost.rng_draws)
    assert_same_film((px, av, va), (opx, oav, ova), "trial %d" % trial)


def test_batching_resume_and_tiles_do_not_change_a_bit():
    bundle, params = cases.load_case("plane_light_48")
    base = hip_render(bundle, params, batch=4)
    opx, oav, ova, ohits, _ = oracle(bundle, params, want_hits=True, num_threads=8)
    assert np.array_equal(base[3], ohits)
    assert_same_film(base[:3], (opx, oav, ova))
    assert_same_xyz(base[4], bundle, opx)
    for batch in (1, 3):
        other = hip_render(bundle, params, batch=batch)
        for a, b in zip(base[:5], other[:5]):
            assert np.array_equal(a, b)
    # resume: samples [0,2) then [2,4) on the same film == [0,4)
    p = pydrt.make_params(48, 48, spp=4, max_depth=8, seed=1, batch_spp=2)
    r = pydrt.Renderer(bundle, p)
    r.render(0, 2)
    r.render(2, 2)
    px, av, va = r.read_film()
    r.close()
    assert np.array_equal(px, base[0]) and np.array_equal(av, base[1]) and np.array_equal(va, base[2])
    # row-cyclic tiles (the multi-GPU partition) reassemble to the full frame
    S = bundle.S
    full = base[0].reshape(48, 48, S + 1)
    for rank in range(3):
        pt = pydrt.make_params(48, 48, spp=4, max_depth=8, seed=1, y0=rank, tile_h=16, row_stride=3)
        tpx = hip_render(bundle, pt, record_hits=False)[0]
        assert np.array_equal(tpx.reshape(16, 48, S + 1), full[rank::3])
    # a sub-rectangle
    pt = pydrt.make_params(48, 48, spp=4, max_depth=8, seed=1, x0=8, y0=4, tile_w=24, tile_h=10)
    tpx = hip_render(bundle, pt, record_hits=False)[0]
    assert np.array_equal(tpx.reshape(10, 24, S + 1), full[4:14, 8:32])


def test_long_batches_and_work_queue_shapes_do_not_change_a_bit(monkeypatch):
    """More than 64 samples per kernel pair (the shade kernel walks a pixel's samples in windows of 64) and every shape of
    the shade work queue (one item per pixel group; main pass in pieces with the tail pass as an item of its own, at several
    piece sizes and tail spacings) give the same film, bit for bit, and the oracle's."""
    bundle, _ = cases.load_case("plane_light_16")
    params = pydrt.make_params(16, 16, spp=150, max_depth=8, seed=3)
    base = hip_render(bundle, params, batch=32)
    opx, oav, ova, ohits, _ = oracle(bundle, params, want_hits=True, num_threads=8)
    assert np.array_equal(base[3], ohits)
    assert_same_film(base[:3], (opx, oav, ova))
    assert_same_xyz(base[4], bundle, opx)
    for batch in (100, 150, 64, 65):
        other = hip_render(bundle, params, batch=batch)
        for a, b in zip(base[:5], other[:5]):
            assert np.array_equal(a, b), "batch %d" % batch
    # 256 samples of a pixel in one kernel pair (what a resident context takes on the 1024^2 frame: four windows of 64), and 300 in two
    p300 = pydrt.make_params(16, 16, spp=300, max_depth=8, seed=3)
    ref300 = hip_render(bundle, p300, batch=32)
    for batch in (256, pydrt.BATCH_RESIDENT):
        other = hip_render(bundle, p300, batch=batch)
        for a, b in zip(ref300[:5], other[:5]):
            assert np.array_equal(a, b), "batch %d of 300" % batch
    for subs, period in ((0, 0), (1, 0), (3, 1), (5, 2), (12, 0), (12, 12)):
        monkeypatch.setenv("DRT_SHADE_SUBS", str(subs))
        monkeypatch.setenv("DRT_TAIL_PERIOD", str(period))
        monkeypatch.setenv("DRT_TRACE_CHUNK", "64" if subs % 2 else "4096")
        other = hip_render(bundle, params, batch=70)
        for a, b in zip(base[:5], other[:5]):
            assert np.array_equal(a, b), "subs %d period %d" % (subs, period)
    # a grid without a tail pass (64 wavelengths): pieces of the 16-pixel groups
    monkeypatch.delenv("DRT_TAIL_PERIOD")
    b64 = pydrt.load_scene(os.path.join(cases.REPO, "scenes", "cornell_plane_light.scn"), 16, 16, min_wl=380.0, max_wl=695.0, wl_interval=5.0)
    assert b64.S == 64
    p64 = pydrt.make_params(16, 16, spp=70, max_depth=8, seed=3)
    monkeypatch.setenv("DRT_SHADE_SUBS", "0")
    ref64 = hip_render(b64, p64, batch=70)
    for subs in (2, 16):
        monkeypatch.setenv("DRT_SHADE_SUBS", str(subs))
        other = hip_render(b64, p64, batch=33)
        for a, b in zip(ref64[:5], other[:5]):
            assert np.array_equal(a, b), "S=64 subs %d" % subs


def test_one_shot_call_in_row_blocks_is_the_same_film(monkeypatch):
    """drt_render_tile() renders a large tile (2^18 pixels and more) in row blocks, each with all its samples, so that a block's film rows
    cross PCIe while the next block renders. In eight blocks, seven, two with a record pool that runs out on the way (the fall-back:
    render again, fetch the film whole) and in one piece, the film is the session form's, bit for bit."""
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 512, 512)
    p = pydrt.make_params(512, 512, spp=35, max_depth=6, seed=11, batch_spp=16)
    r = pydrt.Renderer(bundle, p)
    r.render(0, 35)
    want = r.read_film()
    st0 = r.stats()
    r.close()
    S = bundle.S
    for y0 in (0, 255, 504):  # bands of rows at the top, across the middle and at the bottom of the frame against the oracle
        pt = pydrt.make_params(512, 512, spp=35, max_depth=6, seed=11, y0=y0, tile_h=8)
        o = oracle(bundle, pt, num_threads=16)
        rows = slice(y0 * 512, (y0 + 8) * 512)
        assert_same_film((want[0][rows], want[1][rows], want[2][rows]), o[:3], "rows %d.." % y0)
    for env in ({}, {"DRT_ONESHOT_BLOCKS": "1"}, {"DRT_ONESHOT_BLOCKS": "7"}, {"DRT_POOL_BLOCKS": "1", "DRT_ONESHOT_BLOCKS": "2"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for flags in (pydrt.FLAG_FILM_ZERO, 0):
            p1 = pydrt.make_params(512, 512, spp=35, max_depth=6, seed=11, batch_spp=16, flags=flags)
            px, av, va, st = pydrt.render_tile(bundle, p1)
            assert np.array_equal(px, want[0]) and np.array_equal(av, want[1]) and np.array_equal(va, want[2]), (env, flags)
            assert (st.paths, st.shaded_vertices, st.rng_draws) == (st0.paths, st0.shaded_vertices, st0.rng_draws) or env.get("DRT_POOL_BLOCKS")
            if env.get("DRT_POOL_BLOCKS"):
                assert st.redone_launches >= 1
        for k in env:
            monkeypatch.delenv(k)
    # a tile of every other row (what a rank of two renders), and the XYZ film: blocks against one piece
    tall = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 512, 1024)
    for kw in (dict(height=1024, y0=1, tile_h=512, row_stride=2), dict(height=512, mode=pydrt.MODE_XYZ)):
        got = []
        bundle = tall if kw["height"] == 1024 else pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 512, 512)
        for blocks in ("8", "1"):
            monkeypatch.setenv("DRT_ONESHOT_BLOCKS", blocks)
            pk = pydrt.make_params(512, spp=9, max_depth=5, seed=4, batch_spp=4, flags=pydrt.FLAG_FILM_ZERO, **kw)
            if kw.get("mode") == pydrt.MODE_XYZ:
                L = pydrt.hip_lib()
                acc = np.zeros((512 * 512, 8))
                st = pydrt.Stats()
                assert L.drt_render_tile(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(pk), acc.ctypes.data_as(C.POINTER(C.c_double)), None, None, C.byref(st)) == 0
                got.append((acc,))
            else:
                got.append(pydrt.render_tile(bundle, pk)[:3])
            monkeypatch.delenv("DRT_ONESHOT_BLOCKS")
        assert all(np.array_equal(a, b) for a, b in zip(got[0], got[1])), kw
        assert float(np.abs(got[0][0]).sum()) > 0.0


def test_render_in_row_blocks_is_the_same_film(monkeypatch):
    """A drt_render() call for more samples than a kernel pair takes, on a context whose pairs take few samples of a pixel, goes out in
    row blocks (each with all the call's samples) so that the film is passed over less often: same film, same statistics."""
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 96, 200)
    p = pydrt.make_params(96, 200, spp=23, max_depth=7, seed=2, batch_spp=3)
    films = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("DRT_NO_ROW_BLOCKS", "1")
        r = pydrt.Renderer(bundle, p)
        r.render(0, 20)
        r.render(20, 3)
        films.append(r.read_film() + (r.stats(),))
        r.close()
    monkeypatch.delenv("DRT_NO_ROW_BLOCKS")
    for a, b in zip(films[0][:3], films[1][:3]):
        assert np.array_equal(a, b)
    assert (films[0][3].paths, films[0][3].rng_draws, films[0][3].shaded_vertices) == (films[1][3].paths, films[1][3].rng_draws, films[1][3].shaded_vertices)
    o = oracle(bundle, p, num_threads=16)
    assert_same_film(films[0][:3], o[:3])


def test_record_pool_that_runs_out_is_rendered_again_not_wrong(monkeypatch):
    """Vertex records live in a pool sized from the tile's measured blocks per path. If a launch needs more (forced here with
    a pool of one worst-case sample per pixel under launches of 12 samples), its shade kernel and everything queued behind it
    must do nothing, and the library must render those samples again in worst-case-sized launches: same film, bit for bit,
    same statistics apart from the wasted work, and the statistics say it happened."""
    bundle, _ = cases.load_case("plane_light_48")
    p = pydrt.make_params(48, 48, spp=30, max_depth=8, seed=3, batch_spp=12)
    r = pydrt.Renderer(bundle, p)
    r.render(0, 30)
    px0, av0, va0 = r.read_film()
    st0 = r.stats()
    r.close()
    assert st0.redone_launches == 0 and 0 < st0.record_pool_peak <= st0.record_pool_blocks
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    r = pydrt.Renderer(bundle, p)
    r.render(0, 7)       # two calls, several launches each, queued before anything is waited for
    r.render(7, 23)
    px1, av1, va1 = r.read_film()
    st1 = r.stats()
    assert st1.redone_launches >= 2 and st1.record_pool_blocks < st0.record_pool_blocks
    assert np.array_equal(px0, px1) and np.array_equal(av0, av1) and np.array_equal(va0, va1)
    # a launch that ran out is counted when it is rendered again, not twice (the kernels count per pair; a pair's counts join
    # the totals only when it was complete)
    assert (st1.paths, st1.closest_hit_scans, st1.shaded_vertices, st1.shadow_scans, st1.rng_draws) == \
           (st0.paths, st0.closest_hit_scans, st0.shaded_vertices, st0.shadow_scans, st0.rng_draws)
    # and the context goes on working: more samples on top, against a fresh run of all of them
    r.render(30, 5)
    px2, _, va2 = r.read_film()
    r.close()
    monkeypatch.delenv("DRT_POOL_BLOCKS")
    p35 = pydrt.make_params(48, 48, spp=35, max_depth=8, seed=3, batch_spp=12)
    r = pydrt.Renderer(bundle, p35)
    r.render(0, 35)
    px3, av3, va3 = r.read_film()
    r.close()
    assert np.array_equal(px2, px3) and np.array_equal(va2, va3)
    assert_same_film((px3, av3, va3), oracle(bundle, p35, num_threads=8)[:3])


def test_device_group_gives_the_single_context_film():
    """drt_group_*: one host thread, several contexts (here 1, 3 and 5 of them, all on GPU 0; 5 > the 4 rows of the last
    tile, so one context gets no rows) with the rows dealt cyclically -- film, resume and statistics equal the single
    context's bit for bit; the one-shot drt_render_tile_multi accumulates into host buffers like drt_render_tile."""
    bundle, params = cases.load_case("plane_light_48")
    base = hip_render(bundle, params, record_hits=False)
    for devices in ([0], [0, 0, 0], [0] * 5):
        g = pydrt.Group(bundle, params, devices)
        assert g.size() == len(devices)
        g.render(0, 1)
        g.render(1, int(params.spp) - 1)
        px, av, va = g.read_film()
        st = g.stats()
        g.close()
        assert np.array_equal(px, base[0]) and np.array_equal(av, base[1]) and np.array_equal(va, base[2])
        assert (st.paths, st.closest_hit_scans, st.shaded_vertices, st.rng_draws) == \
               (base[5].paths, base[5].closest_hit_scans, base[5].shaded_vertices, base[5].rng_draws)
    # a tile with fewer rows than devices, with a row stride of its own, written and read back through the group
    pt = pydrt.make_params(48, 48, spp=4, max_depth=8, seed=1, x0=5, y0=1, tile_w=30, tile_h=4, row_stride=11)
    ref = hip_render(bundle, pt, record_hits=False)
    g = pydrt.Group(bundle, pt, [0] * 5)
    g.render(0, 2)
    half = g.read_film()
    g.close()
    g = pydrt.Group(bundle, pt, [0, 0])
    g.write_film(*half)
    g.render(2, 2)
    px, av, va = g.read_film()
    g.close()
    assert np.array_equal(px, ref[0]) and np.array_equal(av, ref[1]) and np.array_equal(va, ref[2])
    # one-shot form
    L = pydrt.hip_lib()
    f64p = C.POINTER(C.c_double)
    S, n = bundle.S, 48 * 48
    px = np.zeros((n, S + 1)); av = np.zeros((n, S)); va = np.zeros((n, S))
    st = pydrt.Stats()
    devs = (C.c_int32 * 2)(0, 0)
    rc = L.drt_render_tile_multi(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(params), devs, 2, px.ctypes.data_as(f64p),
                                 av.ctypes.data_as(f64p), va.ctypes.data_as(f64p), C.byref(st))
    assert rc == 0, L.drt_last_error()
    assert np.array_equal(px, base[0]) and np.array_equal(va, base[2]) and st.paths == base[5].paths
    with pytest.raises(RuntimeError):
        pydrt.Group(bundle, params, [0, 99])


@pytest.mark.parametrize("name", ["plane_light_48", "gold_mirror", "many_lights", "grid_2p5nm", "grid_4nm", "grid_10nm"])
def test_xyz_film_mode_matches_the_spectral_film(name):
    """DRT_MODE_XYZ keeps 8 accumulators per pixel instead of three spectra: its XYZ equals the spectral film's XYZ (and the
    oracle's) to rounding -- the sums are the same terms in another order -- whatever the batch size, and the film can be read,
    written back and continued; there is no mean / variance to ask for."""
    bundle, params = cases.load_case(name)
    spectral = hip_render(bundle, params, record_hits=False)
    acc0 = None
    opx = oracle(bundle, params)[0]
    assert_same_xyz(spectral[4], bundle, opx, name)
    oxyz = O.oracle_film_to_xyz(bundle, opx)
    spp = int(params.spp)
    for batch in (0, 1, 3):
        p = pydrt.make_params(int(params.width), int(params.height), spp=spp, max_depth=int(params.max_depth), seed=int(params.seed),
                              pixel_scheme=int(params.pixel_scheme), mode=pydrt.MODE_XYZ, batch_spp=batch)
        r = pydrt.Renderer(bundle, p)
        r.render()
        xyz = r.read_xyz()
        acc = r.read_xyz_film()
        st = r.stats()
        assert cases.xyz_rel_err(xyz, spectral[4]) <= 1e-12 and cases.xyz_rel_err(xyz, oxyz) <= REF_XYZ_TOL
        assert np.all(acc[:, 3] == float(spp)) and np.all(acc[:, 7] == 0.0)
        assert (st.paths, st.rng_draws) == (spectral[5].paths, spectral[5].rng_draws)
        with pytest.raises(RuntimeError):
            r.read_film()
        with pytest.raises(RuntimeError, match="DRT_MODE_SPECTRAL"):
            r.read_bgra(0)
        r.close()
        if batch == 0:
            acc0 = acc
    # stop after the first sample, carry the accumulators over to a new context, continue
    if spp >= 2:
        p = pydrt.make_params(int(params.width), int(params.height), spp=spp, max_depth=int(params.max_depth), seed=int(params.seed),
                              pixel_scheme=int(params.pixel_scheme), mode=pydrt.MODE_XYZ)
        r = pydrt.Renderer(bundle, p)
        r.render(0, 1)
        half = r.read_xyz_film()
        r.close()
        r = pydrt.Renderer(bundle, p)
        r.write_xyz_film(half)
        r.render(1, spp - 1)
        assert cases.xyz_rel_err(r.read_xyz(), spectral[4]) <= 1e-12
        r.close()
    # one-shot forms and a device group in XYZ mode
    p = pydrt.make_params(int(params.width), int(params.height), spp=spp, max_depth=int(params.max_depth), seed=int(params.seed),
                          pixel_scheme=int(params.pixel_scheme), mode=pydrt.MODE_XYZ)
    L = pydrt.hip_lib()
    f64p = C.POINTER(C.c_double)
    n = int(params.width) * int(params.height)
    acc = np.zeros((n, 8))
    rc = L.drt_render_tile(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(p), acc.ctypes.data_as(f64p), None, None, None)
    assert rc == 0, L.drt_last_error()
    acc3 = np.zeros((n, 8))
    devs = (C.c_int32 * 3)(0, 0, 0)
    rc = L.drt_render_tile_multi(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(p), devs, 3, acc3.ctypes.data_as(f64p), None, None, None)
    assert rc == 0, L.drt_last_error()
    assert np.array_equal(acc, acc3) and np.array_equal(acc, acc0)  # same launches, same order of sums: the same bits


def test_one_shot_render_tile_accumulates_into_host_buffers():
    bundle, params = cases.load_case("plane_light_16")
    px, av, va, st = pydrt.render_tile(bundle, params)
    o4 = oracle(bundle, params)
    assert_same_film((px, av, va), o4[:3], "4 samples")
    assert st.paths == 16 * 16 * 4 and st.total_ms > 0
    # second call with first_sample = 4 continues the same buffers
    L = pydrt.hip_lib()
    p2 = pydrt.make_params(16, 16, spp=4, max_depth=8, seed=1, first_sample=4)
    st2 = pydrt.Stats()
    f64p = C.POINTER(C.c_double)
    rc = L.drt_render_tile(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(p2), px.ctypes.data_as(f64p), av.ctypes.data_as(f64p),
                           va.ctypes.data_as(f64p), C.byref(st2))
    assert rc == 0
    p8 = pydrt.make_params(16, 16, spp=8, max_depth=8, seed=1)
    assert_same_film((px, av, va), oracle(bundle, p8)[:3], "4 + 4 samples")
    assert np.all(px[:, bundle.S] == 8.0)
    # DRT_FLAG_FILM_ZERO: the caller vouches for zero-filled buffers, nothing is uploaded -- same film as the plain call
    pz = pydrt.make_params(16, 16, spp=4, max_depth=8, seed=1, flags=pydrt.FLAG_FILM_ZERO)
    zx = np.zeros_like(px); za = np.zeros_like(av); zv = np.zeros_like(va)
    rc = L.drt_render_tile(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(pz), zx.ctypes.data_as(f64p), za.ctypes.data_as(f64p),
                           zv.ctypes.data_as(f64p), C.byref(st2))
    assert rc == 0
    assert_same_film((zx, za, zv), o4[:3], "FILM_ZERO")


@pytest.mark.parametrize("scene", ["first_scene.scn", "cornell_plane_light.scn"])
@pytest.mark.parametrize("dark_skip", ["0", "1"])
def test_accumulating_into_a_film_that_holds_minus_zero_nan_infinities_and_subnormals(scene, dark_skip, monkeypatch):
    """render_image adds to the caller's buffers (src/daily_ray_trace.c:732-743); here they arrive with -0, NaN, +-inf, subnormal and huge
    values sprinkled over sum, mean and variance, and samples 7..11 are added: the oracle's film bit for bit -- NaN and infinities in
    the same places, every zero with the oracle's sign -- with the shade kernel's shortcut for dark pixels (which must see that a pixel
    holding -0 is NOT all +0) and without it."""
    monkeypatch.setenv("DRT_DARK_SKIP", dark_skip)
    rng = np.random.default_rng(3)
    bundle = pydrt.load_scene(cases.scene_path(scene), 24, 24)
    S, n = bundle.S, 24 * 24
    p = pydrt.make_params(24, 24, spp=5, max_depth=6, seed=2, first_sample=7)
    specials = np.array([-0.0, np.nan, np.inf, -np.inf, 5e-324, -1e-310, 1e300, -3.5, 0.25])
    px, av, va = np.zeros((n, S + 1)), np.zeros((n, S)), np.zeros((n, S))
    for a in (px, av, va):
        idx = rng.integers(0, a.size, a.size // 6)
        a.reshape(-1)[idx] = specials[rng.integers(0, specials.size, idx.size)]
    px[:, S] = 7.0
    ox, oa, ov, _, ost = oracle(bundle, p, num_threads=8, film=(px, av, va))
    f64p = C.POINTER(C.c_double)
    st = pydrt.Stats()
    assert pydrt.hip_lib().drt_render_tile(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(p), px.ctypes.data_as(f64p), av.ctypes.data_as(f64p),
                                           va.ctypes.data_as(f64p), C.byref(st)) == 0
    assert_same_film((px, av, va), (ox, oa, ov), scene)
    for got, want in ((px, ox), (av, oa), (va, ov)):
        assert np.array_equal(np.signbit(got[got == 0]), np.signbit(want[want == 0]))
    assert np.isnan(ox).sum() > 100 and (ox == 0).sum() > 0 and _counts(st) == _counts(ost)


def test_errors_are_reported_not_swallowed():
    bundle, params = cases.load_case("plane_light_16")
    L = pydrt.hip_lib()
    bad = pydrt.make_params(16, 16, spp=1, max_depth=0)
    assert not L.drt_create(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(bad))
    assert b"depth" in L.drt_last_error()
    bad_dev = pydrt.make_params(16, 16, spp=1, max_depth=2, device=99)
    assert not L.drt_create(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(bad_dev))
    assert len(L.drt_last_error()) > 0
    r = pydrt.Renderer(bundle, params)  # hit recording off
    r.render()
    with pytest.raises(RuntimeError):
        r.read_hit_indices(4)
    r.close()
    # a grid that does not reach the 630 nm the dielectric sampler looks up (the reference reads past its arrays there)
    short = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 16, 16, min_wl=400.0, max_wl=550.0, wl_interval=150.0)
    assert not L.drt_create(C.byref(short.scene), C.byref(short.camera), C.byref(params))
    assert b"630" in L.drt_last_error()
    unknown_mode = pydrt.make_params(16, 16, spp=1, max_depth=2, mode=7)
    assert not L.drt_create(C.byref(bundle.scene), C.byref(bundle.camera), C.byref(unknown_mode))
    assert b"mode" in L.drt_last_error()


def test_large_scene_outside_lds():
    """BASELINE config 5's generator (10k spheres: SoA tables read from HBM, not LDS), reduced image size."""
    bundle = pydrt.synthetic_sphere_scene(10000, 48, 48)
    params = pydrt.make_params(48, 48, spp=2, max_depth=8, seed=11)
    px, av, va, hits, xyz, st = hip_render(bundle, params)
    opx, oav, ova, ohits, ost = oracle(bundle, params, want_hits=True, num_threads=8)
    assert np.array_equal(hits, ohits) and (hits >= 0).any()
    assert (st.closest_hit_scans, st.shaded_vertices, st.rng_draws) == (ost.closest_hit_scans, ost.shaded_vertices, ost.rng_draws)
    assert_same_film((px, av, va), (opx, oav, ova))
    assert_same_xyz(xyz, bundle, opx)


def test_full_size_properties_config2():
    """BASELINE config 2 geometry (cornell_plane_light 1024x1024, depth 8) at 8 spp: size-independent properties,
    plus two image rows checked bit-for-bit against the oracle."""
    w = h = 1024
    spp = 8
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), w, h)
    p = pydrt.make_params(w, h, spp=spp, max_depth=8, seed=1)
    r = pydrt.Renderer(bundle, p)
    r.render(0, spp)
    px, av, va = r.read_film()
    st = r.stats()
    S = bundle.S
    assert st.paths == w * h * spp
    assert np.all(px[:, S] == float(spp))                      # filter sums count the samples exactly
    assert np.isfinite(px).all() and np.isfinite(av).all() and np.isfinite(va).all()
    assert (va >= -1e-18).all()                                   # running variance sums are sums of (c-m_old)(c-m_new) >= 0
    np.testing.assert_allclose(av, px[:, :S] / spp, rtol=1e-9, atol=1e-13)  # running mean == sum / n
    assert 2.45 < st.closest_hit_scans / st.paths < 2.65         # SURVEY: 2.551 scans, 1.645 shaded vertices per path
    assert 1.55 < st.shaded_vertices / st.paths < 1.75
    # idempotence: same samples into a zeroed film give the same bits
    r.reset_film()
    r.render(0, spp)
    px2, av2, va2 = r.read_film()
    assert np.array_equal(px, px2) and np.array_equal(av, av2) and np.array_equal(va, va2)
    # split across calls == one call
    r.reset_film()
    r.render(0, 3)
    r.render(3, spp - 3)
    px3, _, va3 = r.read_film()
    assert np.array_equal(px, px3) and np.array_equal(va, va3)
    r.close()
    # two rows of the full image against the oracle
    for y in (300, 777):
        pt = pydrt.make_params(w, h, spp=spp, max_depth=8, seed=1, y0=y, tile_h=1)
        o = oracle(bundle, pt, num_threads=8)
        assert_same_film((px.reshape(h, w, S + 1)[y], av.reshape(h, w, S)[y], va.reshape(h, w, S)[y]), o[:3], "row %d" % y)


FULL_SIZE_CONFIGS = {
    # BASELINE.json configs 2, 3, 4, 5 exactly as named there (config 2 is also the bench workload; its size-independent
    # properties at 8 spp are the test above, here it runs at its stated 256 spp)
    "config2_plane_light_1024_256spp_d8": (lambda: pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 1024, 1024), 1024, 256, 8),
    "config3_large_box_2048_1024spp_d16": (lambda: pydrt.load_scene(cases.scene_path("cornell_large_box.scn"), 2048, 2048), 2048, 1024, 16),
    "config4_gold_mirror_1024_512spp_d8": (lambda: pydrt.load_scene(cases.scene_path("cornell_gold_mirror.scn"), 1024, 1024), 1024, 512, 8),
    "config5_10k_spheres_4096_64spp_d8": (lambda: pydrt.synthetic_sphere_scene(10000, 4096, 4096), 4096, 64, 8),
}


@pytest.mark.parametrize("name", list(FULL_SIZE_CONFIGS))
def test_full_size_configs_probe_pixels_against_the_oracle(name):
    """The other BASELINE configs at FULL size and sample count on the one GPU (film up to 27.9 GB, 2^32 paths: every
    64-bit index is exercised), film kept in torch tensors so that only probe pixels are copied back: the first, a middle,
    the very last 16 pixels of the frame and the 16 around its brightest pixel must match the oracle's render of those pixels (all samples), and the
    whole-frame invariants must hold."""
    torch = pytest.importorskip("torch")
    load, size, spp, depth = FULL_SIZE_CONFIGS[name]
    bundle = load()
    S, n = bundle.S, size * size
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    params = pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=1)
    r = pydrt.Renderer(bundle, params)
    with torch.cuda.stream(stream):
        t_px = torch.zeros((n, S + 1), dtype=torch.float64, device=dev)
        t_av = torch.zeros((n, S), dtype=torch.float64, device=dev)
        t_va = torch.zeros((n, S), dtype=torch.float64, device=dev)
        r.bind_film(t_px.data_ptr(), t_av.data_ptr(), t_va.data_ptr())
        r.set_stream(stream.cuda_stream)
        r.render(0, spp)
        filt_ok = bool((t_px[:, S] == float(spp)).all().item())
        finite = bool(torch.isfinite(t_px).all().item() and torch.isfinite(t_av).all().item() and torch.isfinite(t_va).all().item())
        var_ok = bool((t_va >= -1e-18).all().item())
        probes = []
        brightest = int(torch.argmax(t_px[:, S // 2]).item())  # a probe that is certainly lit
        by, bx = divmod(brightest, size)
        for y, x0 in ((0, 0), (size // 2 + 3, size // 2 - 8), (size - 1, size - 16), (by, min(max(bx - 8, 0), size - 16))):
            a = (y * size + x0)
            probes.append((y, x0, t_px[a:a + 16].cpu().numpy(), t_av[a:a + 16].cpu().numpy(), t_va[a:a + 16].cpu().numpy()))
    st = r.stats()
    r.close()
    del t_px, t_av, t_va
    torch.cuda.empty_cache()
    assert st.paths == size * size * spp
    assert filt_ok and finite and var_ok
    lit = 0.0
    for y, x0, px, av, va in probes:
        pt = pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=1, x0=x0, y0=y, tile_w=16, tile_h=1)
        opx, oav, ova, _, _ = oracle(bundle, pt, num_threads=8)
        assert_same_film((px, av, va), (opx, oav, ova), "%s probe (%d, %d)" % (name, x0, y))
        lit += float(opx[:, :S].sum())
    assert lit > 0.0  # the probes are not all black


def test_torch_owned_film_and_stream():
    """PyTorch as plumbing: film tensors allocated by torch, kernels on a torch stream. The read-back is enqueued on the
    same stream with no explicit synchronisation in between, so it is right only if the kernels really ran on that stream
    (a handle of 0 -- torch's default stream -- would mean "the context's own stream" to drt_set_stream)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    bundle, params = cases.load_case("plane_light_48")
    S, n = bundle.S, 48 * 48
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    r = pydrt.Renderer(bundle, params)
    with torch.cuda.stream(stream):
        t_px = torch.zeros((n, S + 1), dtype=torch.float64, device=dev)
        t_av = torch.zeros((n, S), dtype=torch.float64, device=dev)
        t_va = torch.zeros((n, S), dtype=torch.float64, device=dev)
        r.bind_film(t_px.data_ptr(), t_av.data_ptr(), t_va.data_ptr())
        r.set_stream(stream.cuda_stream)
        r.render()
        h_px = t_px.to("cpu", non_blocking=False)   # ordered after the kernels by the stream alone
        h_av = t_av.to("cpu", non_blocking=False)
        h_va = t_va.to("cpu", non_blocking=False)
    assert_same_film((h_px.numpy(), h_av.numpy(), h_va.numpy()), oracle(bundle, params)[:3])
    r.close()


def test_bench_two_rank_rehearsal_assembles_the_same_frame():
    """bench.py's N > 1 path (rows cyclic over ranks, row blocks gathered to rank 0 while the next block renders), rehearsed
    as two processes sharing this GPU over gloo, assembles bit for bit the frame of the single-process run."""
    import json
    import subprocess
    import sys
    pytest.importorskip("torch")
    bench = os.path.join(cases.REPO, "bench.py")
    common = ["--size", "96", "--spp", "6", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-oneshot", "--checksum"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")

    def last_json(cmd):
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        return json.loads(lines[0])

    one = last_json([sys.executable, bench] + common)
    three_blocks = last_json([sys.executable, bench, "--gather-blocks", "3"] + common)
    assert one["frame_checksum"] == three_blocks["frame_checksum"]
    two = last_json([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                     "--master-port", "29533", bench, "--gpus", "2", "--backend", "gloo", "--share-device", "--gather-blocks", "3"] + common)
    assert two["n_gpus"] == 2 and two["frame_checksum"] == one["frame_checksum"]
    assert two["config"]["paths_per_step"] == 96 * 96 * 6
    # the same from a plain shell: `python bench.py --gpus 2` starts its ranks itself (no torch.distributed.run on the command line)
    env.pop("WORLD_SIZE", None)
    plain = last_json([sys.executable, bench, "--gpus", "2", "--backend", "gloo", "--share-device", "--gather-blocks", "3"] + common)
    assert plain["n_gpus"] == 2 and plain["frame_checksum"] == one["frame_checksum"]
    # three ranks on an image whose rows do not divide evenly (ranks own 34, 33, 33 rows of 100), default block count
    common[1] = "100"
    one100 = last_json([sys.executable, bench] + common)
    three = last_json([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                       "--master-port", "29534", bench, "--gpus", "3", "--backend", "gloo", "--share-device"] + common)
    assert three["n_gpus"] == 3 and three["frame_checksum"] == one100["frame_checksum"]
    # what the first 8-GPU run will be read by: per-rank kernel / wall / gather-wait times, rows owned, the load imbalance, and
    # rank 0's memory for the assembled frame and the receive buffers -- present and sane in the rehearsal
    pr = three["per_rank_ms"]
    assert [len(pr[k]) for k in ("kernels", "wall", "gather_wait", "rows")] == [3, 3, 3, 3] and pr["rows"] == [34, 33, 33]
    assert all(x > 0 for x in pr["kernels"]) and all(w >= k * 0.5 for w, k in zip(pr["wall"], pr["kernels"]))
    assert 1.0 <= three["load_imbalance"] < 3.0 and three["gather_ms_per_step"] >= 0.0
    assert three["config"]["rank0_frame_GB"] > 0 and three["config"]["rank0_recv_buffers_GB"] > 0 and "gloo" in three["config"]["collective"]
    # BASELINE configs[2] (cornell_large_box 2048^2 x 1024 spp, depth 16, tiled over the ranks) through the same code at a reduced
    # size: two ranks assemble the single-process frame; the line names the config, says it is reduced and is not the headline's;
    # and the CPU baseline is reported at N > 1 too (rank 0, after the timed region)
    c3 = ["--workload", "config3", "--size", "128", "--spp", "8", "--steps", "1", "--warmup", "0", "--no-oneshot", "--checksum"]
    one3 = last_json([sys.executable, bench, "--no-cpu-baseline"] + c3)
    two3 = last_json([sys.executable, bench, "--gpus", "2", "--backend", "gloo", "--share-device"] + c3)
    assert two3["frame_checksum"] == one3["frame_checksum"] and two3["config"]["paths_per_step"] == 128 * 128 * 8
    assert "cornell_large_box.scn 128x128, 8 spp, depth 16" in two3["config"]["workload"] and "REDUCED" in two3["config"]["workload"]
    assert "NOT the headline config" in two3["metric"] and two3["cpu_baseline"]["value"] > 0 and two3["cpu_baseline"]["cores"] == 1
    # a backend that cannot start is a failed run with the rank and the reason on stderr, not a silent fall-back
    bad = subprocess.run([sys.executable, bench, "--gpus", "2", "--backend", "no_such_backend", "--share-device", "--size", "16", "--spp", "1",
                          "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-oneshot"], env=env, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "init_process_group failed" in bad.stderr and not [l for l in bad.stdout.splitlines() if l.startswith("{")]


def test_drt_render_program_checkpoint_and_resume(tmp_path):
    """The POSIX + HIP program end to end (N3): a run checkpointed every 2 samples and cut short after 4, then
    resumed to 6, writes the same three .spd files, bit for bit, as an uninterrupted 6-sample run."""
    import shutil
    import subprocess
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    assert os.path.exists(exe)

    def run(workdir, spp, env_extra):
        os.makedirs(os.path.join(workdir, "output"), exist_ok=True)
        for d in ("scenes", "spectra"):
            if not os.path.exists(os.path.join(workdir, d)):
                os.symlink(os.path.join(cases.REPO, d), os.path.join(workdir, d))
        cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
        cfg = cfg.replace("num_pixel_samples 4", "num_pixel_samples %d" % spp).replace("output_width      800", "output_width      96")
        cfg = cfg.replace("output_height     600", "output_height     64").replace("max_cast_depth    4", "max_cast_depth    6")
        open(os.path.join(workdir, "config.cfg"), "w").write(cfg)
        env = dict(os.environ, **env_extra)
        r = subprocess.run([exe], cwd=workdir, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        return r.stdout

    a = str(tmp_path / "a"); b = str(tmp_path / "b")
    os.makedirs(a); os.makedirs(b)
    run(a, 6, {})
    out1 = run(b, 4, {"DRT_CHECKPOINT_SPP": "2"})
    assert "Checkpoint at 2 / 4 samples" in out1
    out2 = run(b, 6, {"DRT_CHECKPOINT_SPP": "2", "DRT_RESUME": "1"})
    assert "Resuming after 4 samples" in out2
    for f in ("output.spd", "average.spd", "variance.spd", "output.bmp"):
        assert open(os.path.join(a, "output", f), "rb").read() == open(os.path.join(b, "output", f), "rb").read(), f
    # the same program driving several contexts at once (rows dealt over the device list; here all on GPU 0), checkpointed too
    c = str(tmp_path / "c")
    os.makedirs(c)
    out3 = run(c, 6, {"DRT_DEVICES": "0,0,0", "DRT_CHECKPOINT_SPP": "4"})
    assert "Rendering on 3 devices" in out3 and "Checkpoint at 4 / 6 samples" in out3
    for f in ("output.spd", "average.spd", "variance.spd", "output.bmp"):
        assert open(os.path.join(a, "output", f), "rb").read() == open(os.path.join(c, "output", f), "rb").read(), f
    # N2 on the device: the three .bmp files (drt_read_bgra on the resident film) are byte for byte what the host conversion of the
    # written .spd files gives (host/drt_bmp.c, whose arithmetic is pinned to the reference's spectrum_to_rgb_f64 in tests/test_host.py)
    H = pydrt.host_lib()
    f64p = C.POINTER(C.c_double)
    H.drt_host_spd_file_to_bmp.argtypes = [C.c_char_p, C.c_char_p, f64p]
    bundle96 = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 96, 64)
    cmf = np.ascontiguousarray(bundle96.spds()[int(bundle96.scene.cmf_rw):int(bundle96.scene.cmf_rw) + 4])  # rows rw, x, y, z
    for name in ("output", "average", "variance"):
        for d in (a, c):
            host_bmp = os.path.join(d, "output", name + "_host.bmp")
            assert H.drt_host_spd_file_to_bmp(os.path.join(d, "output", name + ".spd").encode(), host_bmp.encode(), cmf.ctypes.data_as(f64p)) == 0
            dev = open(os.path.join(d, "output", name + ".bmp"), "rb").read()
            assert len(dev) == 54 + 96 * 64 * 4 and dev == open(host_bmp, "rb").read(), (name, d)
    assert len(set(open(os.path.join(a, "output", "output.bmp"), "rb").read()[54:])) > 50  # a picture, not a constant
    # and the film agrees with the oracle
    hdr = np.fromfile(os.path.join(a, "output", "output.spd"), dtype=np.uint32, count=5)
    assert list(hdr[1:5]) == [96, 64, 69, 1]
    px = np.fromfile(os.path.join(a, "output", "output.spd"), dtype=np.float64, offset=40).reshape(-1, 70)
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 96, 64)
    p = pydrt.make_params(96, 64, spp=6, max_depth=6, seed=1)
    avg = np.fromfile(os.path.join(a, "output", "average.spd"), dtype=np.float64, offset=40).reshape(-1, 69)
    var = np.fromfile(os.path.join(a, "output", "variance.spd"), dtype=np.float64, offset=40).reshape(-1, 69)
    opx, oav, ova, _, _ = oracle(bundle, p, num_threads=16)
    assert np.isfinite(ova).all()
    with np.errstate(invalid="ignore"):
        norm = ova / np.max(np.maximum(ova, 0.0), axis=1)[:, None]  # the variance is written max-normalised per pixel (host/drt_checkpoint.c)
    assert_same_film((px, avg, var), (opx, oav, norm))


def test_edge_cases_empty_scene_and_single_pixel():
    """No surfaces at all (every path escapes at depth 0), a 1x1 image, one sample, depth 1, an odd-sized tile."""
    empty = """Camera
position 0.0, 0.0, 8.0
target   0.0, 0.0, 0.0
fov 90.0
fdepth 6.0
flength 0.3
Material
name vacuum
refract constant 1.0
base_material
Material
name escape
escape_material
"""
    b = pydrt.load_scene_text(empty, 7, 5)
    p = pydrt.make_params(7, 5, spp=3, max_depth=4, seed=2)
    px, av, va, hits, xyz, st = hip_render(b, p)
    assert (hits[:, 0] == -1).all() and (hits[:, 1:] == -2).all()
    assert np.all(px[:, :b.S] == 0.0) and np.all(px[:, b.S] == 3.0) and np.all(av == 0.0) and np.all(va == 0.0)
    assert st.closest_hit_scans == st.paths == 7 * 5 * 3 and st.shaded_vertices == 0
    opx, oav, ova, ohits, ost = oracle(b, p, want_hits=True)
    assert_same_film((px, av, va), (opx, oav, ova), "empty scene")
    assert np.array_equal(hits, ohits) and st.rng_draws == ost.rng_draws

    b1 = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 1, 1)
    for spp, depth in ((1, 1), (5, 3), (70, 2)):  # 70 samples: more than one batch of the 64-sample cap
        p1 = pydrt.make_params(1, 1, spp=spp, max_depth=depth, seed=9)
        px, av, va, hits, xyz, st = hip_render(b1, p1)
        opx, oav, ova, ohits, ost = oracle(b1, p1, want_hits=True)
        assert np.array_equal(hits, ohits)
        assert_same_film((px, av, va), (opx, oav, ova), "1x1, %d spp" % spp)
        assert_same_xyz(xyz, b1, opx, "1x1, %d spp" % spp)
        assert px[0, b1.S] == float(spp)

    b2 = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 37, 23)
    p2 = pydrt.make_params(37, 23, spp=2, max_depth=5, seed=4, x0=3, y0=1, tile_w=29, tile_h=7, row_stride=3)
    px, av, va, hits, xyz, st = hip_render(b2, p2)
    opx, oav, ova, ohits, ost = oracle(b2, p2, want_hits=True)
    assert np.array_equal(hits, ohits)
    assert_same_film((px, av, va), (opx, oav, ova), "odd tile")
    bad = pydrt.make_params(37, 23, spp=1, max_depth=2, x0=10, tile_w=30)  # tile runs off the image
    assert not pydrt.hip_lib().drt_create(C.byref(b2.scene), C.byref(b2.camera), C.byref(bad))


# ---- round 3 ---------------------------------------------------------------------------------------------------------------

def _render_all(bundle, p, record_hits=True):
    """film, hits, XYZ and statistics of one context (like hip_render, with the caller's params untouched but for the hit flag)"""
    q = pydrt.make_params(int(p.width), int(p.height), spp=int(p.spp), max_depth=int(p.max_depth), seed=int(p.seed), x0=int(p.x0), y0=int(p.y0),
                          tile_w=int(p.tile_w), tile_h=int(p.tile_h), row_stride=int(p.row_stride), first_sample=int(p.first_sample),
                          pixel_scheme=int(p.pixel_scheme), mode=int(p.mode), batch_spp=int(p.batch_spp),
                          flags=pydrt.FLAG_RECORD_HITS if record_hits else 0)
    r = pydrt.Renderer(bundle, q)
    r.render()
    film = (r.read_xyz_film(),) if int(p.mode) == pydrt.MODE_XYZ else r.read_film()
    hits = r.read_hit_indices(int(q.spp)) if record_hits else None
    xyz = r.read_xyz()
    st = r.stats()
    r.close()
    return film, hits, xyz, st


def _counts(st):
    return (st.paths, st.closest_hit_scans, st.shaded_vertices, st.shadow_scans, st.rng_draws)


# wavelength grids whose tail (S mod 64) is 5, 1, 6 and 8 wide -- the widths drt_trace_kernel<true, true> accepts run from 1 to 8;
# every grid brackets 630 nm
TAIL_GRIDS = {69: (380.0, 720.0, 5.0), 65: (380.0, 700.0, 5.0), 70: (400.0, 676.0, 4.0), 72: (400.0, 684.0, 4.0)}


@pytest.mark.parametrize("scene,size,spp,depth", [("cornell_large_box.scn", 24, 3, 16), ("cornell_downward.scn", 20, 3, 6), ("first_scene.scn", 20, 3, 4),
                                                  ("cornell_plane_light.scn", 28, 4, 8), ("cornell_gold_mirror.scn", 24, 3, 8)])
@pytest.mark.parametrize("S", list(TAIL_GRIDS))
def test_tail_wavelengths_in_the_trace_kernel_equal_the_tail_pass(scene, size, spp, depth, S, monkeypatch):
    """One-light scenes scanned out of LDS are traced by drt_trace_kernel<true, true>, which carries the tail wavelengths of the
    paths it can itself (Stats.path_flags says so): every path in an all-plastic scene, and in a scene with glass or gold the paths
    that never meet them -- the others stay with the shade kernel's tail pass, which takes them as tasks. DRT_TRACE_TAIL=0 sends
    every path's tail through the tail pass. Film, hit indices, XYZ and statistics must be the same BIT FOR BIT, in the spectral
    and the XYZ film, for every tail width, and both must be the oracle's. (cornell_downward has the mirror, first_scene the point
    light and no box, cornell_plane_light glass + rough gold + mirror, cornell_gold_mirror smooth gold.)"""
    grid = TAIL_GRIDS[S]
    bundle = pydrt.load_scene(cases.scene_path(scene), size, size, min_wl=grid[0], max_wl=grid[1], wl_interval=grid[2])
    assert bundle.S == S
    opx, oav, ova, ohits, ost = oracle(bundle, pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=5), want_hits=True)
    for mode in (pydrt.MODE_SPECTRAL, pydrt.MODE_XYZ):
        p = pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=5, mode=mode, batch_spp=2)
        monkeypatch.delenv("DRT_TRACE_TAIL", raising=False)
        a = _render_all(bundle, p)
        monkeypatch.setenv("DRT_TRACE_TAIL", "0")
        b = _render_all(bundle, p)
        monkeypatch.delenv("DRT_TRACE_TAIL")
        assert a[3].path_flags & pydrt.PATH_TRACE_TAIL and not (b[3].path_flags & pydrt.PATH_TRACE_TAIL)
        assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), (scene, S, mode)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and _counts(a[3]) == _counts(b[3])
        if mode == pydrt.MODE_SPECTRAL:
            assert np.array_equal(a[1], ohits) and _counts(a[3]) == _counts(ost)
            for v, what in ((a, "trace tail"), (b, "tail pass")):  # each variant on its own, not only the two alike
                assert_same_film(v[0], (opx, oav, ova), "%s S %d %s" % (scene, S, what))
                assert_same_xyz(v[2], bundle, opx, "%s S %d %s" % (scene, S, what))
            spectral_xyz = a[2]
        else:
            assert cases.xyz_rel_err(a[2], spectral_xyz) <= 1e-11


MIRROR_LIT_EXACTLY = """Camera
position 0.0, 0.0, 8.0
target   0.0, 0.0, 0.0
roll     0.0
fov      60.0
fdepth   6.0
flength  0.3
aperture 0.0

Material
name vacuum
refract constant 1.0
base_material

Material
name escape
escape_material

Material
name mirror
mirror csv au_spec_n.csv
bdsfs mirror_bdsf
dir_func sample_specular_direction

Material
name lamp
emission csv au_spec_k.csv

Surface
name floor_mirror
type plane
position -3.0, -3.0, 0.0
pointu 3.0, -3.0, 0.0
pointv -3.0, 3.0, 0.0
material mirror

Surface
name bulb
type point
position 0.0, 0.0, %s
material lamp
"""


@pytest.mark.parametrize("S", [69, 72])
def test_mirror_lit_along_its_exact_reflection_direction(S, monkeypatch):
    """mirror_bdsf is the mirror's spectrum only where the light direction equals the reflected direction EXACTLY (src/bdsf.c:121-132),
    which random scenes never meet. Here they do: the centre pixel's ray (FILM_SAMPLE_CENTER, odd image) runs down the axis onto a
    mirror at z = 0, and a point light sits on that axis. That pixel's film is mirror x emission x the light's weight, through the
    mirror branches of the trace kernel's tail wavelengths, the shade kernel's tail pass (DRT_TRACE_TAIL=0) and its main pass: bit for
    bit the oracle's, for lights at three heights (three weights) and spectra that vary from one wavelength to the next."""
    grid = TAIL_GRIDS[S]
    for height in ("3.3", "2.7", "5.1"):
        bundle = pydrt.load_scene_text(MIRROR_LIT_EXACTLY % height, 9, 9, min_wl=grid[0], max_wl=grid[1], wl_interval=grid[2])
        p = pydrt.make_params(9, 9, spp=2, max_depth=3, seed=1, pixel_scheme=pydrt.FILM_SAMPLE_CENTER)
        opx, oav, ova, ohits, ost = oracle(bundle, p, want_hits=True)
        lit = np.flatnonzero(np.abs(opx[:, :S]).sum(axis=1) > 0)
        assert list(lit) == [40] and np.all(opx[40, :S] > 0) and len(set(opx[40, S - 5:S].tolist())) == 5
        for tail in (None, "0"):
            if tail is None:
                monkeypatch.delenv("DRT_TRACE_TAIL", raising=False)
            else:
                monkeypatch.setenv("DRT_TRACE_TAIL", tail)
            film, hits, xyz, st = _render_all(bundle, p)
            assert bool(st.path_flags & pydrt.PATH_TRACE_TAIL) == (tail is None)
            assert np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
            assert_same_film(film, (opx, oav, ova), "light at %s, DRT_TRACE_TAIL=%s" % (height, tail))
            assert_same_xyz(xyz, bundle, opx, "light at %s, DRT_TRACE_TAIL=%s" % (height, tail))
    monkeypatch.delenv("DRT_TRACE_TAIL", raising=False)


def test_tail_in_trace_kernel_on_tiles_groups_row_blocks_and_a_pool_that_runs_out(monkeypatch):
    """The same A/B (drt_trace_kernel<true, true> against DRT_TRACE_TAIL=0) along every way a launch can be shaped: a strided
    sub-rectangle of the image, a device group of three contexts, drt_render() and the one-shot drt_render_tile() in row
    blocks, and a record pool that runs out and is rendered again. Bit-identical each time."""
    box = pydrt.load_scene(cases.scene_path("cornell_large_box.scn"), 40, 33)
    base = dict(spp=5, max_depth=16, seed=9)

    def ab(fn):
        monkeypatch.delenv("DRT_TRACE_TAIL", raising=False)
        on = fn()
        monkeypatch.setenv("DRT_TRACE_TAIL", "0")
        off = fn()
        monkeypatch.delenv("DRT_TRACE_TAIL")
        return on, off

    def same_films(x, y):
        return all(np.array_equal(a, b) for a, b in zip(x, y))

    # a strided sub-rectangle, samples split over two calls with a first_sample of their own
    pt = pydrt.make_params(40, 33, x0=3, y0=2, tile_w=31, tile_h=9, row_stride=3, first_sample=2, batch_spp=2, **base)
    on, off = ab(lambda: _render_all(box, pt))
    assert on[3].path_flags & pydrt.PATH_TRACE_TAIL and not (off[3].path_flags & pydrt.PATH_TRACE_TAIL)
    assert same_films(on[0], off[0]) and np.array_equal(on[1], off[1]) and _counts(on[3]) == _counts(off[3])
    opx, oav, ova, ohits, _ = oracle(box, pt, want_hits=True)
    assert np.array_equal(on[1], ohits)
    assert_same_film(on[0], (opx, oav, ova), "sub-rectangle, trace tail")
    assert_same_film(off[0], (opx, oav, ova), "sub-rectangle, tail pass")

    # a device group: three contexts on this GPU, rows dealt cyclically
    pg = pydrt.make_params(40, 33, **base)

    def group():
        g = pydrt.Group(box, pg, [0, 0, 0])
        g.render(0, 2)
        g.render(2, 3)
        film, st = g.read_film(), g.stats()
        g.close()
        return film, st
    on, off = ab(group)
    assert on[1].path_flags & pydrt.PATH_TRACE_TAIL and same_films(on[0], off[0]) and _counts(on[1]) == _counts(off[1])
    og = oracle(box, pg, num_threads=8)
    assert_same_film(on[0], og[:3], "group, trace tail")
    assert_same_film(off[0], og[:3], "group, tail pass")
    whole = _render_all(box, pg, record_hits=False)
    assert same_films(on[0], whole[0]) and _counts(on[1]) == _counts(whole[3])

    # drt_render() in row blocks (few samples a pair, many samples a call)
    tall = pydrt.load_scene(cases.scene_path("cornell_large_box.scn"), 64, 160)
    pb = pydrt.make_params(64, 160, spp=14, max_depth=8, seed=2, batch_spp=2)

    def blocks():
        r = pydrt.Renderer(tall, pb)
        r.render(0, 14)
        film, st = r.read_film(), r.stats()
        r.close()
        return film, st
    on, off = ab(blocks)
    assert on[1].path_flags & pydrt.PATH_TRACE_TAIL and same_films(on[0], off[0]) and _counts(on[1]) == _counts(off[1])
    ob = oracle(tall, pb, num_threads=16)
    assert_same_film(on[0], ob[:3], "row blocks, trace tail")
    assert_same_film(off[0], ob[:3], "row blocks, tail pass")
    monkeypatch.setenv("DRT_NO_ROW_BLOCKS", "1")
    plain = blocks()
    monkeypatch.delenv("DRT_NO_ROW_BLOCKS")
    assert same_films(on[0], plain[0])

    # the one-shot call in row blocks (2^18 pixels and more), and with a pool that runs out in a block
    big = pydrt.load_scene(cases.scene_path("cornell_large_box.scn"), 512, 512)
    po = pydrt.make_params(512, 512, spp=24, max_depth=6, seed=3, batch_spp=16, flags=pydrt.FLAG_FILM_ZERO)
    on, off = ab(lambda: pydrt.render_tile(big, po))
    assert on[3].path_flags & pydrt.PATH_TRACE_TAIL and same_films(on[:3], off[:3]) and _counts(on[3]) == _counts(off[3])
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    monkeypatch.setenv("DRT_ONESHOT_BLOCKS", "2")
    redo = pydrt.render_tile(big, po)
    monkeypatch.delenv("DRT_ONESHOT_BLOCKS")
    assert redo[3].redone_launches >= 1 and same_films(redo[:3], on[:3]) and _counts(redo[3]) == _counts(on[3])
    # a session whose pool runs out in the middle of several queued pairs, hit log on
    ps = pydrt.make_params(40, 33, spp=12, max_depth=16, seed=9, batch_spp=4)  # three pairs of four samples
    small = _render_all(box, ps)
    monkeypatch.delenv("DRT_POOL_BLOCKS")
    roomy = _render_all(box, ps)
    assert small[3].redone_launches >= 1 and roomy[3].redone_launches == 0 and small[3].path_flags & pydrt.PATH_TRACE_TAIL
    assert same_films(small[0], roomy[0]) and np.array_equal(small[1], roomy[1]) and _counts(small[3]) == _counts(roomy[3])


@pytest.mark.parametrize("scene,size,spp,depth", [("cornell_large_box.scn", 40, 6, 16), ("cornell_downward.scn", 32, 5, 6), ("init_cornell.scn", 32, 4, 4), ("first_scene.scn", 24, 3, 4)])
@pytest.mark.parametrize("mode", ["spectral", "xyz"])
def test_shade_kernel_without_the_fresnel_code_changes_no_bit(scene, size, spp, depth, mode, monkeypatch):
    """Scenes whose materials list only bp_diffuse_bdsf, bp_glossy_bdsf and mirror_bdsf run the shade kernel's SIMPLE instantiation (no
    Fresnel code, five waves per SIMD: csrc/drt_kernels.h). DRT_NO_SIMPLE_SHADE=1 sends them through the general one: same film, bit for
    bit, with the tail wavelengths in the trace kernel and (DRT_TRACE_TAIL=0) through the tail pass, whose general loop is instantiated
    both ways too."""
    bundle = pydrt.load_scene(cases.scene_path(scene), size, size)
    p = pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=7, mode=pydrt.MODE_XYZ if mode == "xyz" else pydrt.MODE_SPECTRAL, batch_spp=2)
    want = oracle(bundle, p, num_threads=8) if mode == "spectral" else None
    for tail in (None, "0"):
        if tail is None:
            monkeypatch.delenv("DRT_TRACE_TAIL", raising=False)
        else:
            monkeypatch.setenv("DRT_TRACE_TAIL", tail)
        monkeypatch.delenv("DRT_NO_SIMPLE_SHADE", raising=False)
        simple = _render_all(bundle, p)
        monkeypatch.setenv("DRT_NO_SIMPLE_SHADE", "1")
        general = _render_all(bundle, p)
        monkeypatch.delenv("DRT_NO_SIMPLE_SHADE")
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(simple[0], general[0]))
        assert np.array_equal(simple[1], general[1]) and np.array_equal(simple[2], general[2], equal_nan=True) and _counts(simple[3]) == _counts(general[3])
        if want is not None:
            for v, what in ((simple, "SIMPLE"), (general, "general")):
                assert_same_film(v[0], want[:3], "%s %s tail %s" % (scene, what, tail))
                assert_same_xyz(v[2], bundle, want[0], "%s %s tail %s" % (scene, what, tail))
    monkeypatch.delenv("DRT_TRACE_TAIL", raising=False)


@pytest.mark.parametrize("spp,first_sample", [(9000, 0), (300, 4294967295 - 300), (5000, 70000)])
def test_many_samples_and_sample_numbers_up_to_2_to_the_32(spp, first_sample):
    """A tile whose call takes thousands of samples per pixel (dozens of kernel pairs of equal size), sample numbers beyond 16 bits and
    up to 2^32 - 1 (the running mean divides by them), a seed near 2^64 (the path key wraps as the reference's u64 does): every hit
    index, the draw counts and the film equal the oracle's."""
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 64, 64)
    p = pydrt.make_params(64, 64, spp=spp, first_sample=first_sample, max_depth=8, seed=0xFFFFFFFFFFFFFF00, x0=30, y0=40, tile_w=4, tile_h=3)
    film, hits, xyz, st = _render_all(bundle, p)
    opx, oav, ova, ohits, ost = oracle(bundle, p, want_hits=True, num_threads=16)
    assert np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
    assert_same_film(film, (opx, oav, ova))
    assert_same_xyz(xyz, bundle, opx)


@pytest.mark.parametrize("depth", [1, 300, 524])
def test_depth_limits_one_vertex_and_the_deepest_the_records_hold(depth):
    """max_depth 1 (a camera ray, its light sample, nothing else) and the deepest path a record table block can describe (524
    vertices: three blocks in the header, 128 in the table, four vertices each): hit indices, draw counts and film against the
    oracle; one more is refused by drt_create with the reason."""
    bundle = pydrt.load_scene(cases.scene_path("cornell_large_box.scn"), 16, 16)
    p = pydrt.make_params(16, 16, spp=3, max_depth=depth, seed=5)
    film, hits, xyz, st = _render_all(bundle, p)
    opx, oav, ova, ohits, ost = oracle(bundle, p, want_hits=True, num_threads=8)
    assert np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
    assert_same_film(film, (opx, oav, ova), "depth %d" % depth)
    assert_same_xyz(xyz, bundle, opx, "depth %d" % depth)
    if depth == 524:
        with pytest.raises(RuntimeError, match="max_depth 525"):
            pydrt.Renderer(bundle, pydrt.make_params(16, 16, spp=1, max_depth=525, seed=5))


@pytest.mark.parametrize("n_extra", [28, 70, 200])
def test_forty_to_two_hundred_lights(n_extra):
    """test_many_lights.scn with 28, 70 and 200 more plane lights: every vertex samples every light (src/daily_ray_trace.c:286), so a
    vertex record grows to 1, 2 and 8 KB (record blocks of 8, 16 and 64 KB), far beyond what the shade kernel prefetches; with 200
    the scene has 218 surfaces and goes through the hierarchy. Hit indices, draw and shadow-ray counts and the film against the oracle."""
    text = open(cases.scene_path("test_many_lights.scn")).read()
    for k in range(n_extra):
        x, z = -2.8 + 5.6 * (k % 20) / 20.0, -2.5 + 0.25 * (k // 20)
        text += "\nSurface\nname extra%d\ntype plane\nposition %.3f, 2.8, %.3f\npointu %.3f, 2.8, %.3f\npointv %.3f, 2.8, %.3f\nmaterial light%d\n" % (
            k, x, z, x + 0.1, z, x, z - 0.1, k % 3)
    bundle = pydrt.load_scene_text(text, 16, 16)
    p = pydrt.make_params(16, 16, spp=2, max_depth=5, seed=4)
    film, hits, xyz, st = _render_all(bundle, p)
    opx, oav, ova, ohits, ost = oracle(bundle, p, want_hits=True, num_threads=16)
    assert bool(st.path_flags & pydrt.PATH_BVH) == (n_extra == 200)
    assert np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
    assert_same_film(film, (opx, oav, ova), "%d more lights" % n_extra)
    assert_same_xyz(xyz, bundle, opx, "%d more lights" % n_extra)


@pytest.mark.parametrize("n_spheres", [40, 150])
@pytest.mark.parametrize("mode", ["spectral", "xyz"])
def test_more_spectra_than_lds_holds(n_spheres, mode):
    """cornell_plane_light.scn plus 150 materials of their own colours on 40 / 150 small spheres: 328 spectral rows, 181 KB at 69
    samples, more than the 64 KB the shade kernel stages in LDS -- its instantiation that reads the table from memory
    (SPDS_IN_LDS = false), never met by another test; with 150 spheres also through the hierarchy. Against the oracle."""
    import replay_shape_cases
    bundle = pydrt.load_scene_text(replay_shape_cases.many_materials_scene(150, n_spheres), 24, 24)
    assert int(bundle.scene.num_spds) * bundle.S * 8 > 64 * 1024
    p = pydrt.make_params(24, 24, spp=3, max_depth=6, seed=4, mode=pydrt.MODE_XYZ if mode == "xyz" else pydrt.MODE_SPECTRAL)
    film, hits, xyz, st = _render_all(bundle, p)
    opx, oav, ova, ohits, ost = oracle(bundle, pydrt.make_params(24, 24, spp=3, max_depth=6, seed=4), want_hits=True, num_threads=16)
    assert bool(st.path_flags & pydrt.PATH_BVH) == (n_spheres == 150) and np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
    if mode == "spectral":
        assert_same_film(film, (opx, oav, ova))
        assert_same_xyz(xyz, bundle, opx)
    else:  # DRT_MODE_XYZ folds the spectrum per kernel pair: its sums are in another order by design
        assert cases.xyz_rel_err(xyz, O.oracle_film_to_xyz(bundle, opx)) <= REF_XYZ_TOL


@pytest.mark.parametrize("W,H,tile", [(200000, 3, dict(x0=99950, y0=1, tile_w=100, tile_h=2)), (5, 3000000, dict(x0=1, y0=1499995, tile_w=3, tile_h=10)),
                                      (70000, 70000, dict(x0=69990, y0=69995, tile_w=10, tile_h=5)), (70000, 70000, dict(x0=35000, y0=34990, tile_w=12, tile_h=4, row_stride=3))])
def test_tiles_of_images_of_extreme_size(W, H, tile):
    """Tiles of frames that are 200 000 pixels wide, 3 000 000 high, and 70 000 x 70 000 (4.9 G pixels: pixel numbers and path keys
    beyond 32 bits), at the far corner and in the middle: hit indices, draw counts and film against the oracle."""
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, H)
    p = pydrt.make_params(W, H, spp=3, max_depth=6, seed=2, **tile)
    film, hits, xyz, st = _render_all(bundle, p)
    opx, oav, ova, ohits, ost = oracle(bundle, p, want_hits=True, num_threads=8)
    assert np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
    assert_same_film(film, (opx, oav, ova), "%d x %d" % (W, H))
    assert_same_xyz(xyz, bundle, opx, "%d x %d" % (W, H))


_DEGENERATE_ORACLE = {}


@pytest.mark.parametrize("name", list(cases.degenerate_scenes()))
@pytest.mark.parametrize("through_the_hierarchy", [False, True])
def test_degenerate_geometry_and_materials(name, through_the_hierarchy, monkeypatch):
    """tests/cases.py degenerate_scenes(): coincident surfaces (ties go to the lower index), spheres of radius 0 and -0.6, planes whose
    edges are parallel or of length 0, a sphere of radius 900 km next to one of a micron, roughness 0 (a 0 / 0 in ggx: NaN films,
    compared NaN for NaN) with shininess 0, 2.5 and 10^6, the camera inside the glass ball -- by the flat scan and (DRT_FORCE_BVH) through
    the hierarchy: hit indices, draw counts and film against the oracle."""
    if through_the_hierarchy:
        monkeypatch.setenv("DRT_FORCE_BVH", "1")
    bundle = pydrt.load_scene_text(cases.degenerate_scenes()[name], 24, 24)
    p = pydrt.make_params(24, 24, spp=4, max_depth=8, seed=3)
    film, hits, xyz, st = _render_all(bundle, p)
    if name not in _DEGENERATE_ORACLE:  # once per scene, for the flat scan and the hierarchy alike
        _DEGENERATE_ORACLE[name] = oracle(bundle, p, want_hits=True, num_threads=16)
    opx, oav, ova, ohits, ost = _DEGENERATE_ORACLE[name]
    assert bool(st.path_flags & pydrt.PATH_BVH) == through_the_hierarchy
    assert np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
    assert_same_film(film, (opx, oav, ova), name)
    assert_same_xyz(xyz, bundle, opx, name)


def test_hundred_thousand_spheres_through_the_hierarchy():
    """Ten times BASELINE config 5's scene (the same generator, 100 000 spheres; 400 000 were checked by hand the same way): the host
    builds the hierarchy (20 levels of the 32 the traversal stacks hold), the two BVH kernels walk it, and every hit index, the draw
    counts and the film equal the oracle's brute-force scan over all 100 000 surfaces."""
    bundle = pydrt.synthetic_sphere_scene(100000, 64, 64)
    nodes, leaves, depth, stack = pydrt.bvh_stats(bundle)
    assert leaves == 100001 and depth <= stack
    p = pydrt.make_params(64, 64, spp=2, max_depth=8, seed=1)
    film, hits, xyz, st = _render_all(bundle, p)
    opx, oav, ova, ohits, ost = oracle(bundle, p, want_hits=True, num_threads=16)
    assert st.path_flags & pydrt.PATH_BVH and np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
    assert_same_film(film, (opx, oav, ova))
    assert_same_xyz(xyz, bundle, opx)


def test_config1_at_its_stated_size_whole_frame():
    """BASELINE configs[0] exactly as named -- init_cornell.scn 256x256, 4 spp, depth 4, fixed seed -- on the HIP path: every
    hit index, the statistics and the whole film against the oracle (262 144 paths)."""
    bundle = pydrt.load_scene(cases.scene_path("init_cornell.scn"), 256, 256)
    p = pydrt.make_params(256, 256, spp=4, max_depth=4, seed=1)
    film, hits, xyz, st = _render_all(bundle, p)
    opx, oav, ova, ohits, ost = oracle(bundle, p, want_hits=True, num_threads=8)
    assert st.paths == 256 * 256 * 4 and np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
    assert_same_film(film, (opx, oav, ova))
    assert_same_xyz(xyz, bundle, opx)
    assert st.path_flags & pydrt.PATH_TRACE_TAIL  # the legacy scene is all plastic: this is the trace_tail path
    assert st.launches >= 1 and 0.0 < st.min_sample_ms <= st.avg_sample_ms <= st.max_sample_ms


def test_config2_frame_at_full_width_every_path_against_the_oracle():
    """BASELINE configs[1]'s frame -- cornell_plane_light.scn 1024x1024, depth 8 -- at 2 samples per pixel, WHOLE: every hit index
    of all 2 097 152 paths, the statistics and the whole film against the oracle (the 256-spp run of this frame is checked through
    probe pixels and invariants; this one leaves no pixel of the full-width frame unchecked)."""
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 1024, 1024)
    p = pydrt.make_params(1024, 1024, spp=2, max_depth=8, seed=1)
    film, hits, xyz, st = _render_all(bundle, p)
    opx, oav, ova, ohits, ost = oracle(bundle, p, want_hits=True, num_threads=16)
    assert st.paths == 1024 * 1024 * 2 and np.array_equal(hits, ohits) and _counts(st) == _counts(ost)
    assert_same_film(film, (opx, oav, ova))
    assert_same_xyz(xyz, bundle, opx)


@pytest.mark.parametrize("name", list(cases.NAN_CASES))
def test_nan_camera_scene_gives_the_reference_film_nan_for_nan(name, golden_dir):
    """example_scene.scn (a shipped scene whose camera has no fov / fdepth / flength, cases.NAN_CASES): every ray is NaN, nothing
    is hit, the film is NaN where the reference's is and the filter sums count the samples."""
    bundle, params = cases.load_case(name)
    px, av, va, hits, xyz, st = hip_render(bundle, params)
    opx, oav, ova, ohits, ost = oracle(bundle, params, want_hits=True)
    assert np.array_equal(hits, ohits) and (hits[:, 0] == -1).all() and _counts(st) == _counts(ost)
    assert_same_film((px, av, va), (opx, oav, ova), name)
    assert_same_xyz(xyz, bundle, opx, name)
    g = np.load(os.path.join(golden_dir, "render_%s.npz" % name), allow_pickle=False)
    assert fuzz_scenes.same(px, g["pixels"]) and fuzz_scenes.same(av, g["avgs"]) and fuzz_scenes.same(va, g["vars"])
    assert np.isnan(px[:, :bundle.S]).all() and np.all(px[:, bundle.S] == float(params.spp))


def test_bvh_box_test_never_rejects_a_box_the_ray_enters():
    """The hierarchy's f32 slab test (bvh_box_entry, called through drt_selftest_unit) against the exact test in f64 on the box
    shrunk by the builder's padding (2^-19 E): whatever the exact test accepts the f32 test must accept, with an entry bound
    that is not beyond the exact entry -- in particular for rays PARALLEL to an axis (a direction component of exactly 0, or
    one that flushes to 0 / overflows 1/d in f32) whose origin lies inside that slab, the case ADVICE r2 found rejected."""
    rng = np.random.default_rng(12)
    n = 20000
    E = 64.0
    pad = E * 2.0 ** -19
    lo = rng.uniform(-E, E, (n, 3)); hi = lo + rng.uniform(0.01, 30.0, (n, 3))
    lo32, hi32 = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)
    o = rng.uniform(-E, E, (n, 3))
    inside = rng.random(n) < 0.5
    o[inside] = (lo32 + (hi32 - lo32) * rng.uniform(0.05, 0.95, (n, 3)))[inside]
    d = rng.normal(size=(n, 3))
    kinds = rng.integers(0, 6, n)
    axis = rng.integers(0, 3, n)
    tiny = np.array([0.0, -0.0, 1e-40, -1e-39, 3e-39, 1e-31])[kinds]
    par = rng.random(n) < 0.6
    d[np.arange(n)[par], axis[par]] = tiny[par]
    two = par & (rng.random(n) < 0.3)  # parallel to two axes at once
    d[np.arange(n)[two], (axis[two] + 1) % 3] = 0.0
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    got = pydrt.selftest_unit(pydrt.UNIT_BVH_BOX, np.hstack([o, d, lo32, hi32]))[:, 0]
    # the exact test on the box less the padding, in f64 with the division made safe
    ilo, ihi = lo32 + pad, hi32 - pad
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t0, t1 = (ilo - o) / d, (ihi - o) / d
    tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
    parallel = np.abs(d) < 1e-300
    within = (o >= ilo) & (o <= ihi)
    tn = np.where(parallel, np.where(within, -np.inf, np.inf), tn)
    tf = np.where(parallel, np.where(within, np.inf, -np.inf), tf)
    enter, leave = tn.max(axis=1), tf.min(axis=1)
    accept = (enter <= leave) & (leave >= 0.0)
    assert accept.sum() > n // 4 and (accept & par).sum() > 1000
    assert np.all(got[accept] >= 0.0), "%d boxes the ray enters were rejected" % int((got[accept] < 0).sum())
    assert np.all(got[accept] <= np.maximum(enter[accept], 0.0) * (1 + 1e-6) + 1e-3)
    # a ray parallel to an axis with its origin well outside that slab misses the box, and the f32 test may say so
    away = par & ~two & ((o[np.arange(n), axis] < lo32[np.arange(n), axis] - 1.0) | (o[np.arange(n), axis] > hi32[np.arange(n), axis] + 1.0)) & (np.abs(tiny) < 1e-38)
    assert away.sum() > 100 and np.all(got[away] < 0.0)
    # the advisor's example
    one = pydrt.selftest_unit(pydrt.UNIT_BVH_BOX, np.array([[0.3, 0.0, 5.0, 0.0, 0.1 / np.hypot(0.1, 1.0), -1.0 / np.hypot(0.1, 1.0), -1, -1, -1, 1, 1, 1]], dtype=np.float64))
    assert one[0, 0] >= 0.0


def test_axis_parallel_camera_rays_through_the_hierarchy(monkeypatch):
    """End to end for the same finding: an off-axis pinhole camera and pixel centres (FILM_SAMPLE_CENTER) give camera rays with a
    direction component of exactly 0 and an origin that is not 0 on that axis; forced through the hierarchy (DRT_FORCE_BVH) the
    boxes that straddle the origin's coordinate must still be entered: hit indices equal the oracle's linear scan."""
    import re
    text = open(cases.scene_path("cornell_plane_light.scn")).read()
    text = re.sub(r"position\s+0\.0,\s*0\.0,\s*8\.0", "position 0.25, 0.5, 8.0", text, count=1)
    text = re.sub(r"target\s+0\.0,\s*0\.0,\s*0\.0", "target 0.25, 0.5, 0.0", text, count=1)
    b = pydrt.load_scene_text(text, 9, 9)
    cam = b.camera
    zero = 0
    for y in range(9):
        for x in range(9):
            pp = np.array(cam.right) * ((x + 0.5) * cam.pixel_width) + np.array(cam.up) * ((y + 0.5) * cam.pixel_height) + np.array(cam.film_bottom_left)
            dd = np.array(cam.aperture_position) - pp
            zero += int(dd[0] == 0.0 or dd[1] == 0.0)
    assert zero >= 9  # the centre column and the centre row
    p = pydrt.make_params(9, 9, spp=2, max_depth=8, seed=4, pixel_scheme=pydrt.FILM_SAMPLE_CENTER)
    opx, oav, ova, ohits, ost = oracle(b, p, want_hits=True)
    monkeypatch.setenv("DRT_FORCE_BVH", "1")
    px, av, va, hits, xyz, st = hip_render(b, p)
    monkeypatch.delenv("DRT_FORCE_BVH")
    assert st.path_flags & pydrt.PATH_BVH
    assert np.array_equal(hits, ohits), "%d closest-hit indices differ" % int((hits != ohits).sum())
    assert (ohits.reshape(2, 9, 9, -1)[0, :, 4, 0] >= 0).sum() >= 5  # most of the centre column's camera rays do hit something
    assert _counts(st) == _counts(ost)
    assert_same_film((px, av, va), (opx, oav, ova))
    assert_same_xyz(xyz, b, opx)


def test_xyz_and_bmp_bytes_of_a_film_whose_pool_ran_out(monkeypatch):
    """drt_read_xyz / drt_read_bgra straight after drt_render, with a record pool that ran out on the way: the
    conversion must see the film AFTER the skipped samples were rendered again, not the incomplete one."""
    bundle, _ = cases.load_case("plane_light_48")
    p = pydrt.make_params(48, 48, spp=30, max_depth=8, seed=3, batch_spp=12)
    r = pydrt.Renderer(bundle, p)
    r.render(0, 30)
    want_xyz, want_bgra = r.read_xyz(), [r.read_bgra(k) for k in range(3)]
    r.close()
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    for first in ("xyz", "bgra"):
        r = pydrt.Renderer(bundle, p)
        r.render(0, 30)
        if first == "xyz":
            got_xyz = r.read_xyz()       # nothing has synchronised yet: the redo happens inside this call
            got_bgra = [r.read_bgra(k) for k in range(3)]
        else:
            got_bgra = [r.read_bgra(k) for k in range(3)]
            got_xyz = r.read_xyz()
        assert r.stats().redone_launches >= 1
        r.close()
        assert np.array_equal(got_xyz, want_xyz) and all(np.array_equal(a, b) for a, b in zip(got_bgra, want_bgra)), first
    g = pydrt.Group(bundle, p, [0, 0])
    g.render(0, 30)
    st = g.stats()
    g.close()
    assert st.redone_launches >= 1 and st.record_pool_blocks > 0 and st.record_block_bytes > 0  # a group reports what its contexts did


def test_reference_side_binding_drives_the_hip_library():
    """INTEGRATION.md's reference-side stub (include/drt_reference_binding.inc, compiled against the reference's own headers in
    oracle/_ref) with libdrt_hip.so's drt_render_tile behind it: the reference's scene_data / camera_data / config go in, the
    film that comes back is the film of the reference's own pixel loop (src/daily_ray_trace.c:709-752) on that scene."""
    if not O.ref_available():
        pytest.skip("oracle/_ref was not built (it is built where /root/reference exists and travels as a library)")
    R = O.ref_lib()
    L = pydrt.hip_lib()
    for name in ("plane_light_16", "gold_mirror", "lights", "init_cornell"):
        bundle, params = cases.load_case(name)
        R.ref_set_scene(C.byref(bundle.scene))
        S, n = bundle.S, int(params.width) * int(params.height)
        px, av, va = np.zeros((n, S + 1)), np.zeros((n, S)), np.zeros((n, S))
        p1 = pydrt.make_params(int(params.width), int(params.height), spp=int(params.spp), max_depth=int(params.max_depth), seed=1,
                               pixel_scheme=int(params.pixel_scheme))
        fn = C.cast(L.drt_render_tile, O.RENDER_TILE_FN)
        rc = R.ref_run_binding(C.byref(bundle.camera), C.byref(p1), fn, O._ptr(px), O._ptr(av), O._ptr(va))
        assert rc == 0, L.drt_last_error()
        rp, ra, rv = O.ref_render_tile(bundle, p1)
        assert np.array_equal(px[:, S], rp[:, S])
        assert cases.rel_err(px, rp) <= REF_FILM_TOL and cases.rel_err(av, ra) <= REF_FILM_TOL and cases.rel_err(va, rv) <= REF_FILM_TOL, name


def test_rccl_one_rank_gather_of_a_film_block():
    """RCCL itself, on the one GPU there is: a 1-rank process group with backend "nccl" (= RCCL), a real film block rendered on
    the device into a drt_dist.FilmGather buffer, gathered by the collective bench.py uses at N > 1 (always_collective: a world
    of one otherwise just copies) and de-interleaved into the frame -- the frame equals the film read back directly. Run in a
    child process, so the process group does not outlive the test."""
    import subprocess
    import sys
    import textwrap
    pytest.importorskip("torch")
    code = textwrap.dedent("""
        import os, sys
        sys.path[:0] = [%r, %r]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch, torch.distributed as dist
        import pydrt, drt_dist
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        W, H = 96, 40
        bundle = pydrt.load_scene(%r, W, H)
        S = bundle.S
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.set_stream(stream)
        blocks = []
        image = None
        per = 16
        for j0 in range(0, H, per):
            fb = drt_dist.FilmGather(H, W, S, 0, 1, dev, j0=j0, block_rows=min(per, H - j0), image=image, always_collective=True)
            image = fb.image
            blocks.append(fb)
        films = []
        for fb in blocks:
            y0, rows, stride = fb.tile()
            p = pydrt.make_params(W, H, spp=3, max_depth=6, seed=2, y0=y0, tile_h=rows, row_stride=stride)
            r = pydrt.Renderer(bundle, p)
            r.bind_film(fb.region(0).data_ptr(), fb.region(1).data_ptr(), fb.region(2).data_ptr())
            r.set_stream(stream.cuda_stream)
            r.render(0, 3)
            fb.gather_async()
            films.append(r)
        for fb in blocks:
            fb.finish()
        torch.cuda.synchronize()
        whole = pydrt.Renderer(bundle, pydrt.make_params(W, H, spp=3, max_depth=6, seed=2))
        whole.render(0, 3)
        px, av, va = whole.read_film()
        ok = all(torch.equal(image[i].cpu().reshape(W * H, -1), torch.from_numpy(a)) for i, a in enumerate((px, av, va)))
        t = torch.tensor([1.5], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.barrier()
        print("RCCL_OK" if ok and float(t.item()) == 1.5 and float(px.sum()) > 0 else "RCCL_MISMATCH", dist.get_backend())
        for r in films: r.close()
        whole.close()
        dist.destroy_process_group()
    """) % (os.path.join(cases.REPO, "daily-ray-trace_amd"), os.path.join(cases.REPO, "tests"), cases.scene_path("cornell_plane_light.scn"))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "RCCL_OK nccl" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("name", ["plane_light_48", "gold_mirror", "grid_4nm", "grid_2p5nm", "many_lights"])
def test_fresnel_rows_tabulated_per_pair_of_media_change_no_bit(name, monkeypatch):
    """The launcher tabulates, per wavelength and pair of media, the quotients the Fresnel terms start from -- (ir/tr)^2 for glass,
    (tr/ir)^2 - (te/ir)^2 and 4 (tr/ir)^2 (te/ir)^2 for gold -- with the reference's own operations, and the shade kernel reads them
    instead of dividing per vertex. DRT_NO_PAIR_ROWS=1 turns the table off: film, XYZ, hits and statistics are the same bit for bit
    (main pass and tail pass, one and several wavelength sets, spectral and XYZ film)."""
    bundle, params = cases.load_case(name)
    want = oracle(bundle, params, want_hits=True)
    for mode in (pydrt.MODE_SPECTRAL, pydrt.MODE_XYZ):
        p = pydrt.make_params(int(params.width), int(params.height), spp=int(params.spp), max_depth=int(params.max_depth), seed=int(params.seed),
                              pixel_scheme=int(params.pixel_scheme), mode=mode)
        monkeypatch.delenv("DRT_NO_PAIR_ROWS", raising=False)
        a = _render_all(bundle, p)
        monkeypatch.setenv("DRT_NO_PAIR_ROWS", "1")
        b = _render_all(bundle, p)
        monkeypatch.delenv("DRT_NO_PAIR_ROWS")
        assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), (name, mode)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and _counts(a[3]) == _counts(b[3])
        assert float(np.abs(a[0][0]).sum()) > 0.0
        assert np.array_equal(a[1], want[3]) and np.array_equal(b[1], want[3])
        if mode == pydrt.MODE_SPECTRAL:
            for v, what in ((a, "pair rows"), (b, "no pair rows")):
                assert_same_film(v[0], want[:3], "%s %s" % (name, what))
                assert_same_xyz(v[2], bundle, want[0], "%s %s" % (name, what))


@pytest.mark.parametrize("seed", [3, 7, 12, 19, 23, 31, 40, 44, 101, 104])
def test_fresnel_rows_on_random_scenes_with_nested_media(seed, monkeypatch):
    """The same A/B on random scenes: overlapping glass / dense / gold spheres give vertices whose pair of media is NOT (base
    material, surface material) -- those keep the per-vertex divisions -- next to vertices that use the table; NaN for NaN."""
    bundle, params = fuzz_scenes.load(seed, pydrt)
    a = _render_all(bundle, params)
    monkeypatch.setenv("DRT_NO_PAIR_ROWS", "1")
    b = _render_all(bundle, params)
    monkeypatch.delenv("DRT_NO_PAIR_ROWS")
    assert all(fuzz_scenes.same(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) and _counts(a[3]) == _counts(b[3])
    want = oracle(bundle, params)
    for v, what in ((a, "pair rows"), (b, "no pair rows")):
        assert_same_film(v[0], want[:3], "seed %d %s" % (seed, what))
        assert_same_xyz(v[2], bundle, want[0], "seed %d %s" % (seed, what))


@pytest.mark.parametrize("name", ["plane_light_48", "first_scene", "lights", "grid_2p5nm", "spheres_1500"])
def test_dark_pixel_shortcut_changes_no_bit(name, monkeypatch):
    """The shade kernel passes over a sample that gathered and emitted nothing when every accumulator of the pixel is still +0 (the
    update would add +-0 to zeros). The launcher picks that instantiation unless the scene is a closed one (DRT_DARK_SKIP=0 / 1 forces
    the choice): film, XYZ and statistics are the same bit for bit either way, in the spectral and the XYZ film, also when the film
    is carried over from an earlier call (then pixels are no longer dark) and when samples come in several launches."""
    bundle, params = cases.load_case(name)
    want = oracle(bundle, pydrt.make_params(int(params.width), int(params.height), spp=int(params.spp) + 3, max_depth=int(params.max_depth),
                                            seed=int(params.seed), pixel_scheme=int(params.pixel_scheme)), num_threads=8)
    for mode in (pydrt.MODE_SPECTRAL, pydrt.MODE_XYZ):
        got = []
        for flag in ("0", "1"):
            monkeypatch.setenv("DRT_DARK_SKIP", flag)
            p = pydrt.make_params(int(params.width), int(params.height), spp=int(params.spp) + 3, max_depth=int(params.max_depth), seed=int(params.seed),
                                  pixel_scheme=int(params.pixel_scheme), mode=mode, batch_spp=2)
            r = pydrt.Renderer(bundle, p)
            r.render(0, 2)
            r.render(2, int(params.spp) + 1)
            film = (r.read_xyz_film(),) if mode == pydrt.MODE_XYZ else r.read_film()
            got.append((film, r.read_xyz(), r.stats()))
            r.close()
        monkeypatch.delenv("DRT_DARK_SKIP")
        assert all(fuzz_scenes.same(a, b) for a, b in zip(got[0][0], got[1][0])), (name, mode)
        assert fuzz_scenes.same(got[0][1], got[1][1]) and _counts(got[0][2]) == _counts(got[1][2])
        if mode == pydrt.MODE_SPECTRAL:
            for (film, xyz, _), flag in zip(got, ("0", "1")):
                assert_same_film(film, want[:3], "%s DRT_DARK_SKIP=%s" % (name, flag))
                assert_same_xyz(xyz, bundle, want[0], "%s DRT_DARK_SKIP=%s" % (name, flag))
