"""GPU (-m gpu): the material layer -- bdsf() with its seven BDSFs (src/bdsf.c:105-186, the dispatcher src/daily_ray_trace.c:215-229)
and the six direction samplers (src/bdsf.c:188-292) -- one record at a time on the device, through drt_selftest_material
(include/drt_hip.h), against the scene's own device tables.

(a) The reference's answers (tests/golden/unit_bdsf.npz, 192 points of cornell_plane_light): every value within 1e-13 relative per
    element (PI and sin/cos are x87 long double there; unit vectors also 2e-15 absolute), exact zeros, NaNs and RNG states
    identical -- so the truth table of the exact-equality tests is the reference's, not only the magnitudes.
(b) The oracle in DEVICE arithmetic (oracle/drt_oracle.c) on records the fixture lacks: directions exactly at and one ulp off the
    mirror and refracted directions, every pair of media (rows entering, leaving, none for nested media and for lists of both Fresnel
    kinds), on_dot 1, 0, the smallest normal and a subnormal one, mn_dot near 0, shininess 0 / 1 / 1023 / 1024 / 5000 / 2.5, roughness
    0 / 1e-3 / 1, total internal reflection, and a seeded random batch over all of them. Bit-exact: spectra, flags, directions,
    reciprocal pdfs, RNG states and draw counts. The one known difference is pow() in bp_glossy_bdsf (drt_pow_shininess against
    glibc): it is pinned on its own -- the device's power within the ulp bound test_device_arithmetic_is_ieee_and_matches_the_oracle_spec
    pins for it (1 ulp for integer exponents below 1024, 2 for the pow() fallback) -- and every output is then bit-exact against the
    oracle's functions folded with the device's power in place of glibc's.
(c) The "same bits" claims of the device code on every record of (a) and (b): pair rows == no pair rows, SIMPLE == general on every
    list SIMPLE accepts, and a material's own list == the Q1 fold of its single functions (the oracle's dispatcher).

Records of one launch mix materials, overrides and samplers, so the lanes of a wave diverge as they do in the kernels.
Not covered here: the trace / shade kernels' hand-inlined plastic and mirror fast paths (they are not bdsf_at_wavelength; the films
of tests/test_gpu_parity.py cover them) and direct_light_contribution (it needs the shadow ray's geometry: tests/test_gpu_edge_rays.py
holds the next-event code of every kernel that carries it to the oracle on rays built from the scenes' own coordinates, its depth-1
films being direct light and emission alone, and tests/test_edge_rays_cpu.py holds the oracle's direct_light_contribution at such hit
points to the compiled reference's, tests/golden/edge_rays.npz)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cases
from cases import same_bits
import oracle_py as O
import pydrt

pytestmark = pytest.mark.gpu

B = pydrt.BDSF
D = pydrt.DIRF
GATED_EQR = (B["fs_conductor_bdsf"], B["fs_dielectric_reflectance_bdsf"])  # functions that leave bdsf_result alone when the test fails (Q1)
GATED_EQT = (B["fs_dielectric_transmittance_bdsf"],)
FRESNEL = (B["fs_conductor_bdsf"], B["fs_dielectric_reflectance_bdsf"], B["fs_dielectric_transmittance_bdsf"], B["ct_conductor_bdsf"])
EQR, EQT = 1, 2
M64 = (1 << 64) - 1

# materials appended to cornell_plane_light.scn (which has vacuum as base, the plastics, mirror, rough gold and the Q1 dielectric)
EXTRA_MATERIALS = """
Material
name water
refract constant 1.33
bdsfs fs_dielectric_reflectance_bdsf, fs_dielectric_transmittance_bdsf
dir_func sample_reflect_or_transmit_direction

Material
name index_matched
refract constant 1.0
bdsfs fs_dielectric_transmittance_bdsf, fs_dielectric_reflectance_bdsf
dir_func sample_reflect_or_transmit_direction

Material
name mirror_after_fresnel
refract csv glass.csv
mirror rgb 0.813, 0.837, 0.888
bdsfs fs_dielectric_reflectance_bdsf, mirror_bdsf
dir_func sample_specular_direction

Material
name fresnel_after_mirror
refract csv glass.csv
mirror rgb 0.5, 0.6, 0.7
bdsfs mirror_bdsf, fs_dielectric_transmittance_bdsf, fs_dielectric_reflectance_bdsf
dir_func sample_transmit_direction

Material
name smooth_gold
refract csv au_spec_n.csv
extinct csv au_spec_k.csv
bdsfs fs_conductor_bdsf
dir_func sample_specular_direction

Material
name gold_and_glass
refract csv glass.csv
extinct csv au_spec_k.csv
roughness 0.3
bdsfs fs_dielectric_reflectance_bdsf, fs_conductor_bdsf, ct_conductor_bdsf, fs_dielectric_transmittance_bdsf
dir_func sample_reflect_or_transmit_direction

Material
name gold_r0
refract csv au_spec_n.csv
extinct csv au_spec_k.csv
roughness 0.0
bdsfs ct_conductor_bdsf, fs_conductor_bdsf
dir_func sample_ct_direction

Material
name gold_r1e3
refract csv au_spec_n.csv
extinct csv au_spec_k.csv
roughness 0.001
bdsfs ct_conductor_bdsf
dir_func sample_ct_direction

Material
name gold_r1
refract csv au_spec_n.csv
extinct csv au_spec_k.csv
roughness 1.0
bdsfs fs_conductor_bdsf, ct_conductor_bdsf
dir_func sample_ct_direction

Material
name everything
diffuse rgb 0.3, 0.4, 0.5
glossy rgb 0.2, 0.1, 0.3
mirror rgb 0.4, 0.4, 0.2
refract csv glass.csv
extinct csv au_spec_k.csv
shininess 7.0
roughness 0.2
bdsfs mirror_bdsf, bp_glossy_bdsf, fs_dielectric_transmittance_bdsf, bp_diffuse_bdsf, ct_conductor_bdsf, fs_dielectric_reflectance_bdsf, fs_conductor_bdsf
dir_func uniform_sample_hemisphere
"""
for _s, _d in (("0.0", "cos_weighted_sample_hemisphere"), ("1.0", "cos_weighted_sample_hemisphere"), ("1023.0", "uniform_sample_hemisphere"),
               ("1024.0", "cos_weighted_sample_hemisphere"), ("5000.0", "uniform_sample_hemisphere"), ("2.5", "cos_weighted_sample_hemisphere")):
    EXTRA_MATERIALS += ("\nMaterial\nname glossy_%s\ndiffuse rgb 0.3, 0.2, 0.1\nglossy rgb 0.6, 0.5, 0.4\nshininess %s\n"
                        "bdsfs bp_diffuse_bdsf, bp_glossy_bdsf\ndir_func %s\n" % (_s.replace(".", "p"), _s, _d))
EXTRA_MATERIALS += ("\nMaterial\nname glossy_mirror\nglossy rgb 0.6, 0.5, 0.4\nmirror rgb 0.3, 0.3, 0.3\nshininess 1024.0\n"
                    "bdsfs bp_glossy_bdsf, mirror_bdsf, bp_glossy_bdsf\ndir_func sample_specular_direction\n")

TINY_NORMAL = 2.2250738585072014e-308
TINY_SUB = 4.9406564584124654e-322  # 100 units of 2^-1074


# ---- scenes and renderers ------------------------------------------------------------------------------------------------------

_cache = {}


def fixture_scene():
    if "fixture" not in _cache:
        bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 64, 64)
        _cache["fixture"] = (bundle, pydrt.Renderer(bundle, pydrt.make_params(64, 64, spp=1, max_depth=1)))
    return _cache["fixture"]


def material_scene():
    if "materials" not in _cache:
        text = open(cases.scene_path("cornell_plane_light.scn")).read() + EXTRA_MATERIALS
        # one sphere of each added material, so that nothing about the scene treats them as unused
        names = [ln.split()[1] for ln in EXTRA_MATERIALS.splitlines() if ln.startswith("name ")]
        for k, nm in enumerate(names):
            text += cases._surface("s_" + nm, "sphere", "position %.1f, 2.0, -2.0\nradius 0.2" % (-2.5 + 0.25 * k), nm)
        bundle = pydrt.load_scene_text(text, 32, 32)
        _cache["materials"] = (bundle, pydrt.Renderer(bundle, pydrt.make_params(32, 32, spp=1, max_depth=1)))
    return _cache["materials"]


def teardown_module(module):
    for bundle, r in _cache.values():
        r.close()
    _cache.clear()


def mat_list(bundle, m):
    mat = bundle.scene.materials[m]
    return [int(mat.bdsfs[j]) for j in range(int(mat.num_bdsfs))]


def rec_list(bundle, rec):
    return mat_list(bundle, int(rec[10])) if rec[13] < 0 else [int(rec[13])]


def needs_of(lst):
    n = 0
    for b in lst:
        if b in (B["mirror_bdsf"],) + GATED_EQR:
            n |= EQR
        if b in GATED_EQT:
            n |= EQT
    return n


# ---- the oracle, DEVICE arithmetic ---------------------------------------------------------------------------------------------

def f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def o_point(rec):
    return O.make_point(rec[0:3], rec[3:6], rec[6:9], float(rec[9]), int(rec[10]), int(rec[11]), int(rec[12]))


def o_reflect(v, n):
    out = np.zeros(3)
    O.oracle_lib().drt_oracle_reflect(O._v3(v), O._v3(n), f64p(out))
    return out


def o_transmit(v, n, ir, tr):
    out = np.zeros(3)
    O.oracle_lib().drt_oracle_transmit(O._v3(v), O._v3(n), ir, tr, f64p(out))
    return out


_n630 = {}


def refract_at_630(bundle, m):
    """value_at_wl(refract_spd, trans_wl), as the oracle computes it"""
    key = (id(bundle), m)
    if key not in _n630:
        spd = int(bundle.scene.materials[m].refract_spd)
        row = bundle.spds()[spd].copy() if spd >= 0 else np.zeros(bundle.S)
        _n630[key] = O.oracle_lib().drt_oracle_value_at_wl(C.byref(bundle.scene), f64p(row), 630.0)
    return _n630[key]


def mirror_and_refracted(bundle, rec):
    """the directions the exact-equality tests compare against, by the oracle's own reflect / transmit"""
    n, w = np.array(rec[3:6]), -np.array(rec[6:9])
    return o_reflect(w, n), o_transmit(w, n, refract_at_630(bundle, int(rec[11])), refract_at_630(bundle, int(rec[12])))


def fold(lst, per, flags, S):
    """bdsf(), src/daily_ray_trace.c:215-229: bdsf_result zeroed once, a function whose direction test fails leaves it (Q1)"""
    res, acc = np.zeros(S), np.zeros(S)
    for b in lst:
        if not ((b in GATED_EQR and not flags & EQR) or (b in GATED_EQT and not flags & EQT)):
            res = per[b]
        acc = res + acc
    return acc


def glibc_pow(x, y):
    try:
        return math.pow(x, y)
    except (OverflowError, ValueError):
        return float("nan")


def ulps(a, b):
    """distance in units in the last place between two arrays of non-negative doubles (NaN == NaN: 0)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.abs(a.view(np.int64) - b.view(np.int64))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def oracle_evaluate(bundle, recs, dev_pow=True):
    """Expected device output ([n][S + 1]) of evaluation records: the oracle's functions at each record, folded as the oracle's
    dispatcher folds them, bp_glossy_bdsf with the device's power (drt_pow_shininess through drt_selftest_arith) in place of
    glibc's. Checks on the way that the oracle's own dispatcher gives the same fold with glibc's power. Returns (expected, facts)."""
    L = O.oracle_lib()
    O.set_math_mode(O.MATH_DEVICE)
    S, sc = bundle.S, C.byref(bundle.scene)
    spds = bundle.spds()
    n = len(recs)
    # bp_glossy_bdsf's power: (0 > nb) ? 0 : nb with nb = n . normalise(out + in), the device's operations in the device's order
    s = recs[:, 6:9] + recs[:, 14:17]
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        bis = s / ln[:, None]
        nb = (recs[:, 3] * bis[:, 0] + recs[:, 4] * bis[:, 1]) + recs[:, 5] * bis[:, 2]
    base = np.where(0.0 > nb, 0.0, nb)
    shin = np.array([float(bundle.scene.materials[int(m)].shininess) for m in recs[:, 10]])
    has_glossy = np.array([B["bp_glossy_bdsf"] in rec_list(bundle, r) for r in recs])
    dpow = np.zeros(n)
    if has_glossy.any():
        dpow[has_glossy] = pydrt.selftest_arith(7, base[has_glossy], shin[has_glossy])
    gpow = np.array([glibc_pow(float(x), float(y)) if g else 0.0 for x, y, g in zip(base, shin, has_glossy)])
    a_in = np.abs((recs[:, 3] * recs[:, 14] + recs[:, 4] * recs[:, 15]) + recs[:, 5] * recs[:, 16])
    exp = np.zeros((n, S + 1))
    out = np.zeros(S)
    facts = {"eqr": 0, "eqt": 0, "pow_ulps": {}, "pow_differs": 0}
    for i, rec in enumerate(recs):
        lst = rec_list(bundle, rec)
        P = o_point(rec)
        rin = np.ascontiguousarray(rec[14:17])
        refl, trans = mirror_and_refracted(bundle, rec)
        need = needs_of(lst)
        flags = (EQR if (need & EQR) and np.array_equal(rin, refl) else 0) | (EQT if (need & EQT) and np.array_equal(rin, trans) else 0)
        facts["eqr"] += bool(flags & EQR)
        facts["eqt"] += bool(flags & EQT)
        per = {}
        for b in set(lst):
            out[:] = 0.0
            L.drt_oracle_bdsf_func(sc, b, C.byref(P), f64p(rin), f64p(out))
            per[b] = out.copy()
        mat = bundle.scene.materials[int(rec[10])]
        if rec[13] < 0:
            L.drt_oracle_bdsf(sc, C.byref(P), f64p(rin), f64p(out))
            assert same_bits(out, fold(lst, per, flags, S)), "the fold is not the oracle's dispatcher (record %d)" % i
        if has_glossy[i]:
            g = spds[int(mat.glossy_spd)] if int(mat.glossy_spd) >= 0 else np.zeros(S)
            assert same_bits((g * gpow[i]) * a_in[i], per[B["bp_glossy_bdsf"]]), "bp_glossy_bdsf restated wrongly (record %d)" % i
            per[B["bp_glossy_bdsf"]] = (g * (dpow[i] if dev_pow else gpow[i])) * a_in[i]
            u = int(ulps(dpow[i], gpow[i]))
            y = float(shin[i])
            facts["pow_ulps"][y] = max(facts["pow_ulps"].get(y, 0), u)
            facts["pow_differs"] += u != 0
        exp[i, :S] = fold(lst, per, flags, S)
        exp[i, S] = flags
    return exp, facts


def xorshift(x):
    x ^= (x << 13) & M64
    x ^= x >> 7
    x ^= (x << 17) & M64
    return x


def xorshift_inverse(x):
    """the state whose next xorshift step gives x"""
    def inv_shl(y, k):
        v = y
        for _ in range(64 // k + 1):
            v = y ^ ((v << k) & M64)
        return v

    def inv_shr(y, k):
        v = y
        for _ in range(64 // k + 1):
            v = y ^ (v >> k)
        return v
    return inv_shl(inv_shr(inv_shl(x, 17), 7), 13)


def edge_states(rng, n):
    """states whose next draw is exactly 1 or exactly 0 (rng() is (x >> 33) / (2^31 - 1)): uniform_sample_disc then lands on the rim,
    where cos_weighted_sample_hemisphere's `q.q < 1` can fail and the loop draws again; sample_ct_direction gets f = 1 (tan = inf) or 0;
    sample_reflect_or_transmit_direction compares f = 1 or 0 with rd"""
    top = [((1 << 31) - 1) << 33, 0]
    return [xorshift_inverse(top[k % 2] | int(rng.integers(1, 1 << 33))) for k in range(n)]


def oracle_sample(bundle, recs):
    """Expected device output ([n][6]) of sampling records: the oracle's sampler from the record's state; draws counted by stepping
    the generator from the state before to the state after."""
    L = O.oracle_lib()
    O.set_math_mode(O.MATH_DEVICE)
    sc = C.byref(bundle.scene)
    exp = np.zeros((len(recs), 6))
    d = np.zeros(3)
    pdf = C.c_double()
    for i, rec in enumerate(recs):
        dirf = int(bundle.scene.materials[int(rec[10])].dir_func) if rec[13] < 0 else int(rec[13])
        st = int(np.float64(rec[14]).view(np.uint64))
        L.drt_oracle_set_rng_state(st)
        L.drt_oracle_dir_func(sc, dirf, C.byref(o_point(rec)), f64p(d), C.byref(pdf))
        after = int(L.drt_oracle_get_rng_state())
        draws, x = 0, st
        while x != after:
            x = xorshift(x)
            draws += 1
            assert draws < 100000
        exp[i, 0:3] = d
        exp[i, 3] = pdf.value
        exp[i, 4] = np.uint64(after).view(np.float64)
        exp[i, 5] = draws
    return exp


# ---- records -------------------------------------------------------------------------------------------------------------------

def eval_rec(pt, mats, incoming, bdsf=-1, mode=0):
    return np.concatenate([pt[:10], mats, [bdsf], incoming, [mode]]).astype(np.float64)


def sample_rec(pt, mats, dirf, state):
    return np.concatenate([pt[:10], mats, [dirf, np.uint64(state).view(np.float64)]]).astype(np.float64)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def unit(rng):
    v = rng.normal(size=3)
    return v / np.sqrt(dot3(v, v))


def geometries(rng):
    """(normal, out, on_dot) at the angles where kernels go wrong, and a few general ones"""
    z = np.array([0.0, 0.0, 1.0])
    g = [(z, z.copy(), 1.0),                                            # on_dot 1
         (z, np.array([1.0, 0.0, 0.0]), 0.0),                          # on_dot 0
         (z, np.array([1.0, 0.0, TINY_NORMAL]), TINY_NORMAL),          # the smallest normal on_dot
         (z, np.array([0.6, 0.8, TINY_SUB]), TINY_SUB),                # subnormal on_dot
         (z, np.array([np.sqrt(1.0 - 1e-6), 0.0, 1e-3]), 1e-3)]        # near grazing
    for _ in range(3):
        nrm = unit(rng)
        out = unit(rng)
        if dot3(nrm, out) < 0:
            out = -out
        g.append((nrm, out, dot3(nrm, out)))
    return [np.concatenate([[0.1, 0.2, 0.3], n, o, [c]]) for n, o, c in g]


def media(bundle, m, water):
    base = int(bundle.scene.base_material)
    return [(m, base, m), (m, m, base), (m, water, m), (m, m, water)]  # entering, leaving (pair_out, pair_in), nested (no rows)


def incomings(bundle, pt, mats, rng):
    """exactly the mirror and the refracted direction, each one ulp off, and a random one"""
    rec = np.concatenate([pt[:10], mats])
    refl, trans = mirror_and_refracted(bundle, rec)
    res = [refl, trans, unit(rng)]
    for v in (refl, trans):
        w = v.copy()
        w[0] = np.nextafter(w[0], np.inf)
        res.append(w)
        w = v.copy()
        w[2] = np.nextafter(w[2], -np.inf)
        res.append(w)
    return res


def bdsf_materials(bundle):
    return [m for m in range(int(bundle.scene.num_materials)) if int(bundle.scene.materials[m].num_bdsfs) > 0]


def hand_made(bundle, rng):
    names = bundle.material_names()
    water = names.index("water")
    ev, sm = [], []
    geo = geometries(rng)
    for m in bdsf_materials(bundle):
        for mats in media(bundle, m, water):
            for pt in geo:
                for rin in incomings(bundle, pt, mats, rng):
                    for b in [-1] + list(range(7)):
                        ev.append(eval_rec(pt, mats, rin, b))
                for dirf in [-1] + list(range(6)):
                    for st in [int(rng.integers(1, 2 ** 63)) for _ in range(4)] + edge_states(rng, 4):
                        sm.append(sample_rec(pt, mats, dirf, st))
    return np.array(ev), np.array(sm)


def random_batch(bundle, rng, n_eval=20000, n_sample=20000):
    names = bundle.material_names()
    water = names.index("water")
    mats_ok = bdsf_materials(bundle)
    ev, sm = [], []
    while len(ev) < n_eval:
        m = int(rng.choice(mats_ok))
        mats = media(bundle, m, water)[int(rng.integers(0, 4))]
        nrm, out = unit(rng), unit(rng)
        if dot3(nrm, out) < 0:
            out = -out
        pt = np.concatenate([rng.uniform(-2, 2, 3), nrm, out, [dot3(nrm, out)]])
        ins = incomings(bundle, pt, mats, rng)
        b = int(rng.integers(-1, 7))
        lst = mat_list(bundle, m) if b < 0 else [b]
        mode = int(rng.integers(0, 2)) | (pydrt.MAT_MODE_SIMPLE if not set(lst) & set(FRESNEL) and rng.integers(0, 2) else 0)
        ev.append(eval_rec(pt, mats, ins[int(rng.integers(0, len(ins)))], b, mode))
    while len(sm) < n_sample:
        m = int(rng.choice(mats_ok))
        mats = media(bundle, m, water)[int(rng.integers(0, 4))]
        nrm, out = unit(rng), unit(rng)
        if dot3(nrm, out) < 0:
            out = -out
        pt = np.concatenate([rng.uniform(-2, 2, 3), nrm, out, [dot3(nrm, out)]])
        sm.append(sample_rec(pt, mats, int(rng.integers(-1, 6)), int(rng.integers(1, 2 ** 63))))
    return np.array(ev), np.array(sm)


# ---- checks --------------------------------------------------------------------------------------------------------------------

def check_evaluate(bundle, r, recs, what):
    """device == oracle (b), bit for bit; returns the device output"""
    dev = pydrt.selftest_material(r, pydrt.MAT_EVALUATE, recs)
    exp, facts = oracle_evaluate(bundle, recs)
    for y, u in facts["pow_ulps"].items():
        assert u <= (1 if y == int(y) and y < 1024 else 2), "%s: the device's pow(x, %g) is %d ulp from glibc's" % (what, y, u)
    bad = [i for i in range(len(recs)) if not same_bits(dev[i], exp[i])]
    if bad:
        i = bad[0]
        k = np.flatnonzero(~((dev[i] == exp[i]) | (np.isnan(dev[i]) & np.isnan(exp[i]))))
        raise AssertionError("%s: %d of %d records differ from the oracle; first: record %s -> device %s, oracle %s at %s (ulps %s)"
                             % (what, len(bad), len(recs), recs[i].tolist(), dev[i][k[:4]], exp[i][k[:4]], k[:4],
                                ulps(np.abs(dev[i][k[:4]]), np.abs(exp[i][k[:4]]))))
    return dev, facts


def check_sample(bundle, r, recs, what):
    dev = pydrt.selftest_material(r, pydrt.MAT_SAMPLE, recs)
    exp = oracle_sample(bundle, recs)
    bad = [i for i in range(len(recs)) if not same_bits(dev[i], exp[i])]
    assert not bad, "%s: %d of %d sampling records differ from the oracle; first: %s -> device %s, oracle %s" % (
        what, len(bad), len(recs), recs[bad[0]].tolist(), dev[bad[0]].tolist(), exp[bad[0]].tolist())
    return dev


def check_same_bits(bundle, r, recs, dev, what):
    """(c): the device's own shortcuts against its own plain forms, on every record"""
    S = bundle.S
    flip = recs.copy()
    flip[:, 17] = recs[:, 17].astype(np.int64) ^ pydrt.MAT_MODE_UNPAIRED
    alt = pydrt.selftest_material(r, pydrt.MAT_EVALUATE, flip)
    bad = [i for i in range(len(recs)) if not same_bits(alt[i], dev[i])]
    assert not bad, "%s: pair rows and no pair rows differ on %d records, first %s" % (what, len(bad), recs[bad[0]].tolist())
    simple_ok = np.array([not set(rec_list(bundle, rec)) & set(FRESNEL) for rec in recs])
    flip = recs[simple_ok].copy()
    flip[:, 17] = flip[:, 17].astype(np.int64) ^ pydrt.MAT_MODE_SIMPLE
    alt = pydrt.selftest_material(r, pydrt.MAT_EVALUATE, flip)
    bad = [i for i in range(len(flip)) if not same_bits(alt[i], dev[simple_ok][i])]
    assert not bad, "%s: SIMPLE and general instantiations differ on %d records, first %s" % (what, len(bad), flip[bad[0]].tolist())
    # own list == the Q1 fold of the device's single functions at the same point and direction
    own = np.flatnonzero(recs[:, 13] < 0)
    singles, where = [], []
    for i in own:
        for b in mat_list(bundle, int(recs[i, 10])):
            rr = recs[i].copy()
            rr[13] = b
            singles.append(rr)
            where.append((i, b))
    one = pydrt.selftest_material(r, pydrt.MAT_EVALUATE, np.array(singles))
    per = {}
    for (i, b), row in zip(where, one):
        per.setdefault(i, {})[b] = row[:S]
    for i in own:
        f = fold(mat_list(bundle, int(recs[i, 10])), per[i], int(dev[i, S]), S)
        assert same_bits(f, dev[i, :S]), "%s: own list is not the fold of its functions at record %s" % (what, recs[i].tolist())
    return int(simple_ok.sum()), len(singles)


# ---- tests ---------------------------------------------------------------------------------------------------------------------

def fixture_records(golden_dir):
    g = np.load(os.path.join(golden_dir, "unit_bdsf.npz"), allow_pickle=False)
    pts = np.hstack([g["points"][:, :10], g["materials"].astype(np.float64)])
    return g, pts


def test_bdsfs_and_samplers_match_the_reference_fixture(golden_dir):
    bundle, r = fixture_scene()
    g, pts = fixture_records(golden_dir)
    n, S = len(pts), bundle.S
    assert np.all(g["points"][:, 10] == 630.0)  # trans_wl: the device's is fixed at 630 nm
    # per_func: each BDSF alone on a zeroed result at random_in
    per = np.array([eval_rec(pts[i], pts[i, 10:13], g["random_in"][i], b) for i in range(n) for b in range(7)])
    # sum_random / sum_sampled: the material's own list at random_in and at the REFERENCE's sampled direction (exact tests fire there)
    sums = np.array([eval_rec(pts[i], pts[i, 10:13], d[i], -1) for d in (g["random_in"], g["sampled_dir"]) for i in range(n)])
    recs = np.vstack([per, sums])
    dev = pydrt.selftest_material(r, pydrt.MAT_EVALUATE, recs)
    want = np.vstack([g["per_func"].reshape(n * 7, S), g["sum_random"], g["sum_sampled"]])
    got = dev[:, :S]
    assert np.array_equal(got == 0.0, want == 0.0), "exact zeros (the equality tests' truth table) differ from the reference's"
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, equal_nan=True)
    # the flags word: the mirror-direction test fires on the sampled directions of mirror and dielectric points, never at random_in
    assert (dev[n * 7:n * 8, S] == 0).all() and (dev[n * 8:, S] != 0).any()
    # samplers: all six from the same state, and the material's own one (state after included)
    smp = np.array([sample_rec(pts[i], pts[i, 10:13], f, g["rng_state"][i]) for i in range(n) for f in range(6)])
    own = np.array([sample_rec(pts[i], pts[i, 10:13], -1, g["rng_state"][i]) for i in range(n)])
    ds = pydrt.selftest_material(r, pydrt.MAT_SAMPLE, np.vstack([smp, own]))
    np.testing.assert_allclose(ds[:n * 6, :3], g["all_dirs"].reshape(-1, 3), rtol=1e-13, atol=2e-15, equal_nan=True)
    np.testing.assert_allclose(ds[:n * 6, 3], g["all_pdfs"].reshape(-1), rtol=1e-13, atol=0, equal_nan=True)
    np.testing.assert_allclose(ds[n * 6:, :3], g["sampled_dir"], rtol=1e-13, atol=2e-15, equal_nan=True)
    np.testing.assert_allclose(ds[n * 6:, 3], g["sampled_pdf"], rtol=1e-13, atol=0, equal_nan=True)
    assert np.array_equal(ds[n * 6:, 4].copy().view(np.uint64), g["state_after"])
    assert np.array_equal(np.isnan(ds[n * 6:, :4]), np.isnan(np.hstack([g["sampled_dir"], g["sampled_pdf"][:, None]])))
    # the same records against the oracle, bit for bit, and (c) on them
    check_evaluate(bundle, r, recs, "fixture")
    check_sample(bundle, r, np.vstack([smp, own]), "fixture")
    check_same_bits(bundle, r, recs, dev, "fixture")
    print("fixture: %d points, %d evaluation and %d sampling records" % (n, len(recs), len(smp) + len(own)))


def test_hand_made_edges_against_the_oracle():
    bundle, r = material_scene()
    names = bundle.material_names()
    S = bundle.S
    rng = np.random.default_rng(20261015)
    ev, sm = hand_made(bundle, rng)
    perm = rng.permutation(len(ev))  # materials, media and overrides mixed inside every wave
    ev = ev[perm]
    sm = sm[rng.permutation(len(sm))]
    dev, facts = check_evaluate(bundle, r, ev, "hand-made")
    assert facts["eqr"] > 0 and facts["eqt"] > 0
    # the pow() fallback (1024, 5000, 2.5) and the clamped base (pow(0, 0) = 1) were met
    assert {0.0, 1.0, 1023.0, 1024.0, 5000.0, 2.5} <= set(facts["pow_ulps"])
    # Q1 on the dielectric's list: 2R at the mirror direction (carry-over), T at the refracted one, 0 one ulp off either
    diel = names.index("dielectric")
    q1 = np.flatnonzero((ev[:, 10] == diel) & (ev[:, 13] == -1))
    rt = ev[q1].copy()
    rt[:, 13] = B["fs_dielectric_reflectance_bdsf"]
    tt = ev[q1].copy()
    tt[:, 13] = B["fs_dielectric_transmittance_bdsf"]
    single = pydrt.selftest_material(r, pydrt.MAT_EVALUATE, np.vstack([rt, tt]))[:, :S]
    seen = [0, 0, 0]
    for k, i in enumerate(q1):
        refl, trans = mirror_and_refracted(bundle, ev[i])
        rin = ev[i, 14:17]
        if np.array_equal(rin, refl):
            R = single[k]
            assert same_bits(dev[i, :S], R + R) and dev[i, S] == EQR and (R > 0).all()
            seen[0] += 1
        elif np.array_equal(rin, trans):
            assert same_bits(dev[i, :S], single[len(q1) + k]) and dev[i, S] == EQT
            seen[1] += 1
        else:
            assert (dev[i, :S] == 0.0).all() and dev[i, S] == 0
            seen[2] += 1
    assert min(seen) > 0, seen
    ds = check_sample(bundle, r, sm, "hand-made")
    dirf = np.array([int(bundle.scene.materials[int(x[10])].dir_func) if x[13] < 0 else int(x[13]) for x in sm])
    draws = ds[:, 5]
    assert (draws[dirf == D["cos_weighted_sample_hemisphere"]] > 2).any(), "the disc rejection loop never repeated"
    assert (draws[dirf == D["sample_ct_direction"]] > 2).any(), "the GGX rejection loop never repeated"
    # sample_reflect_or_transmit_direction with rd = 1 (total internal reflection from inside: reflect, 1/pdf = 1) and rd = 0
    # (index-matched at normal incidence: transmit, 1/pdf = 1) -- both through the same draw
    rt = dirf == D["sample_reflect_or_transmit_direction"]
    assert (rt & (ds[:, 3] == 1.0)).sum() > 0
    n_simple, n_single = check_same_bits(bundle, r, ev, dev, "hand-made")
    print("hand-made: %d evaluation records (%d also SIMPLE, %d single functions for the fold), %d sampling records; pow differs from "
          "glibc on %d, bounds by exponent %s" % (len(ev), n_simple, n_single, len(sm), facts["pow_differs"], facts["pow_ulps"]))


def test_random_batch_against_the_oracle():
    bundle, r = material_scene()
    rng = np.random.default_rng(1015)
    ev, sm = random_batch(bundle, rng)
    dev, facts = check_evaluate(bundle, r, ev, "random")
    check_sample(bundle, r, sm, "random")
    n_simple, n_single = check_same_bits(bundle, r, ev, dev, "random")
    assert facts["eqr"] > 100 and facts["eqt"] > 100
    print("random: %d evaluation records (%d mirror, %d refracted direction hits; %d also SIMPLE), %d sampling records"
          % (len(ev), facts["eqr"], facts["eqt"], n_simple, len(sm)))


def test_pair_rows_are_used_where_they_exist():
    """The override tables keep a material's pair rows only for a function of their kind, and record_media_word picks pair_out /
    pair_in / none by the media: seen from outside, (c) compares paired with unpaired; here, a conductor's rows are never read for a
    dielectric function and vice versa (a mismatch would not be bit-equal to the oracle in check_evaluate)."""
    bundle, r = material_scene()
    names = bundle.material_names()
    base = int(bundle.scene.base_material)
    rng = np.random.default_rng(7)
    recs = []
    for nm in ("smooth_gold", "gold", "dielectric", "water", "gold_and_glass", "everything"):
        m = names.index(nm)
        for mats in ((m, base, m), (m, m, base)):
            for pt in geometries(rng):
                for rin in incomings(bundle, pt, mats, rng):
                    for b in [-1] + list(FRESNEL):
                        recs.append(eval_rec(pt, mats, rin, b, 0))
    recs = np.array(recs)
    dev, _ = check_evaluate(bundle, r, recs, "pairs")
    check_same_bits(bundle, r, recs, dev, "pairs")


def test_refusals():
    bundle, r = fixture_scene()
    L = pydrt.hip_lib()
    S = bundle.S
    pt = np.array([0, 0, 0, 0, 0, 1, 0, 0, 1, 1.0])
    names = bundle.material_names()
    plastic, diel = names.index("blue_plastic"), names.index("dielectric")
    base = int(bundle.scene.base_material)
    good = eval_rec(pt, [plastic, base, plastic], [0, 0, 1.0])
    out = np.zeros((1, S + 1))

    def call(func, rec, out_stride=S + 1):
        rec = np.ascontiguousarray(rec[None, :])
        o = np.zeros((1, max(out_stride, 1)))
        return L.drt_selftest_material(r.ctx, func, f64p(rec), rec.shape[1], f64p(o), out_stride, 1)

    assert call(pydrt.MAT_EVALUATE, good) == 0
    assert call(pydrt.MAT_EVALUATE, good[:17]) != 0  # narrower than the function reads
    assert call(pydrt.MAT_EVALUATE, good, S) != 0  # no room for the flags word
    assert call(pydrt.MAT_SAMPLE, sample_rec(pt, [plastic, base, plastic], -1, 5)[:14]) != 0
    assert call(pydrt.MAT_SAMPLE, sample_rec(pt, [plastic, base, plastic], -1, 5), 5) != 0
    for bad in (int(bundle.scene.num_materials), -1, 0.5, np.nan):
        for k in range(3):
            rec = good.copy()
            rec[10 + k] = bad
            assert call(pydrt.MAT_EVALUATE, rec) != 0
            assert "material" in L.drt_last_error().decode()
    for b in (7, -2, 2.5):
        rec = good.copy()
        rec[13] = b
        assert call(pydrt.MAT_EVALUATE, rec) != 0
    for f in (6, -2):
        assert call(pydrt.MAT_SAMPLE, sample_rec(pt, [plastic, base, plastic], f, 5)) != 0
    assert call(2, good) != 0
    simple = good.copy()
    simple[17] = pydrt.MAT_MODE_SIMPLE
    assert call(pydrt.MAT_EVALUATE, simple) == 0
    simple[10] = simple[12] = diel  # the dielectric's own list holds Fresnel functions
    assert call(pydrt.MAT_EVALUATE, simple) != 0 and "SIMPLE" in L.drt_last_error().decode()
    simple[13] = B["bp_diffuse_bdsf"]  # ... a plain override of it does not
    assert call(pydrt.MAT_EVALUATE, simple) == 0
    simple[13] = B["ct_conductor_bdsf"]
    assert call(pydrt.MAT_EVALUATE, simple) != 0
    del out
