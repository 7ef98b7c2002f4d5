"""GPU (-m gpu): material updates of a live context (drt_update_spectra, drt_update_materials, their group forms, pydrt's bindings, the
drt_render program's DRT_LIGHT_LEVELS). The rule: an updated context gives bit for bit what a fresh context on
the updated scene gives. Every film comparison is cases.same_bits on all three buffers (the XYZ accumulators in DRT_MODE_XYZ), hit logs
with array_equal, the counting statistics with ==, each against a fresh context on the "after" bundle of tests/material_update_cases.py
AND against the oracle. tests/test_material_update_cpu.py holds the premises (every "after" film differs from its "before" film).

DRT_MODE_XYZ folds the spectrum per kernel pair, so its sums are in another order than the oracle's by design: there the oracle holds
the hit log and the counts exactly and the XYZ image within tests/test_gpu_parity.py's REF_XYZ_TOL of 1e-9; the fresh context holds
the accumulators bit for bit."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import feature_rule as F
import material_update_cases as MU
import matte_rule as M
import oracle_py as O
import pydrt
import ray_query_cases as Q
import scene_update_cases as U

pytestmark = pytest.mark.gpu

XYZ_TOL = 1e-9
HIT_FLOATS = ("position", "normal", "out", "on_dot", "distance")
HIT_INTS = ("index", "surface_material", "incident_material", "transmit_material")
_fresh, _oracle = {}, {}


def assert_same_film(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert cases.same_bits(a, b), "%s buffer %d: %s" % (what, k, cases.first_difference(a, b))


@contextlib.contextmanager
def environment(**env):
    saved = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@contextlib.contextmanager
def context(name, which="before", params=None, **env):
    """a context on a case's scene (DRT_FORCE_BVH and the other knobs are read when the context is created)"""
    c = MU.load(name)
    with environment(DRT_FORCE_BVH="1" if c["forced"] else None, **env):
        r = pydrt.Renderer(c[which], params or c["params"])
    try:
        assert bool(r.stats().path_flags & pydrt.PATH_BVH) == c["bvh"], name
        yield r
    finally:
        r.close()


def read_film(r, p):
    return (r.read_xyz_film(),) if int(p.mode) == pydrt.MODE_XYZ else r.read_film()


def rendered(r, p):
    """(film, hit log, counting statistics) of one drt_render call"""
    r.render()
    return read_film(r, p), r.read_hit_indices(int(p.spp)), cases.stat_counts(r.stats())


def fresh(name, which="after"):
    """a fresh context's (film, hit log, counts) on a case's scene, rendered once"""
    if (name, which) not in _fresh:
        with context(name, which) as r:
            _fresh[(name, which)] = rendered(r, MU.load(name)["params"])
    return _fresh[(name, which)]


def oracle(name):
    if name not in _oracle:
        c = MU.load(name)
        q = MU._params(c["params"], mode=pydrt.MODE_SPECTRAL)
        px, av, va, log, st = cases.oracle_render_device_pow(c["after"], q, want_hits=True)
        _oracle[name] = ((px, av, va), log, cases.stat_counts(st))
    return _oracle[name]


def assert_is_after(got, name, what, with_oracle=True, r=None):
    """a (film, hit log, counts) triple against the fresh context on the "after" scene and against the oracle"""
    film, log, counts = fresh(name)
    assert_same_film(got[0], film, "%s (%s) against a fresh context" % (name, what))
    assert np.array_equal(got[1], log), "%s (%s): hit log against a fresh context" % (name, what)
    assert got[2] == counts, "%s (%s): counts against a fresh context" % (name, what)
    if not with_oracle:
        return
    film, log, counts = oracle(name)
    assert np.array_equal(got[1], log), "%s (%s): hit log against the oracle" % (name, what)
    assert got[2] == counts, "%s (%s): counts against the oracle" % (name, what)
    if int(MU.load(name)["params"].mode) == pydrt.MODE_XYZ:
        err = cases.xyz_rel_err(r.read_xyz(), O.oracle_film_to_xyz(MU.load(name)["after"], film[0]))
        assert err <= XYZ_TOL, "%s (%s): XYZ against the oracle: %g" % (name, what, err)
    else:
        assert_same_film(got[0], film, "%s (%s) against the oracle" % (name, what))


def assert_is_before(got, name, what):
    film, log, counts = fresh(name, "before")
    assert_same_film(got[0], film, "%s (%s) against the scene before" % (name, what))
    assert np.array_equal(got[1], log) and got[2] == counts, "%s (%s)" % (name, what)


def changed_rows(name, to="after"):
    """(first_row, rows) of the smallest range that holds every SPD row in which the case's two scenes differ"""
    c = MU.load(name)
    other = "before" if to == "after" else "after"
    new, old = c[to].spds(), c[other].spds()
    rows = [k for k in range(new.shape[0]) if not cases.same_bits(new[k], old[k])]
    if not rows:
        return 0, new[0:0]
    return rows[0], new[rows[0]:rows[-1] + 1]


def apply(r, name, to="after", device=False):
    """what takes a context of one of the case's scenes to the other: its changed SPD rows, its material parameters"""
    first, rows = changed_rows(name, to)
    if len(rows):
        if device:
            import torch
            rows = torch.from_numpy(rows.copy()).to("cuda:0")
        r.update_spectra(rows, first=first)
    if name in MU.MATERIALS:
        r.update_materials(MU.load(name)[to].materials())


# ------------------------------------------------------------------------------------------------ every case, there and back
@pytest.mark.parametrize("name", MU.ALL)
def test_an_update_in_host_mode_gives_a_fresh_contexts_bits_and_the_old_film_again(name):
    c = MU.load(name)
    p = c["params"]
    with context(name) as r:
        first = rendered(r, p)
        assert_is_before(first, name, "before the update")
        assert not all(cases.same_bits(a, b) for a, b in zip(first[0], fresh(name)[0]))
        r.reset_film()
        apply(r, name)
        assert_is_after(rendered(r, p), name, "host mode", r=r)
        r.reset_film()
        apply(r, name, to="before")
        back = rendered(r, p)
        assert_same_film(back[0], first[0], name + ": the first scene again")
        assert np.array_equal(back[1], first[1]) and back[2] == first[2]


# ------------------------------------------------------------------------------------------------ ranges and history
@pytest.mark.parametrize("name", ["nan_and_zero", "lights_bvh"])
def test_ranges_and_history(name):
    c = MU.load(name)
    p = c["params"]
    after = c["after"].spds()
    n = after.shape[0]
    first, rows = changed_rows(name)
    assert first > 4 and len(rows) > 2  # first > 0, count < n, and unchanged rows in between
    with context(name) as r:
        r.update_spectra(after[4:], first=4)  # everything but the observer's rows
        assert_is_after(rendered(r, p), name, "rows 4 .. n")
        r.reset_film()
        # two updates in a row equal the second alone: first other values altogether, then the case's
        other = after[4:] * 0.5 + 0.125
        r.update_spectra(other, first=4)
        r.update_spectra(rows[:1], first=first)  # a part of it ...
        r.update_spectra(after[4:], first=4)
        assert_is_after(rendered(r, p), name, "two updates in a row", with_oracle=False)
        r.reset_film()
        # row by row, last row first
        r.update_spectra(c["before"].spds()[4:], first=4)
        for k in reversed(range(len(rows))):
            r.update_spectra(rows[k:k + 1], first=first + k)
        assert_is_after(rendered(r, p), name, "row by row", with_oracle=False)
        # count == 0: a successful no-op, whatever the film holds
        r.update_spectra(after[0:0])
        r.update_spectra(after[0:0], first=n)
        r.update_materials(c["after"].materials()[0:0])
        r.update_materials([], first=int(c["after"].scene.num_materials))
        r.reset_film()
        assert_is_after(rendered(r, p), name, "after count == 0", with_oracle=False)


def test_spectra_then_materials_and_materials_then_spectra():
    """the glass's refract row and the GGX roughness of one scene, in both orders: each call keeps what the other has written
    (drt_update_materials copies whole records, refract_i0 / refract_i1 included)"""
    glass, rough = MU.load("glass_refract"), MU.load("roughness")
    p = glass["params"]
    both = MU.with_tables(glass["before"], spds=glass["after"].spds(), materials=rough["after"].materials())
    with environment(DRT_FORCE_BVH=None):
        r = pydrt.Renderer(both, p)
    try:
        want = rendered(r, p)
    finally:
        r.close()
    px, av, va, log, st = cases.oracle_render_device_pow(both, p, want_hits=True)
    assert_same_film(want[0], (px, av, va), "both edits against the oracle")
    assert np.array_equal(want[1], log) and want[2] == cases.stat_counts(st)
    for k in (1, 2):
        assert not np.array_equal(want[1], fresh(("glass_refract", "roughness")[k - 1])[1])  # neither edit alone
    for order in ("spectra first", "materials first"):
        with context("glass_refract") as r:
            steps = [lambda: apply(r, "glass_refract"), lambda: apply(r, "roughness")]
            for step in (steps if order == "spectra first" else steps[::-1]):
                step()
            got = rendered(r, p)
            assert_same_film(got[0], want[0], order)
            assert np.array_equal(got[1], want[1]) and got[2] == want[2], order


# ------------------------------------------------------------------------------------------------ device mode
@pytest.mark.parametrize("name", ["wall_diffuse", "glass_refract", "base_refract", "grid_2p5nm_60_rows", "spheres_1500", "xyz", "nan_and_zero"])
def test_device_mode_gives_host_modes_bits_and_the_mirrors_are_read_back(name):
    pytest.importorskip("torch")
    c = MU.load(name)
    p = c["params"]
    with context(name) as r:
        assert_is_before(rendered(r, p), name, "before the update")
        r.reset_film()
        apply(r, name, device=True)
        assert_is_after(rendered(r, p), name, "device mode", r=r)
        # a host-mode update of a part after it starts from the device's rows: back and forth on the first changed row only
        r.reset_film()
        first, rows = changed_rows(name)
        r.update_spectra(c["before"].spds()[first:first + 1], first=first)
        r.update_spectra(rows[:1], first=first)
        assert_is_after(rendered(r, p), name, "host mode after device mode", with_oracle=False)
        # and drt_update_materials, whose records carry refract_i0 / refract_i1, after a device-mode update
        r.reset_film()
        apply(r, name, to="before", device=True)
        apply(r, name, device=True)
        r.update_materials(c["after"].materials())
        assert_is_after(rendered(r, p), name, "materials after device mode", with_oracle=False)


def test_device_mode_then_features_takes_the_colour_table_from_the_new_spectra():
    pytest.importorskip("torch")
    name = "wall_diffuse"
    c = MU.load(name)
    p = c["params"]
    with context(name) as r:
        apply(r, name, device=True)
        r.render_features(n_samples=3, first_sample=1)
        mean, m2, ids = r.read_features()
    wmean, wm2, wids, _, _ = F.features(c["after"], p, n_samples=3, first_sample=1)
    bmean = F.features(c["before"], p, n_samples=3, first_sample=1)[0]
    assert cases.same_bits(mean, wmean) and cases.same_bits(m2, wm2) and np.array_equal(ids, wids)
    assert not cases.same_bits(wmean, bmean)  # the albedo channels tell the two walls apart


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name", ["glass_refract", "spheres_1500"])
def test_refusals_change_nothing(name):
    torch = pytest.importorskip("torch")
    c = MU.load(name)
    p = c["params"]
    L = pydrt.hip_lib()
    after = c["after"].spds()
    n, S = after.shape
    sc = c["after"].scene
    n_mat = int(sc.num_materials)
    first, rows = changed_rows(name)
    plastic = MU.material(c["after"], bdsfs=[MU.DIFFUSE, MU.GLOSSY])
    with context(name) as r:
        def refused(match, call):
            with pytest.raises(RuntimeError, match=match):
                call()

        def changed(**fields):
            mats = c["after"].materials()
            for f, v in fields.items():
                if f == "bdsfs":
                    mats[plastic].bdsfs[1] = v
                else:
                    setattr(mats[plastic], f, v)
            mats[plastic].shininess = 5.0
            return mats
        # a film with samples
        r.render()
        refused("drt_update_spectra: the film holds samples", lambda: r.update_spectra(rows, first=first))
        refused("drt_update_spectra: the film holds samples", lambda: r.update_spectra(torch.from_numpy(rows.copy()).to("cuda:0"), first=first))
        refused("drt_update_materials: the film holds samples", lambda: r.update_materials(changed()))
        r.reset_film()
        # the observer's rows, alone and inside a range
        for row, what in ((int(sc.cmf_rw), "cmf_rw"), (int(sc.cmf_x), "cmf_x"), (int(sc.cmf_y), "cmf_y"), (int(sc.cmf_z), "cmf_z")):
            refused("row %d is the scene's %s" % (row, what), lambda: r.update_spectra(after[row:row + 1], first=row))
        refused("is the scene's cmf_", lambda: r.update_spectra(after))
        refused("is the scene's cmf_z", lambda: r.update_spectra(torch.from_numpy(after[3:].copy()).to("cuda:0"), first=3))
        # rows and materials out of range, null with count > 0, unknown flags
        refused("rows \\[5, %d\\) of %d" % (n + 1, n), lambda: r.update_spectra(after[4:], first=5))
        refused("rows \\[%d, %d\\) of %d" % (n + 1, n + 1, n), lambda: r.update_spectra(after[0:0], first=n + 1))
        refused("materials \\[1, %d\\) of %d" % (n_mat + 1, n_mat), lambda: r.update_materials(c["after"].materials(), first=1))
        assert L.drt_update_spectra(r.ctx, None, first, 1, 0) != 0 and b"rows is null" in L.drt_last_error()
        assert L.drt_update_materials(r.ctx, None, 0, 1, 0) != 0 and b"materials is null" in L.drt_last_error()
        assert L.drt_update_spectra(r.ctx, rows.ctypes.data, first, len(rows), 2) != 0 and b"unknown flags" in L.drt_last_error()
        assert L.drt_update_spectra(r.ctx, rows.ctypes.data, first, len(rows), 4 | pydrt.SPECTRA_DEVICE) != 0 and b"unknown flags" in L.drt_last_error()
        mats = changed()
        assert L.drt_update_materials(r.ctx, C.cast(mats, C.c_void_p), 0, n_mat, 1) != 0 and b"unknown flags" in L.drt_last_error()
        assert L.drt_update_spectra(None, rows.ctypes.data, first, len(rows), 0) != 0 and L.drt_update_materials(None, C.cast(mats, C.c_void_p), 0, n_mat, 0) != 0
        # a material field other than shininess and roughness: the message names the first material and field
        refused("material %d: bdsfs\\[1\\] %d, was %d" % (plastic, MU.MIRROR, MU.GLOSSY), lambda: r.update_materials(changed(bdsfs=MU.MIRROR)))
        refused("material %d: dir_func 1, was 0" % plastic, lambda: r.update_materials(changed(dir_func=1)))
        refused("material %d: is_emissive 1, was 0" % plastic, lambda: r.update_materials(changed(is_emissive=1)))
        refused("material %d: is_black_body 1, was 0" % plastic, lambda: r.update_materials(changed(is_black_body=1)))
        refused("material %d: num_bdsfs 1, was 2" % plastic, lambda: r.update_materials(changed(num_bdsfs=1)))
        was = int(sc.materials[plastic].diffuse_spd)
        refused("material %d: diffuse_spd %d, was %d" % (plastic, was + 1, was), lambda: r.update_materials(changed(diffuse_spd=was + 1)))
        refused("material %d: mirror_spd %d, was -1" % (plastic, was), lambda: r.update_materials(changed(mirror_spd=was)))  # not given stays not given
        refused("material %d: emission_spd" % plastic, lambda: r.update_materials(changed(emission_spd=was)))
        one = changed(glossy_spd=-1)
        refused("material %d: glossy_spd -1" % plastic, lambda: r.update_materials(one[plastic:plastic + 1], first=plastic))
        refused("material %d: refract_spd" % plastic, lambda: r.update_materials(changed(refract_spd=was)))
        refused("material %d: extinct_spd" % plastic, lambda: r.update_materials(changed(extinct_spd=was)))
        with pytest.raises(ValueError):
            r.update_spectra(np.zeros((2, S + 1)))
        with pytest.raises(ValueError):
            r.update_spectra(torch.zeros((2, S), dtype=torch.float64))  # not on the context's device
        assert_is_before(rendered(r, p), name, "after every refusal")
        # (a refused drt_update_materials has not let its shininess through either: the film above says so)


# ------------------------------------------------------------------------------------------------ the other passes
@pytest.mark.parametrize("name", ["glass_refract", "spheres_1500"])
def test_the_other_passes_see_the_new_scene(name):
    c = MU.load(name)
    p = c["params"]
    after = c["after"]
    with context(name) as r:
        r.render_features(n_samples=2)
        r.render_mattes(n_samples=2)
        r.read_features()
        r.read_mattes()
        apply(r, name)
        with pytest.raises(RuntimeError, match="no feature buffers"):  # a pass taken before the update describes the old scene
            r.read_features()
        with pytest.raises(RuntimeError):
            r.read_mattes()
        r.render_features(n_samples=3, first_sample=1)
        mean, m2, ids = r.read_features()
        wmean, wm2, wids, _, _ = F.features(after, p, n_samples=3, first_sample=1)
        assert cases.same_bits(mean, wmean) and cases.same_bits(m2, wm2) and np.array_equal(ids, wids)
        r.render_mattes(n_samples=3)
        for a, b in zip(r.read_mattes(), M.mattes(after, p, n_samples=3)):
            assert np.array_equal(a, b)
        r.render_mattes(n_samples=2)
        r.update_materials(after.materials())  # the same values: a successful update all the same
        with pytest.raises(RuntimeError):
            r.read_mattes()
        # ray queries: 4096 seeded rays against a fresh context's answers (geometry is what they read: not a bit may move)
        ro, rd, p0, p1 = U.seeded_rays({"after": after}, n=4096, seed=23)
        hits, vis = r.cast_rays(ro, rd), r.test_visibility(p0, p1)
        with context(name, "after") as f:
            fhits, fvis = f.cast_rays(ro, rd), f.test_visibility(p0, p1)
        for field in HIT_INTS:
            assert np.array_equal(hits[field], fhits[field]), field
        for field in HIT_FLOATS:
            assert cases.same_bits(hits[field], fhits[field]), field
        assert np.array_equal(vis, fvis) and (hits["index"] >= 0).any() and (hits["index"] < 0).any()
        want = Q.oracle_hits(after, ro, rd)
        assert np.array_equal(hits["index"], want["index"])
        film, log, _ = rendered(r, p)
        assert np.array_equal(log, fresh(name)[1])


def test_denoise_after_an_update():
    name = "glass_refract"
    c = MU.load(name)
    p = c["params"]
    with context(name, "after") as r:
        r.render()
        want_report = r.denoise(radius=2, patch=1, k=1.0)["unusable"]
        want = r.read_denoised()
    with context(name) as r:
        apply(r, name)
        r.render()
        assert r.denoise(radius=2, patch=1, k=1.0)["unusable"] == want_report
        got = r.read_denoised()
        assert cases.same_bits(got[0], want[0]) and cases.same_bits(got[1], want[1])


@pytest.mark.parametrize("name", ["glass_refract", "roughness"])
def test_render_adaptive_after_an_update(name):
    c = MU.load(name)
    q = MU._params(c["params"], hits=False)
    q.flags = 0
    args = (2, 5, 2, 0.05)
    with context(name, "after", params=q) as r:
        want_report = r.render_adaptive(*args)
        want = r.read_film(), r.read_sample_counts(), cases.stat_counts(r.stats())
    with context(name, params=q) as r:
        apply(r, name)
        report = r.render_adaptive(*args)
        assert report == want_report
        assert_same_film(r.read_film(), want[0], "adaptive after an update")
        assert np.array_equal(r.read_sample_counts(), want[1]) and cases.stat_counts(r.stats()) == want[2]
        assert len(np.unique(want[1])) > 1  # the rounds really told pixels apart


def test_an_update_under_a_bound_ray_table():
    name = "glass_refract"
    c = MU.load(name)
    p = c["params"]
    table = pydrt.equirect_rays(c["before"], int(p.width), int(p.height))
    with context(name, "after") as r:
        r.bind_rays(*table)
        want = rendered(r, p)
    with context(name) as r:
        r.bind_rays(*table)
        first = rendered(r, p)
        r.reset_film()
        apply(r, name)
        assert r.stats().path_flags & pydrt.PATH_RAYS
        got = rendered(r, p)
        assert_same_film(got[0], want[0], "the table over the new spectra")
        assert np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert not cases.same_bits(got[0][0], first[0][0])
        r.reset_film()
        r.bind_rays(None)
        assert_is_after(rendered(r, p), name, "unbound again", with_oracle=False)


@pytest.mark.parametrize("name", ["glass_refract", "shininess", "roughness"])
def test_selftest_material_after_an_update(name):
    """drt_selftest_material makes its override tables from the host's mirror of the materials: after an update (host mode, and for a
    spectra case device mode too) they are a fresh context's"""
    c = MU.load(name)
    b = c["after"]
    rng = np.random.default_rng(31)
    base = int(b.scene.base_material)
    ev, sm = [], []
    for m in [i for i in range(int(b.scene.num_materials)) if int(b.scene.materials[i].num_bdsfs) > 0]:
        for mats in ((m, base, m), (m, m, base)):
            for _ in range(8):
                nrm, out, rin = (v / np.sqrt((v * v).sum()) for v in rng.normal(size=(3, 3)))
                if (nrm * out).sum() < 0:
                    out = -out
                pt = np.concatenate([rng.uniform(-2, 2, 3), nrm, out, [(nrm * out).sum()]])
                for bdsf in [-1] + MU.bdsfs_of(b.scene.materials[m]):
                    ev.append(np.concatenate([pt, mats, [bdsf], rin, [0]]))
                sm.append(np.concatenate([pt, mats, [-1, np.uint64(rng.integers(1, 2 ** 63)).view(np.float64)]]))
    ev, sm = np.array(ev, dtype=np.float64), np.array(sm, dtype=np.float64)

    def both(r):
        return pydrt.selftest_material(r, pydrt.MAT_EVALUATE, ev), pydrt.selftest_material(r, pydrt.MAT_SAMPLE, sm)
    with context(name, "after") as r:
        want = both(r)
    modes = [False] + ([True] if name in MU.SPECTRA and pytest.importorskip("torch") else [])
    for device in modes:
        with context(name) as r:
            old = both(r)  # the tables are made here, from the scene before
            assert not (cases.same_bits(old[0], want[0]) and cases.same_bits(old[1], want[1]))
            apply(r, name, device=device)
            got = both(r)
            assert cases.same_bits(got[0], want[0]) and cases.same_bits(got[1], want[1]), (name, device)


def test_a_redone_launch_after_a_longer_paths_edit_costs_no_bit():
    """the pool is not measured again: with a pool as small as it gets, the launches that run out are rendered again"""
    name = "glass_refract"
    c = MU.load(name)
    p = c["params"]
    q = MU._params(p)
    q.spp, q.batch_spp = 12, 4  # three pairs of four samples, in a pool made for one sample per pixel
    with context(name, "after", params=q) as r:
        want = rendered(r, q)
        assert r.stats().redone_launches == 0
    with context(name, params=q, DRT_POOL_BLOCKS="1") as r:
        apply(r, name)
        got = rendered(r, q)
        assert r.stats().redone_launches >= 1
        assert_same_film(got[0], want[0], "a pool of one worst-case sample per pixel")
        assert np.array_equal(got[1], want[1]) and got[2] == want[2]


# ------------------------------------------------------------------------------------------------ groups
@pytest.mark.parametrize("name", ["glass_refract", "spheres_1500"])
def test_the_group_forms(name):
    torch = pytest.importorskip("torch")
    c = MU.load(name)
    q = MU._params(c["params"], hits=False)
    q.flags = 0  # (hit recording is per context)
    first, rows = changed_rows(name)
    mats = c["after"].materials()
    plastic = MU.material(c["after"], bdsfs=[MU.DIFFUSE, MU.GLOSSY])
    mats[plastic].shininess = 12.5
    with context(name, params=q) as r:
        r.update_spectra(rows, first=first)
        r.update_materials(mats)
        r.render()
        want = r.read_film(), cases.stat_counts(r.stats())
    with context(name, params=q) as r:
        r.render()
        before = r.read_film()
    with environment(DRT_FORCE_BVH="1" if c["forced"] else None):
        g = pydrt.Group(c["before"], q, devices=[0, 0, 0])
    try:
        g.render()
        assert_same_film(g.read_film(), before, "the group before")
        # every context refuses: all stay as they were
        rc = g.L.drt_group_update_spectra(g.g, rows.ctypes.data, first, len(rows), 0)
        assert rc != 0 and b"drt_group_update_spectra: the film holds samples" in g.L.drt_last_error()
        rc = g.L.drt_group_update_materials(g.g, C.cast(mats, C.c_void_p), 0, len(mats), 0)
        assert rc != 0 and b"drt_group_update_materials: the film holds samples" in g.L.drt_last_error()
        g.reset_film()
        with pytest.raises(ValueError):
            g.update_spectra(torch.zeros((1, c["after"].S), dtype=torch.float64))  # device mode is per context
        assert g.L.drt_group_update_spectra(g.g, rows.ctypes.data, first, len(rows), pydrt.SPECTRA_DEVICE) != 0 and b"host pointers only" in g.L.drt_last_error()
        with pytest.raises(RuntimeError, match="is the scene's cmf_rw"):
            g.update_spectra(c["after"].spds())
        wrong = c["after"].materials()
        wrong[plastic].dir_func = 1
        wrong[plastic].roughness = 0.5
        with pytest.raises(RuntimeError, match="material %d: dir_func" % plastic):
            g.update_materials(wrong)
        g.render()
        assert_same_film(g.read_film(), before, "the group after the refusals")
        g.reset_film()
        g.update_spectra(rows, first=first)
        g.update_materials(mats)
        g.render()
        assert_same_film(g.read_film(), want[0], "the group after the update")
        assert cases.stat_counts(g.stats()) == want[1]
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ the program
def test_drt_render_program_with_light_levels(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    W, H, SPP, DEPTH, LEVELS = 16, 16, 2, 3, (1.0, 0.25, 3.0)
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("num_pixel_samples 4", "num_pixel_samples %d" % SPP).replace("max_cast_depth    4", "max_cast_depth    %d" % DEPTH)
    cfg = cfg.replace("output_width      800", "output_width      %d" % W).replace("output_height     600", "output_height     %d" % H)
    assert "output_width      16" in cfg and "output_height     16" in cfg and "num_pixel_samples 2" in cfg and "max_cast_depth    3" in cfg

    def run(name, **env):
        d = tmp_path / name
        os.makedirs(d / "output")
        for sub in ("scenes", "spectra"):
            os.symlink(os.path.join(cases.REPO, sub), d / sub)
        (d / "config.cfg").write_text(cfg)
        full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
        full.update(env)
        r = subprocess.run([exe], cwd=d, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        return d / "output"

    levels = ",".join(repr(k) for k in LEVELS)
    out = run("levels", DRT_LIGHT_LEVELS=levels)
    plain = run("plain")
    names = ("output", "average", "variance")
    assert sorted(os.listdir(out)) == sorted("%s.%04d.%s" % (n, k, e) for n in names for k in range(len(LEVELS)) for e in ("spd", "bmp"))
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, H)
    p = pydrt.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=1)
    S = bundle.S
    r = pydrt.Renderer(bundle, p)
    try:
        for k, level in enumerate(LEVELS):
            r.reset_film()
            first, rows = MU.light_level_rows(bundle, level)
            r.update_spectra(rows, first=first)
            r.render()
            px, av, va = r.read_film()
            fpx = np.fromfile(out / ("output.%04d.spd" % k), dtype=np.float64, offset=40).reshape(-1, S + 1)
            fav = np.fromfile(out / ("average.%04d.spd" % k), dtype=np.float64, offset=40).reshape(-1, S)
            fva = np.fromfile(out / ("variance.%04d.spd" % k), dtype=np.float64, offset=40).reshape(-1, S)
            with np.errstate(invalid="ignore", divide="ignore"):
                norm = va / np.max(np.maximum(va, 0.0), axis=1)[:, None]  # written max-normalised per pixel (host/drt_checkpoint.c)
            assert_same_film((fpx, fav, fva), (px, av, norm), "level %g" % level)
            assert np.all(fpx[:, -1] == SPP) and np.any(fpx[:, :-1] != 0.0)
    finally:
        r.close()
    for n in names:  # level 1 is the plain run, byte for byte; level 0.25 is another picture
        for e in ("spd", "bmp"):
            assert open(out / ("%s.0000.%s" % (n, e)), "rb").read() == open(plain / ("%s.%s" % (n, e)), "rb").read(), (n, e)
    assert open(out / "output.0001.spd", "rb").read() != open(out / "output.0000.spd", "rb").read()
    two = run("two", DRT_LIGHT_LEVELS=levels, DRT_DEVICES="0,0")
    for f in sorted(os.listdir(out)):
        assert open(two / f, "rb").read() == open(out / f, "rb").read(), f
