"""GPU (-m gpu): lobe films (drt_bind_lobes).

The rule is in include/drt_hip.h and tests/lobe_rule.py. Every expected film comes from the existing oracle (tests/lobe_cases.py):
  1. a map with all 15 entries on one film makes that film the main film and the oracle's, bit for bit, in every launch shape; the
     films no entry names hold the samples' zeros;
  2. film 0 of {emission, direct[K] -> 0, the rest -> 1} at the case's own depth is the oracle's render at max_depth = 1 of the bundle
     with every list restricted to K, on all pixels;
  3. film 0 of {emission, direct[K], indirect[K] -> 0, the rest -> 1} at max_depth = 2 is the oracle's depth-2 render with only
     material M restricted to K, on the pixels whose samples all hit M first and never hit M second;
  4. the films of "functions" and of "standard" add up to the main film within gamma (lobe_rule.gamma);
  5. routing: unlisted functions' films stay zero, films the oracle tells apart differ, a NONE entry changes no other film;
  6. ray tables, material updates, groups, readouts, refusals, resources and the host program, as tests/test_gpu_buckets.py.
Comparisons are cases.same_bits on all three buffers except in 4. tests/test_lobes_cpu.py holds the premises on the oracle alone.

example_scene: its camera rays are NaN and so is every sample's vignette. By the rule value^c * vignette goes through the film update
of EVERY film, so the films no entry names hold 0.0 * NaN = NaN there, not +0; their filter column still counts the samples.
Cases are at most 32 x 32 pixels (one replay shape is 4 x 64)."""
import contextlib
import gc
import os
import re
import subprocess

import numpy as np
import pytest

import bucket_cases as BC
import cases
import lobe_cases as LC
import lobe_rule as LR
import oracle_py as O
import pydrt

pytestmark = pytest.mark.gpu

BASE = LC.BASE
NAN_CASE = "example_scene"


@contextlib.contextmanager
def environment(**knobs):
    saved = {k: os.environ.get(k) for k in knobs}
    try:
        for k, v in knobs.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def read_lobes(r, n):
    return [r.read_lobe_film(c) for c in range(n)]


def render_with_lobes(bundle, params, n, entries, calls=None, before_render=None, after=None):
    """(main film, [lobe films], stats, batch_spp) of a fresh context bound to n films and the map `entries` (a lobe_rule list or a
    preset's name); after(r): more to do before it closes"""
    r = pydrt.Renderer(bundle, params)
    try:
        if before_render:
            before_render(r)
        r.bind_lobes(entries if isinstance(entries, str) else LC.to_map(entries), n)
        for first, count in (calls or [(None, None)]):
            r.render(first, count)
        out = r.read_film(), read_lobes(r, n), r.stats(), r.batch_spp()
        if after:
            after(r)
        return out
    finally:
        r.close()


def assert_unnamed(film, spp, nan, what):
    """a film no entry names: every sample worth +0 (NaN in the all-NaN case: 0.0 * the NaN vignette), the filter column counts"""
    px, av, va = film
    assert np.array_equal(px[:, -1], np.full(px.shape[0], float(spp))), "%s: filter column" % what
    if nan:
        assert np.isnan(px[:, :-1]).all() and np.isnan(av).all() and np.isnan(va).all(), "%s: not all NaN" % what
    else:
        want = LR.empty_film(px.shape[0], av.shape[1], list(range(spp)))
        LC.assert_film((px, av, va), want, what)


# the two configurations every all-to-one case runs in: film 0 of 1 (drt_lobe_kernel<1, *>) and film 3 of 4 (<4, *>)
BOTH = pytest.mark.parametrize("n, film", [(1, 0), (4, 3)], ids=["film0of1", "film3of4"])


def check_all_to_one(name, what, n=4, film=3, calls=None, before_render=None, bundle_params=None, want=None, **changes):
    """all 15 entries on `film` of n: that film, the main film and the oracle are equal; the other films are unnamed"""
    bundle, params = bundle_params or LC.load(name)
    p = LC.params_with(params, **changes)
    main, films, st, batch = render_with_lobes(bundle, p, n, LR.all_to(film), calls=calls, before_render=before_render)
    if want is None:
        want = BC.film_device(name, **{k: v for k, v in changes.items() if k != "batch_spp"})[:3]
    LC.assert_film(main, want, "%s: %s, the main film against the oracle" % (what, name))
    LC.assert_film(films[film], want, "%s: %s, film %d of %d against the oracle" % (what, name, film, n))
    LC.assert_film(films[film], main, "%s: %s, film %d of %d against the main film" % (what, name, film, n))
    total = sum(count if count is not None else int(p.spp) for _, count in (calls or [(None, None)]))
    for c in range(n):
        if c != film:
            assert_unnamed(films[c], total, name == NAN_CASE, "%s: %s, film %d of %d, which no entry names" % (what, name, c, n))
    return main, films, st, batch


# ------------------------------------------------------------------------------------------------ 1. all to one
@pytest.mark.parametrize("name", LC.ALL_CASES)
def test_all_entries_on_one_film_give_the_main_film(name):
    bundle, _ = LC.load(name)
    main, films, st, _ = check_all_to_one(name, "n = 1", n=1, film=0)
    check_all_to_one(name, "film 3 of 4")
    if name == "grid_2p5nm":
        assert bundle.S == 137  # three wavelength sets
    if name == "spheres_1500":
        assert st.path_flags & pydrt.PATH_BVH, "spheres_1500 is meant to go through the hierarchy pipeline"
    if name == NAN_CASE:
        assert np.isnan(films[0][0][:, :-1]).all() and np.isnan(films[0][1]).all()
    else:
        assert (main[2] != 0).any()
        assert cases.stat_counts(st) == cases.stat_counts(BC.film_device(name)[4])


@BOTH
def test_a_launch_that_starts_at_sample_five(n, film):
    _, _, st, _ = check_all_to_one(BASE, "samples 5..10", n=n, film=film, **BC.changes_for(6, 5))
    assert st.launches == 1


@BOTH
@pytest.mark.parametrize("batch", [1, 3])
def test_several_calls_and_small_batches_continue_every_film(batch, n, film):
    """render(0, 3); render(3, 5); render(8, 1) in pairs of 1 and of 3 samples"""
    _, _, st, got = check_all_to_one(BASE, "three calls, batch_spp %d" % batch, calls=[(0, 3), (3, 5), (8, 1)], n=n, film=film,
                                       **BC.changes_for(9, batch_spp=batch))
    assert got == batch and st.launches == {1: 9, 3: 4}[batch]


@BOTH
@pytest.mark.parametrize("spp", [65, 130])
def test_header_windows_of_65_and_130_samples_in_one_pair(spp, n, film):
    _, _, st, batch = check_all_to_one(BASE, "%d samples in one pair" % spp, n=n, film=film, **BC.changes_for(spp))
    assert batch >= spp and st.launches == 1, "one kernel pair is meant to take all %d samples (batch_spp %d, %d pairs)" % (spp, batch, st.launches)


def shape_case(name, n, film):
    import replay_shape_cases as RS
    _, spp = BC.REPLAY_SHAPES[name]
    bundle, params = RS.load(name)
    want = RS.oracle_film(name, bundle, params, spp=spp)
    _, _, st, _ = check_all_to_one(name, "replay shape", bundle_params=(bundle, params), want=want, n=n, film=film, spp=spp)
    return bundle, RS.params_with(params, spp=spp), st


@BOTH
def test_a_4_x_64_tile_in_row_blocks(n, film):
    """four row blocks of 16 rows, each in pairs of 4 samples: the lobe films start at the block's first pixel"""
    import replay_shape_cases as RS
    with environment(DRT_NO_ROW_BLOCKS=None, DRT_POOL_BLOCKS=None):
        _, p, st = shape_case("blocks_4x64", n, film)
    plan = RS.BLOCK_PLANS["blocks_4x64"]
    assert (int(p.tile_w), int(p.tile_h)) == (4, 64) and st.launches == plan["blocks"] * len(plan["pairs"]) and st.redone_launches == 0


@BOTH
def test_a_table_outside_lds_and_four_wavelength_sets(n, film):
    """S = 256: drt_lobe_kernel<1, false> and <4, false>, four items per pixel"""
    import replay_shape_cases as RS
    bundle, _, _ = shape_case("lds_s256", n, film)
    assert bundle.S == 256 and RS.table_bytes(bundle) > RS.LDS_BYTES


@BOTH
def test_a_record_pool_that_runs_out_is_rendered_again_lobe_films_included(monkeypatch, n, film):
    """DRT_POOL_BLOCKS=1: the launches that ran out leave the lobe films untouched, as the main film, and are rendered again"""
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    _, _, st, _ = check_all_to_one(BASE, "tiny record pool", n=n, film=film, **BC.changes_for(8))
    assert st.redone_launches > 0, "no launch ran out of record blocks"


@BOTH
def test_behind_a_forced_hierarchy(n, film):
    with environment(DRT_FORCE_BVH="1"):
        _, _, st, _ = check_all_to_one(BASE, "DRT_FORCE_BVH", n=n, film=film, **BC.changes_for(8))
    assert st.path_flags & pydrt.PATH_BVH


# ------------------------------------------------------------------------------------------------ 2. direct layers
@pytest.mark.parametrize("name, cls", LC.direct_pairs(), ids=["%s-%s" % t for t in LC.direct_pairs()])
def test_a_class_direct_layer_is_the_oracles_depth_one_render_of_the_restricted_lists(name, cls):
    bundle, params = LC.load(name)
    K = LR.CLASSES[cls]
    main, films, _, _ = render_with_lobes(bundle, params, 2, LR.class_direct_map(K))
    want = LC.oracle_film(name, True, K, max_depth=1)[:3]
    LC.assert_film(films[0], want, "%s, class %s: film 0 at depth %d against the restricted oracle at depth 1" % (name, cls, int(params.max_depth)))
    LC.assert_film(main, BC.film_device(name)[:3], "%s: the main film" % name)
    assert not cases.same_bits(films[0][0], main[0]), "film 0 is the whole film"


# ------------------------------------------------------------------------------------------------ 3. direct plus indirect
@pytest.mark.parametrize("name, material, cls", LC.indirect_triples(), ids=["%s-m%d-%s" % t for t in LC.indirect_triples()])
def test_a_class_layer_at_depth_two_is_the_oracles_render_with_one_material_restricted(name, material, cls):
    bundle, params = LC.load(name)
    K = LR.CLASSES[cls]
    p = LC.params_with(params, max_depth=2)
    _, films, _, _ = render_with_lobes(bundle, p, 2, LR.class_map(K))
    want = LC.oracle_film(name, True, K, only_material=material, max_depth=2)[:3]
    pixels = LC.qualifying_pixels(name, material, device=True)
    assert len(pixels) == LC.INDIRECT_PIXELS[name][material] >= 3
    LC.assert_film([a[pixels] for a in films[0]], [a[pixels] for a in want],
                   "%s, material %d, class %s: film 0 on the %d pixels that hit it first" % (name, material, cls, len(pixels)))


# ------------------------------------------------------------------------------------------------ 4. the sum identity, 5. routing
@pytest.mark.parametrize("name", LC.ALL_CASES)
def test_the_presets_films_add_up_to_the_main_film_and_unlisted_functions_stay_zero(name):
    bundle, params = LC.load(name)
    spp = int(params.spp)
    listed = {f for lst in LC.material_lists(bundle) for f in lst}
    for preset in ("functions", "standard"):
        want, names = LR.PRESETS[preset]
        n = len(names)
        main, films, _, _ = render_with_lobes(bundle, params, n, preset)
        LC.assert_film(main, BC.film_device(name)[:3], "%s, %s: the main film" % (name, preset))
        g = LC.gamma_for(name, n)
        bad, worst = LR.sum_identity_violations([f[0] for f in films], main[0], g)
        print("%s, %s: worst |sum - main| / magnitude = %.3g, gamma = %.3g" % (name, preset, worst, g))
        assert bad == 0, "%s, %s: %d elements beyond gamma = %.3g (worst %.3g)" % (name, preset, bad, g, worst)
        for c in range(n):
            assert np.array_equal(films[c][0][:, -1], np.full(films[c][0].shape[0], float(spp))), "every film takes every sample"
        if preset == "functions":
            for f in range(LR.NUM):
                if f not in listed:
                    assert_unnamed(films[1 + f], spp, name == NAN_CASE, "%s: the film of %s, which no material lists" % (name, LR.FUNCTIONS[f]))
            if name != NAN_CASE:
                assert sum(1 for f in films if f[0][:, :-1].any()) >= 2, "%s: one film holds everything" % name


@pytest.mark.parametrize("name", LC.DIRECT_CASES)
def test_films_the_oracle_tells_apart_differ_on_the_device(name):
    """tests/test_lobes_cpu.py shows on the oracle that the diffuse and the glossy layers differ from one another, from the emission
    alone and from the whole film in each of these cases: so do the films of bp_diffuse, bp_glossy and emission here"""
    bundle, params = LC.load(name)
    main, films, _, _ = render_with_lobes(bundle, params, 8, "functions")
    e, d, g = films[0], films[1 + LR.F["bp_diffuse_bdsf"]], films[1 + LR.F["bp_glossy_bdsf"]]
    for a, b, what in ((d, g, "diffuse and glossy"), (d, e, "diffuse and emission"), (g, e, "glossy and emission"), (d, main, "diffuse and the main film"),
                       (g, main, "glossy and the main film")):
        for k in range(2):
            assert not cases.same_bits(a[k], b[k]), "%s: %s hold the same %s" % (name, what, ("sums", "means")[k])


def test_an_entry_on_no_film_changes_no_other_film():
    """"functions" with ct_conductor's two entries on DRT_LOBE_NONE and seven films, against "functions" itself, where they go to an
    eighth film: films 0 to 6 are the same bits"""
    bundle, params = LC.load(BASE)
    full, _ = LR.PRESETS["functions"]
    ct = LR.F["ct_conductor_bdsf"]
    assert full[1 + ct] == full[1 + LR.NUM + ct] == 7 and [ct] in LC.material_lists(bundle)
    none = list(full)
    none[1 + ct] = none[1 + LR.NUM + ct] = LR.NONE
    _, eight, _, _ = render_with_lobes(bundle, params, 8, full)
    _, seven, _, _ = render_with_lobes(bundle, params, 7, none)
    LC.assert_films(seven, eight[:7], "ct_conductor on no film against on film 7")
    assert eight[7][0][:, :-1].any(), "film 7 holds something that went nowhere"
    # and emission on no film
    none = list(full)
    none[0] = LR.NONE
    _, films, _, _ = render_with_lobes(bundle, params, 8, none)
    LC.assert_films(films[1:], eight[1:], "emission on no film")
    assert_unnamed(films[0], int(params.spp), False, "film 0 without the emission")
    assert eight[0][0][:, :-1].any()


# ------------------------------------------------------------------------------------------------ 6. the rest
@BOTH
def test_a_ray_table_of_the_cameras_centre_rays(n, film):
    import ray_film_cases as R
    bundle, params = LC.load(BASE)
    table = R.centre_rays(bundle, int(params.width), int(params.height))
    _, _, st, _ = check_all_to_one(BASE, "ray table", before_render=lambda r: r.bind_rays(*table), n=n, film=film,
                                   **BC.changes_for(8, pixel_scheme=pydrt.FILM_SAMPLE_CENTER))
    assert st.path_flags & pydrt.PATH_RAYS


def test_after_update_materials_and_reset_film_the_lobe_films_are_a_fresh_contexts():
    bundle, params = LC.load(BASE)
    p = LC.params_with(params, spp=8)
    text = open(cases.scene_path(cases.RENDER_CASES[BASE][0])).read()
    assert "shininess 100.0" in text
    after = pydrt.load_scene_text(text.replace("shininess 100.0", "shininess 30.0"), int(params.width), int(params.height))
    fresh_main, fresh_films, _, _ = render_with_lobes(after, p, 7, "standard")
    r = pydrt.Renderer(bundle, p)
    try:
        r.bind_lobes("standard")
        r.render()
        before = read_lobes(r, 7)
        r.reset_film()
        r.update_materials(after.materials())
        assert not any(a.any() for f in read_lobes(r, 7) for a in f), "drt_reset_film zeroes the lobe films"
        r.render()
        main, films = r.read_film(), read_lobes(r, 7)
    finally:
        r.close()
    LC.assert_film(main, fresh_main, "updated context against a fresh one, main film")
    LC.assert_films(films, fresh_films, "updated context against a fresh one")
    assert not cases.same_bits(before[3][0], films[3][0]), "the update changes the glossy direct film"
    assert cases.same_bits(before[1][0], films[1][0]), "and leaves the diffuse direct film alone"


def test_a_groups_assembled_lobe_films_are_a_single_contexts():
    bundle, params = LC.load(BASE)
    p = LC.params_with(params, spp=8)
    _, want, _, _ = render_with_lobes(bundle, p, 7, "standard")
    g = pydrt.Group(bundle, p, devices=[0, 0, 0])
    try:
        with pytest.raises(RuntimeError, match="no lobes are bound"):
            g.read_lobe_film(0)
        with pytest.raises(RuntimeError, match="9 films, at most 8"):
            g.bind_lobes(pydrt.lobe_map(default=0), 9)
        with pytest.raises(RuntimeError, match="emission to film 2 of 2"):
            g.bind_lobes(pydrt.lobe_map(emission=2, default=0), 2)
        g.bind_lobes("standard")
        g.render()
        main, films = g.read_film(), [g.read_lobe_film(c) for c in range(7)]
        with pytest.raises(RuntimeError, match="film 7 of 7"):
            g.read_lobe_film(7)
        with pytest.raises(RuntimeError, match="drt_reset_film first"):
            g.bind_lobes("functions")
        with pytest.raises(RuntimeError, match="lobes are bound"):
            g.bind_depth_cuts([1])
        with pytest.raises(RuntimeError, match="lobes are bound"):
            g.bind_sensor(np.ones((1, bundle.S)))
        with pytest.raises(RuntimeError, match="lobes are bound"):
            g.bind_buckets(2)
        LC.assert_films([g.read_lobe_film(c) for c in range(7)], films, "after the group's refusals")
        g.reset_film()
        g.bind_lobes(None)
        with pytest.raises(RuntimeError, match="no lobes are bound"):
            g.read_lobe_film(0)
    finally:
        g.close()
    LC.assert_film(main, BC.film_device(BASE, **BC.changes_for(8))[:3], "a group of three contexts, the main film")
    LC.assert_films(films, want, "a group of three contexts")


def test_binding_lobes_changes_nothing_else():
    """the main film, the statistics' counts and the hit log: the same bits with lobes bound and without"""
    bundle, params = LC.load(BASE)
    p = LC.params_with(params, spp=8, flags=pydrt.FLAG_RECORD_HITS)
    out = []
    for preset in (None, "standard"):
        r = pydrt.Renderer(bundle, p)
        try:
            r.bind_lobes(preset)
            r.render()
            out.append((r.read_film(), r.read_hit_indices(8), r.stats(), r.read_xyz()))
        finally:
            r.close()
    (film0, hits0, st0, xyz0), (film1, hits1, st1, xyz1) = out
    LC.assert_film(film1, film0, "the main film with lobes bound against without")
    assert np.array_equal(hits0, hits1) and cases.same_bits(xyz0, xyz1)
    assert np.array_equal(hits0, BC.film_device(BASE, **BC.changes_for(8))[3])
    assert cases.stat_counts(st0) == cases.stat_counts(st1) and st0.launches == st1.launches


def host_bgra(bundle, width, height, mean, tmp_path):
    """the pixel bytes host/drt_bmp.c gives a spectral film without a filter column (as tests/test_gpu_buckets.py)"""
    import ctypes as C
    H = pydrt.host_lib()
    f64p = C.POINTER(C.c_double)
    H.drt_host_spd_file_to_bmp.argtypes = [C.c_char_p, C.c_char_p, f64p]
    H.drt_host_write_spd.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, f64p]
    sc = bundle.scene
    spd, bmp = str(tmp_path / "mean.spd"), str(tmp_path / "mean.bmp")
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    assert H.drt_host_write_spd(spd.encode(), width, height, bundle.S, 0, float(sc.min_wavelength), float(sc.wavelength_interval),
                                mean.ctypes.data_as(f64p)) == 0
    rows = [int(sc.cmf_rw), int(sc.cmf_x), int(sc.cmf_y), int(sc.cmf_z)]
    cmf = np.ascontiguousarray(bundle.spds()[rows])
    assert H.drt_host_spd_file_to_bmp(spd.encode(), bmp.encode(), cmf.ctypes.data_as(f64p)) == 0
    return np.frombuffer(open(bmp, "rb").read()[54:], dtype=np.uint8).reshape(-1, 4)


def test_the_xyz_and_bgra_readouts_are_the_existing_conversions_of_a_lobe_film(tmp_path):
    bundle, params = LC.load(BASE)
    p = LC.params_with(params, spp=8)
    r = pydrt.Renderer(bundle, p)
    try:
        r.bind_lobes("standard")
        r.render()
        films = read_lobes(r, 7)
        xyz = [r.read_lobe_xyz(c) for c in (1, 4)]
        bgra = [r.read_lobe_bgra(c) for c in (1, 4)]
        main_bgra = r.read_bgra(1)
        ptrs = [r.lobe_film_device_ptrs(c) for c in range(7)]
        assert len({q for f in ptrs for q in f} | set(r.film_device_ptrs())) == 3 * 7 + 3 and all(q for f in ptrs for q in f)
        with pytest.raises(RuntimeError, match="which = 3"):
            r.read_lobe_bgra(1, 3)
    finally:
        r.close()
    for k, c in enumerate((1, 4)):
        want = O.oracle_film_to_xyz(bundle, films[c][0])
        assert cases.same_bits(xyz[k], want), "XYZ of film %d: %s" % (c, cases.first_difference(xyz[k], want))
        want = host_bgra(bundle, int(p.tile_w), int(p.tile_h), films[c][1], tmp_path)
        assert np.array_equal(bgra[k], want), "BGRA of film %d" % c
    assert len(np.unique(bgra[0][:, :3])) > 20 and not np.array_equal(bgra[0], bgra[1]) and not np.array_equal(bgra[0], main_bgra)


def test_every_refusal_says_why_and_leaves_the_context_as_it_was():
    bundle, params = LC.load(BASE)
    p = LC.params_with(params, spp=8)
    _, want, _, _ = render_with_lobes(bundle, p, 7, "standard")
    gc.collect()
    r = pydrt.Renderer(bundle, p)

    def state():
        n = getattr(r, "n_lobes", 0)
        return r.read_film(), read_lobes(r, n) if n else None, cases.stat_counts(r.stats()), pydrt.selftest_live_resources()

    def refused(call, why):
        before = state()
        with pytest.raises(RuntimeError, match=why):
            call()
        after = state()
        LC.assert_film(after[0], before[0], "main film across the refusal '%s'" % why)
        if before[1] is not None:
            LC.assert_films(after[1], before[1], "across the refusal '%s'" % why)
        assert after[2:] == before[2:], why

    zero = pydrt.lobe_map(default=0)
    try:
        for read in (lambda: r.read_lobe_film(0), lambda: r.lobe_film_device_ptrs(0), lambda: r.read_lobe_xyz(0), lambda: r.read_lobe_bgra(0)):
            refused(read, "no lobes are bound")
        refused(lambda: r.bind_lobes(zero, 9), "9 films, at most 8")
        refused(lambda: pydrt._check(r.L.drt_bind_lobes(r.ctx, 2, None), "drt_bind_lobes"), "null map")
        refused(lambda: r.bind_lobes(pydrt.lobe_map(emission=1, default=0), 1), "emission to film 1 of 1")
        refused(lambda: r.bind_lobes(pydrt.lobe_map(direct={"mirror": 5}, default=0), 5), "direct light of function 2 to film 5 of 5")
        refused(lambda: r.bind_lobes(pydrt.lobe_map(indirect={"ct_conductor": 7}, default=0), 3), "indirect light of function 6 to film 7 of 3")
        r.bind_depth_cuts((1, 2))
        refused(lambda: r.bind_lobes("standard"), "depth cuts are bound")
        r.bind_depth_cuts(None)
        r.bind_sensor(np.ones((2, bundle.S)))
        refused(lambda: r.bind_lobes("standard"), "a sensor is bound")
        r.bind_sensor(None)
        r.bind_buckets(2)
        refused(lambda: r.bind_lobes("standard"), "buckets are bound")
        r.bind_buckets(0)
        r.bind_lobes("standard")
        refused(lambda: r.bind_depth_cuts((1, 2)), "lobes are bound")
        refused(lambda: r.bind_sensor(np.ones((2, bundle.S))), "lobes are bound")
        refused(lambda: r.bind_buckets(2), "lobes are bound")
        refused(lambda: r.render_adaptive(2, 4, 1, 0.1), "lobes bound")
        refused(lambda: r.render_adaptive_continue(4, 1, 0.1), "lobes bound")
        refused(lambda: r.render_sample_map(np.full(r.n_pixels, 2, dtype=np.uint32)), "lobes bound")
        refused(lambda: r.read_lobe_film(7), "film 7 of 7")
        r.render(0, 2)
        r.render(2, 6)
        refused(lambda: r.bind_lobes("functions"), "already holds samples")
        refused(lambda: pydrt._check(r.L.drt_read_lobe_xyz(r.ctx, 0, None), "drt_read_lobe_xyz"), "null argument")
        LC.assert_films(read_lobes(r, 7), want, "after the refusals")
        r.bind_lobes(None)  # (the unbind passes on a film that holds samples; a bind after it does not)
        refused(lambda: r.bind_lobes("standard"), "already holds samples")
        LC.assert_film(r.read_film(), BC.film_device(BASE, **BC.changes_for(8))[:3], "after the refusals, the main film")
        # unbound after a reset: adaptive sampling works again, and a film that holds an adaptive render takes no lobes
        r.reset_film()
        r.render_adaptive(2, 4, 1, 0.1)
        refused(lambda: r.bind_lobes("standard"), "drt_reset_film first")
        r.reset_film()
        r.bind_lobes("standard")
        r.render()
        LC.assert_films(read_lobes(r, 7), want, "bound again after an adaptive render and a reset")
    finally:
        r.close()
    x = pydrt.Renderer(bundle, LC.params_with(params, mode=pydrt.MODE_XYZ))
    try:
        with pytest.raises(RuntimeError, match="DRT_MODE_XYZ"):
            x.bind_lobes("standard")
        x.render()
        assert np.isfinite(x.read_xyz()).all()
    finally:
        x.close()


def test_live_resources_after_bind_rebind_unbind_and_close():
    bundle, params = LC.load(BASE)
    p = LC.params_with(params, spp=8)
    gc.collect()
    base = pydrt.selftest_live_resources()
    now = lambda: tuple(a - b for a, b in zip(pydrt.selftest_live_resources(), base))
    r = pydrt.Renderer(bundle, p)
    try:
        r.render()
        r.read_film()
        r.read_xyz()
        r.read_bgra(1)
        r.reset_film()
        unbound = now()
        r.bind_lobes(pydrt.lobe_map(default=0), 3)
        assert now()[0] == unbound[0] + 9 and now()[1:] == unbound[1:], "three buffers per film"
        r.render()
        r.read_lobe_xyz(0)
        r.read_lobe_bgra(2)
        assert now()[0] == unbound[0] + 9, "the readouts use the main film's buffers"
        r.reset_film()
        r.bind_lobes("functions")
        assert now()[0] == unbound[0] + 24, "the earlier films are released by the next bind"
        r.render()
        assert r.read_lobe_film(7)[1].shape == (r.n_pixels, bundle.S)
        r.reset_film()
        r.bind_lobes(None)
        assert now() == unbound
        r.bind_lobes("standard")
        r.render()
        assert now()[0] == unbound[0] + 21
    finally:
        r.close()
    gc.collect()
    assert now() == (0, 0, 0, 0), "%s still held (device, pinned, events, streams)" % (now(),)


# ------------------------------------------------------------------------------------------------ the host program
def test_drt_render_program_with_the_standard_lobes(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    W, H, SPP = 24, 16, 4
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("output_width      800", "output_width      %d" % W).replace("output_height     600", "output_height     %d" % H)
    cfg, k = re.subn(r"(?m)^num_pixel_samples\s+\S+", "num_pixel_samples %d" % SPP, cfg)
    assert k == 1
    depth = int(re.search(r"(?m)^max_cast_depth\s+(\d+)", cfg).group(1))

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
        return d, r.stdout

    plain, _ = run("plain")
    d, text = run("lobes", DRT_LOBES="standard", DRT_DEVICES="0,0")
    assert "Lobe films: 7 films" in text
    for f in ("output.spd", "average.spd", "variance.spd", "output.bmp", "average.bmp", "variance.bmp"):
        assert open(plain / "output" / f, "rb").read() == open(d / "output" / f, "rb").read(), f
    extra = ["%s.spd.lobe%d.spd" % (f, c) for f in ("output", "average", "variance") for c in range(7)]
    extra += ["output.spd.lobe%d.bmp" % c for c in range(7)] + ["output.spd.lobes.txt"]
    assert sorted(os.listdir(d / "output")) == sorted(os.listdir(plain / "output") + extra)  # and no temporary file is left
    names = LR.PRESETS["standard"][1]
    assert open(d / "output" / "output.spd.lobes.txt").read() == "".join("%d %s\n" % (c, n) for c, n in enumerate(names))
    # the same render through pydrt
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, H)
    r = pydrt.Renderer(bundle, pydrt.make_params(W, H, spp=SPP, max_depth=depth, seed=1))
    try:
        r.bind_lobes("standard")
        r.render()
        films = read_lobes(r, 7)
        pictures = [r.read_lobe_bgra(c) for c in range(7)]
    finally:
        r.close()

    def tail(f, shape):
        raw = open(d / "output" / f, "rb").read()
        size = int(np.prod(shape)) * 8
        assert len(raw) > size, f
        return np.frombuffer(raw[-size:], dtype=np.float64).reshape(shape)

    for c, (px, av, _) in enumerate(films):
        assert cases.same_bits(tail("output.spd.lobe%d.spd" % c, px.shape), px), "film %d, sums" % c
        assert cases.same_bits(tail("average.spd.lobe%d.spd" % c, av.shape), av), "film %d, means" % c
        assert np.array_equal(px[:, -1], np.full(px.shape[0], float(SPP)))
        bmp = np.frombuffer(open(d / "output" / ("output.spd.lobe%d.bmp" % c), "rb").read()[-W * H * 4:], dtype=np.uint8).reshape(H, W, 4)
        want = pictures[c].reshape(H, W, 4)
        assert np.array_equal(bmp, want) or np.array_equal(bmp, want[::-1]), "film %d: the picture is not drt_read_lobe_bgra's" % c
    assert not cases.same_bits(films[1][1], films[2][1]) and len(np.unique(pictures[1][:, :3])) > 10
