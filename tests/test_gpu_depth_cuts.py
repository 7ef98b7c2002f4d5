"""GPU (-m gpu): depth-cut films (drt_bind_depth_cuts).

The rule: cut d of one render equals, bit for bit, the oracle's render of the same case with max_depth = d
(depth_cut_cases.oracle_at: cases.oracle_render_device_pow on a copy of the params). Every test compares all three buffers of every
cut film with cases.same_bits, and the main film against the oracle at full depth. tests/test_depth_cuts_cpu.py shows, on the oracle
alone, that the shorter render walks the first vertices of the full one and that neighbouring cuts of every case differ, so a kernel
that ignores the depth cannot pass here. Sizes, samples and depths are those of tests/cases.py."""
import gc

import numpy as np
import pytest

import cases
import depth_cut_cases as DC
import pydrt

pytestmark = pytest.mark.gpu

BASE = "plane_light_16"
BASE_CUTS = DC.CUTS[BASE]


def cut_films(r, n):
    return [r.read_depth_film(c) for c in range(n)]


def render_with_cuts(bundle, params, depths, calls=None):
    """(main film, [cut films], stats) of a fresh context bound to `depths`"""
    r = pydrt.Renderer(bundle, params)
    try:
        r.bind_depth_cuts(depths)
        for first, n in (calls or [(None, None)]):
            r.render(first, n)
        return r.read_film(), cut_films(r, len(depths)), r.stats()
    finally:
        r.close()


def assert_cuts_are_the_oracles(name, depths, main, cuts, what, **changes):
    D = int(DC.load(name)[1].max_depth)
    DC.assert_film(main, DC.oracle_at(name, D, **changes)[:3], "%s: %s, the main film against the oracle" % (what, name))
    for c, d in enumerate(depths):
        DC.assert_film(cuts[c], DC.oracle_at(name, d, **changes)[:3], "%s: %s, cut %d (depth %d) against the oracle at that depth" % (what, name, c, d))


@pytest.mark.parametrize("name", sorted(DC.ALL_CUTS))
def test_every_cut_film_is_the_oracles_render_at_that_depth(name):
    bundle, params = DC.load(name)
    depths = DC.ALL_CUTS[name]
    main, cuts, st = render_with_cuts(bundle, params, depths)
    if name == "spheres_1500":
        assert st.path_flags & pydrt.PATH_BVH, "spheres_1500 is meant to go through the hierarchy pipeline"
    if name == "example_scene":
        assert np.isnan(cuts[0][0][:, :-1]).all() and np.isnan(cuts[-1][1]).all()
    assert_cuts_are_the_oracles(name, depths, main, cuts, "one render")
    assert cases.stat_counts(st) == cases.stat_counts(DC.oracle_at(name, int(params.max_depth))[4])


def test_the_cut_at_max_depth_is_the_main_film_from_the_device_alone():
    bundle, params = DC.load(BASE)
    assert BASE_CUTS[-1] == int(params.max_depth)
    main, cuts, _ = render_with_cuts(bundle, params, BASE_CUTS)
    DC.assert_film(cuts[-1], main, "the cut at max_depth against the main film")
    assert not cases.same_bits(cuts[0][0], main[0])


def test_binding_cuts_changes_nothing_else():
    """the main film, the statistics' counts and the hit log: the same bits with cuts bound and without"""
    bundle, params = DC.load(BASE)
    p = DC.params_at(params, int(params.max_depth), flags=pydrt.FLAG_RECORD_HITS)
    out = []
    for depths in (None, BASE_CUTS):
        r = pydrt.Renderer(bundle, p)
        try:
            if depths:
                r.bind_depth_cuts(depths)
            r.render()
            out.append((r.read_film(), r.read_hit_indices(int(p.spp)), r.stats(), r.read_xyz()))
        finally:
            r.close()
    (film0, hits0, st0, xyz0), (film1, hits1, st1, xyz1) = out
    DC.assert_film(film1, film0, "the main film with cuts bound against without")
    assert np.array_equal(hits0, hits1) and cases.same_bits(xyz0, xyz1)
    assert cases.stat_counts(st0) == cases.stat_counts(st1) and st0.launches == st1.launches


def test_one_call_several_calls_and_a_small_batch_give_the_same_cut_films():
    bundle, params = DC.load(BASE)
    spp = int(params.spp)
    assert spp == 4
    ways = {
        "one call": (params, None),
        "three calls": (params, [(0, 1), (1, 2), (3, 1)]),
        "batch_spp 1": (DC.params_at(params, int(params.max_depth), batch_spp=1), None),
        "batch_spp 3": (DC.params_at(params, int(params.max_depth), batch_spp=3), None),
    }
    for what, (p, calls) in ways.items():
        main, cuts, st = render_with_cuts(bundle, p, BASE_CUTS, calls=calls)
        if what == "batch_spp 1":
            assert st.launches == spp
        assert_cuts_are_the_oracles(BASE, BASE_CUTS, main, cuts, what)


def test_a_record_pool_that_runs_out_is_rendered_again_cut_films_included(monkeypatch):
    """DRT_POOL_BLOCKS=1: the launches that ran out leave the cut films untouched, as the main film, and are rendered again"""
    bundle, params = DC.load(BASE)
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    main, cuts, st = render_with_cuts(bundle, params, BASE_CUTS)
    assert st.redone_launches > 0, "no launch ran out of record blocks"
    assert_cuts_are_the_oracles(BASE, BASE_CUTS, main, cuts, "tiny record pool")


def test_a_ray_table_of_the_cameras_centre_rays_gives_the_cameras_cut_films():
    import ray_film_cases as R
    bundle, params = DC.load(BASE)
    w, h = int(params.width), int(params.height)
    assert float(bundle.camera.aperture_radius) == 0.0
    p = DC.params_at(params, int(params.max_depth), pixel_scheme=pydrt.FILM_SAMPLE_CENTER)
    table = R.centre_rays(bundle, w, h)
    r = pydrt.Renderer(bundle, p)
    try:
        r.bind_rays(*table)
        r.bind_depth_cuts(BASE_CUTS)
        r.render()
        assert r.stats().path_flags & pydrt.PATH_RAYS
        main, cuts = r.read_film(), cut_films(r, len(BASE_CUTS))
    finally:
        r.close()
    assert_cuts_are_the_oracles(BASE, BASE_CUTS, main, cuts, "ray table", pixel_scheme=pydrt.FILM_SAMPLE_CENTER)


def test_after_update_materials_and_reset_film_the_cut_films_are_a_fresh_contexts():
    bundle, params = DC.load(BASE)
    text = open(cases.scene_path(cases.RENDER_CASES[BASE][0])).read()
    assert "shininess 100.0" in text
    after = pydrt.load_scene_text(text.replace("shininess 100.0", "shininess 30.0"), int(params.width), int(params.height))
    fresh_main, fresh_cuts, _ = render_with_cuts(after, params, BASE_CUTS)
    r = pydrt.Renderer(bundle, params)
    try:
        r.bind_depth_cuts(BASE_CUTS)
        r.render()
        before_cuts = cut_films(r, len(BASE_CUTS))
        r.reset_film()
        r.update_materials(after.materials())
        assert not any(a.any() for film in cut_films(r, len(BASE_CUTS)) for a in film), "drt_reset_film zeroes the cut films"
        r.render()
        main, cuts = r.read_film(), cut_films(r, len(BASE_CUTS))
    finally:
        r.close()
    DC.assert_film(main, fresh_main, "updated context against a fresh one, main film")
    for c in range(len(BASE_CUTS)):
        DC.assert_film(cuts[c], fresh_cuts[c], "updated context against a fresh one, cut %d" % c)
    assert not cases.same_bits(before_cuts[-1][0], cuts[-1][0]), "the update changes the film"
    DC.assert_film(before_cuts[0], DC.oracle_at(BASE, BASE_CUTS[0])[:3], "before the update, cut 0")


def test_a_groups_assembled_cut_films_are_a_single_contexts():
    bundle, params = DC.load(BASE)
    g = pydrt.Group(bundle, params, devices=[0, 0, 0])
    try:
        g.bind_depth_cuts(BASE_CUTS)
        g.render()
        main, cuts = g.read_film(), [g.read_depth_film(c) for c in range(len(BASE_CUTS))]
        with pytest.raises(RuntimeError, match="cut 5 of 5"):
            g.read_depth_film(len(BASE_CUTS))
        with pytest.raises(RuntimeError, match="drt_reset_film first"):
            g.bind_depth_cuts([1])
        g.reset_film()
        g.bind_depth_cuts(None)
        with pytest.raises(RuntimeError, match="no depth cuts are bound"):
            g.read_depth_film(0)
    finally:
        g.close()
    assert_cuts_are_the_oracles(BASE, BASE_CUTS, main, cuts, "a group of three contexts")


def test_read_outs_of_a_cut_film_are_the_main_read_outs_of_a_render_at_that_depth():
    """drt_read_depth_xyz / drt_read_depth_bgra / drt_depth_film_device_ptrs: the existing conversion kernels over the cut's buffers"""
    bundle, params = DC.load(BASE)
    d = BASE_CUTS[1]
    short = pydrt.Renderer(bundle, DC.params_at(params, d))
    try:
        short.render()
        want_xyz, want_bgra = short.read_xyz(), [short.read_bgra(w) for w in range(3)]
    finally:
        short.close()
    r = pydrt.Renderer(bundle, params)
    try:
        r.bind_depth_cuts(BASE_CUTS)
        r.render()
        assert cases.same_bits(r.read_depth_xyz(1), want_xyz)
        for w in range(3):
            assert np.array_equal(r.read_depth_bgra(1, w), want_bgra[w])
        ptrs = [r.depth_film_device_ptrs(c) for c in range(len(BASE_CUTS))]
        assert all(p for t in ptrs for p in t) and len({p for t in ptrs for p in t} | set(r.film_device_ptrs())) == 3 * len(BASE_CUTS) + 3
        with pytest.raises(RuntimeError, match="which = 3"):
            r.read_depth_bgra(1, 3)
    finally:
        r.close()


def test_every_refusal_says_why_and_leaves_the_context_rendering_as_before():
    bundle, params = DC.load(BASE)
    D = int(params.max_depth)
    r = pydrt.Renderer(bundle, params)
    try:
        for depths, why in (((1, 2, 3, 4, 5, 6, 7, 8, 9), "9 cuts, at most 8"), ((0, 1), "depth 0, not in 1..max_depth"), ((1, D + 1), "not in 1..max_depth = %d" % D),
                            ((2, 1), "not strictly ascending"), ((1, 2, 2), "not strictly ascending")):
            with pytest.raises(RuntimeError, match=why):
                r.bind_depth_cuts(depths)
        with pytest.raises(RuntimeError, match="no depth cuts are bound"):
            r.read_depth_film(0)
        r.bind_depth_cuts(BASE_CUTS)
        with pytest.raises(RuntimeError, match="cut 5 of 5"):
            r.read_depth_film(len(BASE_CUTS))
        with pytest.raises(RuntimeError, match="depth cuts bound"):
            r.render_adaptive(2, 4, 1, 0.1)
        with pytest.raises(RuntimeError, match="depth cuts bound"):
            r.render_adaptive_continue(4, 1, 0.1)
        r.render()
        with pytest.raises(RuntimeError, match="already holds samples"):  # other cuts on a film with samples
            r.bind_depth_cuts((1, 2))
        main, cuts = r.read_film(), cut_films(r, len(BASE_CUTS))
        assert_cuts_are_the_oracles(BASE, BASE_CUTS, main, cuts, "after the refusals")
        # unbound after a reset: adaptive sampling works again, and a film that holds an adaptive render takes no cuts
        r.reset_film()
        r.bind_depth_cuts(None)
        r.render_adaptive(2, 4, 1, 0.1)
        with pytest.raises(RuntimeError, match="adaptive render"):
            r.bind_depth_cuts((1, 2))
        r.reset_film()
        r.bind_depth_cuts((1, 2))
        r.render()
        DC.assert_film(r.read_depth_film(1), DC.oracle_at(BASE, 2)[:3], "bound again after an adaptive render and a reset")
    finally:
        r.close()
    x = pydrt.Renderer(bundle, DC.params_at(params, D, mode=pydrt.MODE_XYZ))
    try:
        with pytest.raises(RuntimeError, match="DRT_MODE_XYZ"):
            x.bind_depth_cuts((1, 2))
        x.render()
        assert np.isfinite(x.read_xyz()).all()
    finally:
        x.close()


def test_live_resources_are_back_at_the_baseline_after_close_and_after_an_unbind():
    bundle, params = DC.load(BASE)
    gc.collect()
    base = pydrt.selftest_live_resources()
    now = lambda: tuple(a - b for a, b in zip(pydrt.selftest_live_resources(), base))
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        r.read_film()
        r.reset_film()
        unbound = now()
        r.bind_depth_cuts(BASE_CUTS)
        assert now()[0] == unbound[0] + 3 * len(BASE_CUTS), "three device buffers per cut"
        r.render()
        r.read_depth_xyz(0)
        r.reset_film()
        r.bind_depth_cuts((1,))
        assert now()[0] == unbound[0] + 3 + 1, "the earlier films are released by the next bind (and d_xyz was made)"
        r.bind_depth_cuts(None)
        assert now()[0] == unbound[0] + 1 and now()[1:] == unbound[1:]
        r.bind_depth_cuts(BASE_CUTS)
        r.render()
        assert now()[0] > 0
    finally:
        r.close()
    gc.collect()
    assert now() == (0, 0, 0, 0), "%s still held (device, pinned, events, streams)" % (now(),)
