"""GPU (-m gpu): what the launcher holds is released. pydrt.selftest_live_resources() reports the process-wide counts of live device
allocations, pinned host allocations, HIP events and HIP streams held through the owning types of csrc/drt_owned.h; every check here
is on the difference from a baseline taken at the start of the test, so contexts other tests left alive do not matter. Each context
calls every feature that allocates on first use once, at 16 x 16 pixels and 2 samples; before close() the device and event counts are
above the baseline (a zero afterwards is not vacuous), after close() all four are back at it.

With the hand-kept list of drt_destroy that this replaces, d_ainfo (adaptive_alloc) was never freed by drt_destroy: every
back-at-the-baseline check of a context that had rendered adaptively (the flat, hierarchy and cycle tests) would have found the device
count one too high, and the cycle test a count growing by one per cycle."""
import gc

import numpy as np
import pytest

import cases
import pydrt
import ray_film_cases as R

pytestmark = pytest.mark.gpu

W = H = 16
SPP = 2
DEVICE, PINNED, EVENTS, STREAMS = range(4)


class Counts:
    """the four counters, relative to where they were when this was made"""

    def __init__(self):
        gc.collect()
        self.base = pydrt.selftest_live_resources()

    def now(self):
        return tuple(a - b for a, b in zip(pydrt.selftest_live_resources(), self.base))

    def held(self):
        """just before a close(): something is there to be released"""
        d = self.now()
        assert d[DEVICE] > 0 and d[EVENTS] > 0 and d[STREAMS] > 0, d
        return d

    def released(self, what):
        gc.collect()
        assert self.now() == (0, 0, 0, 0), "%s: %s still held (device, pinned, events, streams)" % (what, self.now())


def gold_scene(tail):
    """the flat gold-and-mirror scene of cases.RENDER_CASES: S = 69 (a tail of 5: d_tail_stage and d_tail_resume exist) or S = 64 (none)"""
    return pydrt.load_scene(cases.scene_path(cases.RENDER_CASES["gold_mirror"][0]), W, H, max_wl=720.0 if tail else 695.0)


def params(**kw):
    return pydrt.make_params(W, H, spp=SPP, max_depth=4, seed=3, **kw)


def material_record(bundle):
    """one drt_selftest_material record: the first material with a BDSF list, seen along its normal"""
    mats = bundle.materials()
    m = next(i for i in range(len(mats)) if int(mats[i].num_bdsfs) > 0 and not int(mats[i].is_emissive))
    base = int(bundle.scene.base_material)
    return np.array([[0, 0, 0, 0, 0, 1, 0, 0, 1, 1.0, m, base, m, -1, 0, 0, 1.0, 0]], dtype=np.float64)


def exercise(bundle, counts, hierarchy=False):
    """One call of everything that allocates on first use, in two contexts (hit recording and adaptive sampling exclude each other).
    Returns the counts at named points, for the cycle test."""
    marks = {}
    r = pydrt.Renderer(bundle, params(flags=pydrt.FLAG_RECORD_HITS))
    try:
        r.render()
        r.read_xyz()
        r.read_bgra(1)
        assert r.read_hit_indices(SPP).shape == (W * H * SPP, 4)
        marks["hits"] = counts.held()
    finally:
        r.close()
    counts.released("the hit-recording context")

    o, d, w = R.centre_rays(bundle, W, H)
    rec = material_record(bundle)
    r = pydrt.Renderer(bundle, params())
    try:
        assert bool(r.stats().path_flags & pydrt.PATH_BVH) == hierarchy
        assert r.render_adaptive(2, 4, 2, 0.05)["rounds"] >= 1
        first = counts.held()
        r.render_adaptive_continue(8, 2, 0.05)
        assert counts.now() == first
        r.reset_film()
        r.render_adaptive(2, 4, 2, 0.05)
        assert counts.now() == first, "a second adaptive render holds what the first held"
        marks["adaptive"] = first
        r.denoise(radius=2, patch=1)
        r.read_denoised_bgra()
        r.render_features(n_samples=2)
        r.read_feature_bgra(pydrt.FEATURE_NORMAL, -1.0, 1.0)
        r.render_mattes(n_samples=2)
        r.read_matte(0, [0])
        r.read_matte_bgra(0)
        ro, rd = o.reshape(-1, 3), d.reshape(-1, 3)
        assert r.cast_rays(ro, rd).shape == (W * H,)
        assert r.test_visibility(ro, ro + rd).shape == (W * H,)
        r.cast_pixels(np.array([[0, 0], [3, 4]]), np.array([0, 1]))
        marks["passes"] = counts.now()
        r.reset_film()
        r.bind_rays(o, d, w)
        bound = counts.now()
        assert bound[DEVICE] == marks["passes"][DEVICE] + 3
        r.bind_rays(np.stack([o, o]), np.stack([d, d]), np.stack([w, w]))  # another table, two layers: the old copies are freed
        assert counts.now() == bound
        r.bind_rays(None)
        assert counts.now() == marks["passes"]
        r.set_camera(bundle)
        r.update_surfaces(pydrt.surface_rows(bundle))
        r.update_spectra(bundle.spds()[4:], first=4)  # everything but the observer's rows
        pydrt.selftest_material(r, pydrt.MAT_EVALUATE, rec)
        variants = counts.now()
        r.update_materials(bundle.materials())
        pydrt.selftest_material(r, pydrt.MAT_EVALUATE, rec)
        assert counts.now()[DEVICE] == variants[DEVICE], "the variants are made again in the same allocation"
        assert r.update_report()["updates"] >= 2
        if hierarchy:
            r.update_surfaces(pydrt.surface_rows(bundle), rebuild=True)
            r.rebuild_hierarchy()
            nodes, leaf = r.read_hierarchy()
            assert len(leaf) == r.hierarchy_report()["leaf_surfaces"] and r.hierarchy_report()["device_builds"] == 1
        r.render()
        r.read_film()
        marks["all"] = counts.held()
        assert marks["all"][PINNED] > 0
    finally:
        r.close()
    counts.released("the context that called everything")
    return marks


@pytest.mark.parametrize("tail", [False, True], ids=["S64", "S69"])
def test_a_flat_context_releases_everything(tail):
    bundle = gold_scene(tail)
    assert bundle.S == (69 if tail else 64)
    exercise(bundle, Counts())


def test_a_hierarchy_context_releases_everything():
    """128 spheres: the smallest count of the generator above build_device_scene's 96 surfaces"""
    exercise(pydrt.synthetic_sphere_scene(128, W, H), Counts(), hierarchy=True)


def test_an_xyz_context_holds_one_film_buffer():
    counts = Counts()
    r = pydrt.Renderer(gold_scene(True), params(mode=pydrt.MODE_XYZ))
    try:
        px, av, va = r.film_device_ptrs()
        assert px and not av and not va
        r.render()
        assert r.read_xyz_film().shape == (W * H, 8)
        counts.held()
    finally:
        r.close()
    counts.released("the XYZ context")


def test_a_bound_film_is_the_callers():
    import torch

    bundle = gold_scene(True)
    S, n = bundle.S, W * H
    counts = Counts()
    r = pydrt.Renderer(bundle, params())
    try:
        r.render()  # (the timing events are made here)
        r.reset_film()
        own = counts.now()
        t = [torch.full((n, k), v, dtype=torch.float64, device="cuda:0") for k, v in ((S + 1, 1.5), (S, 2.5), (S, 3.5))]
        r.bind_film(*(x.data_ptr() for x in t))
        assert counts.now()[DEVICE] == own[DEVICE] - 3, "the context's own film goes when another is bound"
        film = [np.arange(n * k, dtype=np.float64).reshape(n, k) + c for k, c in ((S + 1, 0.25), (S, 0.5), (S, 0.75))]
        r.write_film(*film)
        counts.held()
    finally:
        r.close()
    torch.cuda.synchronize()
    for x, want in zip(t, film):  # still readable, and what was last written: the launcher did not free them
        assert np.array_equal(x.cpu().numpy(), want)
    del t
    counts.released("the context with a bound film")


def test_refused_calls_leave_nothing_behind():
    bundle = cases.load_case("large_box")[0]
    counts = Counts()
    with pytest.raises(RuntimeError, match="max_depth 525"):
        pydrt.Renderer(bundle, pydrt.make_params(16, 16, spp=1, max_depth=525, seed=5))
    counts.released("a refused drt_create")
    bundle = gold_scene(True)
    o, d, w = R.centre_rays(bundle, W, H)
    r = pydrt.Renderer(bundle, params())
    try:
        r.render()
        before = counts.now()
        with pytest.raises(RuntimeError, match="film holds samples"):
            r.bind_rays(o, d, w)
        assert counts.now() == before
        r.reset_film()
        wrong = pydrt.surfaces_from_rows(pydrt.surface_rows(bundle))
        wrong[3].type = pydrt.GEO_POINT if int(wrong[3].type) != pydrt.GEO_POINT else pydrt.GEO_SPHERE
        with pytest.raises(RuntimeError, match="surface 3: type"):
            r.update_surfaces(wrong)
        assert counts.now() == before
    finally:
        r.close()
    counts.released("the context after two refusals")


def test_a_group_releases_everything():
    bundle = gold_scene(True)
    o, d, w = R.centre_rays(bundle, W, H)
    counts = Counts()
    g = pydrt.Group(bundle, params(), devices=[0, 0])
    try:
        g.render()
        g.read_film()
        g.render_features(2)
        g.denoise(radius=2, patch=1)
        g.reset_film()
        g.bind_rays(o, d, w)
        held = counts.held()
        assert held[STREAMS] == 2
    finally:
        g.close()
    counts.released("the group")


def test_three_cycles_hold_the_same_at_every_point():
    bundle = gold_scene(True)
    counts = Counts()
    marks = [exercise(bundle, counts) for _ in range(3)]
    assert marks[1] == marks[0] and marks[2] == marks[0]
