"""GPU (-m gpu): the path kernels on the edge-ray tables (tests/edge_ray_cases.py): ray films whose first rays are built from the
scene's own coordinates, so that the LDS row scans, the bounce kernel's walk and the next-event code written inline in five kernels
meet first hits exactly on a rectangle's edge, rays inside a wall's plane, spheres touched with a discriminant of 0, origins on a
surface and the point where a point light sits. The ground truth is the oracle rendering from the same table
(edge_ray_cases.expected); tests/test_edge_rays_cpu.py holds the premises and the oracle to the compiled reference on these rays.

Film comparisons are cases.same_bits on all three buffers, the hit log np.array_equal, the statistics cases.stat_counts (paths, scans,
shaded vertices, shadow scans, RNG draws). Each test renders at most about 3800 x 3 paths."""
import contextlib
import os

import numpy as np
import pytest

import cases
import edge_ray_cases as E
import pydrt
import ray_query_cases as RQ

pytestmark = pytest.mark.gpu

KNOBS = ("DRT_FORCE_BVH", "DRT_POOL_BLOCKS", "DRT_NO_SIMPLE_SHADE", "DRT_NO_FIXED_LISTS", "DRT_NO_CLOSED_SHADE", "DRT_NO_PAIR_ROWS",
         "DRT_TRACE_TAIL")
PIPELINES = [(name, forced) for name in E.SCENES for forced in (False, True) if not (forced and name in E.ALWAYS_BVH)]
_single = {}


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    """every test starts without the A/B switches; those it sets itself are taken back when it ends"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def assert_same_film(got, want, what):
    for buf, a, b in zip(("pixels", "means", "variances"), got, want):
        assert cases.same_bits(a, b), "%s, %s: %s" % (what, buf, cases.first_difference(a, b))


def assert_is_the_oracles(got, want, what, counts=True):
    """(film, hit log, stats) of the device against expected()'s (pixels, means, variances, hit log, stats)"""
    film, log, st = got
    assert_same_film(film, want[:3], what)
    bad = np.argwhere(log != want[3])
    assert not len(bad), "%s, hit log: %d entries differ, first (path %d, depth %d): %d against %d" % (
        what, len(bad), bad[0][0], bad[0][1], log[tuple(bad[0])], want[3][tuple(bad[0])])
    assert np.array_equal(log, want[3])
    if counts:
        assert cases.stat_counts(st) == cases.stat_counts(want[4]), what + ": counts"


@contextlib.contextmanager
def bound(name, order, **changes):
    """a context on the scene with the table bound (the switches in the environment are read when it is created)"""
    t, p = E.table(name, order), E.params_of(name, order, **changes)
    r = pydrt.Renderer(E.load(name)[0], p)
    try:
        r.bind_rays(t["origins"], t["dirs"])
        assert r.stats().path_flags & pydrt.PATH_RAYS
        yield r, p
    finally:
        r.close()


def rendered(name, order, **changes):
    """(film, hit log, stats) of one drt_render call from the table"""
    with bound(name, order, **changes) as (r, p):
        r.render()
        return r.read_film(), r.read_hit_indices(int(p.spp)), r.stats()


# ------------------------------------------------------------------------------------------------ every scene x pipeline
@pytest.mark.parametrize("name, forced", PIPELINES, ids=["%s%s" % (n, "-bvh" if f else "") for n, f in PIPELINES])
def test_every_scene_through_both_pipelines_in_both_orders(name, forced, monkeypatch):
    if forced:
        monkeypatch.setenv("DRT_FORCE_BVH", "1")
    for order in E.ORDERS:
        got = rendered(name, order)
        assert bool(got[2].path_flags & pydrt.PATH_BVH) == (forced or name in E.ALWAYS_BVH), "which pipeline ran"
        want = E.expected(name, order)
        assert_is_the_oracles(got, want, "%s %s%s" % (name, order, " behind the hierarchy" if forced else ""))
        assert np.any(want[0][:, :-1] != 0.0) and set(np.unique(want[3][:, 0] >= 0)) == {False, True}


# ------------------------------------------------------------------------------------------------ shade and record switches
SWITCHES = [{"DRT_FORCE_BVH": "1"}, {"DRT_POOL_BLOCKS": "1"}, {"DRT_NO_SIMPLE_SHADE": "1"}, {"DRT_NO_FIXED_LISTS": "1"},
            {"DRT_NO_CLOSED_SHADE": "1"}, {"DRT_NO_PAIR_ROWS": "1"}, {"DRT_TRACE_TAIL": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=["%s=%s" % kv for e in SWITCHES for kv in e.items()])
@pytest.mark.parametrize("name", ["plane_light_16", "gold_mirror"])
def test_the_a_b_switches_give_the_oracles_bits(name, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = rendered(name, "mixed")
    st = got[2]
    # a launch that ran out of record blocks is rendered again: its scans and draws are counted twice, the film and the log are not
    assert_is_the_oracles(got, E.expected(name, "mixed"), "%s %s" % (name, env), counts="DRT_POOL_BLOCKS" not in env)
    if "DRT_POOL_BLOCKS" in env:
        assert st.redone_launches > 0
    else:
        assert st.redone_launches == 0
    assert bool(st.path_flags & pydrt.PATH_BVH) == ("DRT_FORCE_BVH" in env)
    if "DRT_TRACE_TAIL" in env:
        assert not st.path_flags & pydrt.PATH_TRACE_TAIL


# ------------------------------------------------------------------------------------------------ depth and samples
def test_depth_one_is_direct_light_and_emission_only():
    name = "plane_light_16"
    S = E.load(name)[0].S
    for order in E.ORDERS:
        got = rendered(name, order, max_depth=1)
        want = E.expected(name, order, max_depth=1)
        assert_is_the_oracles(got, want, "%s %s at depth 1" % (name, order))
        assert got[1].shape[1] == 1 and got[2].closest_hit_scans == got[2].paths
        # where the first ray ends on a black body or escapes, the sums are emission or nothing, put together by hand; elsewhere they
        # are direct light alone, which the oracle's film above holds (tests/test_edge_rays_cpu.py puts that together by hand too)
        d1 = E.depth_one_sums(name, order)
        plain = d1["plain"]
        assert plain.any() and np.any(d1["sums"][plain] != 0.0) and not np.all(d1["sums"][plain] != 0.0)
        assert cases.same_bits(got[0][0][plain, :S], d1["sums"][plain]), cases.first_difference(got[0][0][plain, :S], d1["sums"][plain])


def test_depth_eight_five_samples_in_launches_of_two_and_in_two_calls():
    name, order, changes = "plane_light_16", "mixed", dict(max_depth=8, spp=5, batch_spp=2)
    want = E.expected(name, order, **changes)
    got = rendered(name, order, **changes)
    assert got[2].launches >= 3, "5 samples in launches of 2"
    assert_is_the_oracles(got, want, "%s depth 8, 5 spp in launches of 2" % name)
    assert np.any(want[3][:, 4:] >= 0), "paths longer than the tables' depth 4"
    with bound(name, order, **changes) as (r, p):
        r.render(0, 3)
        r.render(3, 2)
        assert_same_film(r.read_film(), want[:3], "%s in two calls" % name)


# ------------------------------------------------------------------------------------------------ depth cuts
@pytest.mark.parametrize("name, forced", [("plane_light_16", False), ("lights", True)])
def test_depth_cuts_bound_before_the_render(name, forced, monkeypatch):
    if forced:
        monkeypatch.setenv("DRT_FORCE_BVH", "1")
    cuts = (1, 2, 4)
    with bound(name, "mixed") as (r, p):
        r.bind_depth_cuts(cuts)
        r.render()
        assert bool(r.stats().path_flags & pydrt.PATH_BVH) == forced
        main, log, st = r.read_film(), r.read_hit_indices(int(p.spp)), r.stats()
        films = [r.read_depth_film(c) for c in range(len(cuts))]
    assert_is_the_oracles((main, log, st), E.expected(name, "mixed"), name + " main film with cuts bound")
    for d, film in zip(cuts, films):
        assert_same_film(film, E.expected(name, "mixed", max_depth=d)[:3], "%s cut at depth %d" % (name, d))
    assert not cases.same_bits(films[0][0], films[1][0]) and not cases.same_bits(films[1][0], films[2][0])


# ------------------------------------------------------------------------------------------------ a tree built on the device
@pytest.mark.parametrize("name", ["deg_coincident_surfaces", "fuzz_17"])
def test_a_tree_built_on_the_device_gives_the_same_bits(name, monkeypatch):
    monkeypatch.setenv("DRT_FORCE_BVH", "1")
    want = E.expected(name, "mixed")
    with bound(name, "mixed") as (r, p):
        assert r.stats().path_flags & pydrt.PATH_BVH and r.hierarchy_report()["device_builds"] == 0
        r.render()
        before = (r.read_film(), r.read_hit_indices(int(p.spp)), r.stats())
        assert_is_the_oracles(before, want, name + " before the rebuild")
        r.reset_film()
        r.rebuild_hierarchy()
        r.render()
        rep = r.hierarchy_report()
        assert rep["device_builds"] == 1 and rep["built_by"] == 1
        after = (r.read_film(), r.read_hit_indices(int(p.spp)), r.stats())
    assert_same_film(after[0], before[0], name + " after the rebuild against before")
    assert np.array_equal(after[1], before[1])
    assert_is_the_oracles(after, want, name + " after the rebuild", counts=False)  # (the context's counts run on over both renders)


# ------------------------------------------------------------------------------------------------ the query kernels on the same rays
@contextlib.contextmanager
def plain_context(name):
    bundle, p = E.load(name)
    r = pydrt.Renderer(bundle, p)
    try:
        yield r
    finally:
        r.close()


def fixture_pairs(golden_dir, name):
    """the pairs tests/golden/edge_rays.npz records answers for, made again from the hit records it holds"""
    z = np.load(os.path.join(golden_dir, "edge_rays.npz"), allow_pickle=False)
    g = {k: z["%s.%s" % (name, k)] for k in ("o", "d", "index", "position", "visible")}
    p0, p1 = E.visibility_pairs(E.load(name)[0], g["o"], g["d"], g["index"], g["position"])
    assert len(p0) == len(g["visible"])
    return p0, p1


@pytest.mark.parametrize("forced", [False, True], ids=["flat", "bvh"])
@pytest.mark.parametrize("name", ["plane_light_16", "deg_awkward_lights"])
def test_the_query_kernels_on_the_lattice_rays(name, forced, monkeypatch, golden_dir):
    if forced:
        monkeypatch.setenv("DRT_FORCE_BVH", "1")
    bundle = E.load(name)[0]
    ro, rd = E.lattice_rays(name)
    p0, p1 = fixture_pairs(golden_dir, name)
    with plain_context(name) as r:
        assert bool(r.stats().path_flags & pydrt.PATH_BVH) == forced
        hits = r.cast_rays(ro, rd)
        vis = r.test_visibility(p0, p1)
    key = ("query", name)
    if key not in _single:
        want = RQ.oracle_hits(bundle, ro, rd)
        want["distance"] = RQ.oracle_distances(bundle, ro, rd, want["index"])
        _single[key] = (want, RQ.oracle_visible(bundle, p0, p1))
    want, want_vis = _single[key]
    for f in ("index", "surface_material", "incident_material", "transmit_material"):
        bad = np.flatnonzero(hits[f] != want[f])
        assert not len(bad), "%s %s: %d differ, first ray %d (o %r, d %r): %d against %d" % (
            name, f, len(bad), bad[0], ro[bad[0]].tolist(), rd[bad[0]].tolist(), hits[f][bad[0]], want[f][bad[0]])
    on = want["index"] >= 0
    assert on.any() and (~on).any()
    for f in ("position", "normal", "out", "on_dot", "distance"):
        assert cases.same_bits(hits[f][on], want[f][on]), "%s %s: %s" % (name, f, cases.first_difference(hits[f][on], want[f][on]))
    bad = np.flatnonzero(vis != want_vis)
    assert not len(bad), "%s visibility: %d of %d pairs differ, first %d: %r -> %r" % (name, len(bad), len(vis), bad[0], p0[bad[0]].tolist(), p1[bad[0]].tolist())
    assert set(np.unique(vis)) == {0, 1}


# ------------------------------------------------------------------------------------------------ a group
def test_a_group_of_three_assembles_the_single_contexts_film():
    name, order = "lights", "mixed"
    t, p = E.table(name, order), E.params_of(name, order, flags=0)
    r = pydrt.Renderer(E.load(name)[0], p)
    try:
        r.bind_rays(t["origins"], t["dirs"])
        r.render()
        single = r.read_film()
    finally:
        r.close()
    g = pydrt.Group(E.load(name)[0], p, devices=[0, 0, 0])
    try:
        assert g.size() == 3
        g.bind_rays(t["origins"], t["dirs"])
        assert g.stats().path_flags & pydrt.PATH_RAYS
        g.render()
        film = g.read_film()
    finally:
        g.close()
    assert_same_film(film, single, "%s: a group of three against one context" % name)
    assert_same_film(film, E.expected(name, order)[:3], "%s: a group of three against the oracle" % name)
