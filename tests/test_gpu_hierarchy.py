"""GPU (-m gpu): device hierarchy builds (drt_rebuild_hierarchy, drt_get_hierarchy_report, drt_read_hierarchy, the group form, pydrt's
bindings). Two rules. The tree the device builds is the one tests/hierarchy_rule.py states, byte for byte: child,
count and the leaf order, from boxes computed in numpy. And no result moves: films (cases.same_bits on all three buffers), hit logs
(array_equal) and the counting statistics (==) are those of the context before the build, of a fresh context, and of the oracle.
tests/test_hierarchy_cpu.py holds the premises (the rule's trees are valid and at most 32 levels deep). The scenes run from 1 to 20001
tree surfaces (tests/hierarchy_cases.py); tests/test_gpu_build_passes.py holds the sort and the topology passes alone, on keys made for them."""
import contextlib
import os

import numpy as np
import pytest

import cases
import hierarchy_cases as HC
import hierarchy_rule as R
import pydrt
import ray_query_cases as Q
import scene_update_cases as U

pytestmark = pytest.mark.gpu

CASES = ["spheres_1500", "spheres_96", "lights_all_bvh", "one_sphere", "two_surfaces", "parallel_edges", "coincident_300", "deep_64",
         # past one tile of the sort, one block of a level, one wave of the bounds pass (tests/hierarchy_cases.py)
         "three_spheres", "four_spheres", "five_spheres", "spheres_1024", "spheres_2049", "spheres_4097", "lattice_5000", "planes_first",
         "planes_last_only_bounded", "spheres_20000"]
RAY_CASES = ("spheres_1500", "spheres_20000")  # 4096 seeded rays and pairs after the build (spheres_20000's film is one sample per pixel: the
# oracle's scan of 20001 surfaces per vertex keeps that to a fraction of a second, and the queries to about a second)
HIT_FLOATS = ("position", "normal", "out", "on_dot", "distance")
HIT_INTS = ("index", "surface_material", "incident_material", "transmit_material")
_fresh, _oracle, _rule = {}, {}, {}


def assert_same_film(got, want, what):
    for name, a, b in zip(("pixels", "avgs", "vars"), got, want):
        assert cases.same_bits(a, b), "%s %s: %s" % (what, name, cases.first_difference(a, b))


def assert_same(got, want, what):
    """(film, hit log, counts) triples"""
    assert_same_film(got[0], want[0], what)
    assert np.array_equal(got[1], want[1]), what + ": hit log"
    assert got[2] == want[2], what + ": counts"


@contextlib.contextmanager
def context(name, which="after", params=None):
    """a context on a case's scene (DRT_FORCE_BVH is read when the context is created)"""
    c = HC.load(name)
    saved = os.environ.pop("DRT_FORCE_BVH", None)
    if c["forced"]:
        os.environ["DRT_FORCE_BVH"] = "1"
    try:
        r = pydrt.Renderer(c[which], params or c["params"])
    finally:
        os.environ.pop("DRT_FORCE_BVH", None)
        if saved is not None:
            os.environ["DRT_FORCE_BVH"] = saved
    try:
        assert bool(r.stats().path_flags & pydrt.PATH_BVH) == c["bvh"], name
        yield r
    finally:
        r.close()


def rendered(r, p):
    r.render()
    return r.read_film(), r.read_hit_indices(int(p.spp)), cases.stat_counts(r.stats())


def fresh(name, which="after"):
    if (name, which) not in _fresh:
        with context(name, which) as r:
            _fresh[(name, which)] = rendered(r, HC.load(name)["params"])
    return _fresh[(name, which)]


def oracle(name):
    if name not in _oracle:
        c = HC.load(name)
        px, av, va, log, st = cases.oracle_render_device_pow(c["after"], c["params"], want_hits=True)
        _oracle[name] = ((px, av, va), log, cases.stat_counts(st))
    return _oracle[name]


def rule(name, which="after"):
    if (name, which) not in _rule:
        _rule[(name, which)] = R.build_rows(pydrt.surface_rows(HC.load(name)[which]))
    return _rule[(name, which)]


def assert_is_the_rules_tree(r, want, what):
    """drt_read_hierarchy against the rule: links and leaf order exactly, every box around what hangs below it, at most 32 levels"""
    nodes, leaf = r.read_hierarchy()
    rep = r.hierarchy_report()
    m = len(want["order"])
    assert (rep["nodes"], rep["leaf_surfaces"]) == (max(m - 1, 1), m) == (len(nodes), len(leaf)), what
    assert np.array_equal(nodes["child"], want["child"]), what + ": child"
    assert np.array_equal(nodes["count"], want["count"]), what + ": count"
    assert np.array_equal(leaf, want["leaf_surface"]), what + ": leaf order"
    assert rep["depth"] == want["depth"] <= R.BVH_STACK, what
    assert_boxes_hold(nodes, want["order"], want, what)
    return nodes, leaf


def assert_boxes_hold(nodes, order, boxes, what):
    """every child's box around what hangs below it: the nodes of an inner child, boxes["lo"], boxes["hi"] of the tree position
    order[slot] of a leaf"""
    with np.errstate(invalid="ignore"):
        for i in range(len(nodes)):
            for c in range(2):
                lo, hi = nodes["lo"][i, c].astype(np.float64), nodes["hi"][i, c].astype(np.float64)
                if nodes["count"][i, c] == 0:
                    k = nodes["child"][i, c]
                    assert (lo <= nodes["lo"][k].min(axis=0)).all() and (hi >= nodes["hi"][k].max(axis=0)).all(), "%s: node %d child %d" % (what, i, c)
                elif nodes["count"][i, c] == 1:
                    k = order[(-2 - nodes["child"][i, c]) // 8]
                    assert (lo <= boxes["lo"][k]).all() and (hi >= boxes["hi"][k]).all(), "%s: node %d leaf %d" % (what, i, c)


def assert_hits(got, want, what):
    for f in HIT_INTS:
        assert np.array_equal(got[f], want[f]), "%s %s" % (what, f)
    for f in HIT_FLOATS:
        assert cases.same_bits(got[f], want[f]), "%s %s: %s" % (what, f, cases.first_difference(got[f], want[f]))


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", CASES)
def test_the_device_builds_the_rules_tree(name):
    c = HC.load(name)
    before_update = name == "spheres_1500"  # this one is built after its update: the boxes are the derive kernel's of moved surfaces
    with context(name, "before" if before_update else "after") as r:
        rep = r.hierarchy_report()
        assert (rep["built_by"], rep["device_builds"], rep["kernel_ms"]) == (0, 0, 0.0)
        if before_update:
            r.update_surfaces(pydrt.surface_rows(c["after"]))
        r.rebuild_hierarchy()
        assert_is_the_rules_tree(r, rule(name), name)
        rep = r.hierarchy_report()
        m = rep["leaf_surfaces"]
        assert (rep["built_by"], rep["device_builds"]) == (1, 1) and (rep["kernel_ms"] > 0.0) == (m >= 2)
        assert r.update_report()["refits_since_build"] == 0


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", CASES)
def test_no_result_moves(name):
    c = HC.load(name)
    p = c["params"]
    with context(name) as r:
        first = rendered(r, p)
        r.reset_film()
        r.rebuild_hierarchy()
        built = rendered(r, p)
        assert_same(built, first, name + ": after the build against before it")
        assert_same(built, oracle(name), name + ": after the build against the oracle")
        if name in ("coincident_300", "deep_64"):  # (the two scenes of this file's own: camera rays do meet them)
            assert np.any(built[1][:, 0] >= 0) and np.any(built[1][:, 0] < 0)
        if name in RAY_CASES:
            ro, rd, p0, p1 = HC.seeded_rays(name)
            hits, vis = r.cast_rays(ro, rd), r.test_visibility(p0, p1)
            want = Q.oracle_hits(c["after"], ro, rd)
            want["distance"] = Q.oracle_distances(c["after"], ro, rd, want["index"])
            assert_hits(hits, want, name + ": rays after the build")
            assert (want["index"] >= 0).any() and (want["index"] < 0).any()
            assert np.array_equal(vis, Q.oracle_visible(c["after"], p0, p1)) and set(np.unique(vis)) == {0, 1}
    _fresh[(name, "after")] = first


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", ["spheres_1500", "lights_all_bvh"])
def test_a_build_in_the_middle_of_a_film(name):
    p = HC.load(name)["params"]
    spp, n_pix = int(p.spp), int(p.tile_w) * int(p.tile_h)
    assert spp >= 2
    film, log, counts = fresh(name)
    with context(name) as r:
        r.render(0, 1)
        r.rebuild_hierarchy()
        r.render(1, spp - 1)
        assert_same_film(r.read_film(), film, name + ": one film around a build")
        assert np.array_equal(r.read_hit_indices(spp - 1), log[n_pix:])  # the log holds the last call's samples, sample by sample
        assert cases.stat_counts(r.stats()) == counts


# ------------------------------------------------------------------------------------------------ 4
def test_the_gap_closed_a_device_mode_update_then_a_build():
    torch = pytest.importorskip("torch")
    name = "spheres_1500"
    c = HC.load(name)
    with context(name, "before") as r:
        rows = torch.from_numpy(pydrt.surface_rows(c["after"])).to("cuda:0")
        r.update_surfaces(rows)
        assert r.update_report()["refits_since_build"] == 1
        r.rebuild_hierarchy()
        rep = r.update_report()
        assert rep["refits_since_build"] == 0 and rep["updates"] == 1
        assert_same(rendered(r, c["params"]), fresh(name), name + ": device-mode update, then a build")
        assert_is_the_rules_tree(r, rule(name), name)


# ------------------------------------------------------------------------------------------------ 5, 6
@pytest.mark.parametrize("rebuild", [False, True])
def test_a_build_then_a_host_mode_update(rebuild):
    name = "spheres_1500"
    c = HC.load(name)
    with context(name, "before") as r:
        r.rebuild_hierarchy()
        r.update_surfaces(pydrt.surface_rows(c["after"]), rebuild=rebuild)  # a refit through the maps the device made, or the host's own tree again
        rep, hrep = r.update_report(), r.hierarchy_report()
        assert rep["updates"] == 1 and rep["refits_since_build"] == (0 if rebuild else 1)
        assert (hrep["built_by"], hrep["device_builds"]) == ((0, 1) if rebuild else (1, 1))
        assert_same(rendered(r, c["params"]), fresh(name), name + ": a build, then an update")
        nodes, leaf = r.read_hierarchy()
        if not rebuild:  # the refit kept the links the device made for the scene before
            assert np.array_equal(nodes["child"], rule(name, "before")["child"]) and np.array_equal(leaf, rule(name, "before")["leaf_surface"])
        # and a device build again, in any order
        r.reset_film()
        r.rebuild_hierarchy()
        assert_is_the_rules_tree(r, rule(name), name + ": built again")
        assert r.hierarchy_report()["device_builds"] == 2 and r.hierarchy_report()["built_by"] == 1
        assert_same(rendered(r, c["params"]), fresh(name), name + ": and a build again")


# ------------------------------------------------------------------------------------------------ 7
def test_two_builds_in_a_row_give_the_same_bytes():
    name = "spheres_96"
    with context(name) as r:
        r.rebuild_hierarchy()
        a = r.read_hierarchy()
        r.rebuild_hierarchy()
        r.rebuild_hierarchy()  # (and one whose copy for the host nobody waited for)
        b = r.read_hierarchy()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert r.hierarchy_report()["device_builds"] == 3


# ------------------------------------------------------------------------------------------------ 4 to 7 past one tile
@pytest.mark.parametrize("name", HC.MULTI_TILE)
def test_a_device_mode_update_then_a_build_past_one_tile(name):
    torch = pytest.importorskip("torch")
    c = HC.load(name)
    with context(name, "before") as r:
        r.update_surfaces(torch.from_numpy(pydrt.surface_rows(c["after"])).to("cuda:0"))
        assert r.update_report()["refits_since_build"] == 1
        r.rebuild_hierarchy()
        assert r.update_report()["refits_since_build"] == 0
        assert_same(rendered(r, c["params"]), fresh(name), name + ": device-mode update, then a build")
        assert_is_the_rules_tree(r, rule(name), name)


@pytest.mark.parametrize("rebuild", [False, True])
@pytest.mark.parametrize("name", HC.MULTI_TILE)
def test_a_build_then_a_host_mode_update_past_one_tile(name, rebuild):
    """the refit goes through the maps the device made and the level_first hierarchy_adopt makes of the device's level counts: five
    tiles of the sort, levels of more than one block"""
    c = HC.load(name)
    with context(name, "before") as r:
        r.rebuild_hierarchy()
        assert_is_the_rules_tree(r, rule(name, "before"), name + ": before")
        r.update_surfaces(pydrt.surface_rows(c["after"]), rebuild=rebuild)
        rep, hrep = r.update_report(), r.hierarchy_report()
        assert rep["updates"] == 1 and rep["refits_since_build"] == (0 if rebuild else 1)
        assert (hrep["built_by"], hrep["device_builds"]) == ((0, 1) if rebuild else (1, 1))
        assert_same(rendered(r, c["params"]), fresh(name), name + ": a build, then an update")
        nodes, leaf = r.read_hierarchy()
        if not rebuild:  # the links are the build's, every box is around what the update put below it
            assert np.array_equal(nodes["child"], rule(name, "before")["child"]) and np.array_equal(leaf, rule(name, "before")["leaf_surface"])
            assert_boxes_hold(nodes, rule(name, "before")["order"], rule(name), name + ": refitted")
        r.reset_film()
        r.rebuild_hierarchy()
        assert_is_the_rules_tree(r, rule(name), name + ": built again")
        assert_same(rendered(r, c["params"]), fresh(name), name + ": and a build again")


@pytest.mark.parametrize("name", HC.MULTI_TILE)
def test_two_builds_in_a_row_give_the_same_bytes_past_one_tile(name):
    with context(name) as r:
        r.rebuild_hierarchy()
        a = r.read_hierarchy()
        r.rebuild_hierarchy()
        r.rebuild_hierarchy()
        b = r.read_hierarchy()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert r.hierarchy_report()["device_builds"] == 3


# ------------------------------------------------------------------------------------------------ 8
def test_nothing_else_moves():
    name = "spheres_1500"
    c = HC.load(name)
    L = pydrt.hip_lib()
    with context(name) as r:
        r.render_features(n_samples=2)
        r.render_mattes(n_samples=2)
        features, mattes = r.read_features(), r.read_mattes()
        updates = r.update_report()["updates"]
        r.rebuild_hierarchy()
        assert r.update_report()["updates"] == updates == 0
        for a, b in zip(r.read_features() + r.read_mattes(), features + mattes):  # passes taken before the build still read
            assert a.tobytes() == b.tobytes()
        tree = r.read_hierarchy()
        assert L.drt_rebuild_hierarchy(r.ctx, 1) != 0 and b"unknown flags" in L.drt_last_error()
        assert L.drt_rebuild_hierarchy(r.ctx, 4) != 0 and b"unknown flags" in L.drt_last_error()
        assert r.hierarchy_report()["device_builds"] == 1 and r.read_hierarchy()[0].tobytes() == tree[0].tobytes()
    assert L.drt_rebuild_hierarchy(None, 0) != 0 and b"null" in L.drt_last_error()
    assert L.drt_group_rebuild_hierarchy(None, 0) != 0 and b"null" in L.drt_last_error()
    lds = "plane_light_16"  # a context without the hierarchy: the call succeeds and changes nothing
    p = HC.load(lds)["params"]
    with context(lds) as r:
        first = rendered(r, p)
        r.reset_film()
        r.rebuild_hierarchy()
        assert_same(rendered(r, p), first, lds + ": a build without a hierarchy")
        rep = r.hierarchy_report()
        assert (rep["nodes"], rep["leaf_surfaces"], rep["device_builds"], rep["built_by"]) == (0, 0, 0, 0)
        assert r.update_report()["updates"] == 0
        with pytest.raises(RuntimeError, match="no hierarchy"):
            r.read_hierarchy()


# ------------------------------------------------------------------------------------------------ 9
def test_a_pending_extent_violation_stays_pending():
    torch = pytest.importorskip("torch")
    name = "spheres_1500"
    c = HC.load(name)
    with context(name, "before") as r:
        bad = pydrt.surface_rows(c["before"])[:1].copy()
        bad[0, U.ROW_POS] = (2.0 ** 28, 0.0, 0.0)
        r.update_surfaces(torch.from_numpy(bad).to("cuda:0"))
        r.rebuild_hierarchy()
        with pytest.raises(RuntimeError, match="2\\^27"):
            r.synchronize()
        r.update_surfaces(torch.from_numpy(pydrt.surface_rows(c["after"])).to("cuda:0"))  # a good update clears it, through the device-made maps
        r.synchronize()
        assert_same(rendered(r, c["params"]), fresh(name), name + ": after the violation was mended")


# ------------------------------------------------------------------------------------------------ 10
def test_the_group_form():
    name = "spheres_1500"
    c = HC.load(name)
    q = U._params(c["params"], hits=False)
    q.flags = 0  # (hit recording is per context)
    with context(name, params=q) as r:
        r.render()
        want = r.read_film(), cases.stat_counts(r.stats())
    g = pydrt.Group(c["after"], q, devices=[0, 0, 0])
    try:
        g.rebuild_hierarchy()
        g.render()
        assert_same_film(g.read_film(), want[0], "the group after a build")
        assert cases.stat_counts(g.stats()) == want[1]
        assert g.L.drt_group_rebuild_hierarchy(g.g, 2) != 0 and b"unknown flags" in g.L.drt_last_error()
    finally:
        g.close()
