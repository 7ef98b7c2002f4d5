"""Device hierarchy builds (drt_rebuild_hierarchy): the inputs of tests/test_hierarchy_cpu.py and
tests/test_gpu_hierarchy.py that tests/scene_update_cases.py does not have -- the two scenes made to take the rule's other paths, and
the scenes that take the build's passes past one tile of the sort, one block of a level and one wave of the bounds pass."""
import numpy as np

import pydrt
import scene_update_cases as U

DEEP_EXTENT = 16.0


def coincident_spheres(n=300):
    """n spheres with one centre and different radii: every key is equal, every split is the median's. The centre is the origin, where
    a box is symmetric and its centre exact whatever the radius."""
    return [("sphere", (0.0, 0.0, 0.0), 0.5 + 0.01 * k) for k in range(n)]


def deep_spheres():
    """64 spheres whose tree is 63 inner levels deep without the rule's depth budget: coordinates that halve along the three axes in
    turn, so every key but one has a highest set bit of its own and every split by that bit peels one sphere off. Per axis: one
    sphere at the extent (quantised to 2^21 - 1) and twenty at 1.5 * extent / 2^(k + 1), k = 1 .. 20 (quantised to 2^(20 - k) +
    2^(19 - k) for k < 20 and to 1 for k = 20: the factor 1.5 keeps the highest bit clear of the rounding of a box's centre); the last
    sphere sits at the origin (key 0)."""
    s = []
    for k in range(21):
        for axis in range(3):
            p = [0.0, 0.0, 0.0]
            p[axis] = DEEP_EXTENT if k == 0 else 1.5 * DEEP_EXTENT / 2.0 ** (k + 1)
            s.append(("sphere", tuple(p), 1.0))
    return s + [("sphere", (0.0, 0.0, 0.0), 1.0)]


FLAT_U, FLAT_V = (1.0, 0.0, 0.0), (2.0, 0.0, 0.0)  # parallel edge vectors: no normal, an unbounded box (as parallel_edges' last plane)
PARAMS_SMALL = dict(spp=3, max_depth=4, seed=21)    # the forced small cases of scene_update_cases
PARAMS_LARGE = dict(spp=2, max_depth=3, seed=33)


def scene(surfaces):
    """scene_update_cases.small_scene with one more kind: ("flat_plane", position), a white plane whose edge vectors are parallel"""
    b = U.small_scene([("sphere", s[1], 1.0) if s[0] == "flat_plane" else s for s in surfaces])
    flat = [i for i, s in enumerate(surfaces) if s[0] == "flat_plane"]
    if not flat:
        return b
    rows = pydrt.surface_rows(b)
    head = rows[:, 0].copy().view("<u4").reshape(-1, 2)
    head[flat, 0] = pydrt.GEO_PLANE
    rows[:, 0] = head.reshape(-1).view("<f8")
    rows[flat, U.ROW_RADIUS] = 0.0
    rows[flat, U.ROW_NORMAL], rows[flat, U.ROW_U], rows[flat, U.ROW_V] = np.nan, FLAT_U, FLAT_V
    return U.with_rows(b, rows)


def few_spheres(n):
    """n spheres in the camera's view, every centre and radius its own"""
    return [("sphere", (2.5 * k - 1.25 * (n - 1), 0.75 * (k % 2) - 0.5, -5.0 - 1.5 * k), 1.0 + 0.125 * k) for k in range(n)]


def seeded_spheres(n, seed):
    rng = np.random.default_rng(seed)
    return [("sphere", tuple(rng.uniform((-8.0, -8.0, -24.0), (8.0, 8.0, -4.0))), float(rng.uniform(0.4, 1.2))) for _ in range(n)]


def flat_planes(n):
    return [("flat_plane", (-1.0 + 0.01 * k, -1.0, 0.0)) for k in range(n)]


LATTICE_SITES, LATTICE_PER_SITE = 1000, 5


def lattice_rows(rows, jitter=None):
    """the first 5000 rows as spheres on a 10 x 10 x 10 lattice in the camera's view, five to a site with different radii: sphere k sits
    on site k % 1000, so the five equal keys of a site come from five different tiles of the sort and only stability orders them"""
    n = LATTICE_SITES * LATTICE_PER_SITE
    site = np.arange(n) % LATTICE_SITES
    rows = rows.copy()
    rows[:n, U.ROW_POS] = np.stack([-9.0 + 2.0 * (site % 10), -9.0 + 2.0 * (site // 10 % 10), -28.0 + 2.0 * (site // 100)], axis=1)
    rows[:n, U.ROW_RADIUS] = 0.15 + 0.1 * (np.arange(n) // LATTICE_SITES)
    if jitter is not None:
        rows[:n, U.ROW_POS] += jitter.uniform(-0.9, 0.9, (n, 3))
    return rows


def _build(name):
    light = ("point_light", (5.0, 10.0, 10.0))  # never intersected: the tree holds the spheres and planes alone
    if name in ("coincident_300", "deep_64"):
        b = U.small_scene((coincident_spheres() if name == "coincident_300" else deep_spheres()) + [light])
        return U._case(b, b, pydrt.make_params(16, 16, spp=2, max_depth=3, seed=33), forced=True)
    if name in FEW:
        b = scene(few_spheres(FEW[name]) + [light])
        return U._case(b, b, pydrt.make_params(16, 16, **PARAMS_SMALL), forced=True)
    if name == "planes_first":  # the first wave of the bounds pass has no bounded lane
        b = scene(flat_planes(70) + seeded_spheres(200, 70) + [light])
        return U._case(b, b, pydrt.make_params(16, 16, **PARAMS_LARGE), bvh=True)
    if name == "planes_last_only_bounded":  # 133 tree surfaces: the three bounded ones in the last, partial wave
        b = scene(flat_planes(130) + few_spheres(3) + [light])
        return U._case(b, b, pydrt.make_params(16, 16, **PARAMS_LARGE), bvh=True)
    if name == "lattice_5000":  # "before": every sphere off its site
        base = pydrt.synthetic_sphere_scene(LATTICE_SITES * LATTICE_PER_SITE, 16, 16)
        rows = pydrt.surface_rows(base)
        before, after = U.with_rows(base, lattice_rows(rows, np.random.default_rng(5000))), U.with_rows(base, lattice_rows(rows))
        return U._case(before, after, pydrt.make_params(16, 16, **PARAMS_LARGE), bvh=True)
    n = SPHERES[name]
    b = pydrt.synthetic_sphere_scene(n, 16, 16)
    if name == "spheres_20000":  # (the generator's radii are for this many: most camera rays hit)
        return U._case(b, b, pydrt.make_params(16, 16, spp=1, max_depth=3, seed=33), bvh=True)
    rows = pydrt.surface_rows(b)
    rows[:n, U.ROW_RADIUS] *= 3.0
    b = U.with_rows(b, rows)
    rows = rows.copy()
    rng = np.random.default_rng(n)
    rows[:n, U.ROW_POS] += rng.uniform(-1.0, 1.0, (n, 3))
    rows[:n, U.ROW_RADIUS] *= rng.uniform(0.7, 1.3, n)
    return U._case(b, U.with_rows(b, rows), pydrt.make_params(16, 16, **PARAMS_LARGE), bvh=True)


FEW = {"three_spheres": 3, "four_spheres": 4, "five_spheres": 5}  # a root with a leaf and an inner child, and the two next sizes
SPHERES = {"spheres_1024": 1024, "spheres_2049": 2049, "spheres_4097": 4097, "spheres_20000": 20000}  # + the plane light: m = n + 1
OWN = ["coincident_300", "deep_64"] + list(FEW) + ["spheres_1024", "spheres_2049", "spheres_4097", "lattice_5000", "planes_first",
                                                   "planes_last_only_bounded", "spheres_20000"]
MULTI_TILE = ["spheres_4097", "lattice_5000"]  # the cases whose "before" and "after" differ: updates through a device-built tree
_own = {}


def load(name):
    """a case of scene_update_cases, or one of this file's own (OWN), built once. coincident_300, deep_64 and the three smallest are
    forced behind the tree; the others take it unforced. Their "before" and "after" are one scene except for MULTI_TILE."""
    if name not in OWN:
        return U.load(name)
    if name not in _own:
        _own[name] = _build(name)
    return _own[name]


def seeded_rays(name, n=4096):
    """scene_update_cases.seeded_rays on a case of either file"""
    return U.seeded_rays(load(name), n=n)


def sphere_rows(spheres):
    """raw surface rows of ("sphere", position, radius) tuples, for the rule alone (the material word stays 0)"""
    rows = np.zeros((len(spheres), pydrt.SURFACE_ROW))
    head = np.zeros(len(spheres), dtype=[("type", "<u4"), ("material", "<u4")])
    head["type"] = pydrt.GEO_SPHERE
    rows[:, 0] = head.view("<f8")
    for i, s in enumerate(spheres):
        rows[i, U.ROW_POS], rows[i, U.ROW_RADIUS] = s[1], s[2]
    return rows
