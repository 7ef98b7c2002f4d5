"""Scene updates (drt_set_camera, drt_update_surfaces): the cases of tests/test_scene_update_cpu.py and
tests/test_gpu_scene_update.py. A case is a scene before, the scene after -- the same surface count, types and materials, other
positions, radii, normals and edge vectors, or another camera -- and the params both are rendered with. What an updated context must
equal is a fresh context on the "after" bundle, so nothing here knows how an update works."""
import ctypes as C

import numpy as np

import cases
import pydrt

ROW_POS, ROW_RADIUS, ROW_NORMAL, ROW_U, ROW_V = slice(1, 4), 4, slice(5, 8), slice(8, 11), slice(11, 14)

_cases = {}


def with_rows(bundle, rows, camera=None):
    """a bundle that shares `bundle`'s materials and spectra and has surfaces of its own, made from raw rows"""
    sa = pydrt.surfaces_from_rows(rows)
    sc = pydrt.Scene()
    C.memmove(C.byref(sc), C.byref(bundle.scene), C.sizeof(pydrt.Scene))
    sc.surfaces = C.cast(sa, C.POINTER(pydrt.Surface))
    return pydrt.SceneBundle(sc, bundle.camera if camera is None else camera, keep=(sa, bundle))


def set_plane(rows, i, o, pu, pv):
    u, v, n = pydrt.plane_from_points(o, pu, pv)
    rows[i, ROW_POS], rows[i, ROW_NORMAL], rows[i, ROW_U], rows[i, ROW_V] = o, n, u, v


def _params(p, hits=True):
    q = pydrt.Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(pydrt.Params))
    q.batch_spp = 2
    if hits:
        q.flags = int(q.flags) | pydrt.FLAG_RECORD_HITS
    return q


def _case(before, after, params, bvh=False, forced=False):
    return {"before": before, "after": after, "params": _params(params), "bvh": bvh or forced, "forced": forced}


def small_scene(surfaces, width=16, height=16):
    """spheres and lights of the sphere scene's materials (pydrt.synthetic_sphere_scene) through its camera: surfaces are
    ("sphere", position, radius), ("plane_light", o, pu, pv) or ("point_light", position)"""
    base = pydrt.synthetic_sphere_scene(1, width, height)
    names = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), width, height).material_names()
    white, light = names.index("white_plastic"), names.index("light")
    rows = np.zeros((len(surfaces), pydrt.SURFACE_ROW))
    head = np.zeros(len(surfaces), dtype=[("type", "<u4"), ("material", "<u4")])
    for i, s in enumerate(surfaces):
        if s[0] == "sphere":
            head[i] = (pydrt.GEO_SPHERE, white)
            rows[i, ROW_POS], rows[i, ROW_RADIUS] = s[1], s[2]
        elif s[0] == "plane_light":
            head[i] = (pydrt.GEO_PLANE, light)
            set_plane(rows, i, *s[1:])
        else:
            head[i] = (pydrt.GEO_POINT, light)
            rows[i, ROW_POS] = s[1]
    rows[:, 0] = head.view("<f8")
    sc = pydrt.Scene()
    C.memmove(C.byref(sc), C.byref(base.scene), C.sizeof(pydrt.Scene))
    sa = pydrt.surfaces_from_rows(rows)
    sc.surfaces, sc.num_surfaces = C.cast(sa, C.POINTER(pydrt.Surface)), len(surfaces)
    return pydrt.SceneBundle(sc, base.camera, keep=(sa, base))


def sphere_camera(position, target, w, h):
    """the sphere scene's camera (pydrt.synthetic_sphere_scene) from another place"""
    return pydrt.init_camera(position, target, 0.0, 60.0, 6.0, 0.3, 0.0, w, h)


def _build(name):
    if name.startswith("cam_"):
        scene = name[4:]
        b, p = cases.load_case(scene)
        w, h = int(p.width), int(p.height)
        if scene == "plane_light_16":
            cam = pydrt.turntable_camera(b, w, h, 1, 8)
        elif scene == "lens":  # test_lens.scn: (0, 0, 8) -> (0, 0, 0), fov 90, fdepth 7, flength 0.3, aperture 0.05
            cam = pydrt.init_camera((0.5, 0.3, 8.0), (0.0, 0.0, 0.0), 0.0, 90.0, 6.0, 0.3, 0.08, w, h)
        else:
            cam = sphere_camera((5.0, 3.0, 28.0), (0.0, 0.0, -20.0), w, h)
        return _case(b, with_rows(b, pydrt.surface_rows(b), cam), p, bvh=scene == "spheres_1500")
    if name.startswith("lights_"):  # test_lights.scn: 2 the plane light, 3 the sphere light, 4 the point light
        forced = name.endswith("_bvh")
        which = name[7:].replace("_bvh", "")
        b, p = cases.load_case("lights")
        rows = pydrt.surface_rows(b)
        if which in ("plane", "all"):
            set_plane(rows, 2, (-0.5, 3.2, 1.2), (1.8, 3.2, 1.0), (-0.5, 3.4, -1.0))
        if which in ("sphere", "all"):
            rows[3, ROW_POS], rows[3, ROW_RADIUS] = (2.0, 0.8, 0.5), 0.55
        if which in ("point", "all"):
            rows[4, ROW_POS] = (-2.0, 1.5, 0.5)
        return _case(b, with_rows(b, rows), p, forced=forced)
    if name == "plane_light_16":  # cornell_plane_light.scn: 7 the slanted mirror plane, 5 the gold ball
        b, p = cases.load_case(name)
        rows = pydrt.surface_rows(b)
        set_plane(rows, 7, (-1.2, 1.0, -2.2), (-1.0, -1.0, -2.8), (0.9, 1.1, -2.6))
        rows[5, ROW_POS], rows[5, ROW_RADIUS] = (1.5, -2.0, 0.0), 0.9
        return _case(b, with_rows(b, rows), p)
    if name == "many_lights":  # test_many_lights.scn: 3 the sphere light, 4 .. 14 the eleven plane lights
        b, p = cases.load_case(name)
        rows = pydrt.surface_rows(b)
        rows[3, ROW_POS] += (0.3, 0.2, -0.4)
        rows[3, ROW_RADIUS] = 0.35
        for i in range(4, 15):
            rows[i, ROW_POS] += (0.1, -0.05 - 0.01 * i, 0.2)
            rows[i, ROW_U] *= 1.0 + 0.02 * i
        return _case(b, with_rows(b, rows), p)
    if name == "spheres_1500":
        b, p = cases.load_case(name)
        rows = pydrt.surface_rows(b)
        rng = np.random.default_rng(1500)
        rows[:1500, ROW_POS] += rng.uniform(-1.0, 1.0, (1500, 3))
        rows[:1500, ROW_RADIUS] *= rng.uniform(0.7, 1.6, 1500)
        return _case(b, with_rows(b, rows), p, bvh=True)
    if name == "spheres_1500_far":  # one sphere and the camera at 16 times the extent the context was made for
        b, p = cases.load_case("spheres_1500")
        rows = pydrt.surface_rows(b)
        rows[0, ROW_POS], rows[0, ROW_RADIUS] = (640.0, 0.0, -10.0), 4.0
        cam = sphere_camera((640.0, 0.0, 30.0), (640.0, 0.0, -20.0), int(p.width), int(p.height))
        return _case(b, with_rows(b, rows, cam), p, bvh=True)
    if name in ("one_sphere", "two_surfaces", "spheres_96"):
        p = pydrt.make_params(16, 16, spp=3, max_depth=4, seed=21)
        if name == "one_sphere":  # a root with one child: the point light is never intersected
            b = small_scene([("sphere", (0.0, 0.0, -5.0), 3.0), ("point_light", (5.0, 10.0, 10.0))])
            a = small_scene([("sphere", (1.0, 0.5, -6.0), 2.5), ("point_light", (-4.0, 9.0, 12.0))])
            return _case(b, a, p, forced=True)
        if name == "two_surfaces":
            light = ("plane_light", (-5.0, 25.0, 5.0), (5.0, 25.0, 5.0), (-5.0, 25.0, -5.0))
            b = small_scene([("sphere", (0.0, 0.0, -5.0), 3.0), light])
            a = small_scene([("sphere", (-1.0, 1.5, -4.0), 3.5), ("plane_light", (-4.0, 20.0, 6.0), (6.0, 21.0, 5.0), (-4.0, 20.0, -5.0))])
            return _case(b, a, p, forced=True)
        b = pydrt.synthetic_sphere_scene(96, 16, 16)  # 96 spheres + the plane light: the smallest scene that takes the tree unforced
        rows = pydrt.surface_rows(b)
        rows[:96, ROW_RADIUS] *= 12.0  # (the generator's radii are for thousands of spheres)
        b = with_rows(b, rows)
        rows = rows.copy()
        rng = np.random.default_rng(96)
        rows[:96, ROW_POS] += rng.uniform(-3.0, 3.0, (96, 3))
        rows[:96, ROW_RADIUS] *= rng.uniform(0.7, 1.3, 96)
        return _case(b, with_rows(b, rows), p, bvh=True)
    if name == "parallel_edges":  # cases.degenerate_scenes(): the last plane's edges are parallel AFTER the update (the unbounded box)
        a = pydrt.load_scene_text(cases.degenerate_scenes()["plane_with_parallel_edges"], 16, 16)
        p = pydrt.make_params(16, 16, spp=2, max_depth=4, seed=11)
        rows = pydrt.surface_rows(a)
        last = rows.shape[0] - 1
        set_plane(rows, last, (-1.0, -1.0, 0.0), (0.0, -1.0, 0.0), (-1.0, 0.5, 0.5))
        return _case(with_rows(a, rows), a, p, forced=True)
    raise KeyError(name)


CAMERA = ["cam_plane_light_16", "cam_lens", "cam_spheres_1500"]
LDS_SURFACES = ["lights_plane", "lights_sphere", "lights_point", "lights_all", "plane_light_16", "many_lights"]
BVH_SURFACES = ["spheres_1500", "lights_all_bvh", "one_sphere", "two_surfaces", "spheres_96", "parallel_edges"]
SAME_LOG = ["lights_point"]  # the one case whose hit log cannot differ
ALL = CAMERA + LDS_SURFACES + BVH_SURFACES + ["spheres_1500_far"]


def load(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def seeded_rays(name, n=4096, seed=7, centre=None):
    """(origins, dirs, p0, p1) of n rays and n pairs, seeded: origins and points in a box around `centre` (default: where the
    "after" surfaces have their anchor points), unit directions. `name` may be a case itself (tests/hierarchy_cases.py has its own)."""
    c = load(name) if isinstance(name, str) else name
    rows = pydrt.surface_rows(c["after"])
    pos = rows[:, ROW_POS]
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    if centre is not None:
        lo, hi = np.asarray(centre) - 30.0, np.asarray(centre) + 30.0
    rng = np.random.default_rng(seed)
    ro = rng.uniform(lo, hi, (n, 3))
    rd = rng.normal(size=(n, 3))
    rd /= np.sqrt((rd * rd).sum(axis=1))[:, None]
    p0, p1 = rng.uniform(lo, hi, (n, 3)), rng.uniform(lo, hi, (n, 3))
    p1[: n // 2] = p0[: n // 2] + rng.normal(size=(n // 2, 3)) * 1.5  # near pairs: half of them see each other
    return ro, rd, p0, p1
