"""The inputs of the ray-query tests (drt_cast_rays, drt_test_visibility, drt_cast_pixels) and what the oracle
answers to them. Not a test file: tests/test_ray_query_cpu.py checks with the oracle alone that these inputs are worth running, and
tests/test_gpu_ray_query.py runs them on the device. Everything here is computed once per scene and handed out unchanged.

Per scene, the rays are
  (a) the camera rays of all pixels for samples 0 and 1, restated as tests/feature_rule.py restates them;
  (b) second-generation rays from the oracle's hit positions of (a): the mirror direction about the hit normal, and seeded random
      unit directions;
  (c) rays with one and with two exact-zero direction components, from points inside the scene's bounds;
  (d) one each of: a NaN direction, a zero direction, an infinite origin, a ray that starts exactly on a surface;
  (e) `scaled`, directions that are not of unit length: every second ray of (b) (all of them, five times over, take the closed scene
      deg_camera_inside_the_glass_ball below the 10 % of misses the CPU test asserts) and rays that graze the scene's spheres, each with d
      multiplied by 0.5, 2, 1 + 2^-20, 1e-3 and 1e3, and the unnormalised directions `light point - hit position`. The rule
      (line_sphere_intersection sets a = 1 whatever |d| is) does not give such a ray the answer of its normalised ray: a grazing ray
      passes its sphere outside by a quarter of what the factor 1 + 2^-20 adds to the discriminant, or inside by as much, so a longer
      d hits a sphere the unit ray misses and a shorter one misses a sphere it hits. "Normalise first" is not a passing
      implementation; tests/test_ray_query_cpu.py asserts that per factor, in every scene that has a sphere (a plane's answer does
      not depend on |d|);
and the visibility pairs are (hit position, a point on each light), (hit position, the hit position of another pixel), p0 == p1,
pairs whose segment ends exactly on a surface (the camera ray's origin and its own hit position), neighbours a step apart and
segments that leave the scene's bounds. The last two and the `away` probe rays (from a shell around the scene, pointing outward) keep
every scene's mix inside the bounds the CPU test asserts.

The one condition of the bitwise comparisons: a division whose quotient is subnormal may be one unit off on
the device. subnormal_quotients() counts them -- the plane intersector's l = (p - o).n / d.n for every ray and plane, restated, and
the components of every normalised vector the oracle hands back -- and the CPU test asserts that there are none."""
import ctypes as C

import numpy as np

import cases
import feature_rule as F
import fuzz_scenes
import oracle_py as O
import pydrt

VIS_FUDGE = np.float64(0.0001)  # src/daily_ray_trace.c:237
_TINY = np.finfo(np.float64).tiny
_f64p = C.POINTER(C.c_double)

LDS_SCENES = ["plane_light_16", "lights", "lens", "gold_mirror"]
DEGENERATE = sorted(cases.degenerate_scenes())
FUZZ_SEEDS = [3, 17, 101]  # 101: a "crowded" seed, more than 96 surfaces, behind the hierarchy
FUZZ_SCENES = ["fuzz_%d" % s for s in FUZZ_SEEDS]
# (scene, forced behind the hierarchy)
ALL_SCENES = ([(n, False) for n in LDS_SCENES] + [("spheres_1500", False)] + [("deg_" + n, False) for n in DEGENERATE]
              + [("deg_" + n, True) for n in DEGENERATE] + [(n, False) for n in FUZZ_SCENES] + [(n, True) for n in FUZZ_SCENES if n != "fuzz_101"])
SCENE_NAMES = sorted({n for n, _ in ALL_SCENES})

# Scenes exempt from the "at least 10 % of the rays miss" bound because they are closed rooms: none. The rooms built on
# cornell_plane_light.scn and cornell_gold_mirror.scn let no ray from inside escape, but the `away` probe rays start outside them,
# so every scene meets the bound.
CLOSED_ROOMS = frozenset()

SCALE_FACTORS = (0.5, 2.0, 1.0 + 2.0 ** -20, 1e-3, 1e3)

_loaded, _sets, _expected = {}, {}, {}


def load(name):
    """(bundle, params) of a scene by name, loaded once"""
    if name not in _loaded:
        if name.startswith("deg_"):
            bundle = pydrt.load_scene_text(cases.degenerate_scenes()[name[4:]], 16, 16)
            params = pydrt.make_params(16, 16, spp=2, max_depth=4, seed=11)
        elif name.startswith("fuzz_"):
            bundle, params = fuzz_scenes.load(int(name[5:]), pydrt)
        else:
            bundle, params = cases.load_case(name)
        _loaded[name] = (bundle, params)
    return _loaded[name]


def camera_rays(name, samples=(0, 1)):
    """(xy [n][2] uint32, sample [n] uint32, origins, dirs): all pixels of the image for each of `samples`, restated"""
    bundle, params = load(name)
    w, h = int(params.width), int(params.height)
    x = np.tile(np.tile(np.arange(w), h), len(samples))
    y = np.tile(np.repeat(np.arange(h), w), len(samples))
    s = np.repeat(np.asarray(samples), w * h)
    px, py, disc = F.sample_draws(bundle, params, x, y, s)
    ro, rd = F.camera_rays(bundle, x, y, px, py, disc)
    return np.stack([x, y], axis=1).astype(np.uint32), s.astype(np.uint32), np.ascontiguousarray(ro), np.ascontiguousarray(rd)


def oracle_hits(bundle, ro, rd):
    """drt_oracle_find_ray_intersection of every ray, DEVICE arithmetic, as a pydrt.RAY_HIT_DTYPE record array. distance is left 0:
    the oracle's scene_point carries none (oracle_distances gives it)."""
    L = O.oracle_lib()
    O.set_math_mode(O.MATH_DEVICE)
    ro, rd = np.ascontiguousarray(ro, dtype=np.float64), np.ascontiguousarray(rd, dtype=np.float64)
    out = np.zeros(ro.shape[0], dtype=pydrt.RAY_HIT_DTYPE)
    pt = O.Point()
    for k in range(ro.shape[0]):
        idx = L.drt_oracle_find_ray_intersection(C.byref(bundle.scene), ro[k].ctypes.data_as(_f64p), rd[k].ctypes.data_as(_f64p), C.byref(pt))
        h = out[k]
        h["index"] = idx
        h["surface_material"] = pt.surface_material
        if idx >= 0:
            h["position"], h["normal"], h["out"] = list(pt.position), list(pt.normal), list(pt.out)
            h["on_dot"] = pt.on_dot
            h["incident_material"], h["transmit_material"] = pt.incident_material, pt.transmit_material
    return out


def moved_origins(ro, rd):
    """o + d * vis_fudge (src/daily_ray_trace.c:339): one multiplication, one addition"""
    with np.errstate(all="ignore"):
        return ro + rd * VIS_FUDGE


def oracle_distances(bundle, ro, rd, index):
    """drt_oracle_line_sphere / drt_oracle_line_plane of each ray's hit surface from the moved origin; 0 for a miss"""
    L = O.oracle_lib()
    O.set_math_mode(O.MATH_DEVICE)
    mo = np.ascontiguousarray(moved_origins(ro, rd))
    rd = np.ascontiguousarray(rd)
    dist = np.zeros(len(index))
    p = lambda a: (C.c_double * 3)(*list(a))
    for k, i in enumerate(index):
        if i < 0:
            continue
        s = bundle.scene.surfaces[int(i)]
        o, d = mo[k].ctypes.data_as(_f64p), rd[k].ctypes.data_as(_f64p)
        if int(s.type) == pydrt.GEO_SPHERE:
            dist[k] = L.drt_oracle_line_sphere(o, d, p(s.position), float(s.radius))
        else:
            dist[k] = L.drt_oracle_line_plane(o, d, p(s.position), p(s.normal), p(s.u), p(s.v))
    return dist


def oracle_visible(bundle, p0, p1):
    L = O.oracle_lib()
    O.set_math_mode(O.MATH_DEVICE)
    p0, p1 = np.ascontiguousarray(p0, dtype=np.float64), np.ascontiguousarray(p1, dtype=np.float64)
    out = np.zeros(p0.shape[0], dtype=np.uint8)
    for k in range(p0.shape[0]):
        out[k] = 1 if L.drt_oracle_points_mutually_visible(C.byref(bundle.scene), p0[k].ctypes.data_as(_f64p), p1[k].ctypes.data_as(_f64p)) else 0
    return out


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def _bounds(bundle):
    """a box inside which the scene's surfaces have their anchor points, shrunk a little: origins for (c)"""
    sc = bundle.scene
    pos = np.array([list(sc.surfaces[i].position) for i in range(int(sc.num_surfaces))])
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    lo, hi = np.maximum(lo, -4.0), np.minimum(hi, 4.0)  # (the far sphere of huge_and_tiny_spheres is not where the scene is)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2 * 0.9, 0.5)
    return mid - half, mid + half


def _light_points(bundle, rng):
    """one point on (or, for a sphere, just outside) every emissive surface"""
    sc = bundle.scene
    pts = []
    for i in range(int(sc.num_surfaces)):
        s = sc.surfaces[i]
        if not int(sc.materials[int(s.material)].is_emissive):
            continue
        p = np.array(list(s.position))
        if int(s.type) == pydrt.GEO_PLANE:
            a, b = rng.uniform(0.2, 0.8, 2)
            p = p + a * np.array(list(s.u)) + b * np.array(list(s.v))
        elif int(s.type) == pydrt.GEO_SPHERE:
            p = p + _unit(rng, 1)[0] * (abs(float(s.radius)) + 1e-3)
        pts.append(p)
    return np.array(pts).reshape(-1, 3)


def spheres_of(bundle):
    sc = bundle.scene
    return [sc.surfaces[i] for i in range(int(sc.num_surfaces)) if int(sc.surfaces[i].type) == pydrt.GEO_SPHERE]


def _grazing(bundle, rng, per_sphere=8, most=8):
    """unit rays along tangents of up to `most` spheres, from 0.5 to 2 radii before the tangent point, moved outward (even rays) or
    inward (odd rays) by 2^-22 t^2 / r: a quarter of the 2^-19 t^2 that |d| = 1 + 2^-20 adds to the rule's discriminant / 4"""
    sph = [s for s in spheres_of(bundle) if 1e-6 < abs(float(s.radius)) < 1e3]
    sph = sph[:: max(1, len(sph) // most)][:most]
    o, d = [], []
    for s in sph:
        c, r = np.array(list(s.position)), abs(float(s.radius))
        nrm = _unit(rng, per_sphere)
        u = np.cross(nrm, _unit(rng, per_sphere))
        u /= np.sqrt((u * u).sum(axis=1))[:, None]
        t = rng.uniform(0.5, 2.0, per_sphere) * r
        off = np.where(np.arange(per_sphere) % 2 == 0, 1.0, -1.0) * 2.0 ** -22 * t * t / r
        o.append(c + (r + off)[:, None] * nrm - t[:, None] * u)
        d.append(u)
    return (np.concatenate(o), np.concatenate(d)) if o else (np.zeros((0, 3)), np.zeros((0, 3)))


def ray_sets(name):
    """{"rays": (origins, dirs), "parts": {set name: slice}, "pairs": (p0, p1), "pair_parts": {...}, "camera": (xy, samples),
    "scaled": (base origins, base unit dirs, factor of every ray of the part `scaled`; 0 = an unnormalised light direction)}"""
    if name in _sets:
        return _sets[name]
    bundle, params = load(name)
    rng = np.random.default_rng(0x5EED + sum(map(ord, name)))
    xy, smp, co, cd = camera_rays(name)
    cam_hits = oracle_hits(bundle, co, cd)
    hit = np.flatnonzero(cam_hits["index"] >= 0)
    parts, O_, D_ = {}, [], []

    def add(label, o, d):
        o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
        start = sum(len(a) for a in O_)
        O_.append(o)
        D_.append(d)
        parts[label] = slice(start, start + len(o))

    add("camera", co, cd)
    take = hit[:: max(1, len(hit) // 192)][:192] if len(hit) else hit
    if len(take):
        p, n, d = cam_hits["position"][take], cam_hits["normal"][take], cd[take]
        add("mirror", p, d - 2.0 * (d * n).sum(axis=1)[:, None] * n)
        add("random", np.repeat(p, 2, axis=0), _unit(rng, 2 * len(take)))
    lo, hi = _bounds(bundle)
    inside = rng.uniform(lo, hi, size=(96, 3))
    d1 = _unit(rng, 48)
    d1[np.arange(48), rng.integers(0, 3, 48)] = 0.0
    d2 = np.zeros((48, 3))
    d2[np.arange(48), rng.integers(0, 3, 48)] = rng.choice([-1.0, 1.0], 48)
    add("one_zero", inside[:48], d1)
    add("two_zeros", inside[48:], d2)
    # probe rays that start on a shell around the scene and point away from it: they miss whatever the scene is
    centre = (lo + hi) / 2
    n_away = max(64, sum(len(a) for a in O_) // 6)
    away = _unit(rng, n_away)
    add("away", centre + away * (3.0 * np.sqrt(((hi - lo) ** 2).sum())), away)
    on_surface = cam_hits["position"][hit[0]] if len(hit) else centre
    on_normal = cam_hits["normal"][hit[0]] if len(hit) else np.array([0.0, 1.0, 0.0])
    add("special", [centre, centre, [np.inf, 0.0, 0.0], on_surface],
        [[np.nan, 0.0, 1.0], [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0], on_normal])
    # (e): after every other part, whose places in the list the other tests rely on
    rng_e = np.random.default_rng(0xE5CA + sum(map(ord, name)))  # its own stream: the draws of the other parts stay what they were
    lights = _light_points(bundle, rng_e)
    so, sd = _grazing(bundle, rng_e)
    if len(take):
        so = np.concatenate([so, O_[1][::2], O_[2][::2]])
        sd = np.concatenate([sd, D_[1][::2], D_[2][::2]])
    lo_, ld_ = np.zeros((0, 3)), np.zeros((0, 3))
    if len(take) and len(lights):
        lo_ = np.concatenate([cam_hits["position"][take][k::2] for k in range(min(2, len(lights)))])
        ld_ = np.concatenate([lights[k] - cam_hits["position"][take][k::2] for k in range(min(2, len(lights)))])
    with np.errstate(all="ignore"):
        ln_ = np.sqrt((ld_ * ld_).sum(axis=1))[:, None]
        scaled = (np.concatenate([so] * len(SCALE_FACTORS) + [lo_]), np.concatenate([sd] * len(SCALE_FACTORS) + [ld_ / ln_]),
                  np.concatenate([np.repeat(np.array(SCALE_FACTORS), len(so)), np.zeros(len(lo_))]))
    add("scaled", scaled[0], np.concatenate([sd * f for f in SCALE_FACTORS] + [ld_]))
    origins, dirs = np.ascontiguousarray(np.concatenate(O_)), np.ascontiguousarray(np.concatenate(D_))

    pair_parts, P0, P1 = {}, [], []

    def add_pairs(label, a, b):
        a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
        start = sum(len(x) for x in P0)
        P0.append(a)
        P1.append(b)
        pair_parts[label] = slice(start, start + len(a))

    pos = cam_hits["position"][take] if len(take) else inside[:8]
    lights = _light_points(bundle, rng)
    for k in range(len(lights)):
        add_pairs("light_%d" % k, pos, np.tile(lights[k], (len(pos), 1)))
    add_pairs("other_pixel", pos, np.roll(pos, len(pos) // 3 + 1, axis=0))
    add_pairs("inside", inside[:64], inside[32:96])
    add_pairs("same_point", pos[:4], pos[:4])
    add_pairs("ends_on_a_surface", co[take] if len(take) else inside[:8], pos)
    # neighbours a step apart (mostly visible) and segments that leave the scene's bounds (occluded wherever there is a wall)
    m = max(32, sum(len(a) for a in P0) // 5)
    base = rng.uniform(lo, hi, size=(m, 3))
    add_pairs("a_step_apart", base, base + _unit(rng, m) * 0.05)
    add_pairs("out_of_bounds", base, centre + _unit(rng, m) * (3.0 * np.sqrt(((hi - lo) ** 2).sum())))
    _sets[name] = {"rays": (origins, dirs), "parts": parts, "pairs": (np.ascontiguousarray(np.concatenate(P0)), np.ascontiguousarray(np.concatenate(P1))),
                   "pair_parts": pair_parts, "camera": (xy, smp), "scaled": scaled}
    return _sets[name]


def expected(name):
    """{"hits": oracle record array with distance filled in, "visible": uint8} of ray_sets(name)"""
    if name not in _expected:
        bundle, _ = load(name)
        s = ray_sets(name)
        ro, rd = s["rays"]
        hits = oracle_hits(bundle, ro, rd)
        hits["distance"] = oracle_distances(bundle, ro, rd, hits["index"])
        _expected[name] = {"hits": hits, "visible": oracle_visible(bundle, *s["pairs"])}
    return _expected[name]


def _subnormal(q):
    q = np.asarray(q)
    return int(np.count_nonzero((q != 0.0) & (np.abs(q) < _TINY)))


def subnormal_quotients(name):
    """Quotients of the set that are subnormal and not zero: the plane intersector's l of every (ray, plane) and (pair, plane), and
    every component of the normals and normalised directions involved."""
    s = ray_sets(name)
    return subnormal_quotients_of(load(name)[0], *s["rays"], *s["pairs"], expected(name)["hits"]["normal"])


def subnormal_quotients_of(bundle, ro, rd, p0, p1, normals):
    """the same count for any rays and pairs on a scene (`normals`: the oracle's hit normals of the rays)"""
    sc = bundle.scene
    planes = [sc.surfaces[i] for i in range(int(sc.num_surfaces)) if int(sc.surfaces[i].type) == pydrt.GEO_PLANE]
    pp = np.array([list(p.position) for p in planes]).reshape(-1, 3)
    pn = np.array([list(p.normal) for p in planes]).reshape(-1, 3)
    count = 0
    with np.errstate(all="ignore"):
        diff = p1 - p0
        ln = np.sqrt((diff * diff).sum(axis=1))
        vd = diff / ln[:, None]
        count += _subnormal(vd)
        for o, d in ((moved_origins(ro, rd), rd), (p0 + vd * VIS_FUDGE, vd)):
            for k in range(len(planes)):
                dn = d[:, 0] * pn[k, 0] + d[:, 1] * pn[k, 1] + d[:, 2] * pn[k, 2]
                t = pp[k][None, :] - o
                num = t[:, 0] * pn[k, 0] + t[:, 1] * pn[k, 1] + t[:, 2] * pn[k, 2]
                count += _subnormal(np.where(dn != 0.0, num / dn, 0.0))
    count += _subnormal(normals)
    return count
