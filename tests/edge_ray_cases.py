"""Edge-ray tables: ray films (drt_bind_rays) whose first rays are built from a scene's own coordinates, so
that the path kernels' scans meet the ties camera rays never do -- first hits exactly on a rectangle's edge or corner, rays inside a
wall's plane (d.n == 0), spheres touched with a discriminant of exactly 0, origins on a surface, points where a point light sits.
Not a test file: tests/test_edge_rays_cpu.py checks with the oracle alone (and with the compiled reference's recorded answers,
tests/golden/edge_rays.npz) that the tables are worth running, tests/test_gpu_edge_rays.py runs them on the device.

lattice_coords(bundle): per axis, the sorted set of the coordinates of every surface's anchor point, every rectangle's four corners
and every sphere's centre and centre +- radius, finite and with |x| < 100.

Ray families, each (origins, dirs) with directions that are exactly +- a unit axis vector:
  through       for each axis and each pair of lattice coordinates on the other two axes, four rays along the axis: from
                0.25 lo + 0.75 hi - 0.0625 (lo, hi: the axis's smallest and largest lattice coordinate) both ways, from hi + 5 going
                down and from lo - 5 going up. At most THROUGH_CAP.
  from_lattice  origins at lattice triples, in the six axis directions. At most LATTICE_CAP.
  borrowed      parts of ray_query_cases.ray_sets(name)["rays"]: mirror, random, one_zero, two_zeros, special and the grazing rays
                before they are scaled -- rays that are not axis-parallel, and the NaN, zero and infinite specials. A context behind
                the hierarchy takes a host table only with |d.d - 1| <= 2^-42 for finite, nonzero directions (RAY_UNIT_TOLERANCE), so
                the one_zero directions, which ray_query_cases leaves shorter than 1 after it zeroes a component, are divided by their
                length here (the zero stays an exact zero), and whatever is still outside the tolerance is left out.
A family above its cap is cut by a seeded choice without replacement, kept in generation order.

table(name, order) packs the three families into a 32-wide image, padded to whole 64-pixel waves with rays that certainly miss (far
outside every scene, pointing away). order "grouped" keeps generation order, so a wave's lanes are alike; "mixed" applies one seeded
permutation, so that every wave holds hits and misses, planes and spheres, and the specials (the first seed of 0, 1, 2 ... under which
every 64-pixel run has a hit and a miss; the CPU test asserts the property).

The ground truth is the oracle rendering from the same table (oracle_py.ray_table), spp 3, max_depth 4, FILM_SAMPLE_CENTER, the hit
log on, the scene's own seed: expected() with the device's power (needs a GPU), expected_cpu() with glibc's."""
import numpy as np

import cases
import oracle_py as O
import pydrt
import ray_query_cases as RQ

WIDTH, WAVE = 32, 64
SPP, MAX_DEPTH = 3, 4
THROUGH_CAP, LATTICE_CAP = 2048, 1024
COORD_BOUND = 100.0
UNIT_TOLERANCE = 2.0 ** -42  # RAY_UNIT_TOLERANCE (csrc/drt_kernels.h)
AXES = np.eye(3)

SHIPPED = ["plane_light_16", "lights", "gold_mirror", "many_lights", "grid_2p5nm", "spheres_1500"]
DEGENERATE = ["deg_" + n for n in sorted(cases.degenerate_scenes())]
FUZZ = ["fuzz_3", "fuzz_17", "fuzz_101"]
SCENES = SHIPPED + DEGENERATE + FUZZ
ALWAYS_BVH = ("spheres_1500", "fuzz_101")  # more surfaces than the LDS tables hold
# built on cornell_plane_light.scn: the premises the CPU test counts hold for these
CORNELL = ["plane_light_16", "grid_2p5nm"] + DEGENERATE
# the scenes whose rays and reference answers tests/golden/edge_rays.npz records (oracle/make_golden.py, gen_edge_rays)
FIXTURE_SCENES = ["plane_light_16", "lights", "deg_awkward_lights", "deg_coincident_surfaces", "deg_zero_and_negative_radius", "fuzz_3"]
ORDERS = ("grouped", "mixed")

_coords, _families, _tables, _first, _device, _cpu = {}, {}, {}, {}, {}, {}


def load(name):
    """(bundle, the scene's own params) by name, loaded once (ray_query_cases' loader: shipped cases, deg_*, fuzz_*)"""
    return RQ.load(name)


def _readonly(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def lattice_coords(bundle):
    """three sorted arrays of coordinates, one per axis"""
    sc = bundle.scene
    pts = []
    for i in range(int(sc.num_surfaces)):
        s = sc.surfaces[i]
        p = np.array(list(s.position))
        pts.append(p)
        if int(s.type) == pydrt.GEO_PLANE:
            u, v = np.array(list(s.u)), np.array(list(s.v))
            pts += [p + u, p + v, (p + u) + v]
        elif int(s.type) == pydrt.GEO_SPHERE:
            r = float(s.radius)
            pts += [p + r, p - r]
    pts = np.array(pts).reshape(-1, 3)
    out = []
    for a in range(3):
        c = pts[:, a]
        out.append(np.unique(c[np.isfinite(c) & (np.abs(c) < COORD_BOUND)]) + 0.0)  # (+ 0.0: no negative zero)
    return out


def _seed(name, salt):
    return [salt, sum(map(ord, name)), len(name)]


def _capped(total, cap, name, salt):
    """the indices in generation order of at most `cap` of `total` rays"""
    if total <= cap:
        return np.arange(total, dtype=np.int64)
    return np.sort(np.random.default_rng(_seed(name, salt)).choice(total, cap, replace=False)).astype(np.int64)


def through(name):
    xs = lattice_coords(load(name)[0])
    n = [len(x) for x in xs]
    per_axis = [4 * n[(a + 1) % 3] * n[(a + 2) % 3] for a in range(3)]
    start = np.concatenate([[0], np.cumsum(per_axis)])
    idx = _capped(int(start[3]), THROUGH_CAP, name, 0xED6E)
    o, d = np.zeros((len(idx), 3)), np.zeros((len(idx), 3))
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        k = idx[(idx >= start[a]) & (idx < start[a + 1])] - start[a]
        rows = np.flatnonzero((idx >= start[a]) & (idx < start[a + 1]))
        pair, which = k // 4, k % 4
        lo, hi = xs[a][0], xs[a][-1]
        inside = 0.25 * lo + 0.75 * hi - 0.0625
        o[rows, b], o[rows, c] = xs[b][pair // n[c]], xs[c][pair % n[c]]
        o[rows, a] = np.choose(which, [inside, inside, hi + 5.0, lo - 5.0])
        d[rows, a] = np.choose(which, [1.0, -1.0, -1.0, 1.0])
    return o, d


def from_lattice(name):
    xs = lattice_coords(load(name)[0])
    n = [len(x) for x in xs]
    idx = _capped(6 * n[0] * n[1] * n[2], LATTICE_CAP, name, 0x1A77)
    point, which = idx // 6, idx % 6
    o = np.stack([xs[0][point // (n[1] * n[2])], xs[1][(point // n[2]) % n[1]], xs[2][point % n[2]]], axis=1)
    d = AXES[which // 2] * np.where(which % 2 == 0, 1.0, -1.0)[:, None] + 0.0
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def _dot(a, b):
    """v_dot's order of operations (tests/test_gpu_plane_limited.py)"""
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def hierarchy_takes(d):
    """what host-mode drt_bind_rays takes behind the hierarchy: zero, NaN and infinite directions, and |d.d - 1| <= 2^-42"""
    with np.errstate(all="ignore"):
        finite = np.isfinite(d).all(axis=1)
        zero = (d == 0.0).all(axis=1)
        return ~finite | zero | (np.abs(_dot(d, d) - 1.0) <= UNIT_TOLERANCE)


def borrowed(name):
    s = RQ.ray_sets(name)
    ro, rd = s["rays"]
    parts = s["parts"]
    o, d = [], []
    for label in ("mirror", "random", "one_zero", "two_zeros", "special"):
        if label not in parts:
            continue
        po, pd = ro[parts[label]], rd[parts[label]]
        if label == "one_zero":
            pd = pd / np.sqrt(_dot(pd, pd))[:, None]
        o.append(po)
        d.append(pd)
    # the grazing rays stand first in every factor's block of `scaled`, before every second mirror and random ray
    base_o, base_d, factor = s["scaled"]
    block = int(np.count_nonzero(factor == RQ.SCALE_FACTORS[0]))
    halves = sum(-(-(parts[label].stop - parts[label].start) // 2) for label in ("mirror", "random") if label in parts)
    o.append(base_o[:block - halves])
    d.append(base_d[:block - halves])
    o, d = np.concatenate(o), np.concatenate(d)
    keep = hierarchy_takes(d)
    return np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep])


def families(name):
    """{"through": (o, d), "from_lattice": (o, d), "borrowed": (o, d)}, made once, read-only"""
    if name not in _families:
        _families[name] = {k: _readonly(*f(name)) for k, f in (("through", through), ("from_lattice", from_lattice), ("borrowed", borrowed))}
    return _families[name]


def lattice_rays(name):
    """through + from_lattice as one (origins, dirs): the rays the fixture records and the query kernels are given"""
    f = families(name)
    return _readonly(np.concatenate([f["through"][0], f["from_lattice"][0]]), np.concatenate([f["through"][1], f["from_lattice"][1]]))


def first_hit_indices(name, ro, rd):
    """the oracle's first-hit index of every ray (DEVICE arithmetic)"""
    return RQ.oracle_hits(load(name)[0], ro, rd)["index"]


def _generation_order(name):
    """(origins [n][3], dirs [n][3], family of every ray) with the padding: n is a multiple of 64"""
    if name not in _first:
        f = families(name)
        o = np.concatenate([f[k][0] for k in ("through", "from_lattice", "borrowed")])
        d = np.concatenate([f[k][1] for k in ("through", "from_lattice", "borrowed")])
        fam = np.concatenate([np.full(len(f[k][0]), i) for i, k in enumerate(("through", "from_lattice", "borrowed"))])
        pad = -len(o) % WAVE
        o = np.concatenate([o, np.tile([1000.0, 1000.0, 1000.0], (pad, 1))])
        d = np.concatenate([d, np.tile([0.0, 0.0, 1.0], (pad, 1))])
        fam = np.concatenate([fam, np.full(pad, 3)])
        _first[name] = _readonly(np.ascontiguousarray(o), np.ascontiguousarray(d), fam, first_hit_indices(name, o, d))
    return _first[name]


def mixed_permutation(name):
    o, d, fam, first = _generation_order(name)
    hit = first >= 0
    for seed in range(64):
        perm = np.random.default_rng(_seed(name, 0x3117 + seed)).permutation(len(o))
        runs = hit[perm].reshape(-1, WAVE)
        if runs.any(axis=1).all() and (~runs).any(axis=1).all():
            return perm
    raise AssertionError(name + ": no permutation of 64 seeds gives every wave a hit and a miss")


def table(name, order):
    """{"origins" [h][32][3], "dirs", "family" [h * 32] (0 through, 1 from_lattice, 2 borrowed, 3 padding), "first" [h * 32]: the
    oracle's first-hit index of every pixel's ray, "params"}, made once, read-only"""
    key = (name, order)
    if key not in _tables:
        assert order in ORDERS
        o, d, fam, first = _generation_order(name)
        if order == "mixed":
            perm = mixed_permutation(name)
            o, d, fam, first = o[perm], d[perm], fam[perm], first[perm]
        h = len(o) // WIDTH
        o, d, fam, first = _readonly(np.ascontiguousarray(o.reshape(h, WIDTH, 3)), np.ascontiguousarray(d.reshape(h, WIDTH, 3)),
                                     np.ascontiguousarray(fam), np.ascontiguousarray(first))
        params = pydrt.make_params(WIDTH, h, spp=SPP, max_depth=MAX_DEPTH, seed=int(load(name)[1].seed),
                                   pixel_scheme=pydrt.FILM_SAMPLE_CENTER, flags=pydrt.FLAG_RECORD_HITS)
        _tables[key] = {"origins": o, "dirs": d, "family": fam, "first": first, "params": params}
    return _tables[key]


def params_of(name, order, **changes):
    """a copy of the table's params with some fields changed"""
    p = pydrt.Params.from_buffer_copy(table(name, order)["params"])
    for k, v in changes.items():
        setattr(p, k, v)
    return p


def _expected(cache, render, name, order, changes):
    key = (name, order, tuple(sorted(changes.items())))
    if key not in cache:
        t = table(name, order)
        with O.ray_table(t["origins"], t["dirs"]):
            px, av, va, hits, st = render(load(name)[0], params_of(name, order, **changes))
        _readonly(px, av, va, hits)
        cache[key] = (px, av, va, hits, st)
    return cache[key]


def expected(name, order, **param_changes):
    """(pixels, means, variances, hit log, stats): the oracle's render from the table with the device's power, what the HIP film must
    equal bit for bit. Made once per (scene, order, changes), read-only."""
    return _expected(_device, lambda b, p: cases.oracle_render_device_pow(b, p, want_hits=True, num_threads=16), name, order, param_changes)


def expected_cpu(name, order, **param_changes):
    """the same render with glibc's power: no GPU needed (the power never steers a path)"""
    return _expected(_cpu, lambda b, p: O.oracle_render_tile(b, p, want_hits=True, num_threads=16, math_mode=O.MATH_DEVICE), name, order, param_changes)


# ------------------------------------------------------------------------------------------------ the fixture's pairs and points
def light_anchors(bundle):
    """the anchor point of every emissive surface, in surface order"""
    sc = bundle.scene
    return np.array([list(sc.surfaces[i].position) for i in range(int(sc.num_surfaces))
                     if int(sc.materials[int(sc.surfaces[i].material)].is_emissive)]).reshape(-1, 3)


PAIR_KINDS_BESIDE_LIGHTS = 3


def visibility_pairs(bundle, ro, rd, index, position):
    """(p0, p1) of the kinds of pair the fixture records, for the rays that hit: (hit position, each light's anchor point),
    (hit position, the next hitting ray's hit position), (origin, hit position), and (origin, hit position + d * vis_fudge): a segment
    that ends one vis_fudge BEHIND the first surface, so that in exact arithmetic the surface stands exactly at the distance the scan
    compares with (`dist < vis_dist`) and in doubles on either side of it or on it -- the one kind that tells `<` from `<=` there."""
    hit = np.flatnonzero(index >= 0)
    pos = position[hit]
    p0, p1 = [], []
    for anchor in light_anchors(bundle):
        p0.append(pos)
        p1.append(np.tile(anchor, (len(pos), 1)))
    p0 += [pos, ro[hit], ro[hit]]
    p1 += [np.roll(pos, -1, axis=0), pos, pos + rd[hit] * RQ.VIS_FUDGE]
    return np.ascontiguousarray(np.concatenate(p0)), np.ascontiguousarray(np.concatenate(p1))


# ------------------------------------------------------------------------------------------------ depth 1, put together by hand
def depth_one_sums(name, order):
    """{"sums" [n][S]: the pixel sums of the max_depth = 1 film put together from the oracle's unit functions alone -- emission where
    the first ray ends on a black body that emits (or escapes into one), nothing where it ends on one that does not, else
    direct_light_contribution at the first hit from the path's own RNG state -- each sample added to the sum in turn; "plain" [n]:
    the pixels that hold emission or nothing, whose sums no power enters}. DEVICE arithmetic, glibc's power."""
    import ctypes as C
    key = (name, order, "depth one")
    if key not in _cpu:
        bundle, _ = load(name)
        t, p = table(name, order), params_of(name, order, max_depth=1)
        L, sc, S = O.oracle_lib(), bundle.scene, bundle.S
        O.set_math_mode(O.MATH_DEVICE)
        spds = bundle.spds()
        ro, rd = (np.array(a.reshape(-1, 3)) for a in (t["origins"], t["dirs"]))
        n = len(ro)
        sums, plain = np.zeros((n, S)), np.zeros(n, dtype=bool)
        f64p = C.POINTER(C.c_double)
        out = np.zeros(S)
        for i in range(n):
            pt = O.Point()
            L.drt_oracle_find_ray_intersection(C.byref(sc), ro[i].ctypes.data_as(f64p), rd[i].ctypes.data_as(f64p), C.byref(pt))
            m = sc.materials[int(pt.surface_material)]
            plain[i] = bool(m.is_black_body)
            for s in range(int(p.spp)):
                if m.is_black_body and not m.is_emissive:
                    break
                if m.is_black_body:
                    c = 1.0 * spds[int(m.emission_spd)]
                else:
                    L.drt_oracle_seed_path(L.drt_oracle_path_key(int(p.seed), int(p.width), int(p.height), i % WIDTH, i // WIDTH, s))
                    L.drt_oracle_direct_light(C.byref(sc), C.byref(pt), out.ctypes.data_as(f64p))
                    c = 1.0 * out
                sums[i] = sums[i] + (0.0 + c) * 1.0
        _cpu[key] = {"sums": _readonly(sums)[0], "plain": _readonly(plain)[0]}
    return _cpu[key]
