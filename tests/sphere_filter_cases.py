"""The inputs of the sphere-filter tests: records for drt_selftest_unit's function 14 (sphere_certainly_missed, csrc/drt_kernels.h),
what the rule answers to them, and a numpy restatement of the filter. Not a test file: tests/test_sphere_filter_cpu.py checks with
the oracle and the restatement that these inputs are worth running, tests/test_gpu_sphere_filter.py runs them on the device.
Everything here is computed once per family and handed out unchanged.

A record is 12 doubles, `o[3] d[3] c[3] r E limit`: the origin as bvh_walk receives it, the direction, the sphere, the extent E the
leaf's pad is for, and the walk's distance limit. THE RULE is the oracle's drt_oracle_line_sphere (the reference's
line_sphere_intersection, a = 1 whatever |d| is): the filter may say "missed" only where that distance is not below the limit. The
restatement (filter32) states the filter in numpy f32 with the fused multiply-adds emulated through f64 (the product of two f32 is
exact in f64; the sum is then rounded twice). It vets inputs and nothing else: the device is never asserted equal to it.

Families (seeded; E = 4, 64, 1e4 and 2^26 in equal parts, the builder refuses extents from 2^27; at most 2^18 records each):
  tangent     rays along a tangent of the sphere from origins inside the cube of E, moved towards the centre or away from it by 0 to 8
              f32 ulps of E (whole and fractional numbers of ulps), radii 1e-7 E to E (log-uniform); a share moved away by 1 to 4
              pads, for the effectiveness bound. limit: +inf, or the rule's distance times 1 - 1e-9, 1, 1 + 1e-9, 1 -+ 2^-23.
  ends        the sphere just behind the origin (origin on the surface, or 1-4 f64 ulps or 1-8 f32 ulps of E inside or outside it, heading
              away; radially outside by 1 to 4 pads); the sphere just beyond the limit (limit = entry distance minus up to 4 pads, plus
              up to half a pad, or times the factors above); the origin inside the sphere; the centre exactly on the ray.
  sizes       r = 0, 0 < r < u E, r = E (the centre at 0) and negative radii: reach32 takes fabs and the intersector squares it.
  components  tangent rays whose direction has one or two components of +0, -0, a subnormal double, values that flush to zero in f32
              (1e-46, 1e-50, 1e-300) or an f32 subnormal (1e-40); and records with a NaN, +inf or -inf in one of o, d, c, r, or a NaN or +inf E.
  length      tangent rays with d multiplied by 1 + k 2^-53 for k = 0, 1, 4, ..., 2^20, the same rays for every k; the limits are drawn
              once and follow each k's own distance under the rule.

EFFECTIVENESS_PADS (m): a unit-direction ray must be flagged when, in exact arithmetic (f64 is enough: see exact_geometry), its line
passes the centre at more than r + m pads, or its sphere lies wholly behind the origin or wholly beyond the limit by the same margin;
a pad is 2^-18 E. m is the smallest whole number for which filter32 flags all such records of all families: 2, as the error bound
next to the filter (below one pad) predicts. With m = 1 it leaves 383 records unflagged (tests/test_sphere_filter_cpu.py prints the count).

With the pad set to 0 (reach32 = |r| to f32, up two steps) filter32 rejects hits within the limit, so the inputs bite:
    tangent 2840 of 262144, ends 1478 of 262144
(test_sphere_filter_cpu.py asserts both counts positive and prints them).

Drift of | |d|^2 - 1 | along what the path does to a direction (direction_drift): see the figures in DRIFT_ULPS' comment.
"""

import numpy as np

import oracle_py as O

F32, F64 = np.float32, np.float64
PAD = 2.0 ** -18            # of E: bvh_sphere_reach32 (csrc/drt_build_rule.h)
EXTENTS = (4.0, 64.0, 1.0e4, 2.0 ** 26)
PER_EXTENT = 1 << 16        # 4 extents: 2^18 records per family
FAMILIES = ("tangent", "ends", "sizes", "components", "length")
UNIT_FAMILIES = ("tangent", "ends", "sizes", "components")  # every direction of unit length (or not finite)
LIMIT_FACTORS = np.array([1.0 - 1e-9, 1.0, 1.0 + 1e-9, 1.0 - 2.0 ** -23, 1.0 + 2.0 ** -23])
LENGTH_K = (0, 1, 4, 16, 64, 256, 1024, 4096, 1 << 14, 1 << 16, 1 << 18, 1 << 20)
EFFECTIVENESS_PADS = 2
# | |d|^2 - 1 | in units of 2^-52, the largest along each chain of direction_drift() (numpy f64, the device's order of operations):
# v_normalise of 2^16 random vectors 2.5; 524 reflections between two tilted mirrors 280.5; 524 passes through a glass slab's faces 1
# (v_transmit restores the length at every step: its component along the normal is sqrt(1 - |the rest|^2))
DRIFT_ULPS = {"normalise": 3, "reflect": 281, "transmit": 1}

_families = {}


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def _normalise(v):
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def _radii(rng, n, E):
    return E * 10.0 ** rng.uniform(-7.0, 0.0, n)


def _centres(rng, r, E):
    """the sphere's box stays inside the cube of E"""
    return rng.uniform(-1.0, 1.0, (len(r), 3)) * (E - np.abs(r))[:, None]


def _back_off(p, u, E):
    """how far p - s u stays inside the cube of E"""
    with np.errstate(all="ignore"):
        s = np.where(u > 0.0, (p + E) / u, np.where(u < 0.0, (E - p) / -u, np.inf))
    return np.maximum(np.min(s, axis=1), 0.0)


def _tangent(rng, n, E, p_in, p_near, r=None, u=None):
    """o, d, c, r of rays along a tangent of their sphere, moved towards the centre (share p_in), away from it by up to 8 f32 ulps of E,
    or away by 1 to 4 pads (share p_near)"""
    r = _radii(rng, n, E) if r is None else r
    c = _centres(rng, r, E)
    if u is None:
        nrm = _unit(rng, n)
        u = _normalise(np.cross(nrm, _unit(rng, n)))
    else:
        nrm = _normalise(np.cross(u, _unit(rng, n)))
    p = c + np.abs(r)[:, None] * nrm
    s = _back_off(p, u, E) * rng.uniform(0.0, 1.0, n)
    ulp = float(np.spacing(F32(E)))
    k = np.where(rng.random(n) < 0.5, rng.integers(0, 9, n).astype(F64), rng.uniform(0.0, 8.0, n))
    kind = rng.random(n)
    off = np.where(kind < p_in, -np.minimum(k * ulp, np.abs(r)),
                   np.where(kind < 1.0 - p_near, k * ulp, rng.uniform(1.0, 4.0, n) * PAD * E))
    o = p + off[:, None] * nrm - s[:, None] * u
    return o, u, c, r


def _records(o, d, c, r, E, limit=np.inf):
    n = len(o)
    rec = np.empty((n, 12))
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9], rec[:, 10], rec[:, 11] = o, d, c, r, E, limit
    return rec


def rule_distance(rec):
    """drt_oracle_line_sphere of every record, device arithmetic"""
    O.set_math_mode(O.MATH_DEVICE)
    rec = np.ascontiguousarray(rec, dtype=F64)
    out = np.empty(len(rec))
    O.oracle_lib().drt_oracle_line_sphere_records(rec.ctypes.data_as(O.f64p), rec.shape[1], len(rec), out.ctypes.data_as(O.f64p))
    return out


def _limit_draws(rng, n):
    return rng.integers(0, len(LIMIT_FACTORS), n), rng.uniform(0.0, 4.0, n), rng.random(n)


def _set_limits(rng, rec, p_inf, draws=None):
    """+inf, or the rule's distance times one of LIMIT_FACTORS; a record without a hit: +inf, or any distance up to 4 E"""
    factor, other, inf = _limit_draws(rng, len(rec)) if draws is None else draws
    dist = rule_distance(rec)
    with np.errstate(all="ignore"):
        near = dist * LIMIT_FACTORS[factor]
    rec[:, 11] = np.where(inf < p_inf, np.inf, np.where(np.isfinite(dist), near, other * rec[:, 10]))
    return rec


def _tangent_family(rng, E, n):
    return _set_limits(rng, _records(*_tangent(rng, n, E, 0.6, 0.15), E), 0.4)


def _ends_family(rng, E, n):
    ulp32 = float(np.spacing(F32(E)))
    q = n // 4
    parts = []
    # (a) the sphere just behind the origin
    r = _radii(rng, q, E)
    c = _centres(rng, r, E)
    nrm = _unit(rng, q)
    d = _unit(rng, q)
    d = np.where(((d * nrm).sum(axis=1) < 0.0)[:, None], -d, d)
    kind = rng.integers(0, 6, q)
    d = np.where((kind >= 4)[:, None], nrm, d)  # radial: the centre on the ray's line, behind the origin
    sign = rng.choice([-1.0, 1.0], q)
    delta = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                      [0.0, sign * rng.integers(1, 5, q) * np.spacing(E), sign * rng.integers(1, 9, q) * ulp32,
                       sign * rng.uniform(0.0, 8.0, q) * ulp32, sign * rng.integers(0, 9, q) * ulp32],
                      rng.uniform(1.0, 4.0, q) * PAD * E)  # kind 5: radially outside by 1 to 4 pads
    delta = np.maximum(delta, -r)
    parts.append(_set_limits(rng, _records(c + (r + delta)[:, None] * nrm, d, c, r, E), 0.6))
    # (b) the sphere just beyond the limit; a third with the centre exactly on the ray
    m = n - 3 * q
    r = _radii(rng, m, E)
    c = _centres(rng, r, E)
    d = _unit(rng, m)
    axis = rng.random(m) < 0.25
    d[axis] = np.eye(3)[rng.integers(0, 3, int(axis.sum()))] * rng.choice([-1.0, 1.0], int(axis.sum()))[:, None]
    s = np.maximum(_back_off(c, d, E) * rng.uniform(0.0, 1.0, m), 1.5 * r)
    side = _normalise(np.cross(d, _unit(rng, m))) * (rng.uniform(0.0, 0.9, m) * r * (rng.random(m) < 0.67))[:, None]
    rec = _records(c - s[:, None] * d + side, d, c, r, E)
    dist = rule_distance(rec)
    with np.errstate(all="ignore"):
        rec[:, 11] = np.where(rng.random(m) < 0.5, dist + rng.uniform(-4.0, 0.5, m) * PAD * E,
                              dist * LIMIT_FACTORS[rng.integers(0, len(LIMIT_FACTORS), m)])
    rec[~np.isfinite(dist), 11] = np.inf
    parts.append(rec)
    # (c) the origin inside the sphere
    r = _radii(rng, q, E)
    c = _centres(rng, r, E)
    o = c + (r * rng.uniform(0.0, 0.999, q) ** (1.0 / 3.0))[:, None] * _unit(rng, q)
    parts.append(_set_limits(rng, _records(o, _unit(rng, q), c, r, E), 0.4))
    # (d) the centre exactly on the ray, ahead or behind: c = o + s d as f64 computes it, and axis-parallel rays where that is exact
    o = rng.uniform(-E, E, (q, 3))
    d = _unit(rng, q)
    axis = rng.random(q) < 0.5
    d[axis] = np.eye(3)[rng.integers(0, 3, int(axis.sum()))] * rng.choice([-1.0, 1.0], int(axis.sum()))[:, None]
    c = o + (_back_off(o, -d, E) * rng.uniform(-0.3, 1.0, q))[:, None] * d
    r = np.minimum(_radii(rng, q, E), E - np.abs(c).max(axis=1))
    parts.append(_set_limits(rng, _records(o, d, c, np.maximum(r, 1e-7 * E), E), 0.4))
    return np.concatenate(parts)


def _sizes_family(rng, E, n):
    q = n // 8
    u24 = 2.0 ** -24
    r = np.concatenate([np.zeros(q), rng.uniform(0.01, 0.9, q) * u24 * E, np.full(3 * q, E), -_radii(rng, n - 5 * q, E)])
    o, d, c, r = _tangent(rng, n, E, 0.75, 0.1, r=r)
    # r = 0 and r < u E: only a ray through the centre hits. Aim these at the centre along an axis, where c - o is exact
    tiny = np.arange(n) < 2 * q
    ax = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], n)[:, None]
    aimed = tiny & (rng.random(n) < 0.8)
    d = np.where(aimed[:, None], ax, d)
    o = np.where(aimed[:, None], c - (_back_off(c, ax, E) * rng.uniform(0.0, 1.0, n))[:, None] * ax, o)
    # r = E: origins inside the sphere as well
    big = (np.abs(r) == E) & (rng.random(n) < 0.5)
    o = np.where(big[:, None], rng.uniform(-0.5, 0.5, (n, 3)) * E, o)
    d = np.where(big[:, None], _unit(rng, n), d)
    return _set_limits(rng, _records(o, d, c, r, E), 0.5)


_SMALL = np.array([0.0, -0.0, 5e-324, -3e-310, 1e-300, 1e-50, -1e-46, 1e-40])


def _components_family(rng, E, n):
    u = _unit(rng, n)
    which = rng.integers(0, 3, n)
    second = rng.random(n) < 0.3
    u[np.arange(n), which] = 0.0
    u[second, (which[second] + 1) % 3] = 0.0
    u = _normalise(u)
    u[np.arange(n), which] = _SMALL[rng.integers(0, len(_SMALL), n)]
    u[second, (which[second] + 1) % 3] = _SMALL[rng.integers(0, len(_SMALL), int(second.sum()))]
    rec = _set_limits(rng, _records(*_tangent(rng, n, E, 0.6, 0.15, u=u), E), 0.4)
    # the last eighth: one of o, d, c, r, E not finite (the limit keeps its value: +inf is one of its ordinary values)
    bad = np.arange(n - n // 8, n)
    rec[bad, rng.integers(0, 11, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    rec[:, 10] = np.abs(rec[:, 10])  # an extent is a largest magnitude: NaN or +inf, never -inf
    return rec


def _length_family(rng, E, n):
    per = n // len(LENGTH_K)
    base = _records(*_tangent(rng, per, E, 0.8, 0.0), E)
    draws = _limit_draws(rng, per)
    out = []
    for k in LENGTH_K:
        rec = base.copy()
        rec[:, 3:6] = rec[:, 3:6] * (1.0 + k * 2.0 ** -53)
        out.append(_set_limits(rng, rec, 0.55, draws))  # the limit follows the rule's distance of the lengthened ray
    return np.concatenate(out)


def length_k(rec):
    """the k of every record of the length family"""
    per = PER_EXTENT // len(LENGTH_K)
    return np.tile(np.repeat(np.array(LENGTH_K), per), len(EXTENTS))


_BUILD = {"tangent": _tangent_family, "ends": _ends_family, "sizes": _sizes_family, "components": _components_family,
          "length": _length_family}


def family(name):
    """{"rec": [n][12] records, "dist": the rule's distance of each, "need": the rule has a hit below the limit}"""
    if name not in _families:
        rec = np.concatenate([_BUILD[name](np.random.default_rng([0x5F11, FAMILIES.index(name), i]), E, PER_EXTENT)
                              for i, E in enumerate(EXTENTS)])
        rec = np.ascontiguousarray(rec)
        dist = rule_distance(rec)
        with np.errstate(invalid="ignore"):
            need = dist < rec[:, 11]
        for a in (rec, dist, need):
            a.setflags(write=False)
        _families[name] = {"rec": rec, "dist": dist, "need": need}
    return _families[name]


def _fma32(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def reach32(r, E, pad=PAD):
    """bvh_sphere_reach32 (csrc/drt_build_rule.h)"""
    with np.errstate(all="ignore"):
        reach = (np.abs(r) + E * pad).astype(F32)
        return np.nextafter(np.nextafter(reach, F32(np.inf)), F32(np.inf))


def filter32(rec, pad=PAD):
    """sphere_certainly_missed on the leaf, the Ray32 and the f32 limit the walk makes of a record; True = "certainly missed" """
    with np.errstate(all="ignore"):
        o, d, c = rec[:, 0:3].astype(F32), rec[:, 3:6].astype(F32), rec[:, 6:9].astype(F32)
        R = reach32(rec[:, 9], rec[:, 10], pad)
        lim = rec[:, 11].astype(F32) * F32(1.00000024)
        cx, cy, cz = c[:, 0] - o[:, 0], c[:, 1] - o[:, 1], c[:, 2] - o[:, 2]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        t = _fma32(cz, dz, _fma32(cy, dy, cx * dx))
        px, py, pz = _fma32(-t, dx, cx), _fma32(-t, dy, cy), _fma32(-t, dz, cz)
        p2 = _fma32(pz, pz, _fma32(py, py, px * px))
        return ((p2 > R * R) | (t + R < F32(0.0)) | (t - R > lim)) & (p2 < F32(np.inf))


def exact_geometry(rec):
    """(distance of the centre from the ray's line, distance of its foot point along the ray) for unit directions, in f64. The cross
    product's error is a few 2^-53 |c - o|, at most 1e-15 E: against a pad of 3.8e-6 E, f64 is exact enough."""
    with np.errstate(all="ignore"):
        w, d = rec[:, 6:9] - rec[:, 0:3], rec[:, 3:6]
        x = np.cross(w, d)
        return np.sqrt((x * x).sum(axis=1)), (w * d).sum(axis=1)


def must_be_flagged(rec, m=EFFECTIVENESS_PADS):
    """the effectiveness bound: finite unit-direction records a filter worth having rejects"""
    with np.errstate(all="ignore"):
        p, t = exact_geometry(rec)
        reach = np.abs(rec[:, 9]) + m * PAD * rec[:, 10]
        return np.isfinite(rec[:, :11]).all(axis=1) & ((p > reach) | (t + reach < 0.0) | (t - reach > rec[:, 11]))


def false_rejections(name, pad=PAD):
    """records of a family whose hit below the limit filter32 would skip"""
    f = family(name)
    return filter32(f["rec"], pad) & f["need"]


# ---- what the path does to a direction (section C) -------------------------------------------------------------------------------

def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _reflect(v, n):
    """v_reflect (csrc/drt_device.h; src/geometry.c:85-90)"""
    return v - n * (2.0 * _dot(v, n))


def _transmit(v, n, ir, tr):
    """v_transmit (src/geometry.c:92-106)"""
    vn = _dot(v, n)
    rel = ir / tr
    v = n * vn - v
    perpend = -(v * rel)
    return perpend + n * -np.sqrt(1.0 - _dot(perpend, perpend))


def _off_one(d):
    return abs(float(_dot(d, d)) - 1.0) / 2.0 ** -52


def direction_drift():
    """the largest | |d|^2 - 1 |, in units of 2^-52, over: v_normalise of 2^16 random vectors; a chain of 524 v_reflect steps (the
    deepest path the records hold) between two mirrors tilted against each other; 524 v_transmit steps in and out of a glass slab"""
    rng = np.random.default_rng(0xD81F7)
    v = rng.normal(size=(1 << 16, 3)) * 10.0 ** rng.uniform(-3, 3, (1 << 16, 1))
    ln = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    u = v / ln[:, None]
    out = {"normalise": float(np.abs(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2] - 1.0).max() / 2.0 ** -52)}
    n1 = np.array([0.0, 0.0, 1.0])
    n2 = _unit(rng, 1)[0]
    d = _unit(rng, 1)[0]
    worst = 0.0
    for b in range(524):
        d = _reflect(d, n1 if b % 2 == 0 else n2)
        worst = max(worst, _off_one(d))
    out["reflect"] = worst
    n = _normalise(np.array([[0.3, -0.2, 1.0]]))[0]
    d = _normalise(np.array([[0.4, 0.5, -1.0]]))[0]
    worst = 0.0
    for b in range(524):
        # into the slab through its upper face, out through its lower face: the normal as the shade kernel turns it against the ray
        d = _transmit(d, n, 1.0, 1.5) if b % 2 == 0 else _transmit(d, n, 1.5, 1.0)
        worst = max(worst, _off_one(d))
    out["transmit"] = worst
    return out
