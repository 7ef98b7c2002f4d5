"""The (base, exponent) arrays the glossy power's tests share, laid out wave by wave, and the rule's values for them (computed once).

How elements meet lanes: drt_selftest_arith launches drt_selftest_kernel (csrc/drt_kernels.h) with blocks of 256 threads, thread
t of block b on element i = 256 b + t, and a gfx950 wave is 64 consecutive threads of a block. So elements 64 w .. 64 w + 63 are
lanes 0 .. 63 of one wave: element i sits in lane i % 64 of wave i // 64, and an array whose length is 7 mod 64 ends in a wave of
7 lanes. drt_pow_shininess reads the exponent of the FIRST ACTIVE lane on its integer path (the lowest element of the wave that
passes the guard), runs the lanes that hold that exponent on scalar branches and the others through the plain loop.

WAVES names each wave's shape; arrays() returns x, y (float64) and the wave each element belongs to. At most 64 x 48 values.
"""
import functools

import numpy as np

import glossy_power_rule as R

SINGLE_EXPONENTS = (0, 1, 2, 3, 16, 32, 100, 255, 1023)
LANES = 64
MAX_VALUES = 64 * 48


def _pool(n, rng):
    """128 bases in [0, 1] for x^n: the ends (+-0, 1, 1 - 2^-53, the least subnormal, 1/2, 2^-60), values whose n-th power falls
    near 2^-1022 (normal / subnormal), 2^-1075 (subnormal / zero) and 2^-969 (where the low word starts to lose bits) -- seven
    neighbouring doubles and twelve scattered ones each -- and uniform values"""
    ends = [0.0, -0.0, 1.0, 1.0 - 2.0 ** -53, 5e-324, 0.5, 2.0 ** -60]
    edges = []
    for e in (1022.0, 1075.0, 969.0):
        edge = 2.0 ** (-e / n) if n >= 1 else 0.5  # (n = 1: 2^-1075 is no double, the "edge" is 0 and its neighbours subnormals)
        edges += [edge + j * float(np.spacing(edge)) for j in range(-3, 4)]
        edges += list(edge * (1.0 + rng.uniform(-2e-3, 2e-3, 12)))
    edges = np.minimum(np.abs(edges), 1.0)
    x = np.concatenate([ends, edges, rng.uniform(0.0, 1.0, 128 - len(ends) - edges.size)])
    assert x.size == 128 and np.all((x >= 0.0) & (x <= 1.0)) and np.signbit(x[1])
    return x


def _build():
    rng = np.random.default_rng(20240607)
    pools = {}

    def pool(n):
        if n not in pools:
            pools[n] = _pool(n, rng)
        return pools[n]

    def bases(ns):
        return np.array([pool(int(n))[rng.integers(0, 128)] for n in ns])

    waves = []  # (name, x[<= 64], y[<= 64])
    for n in SINGLE_EXPONENTS:  # one exponent per wave, two waves each: the whole pool
        p = pool(n)
        waves.append(("one exponent %d, ends and edges" % n, p[:64], np.full(64, float(n))))
        waves.append(("one exponent %d, uniform bases" % n, p[64:], np.full(64, float(n))))
    lane = np.arange(LANES)
    for name, ns in (("two exponents, alternating lanes", np.where(lane % 2 == 0, 100, 32)),
                     ("two exponents, half a wave each", np.where(lane < 32, 3, 1023)),
                     ("three exponents, every third lane", np.array([100, 32, 7])[lane % 3]),
                     ("three exponents, the first lane's is 0", np.array([0, 1, 255])[lane % 3]),
                     ("one lane apart from the first lane's 63", np.where(lane == 41, 99, 100)),
                     ("64 exponents, 0 .. 63 shuffled", rng.permutation(64)),
                     ("64 exponents out of 0 .. 1023", rng.choice(1024, 64, replace=False))):
        waves.append((name, bases(ns), ns.astype(np.float64)))
    # lane 0 on the pow() path, integer-path lanes behind it (the first ACTIVE lane of the loop is then lane 1 or later)
    for name, x0, y0, ns in (("lane 0 non-integer exponent", 0.75, 2.5, np.full(64, 100)),
                             ("lane 0 exponent 1024", 0.999, 1024.0, np.full(64, 100)),
                             ("lane 0 base above 1", 1.5, 100.0, np.full(64, 100)),
                             ("lanes 0-2 and every ninth on pow(), three exponents behind", 0.75, 100.5, np.array([32, 100, 5])[lane % 3])):
        x, y = bases(ns), ns.astype(np.float64)
        x[0], y[0] = x0, y0
        if "ninth" in name:
            x[1], y[1] = -0.25, 32.0   # base below 0
            x[2], y[2] = 0.5, 1e6      # exponent far above 1023
            y[9::9] = 33.5
        waves.append((name, x, y))
    ns = np.full(7, 100)
    waves.append(("a last wave of 7 lanes", bases(ns), ns.astype(np.float64)))
    return waves


WAVES = _build()


def arrays():
    """x, y, wave index of each element; every wave but the last is full, so element i is lane i % 64 of wave i // 64"""
    assert all(w[1].size == LANES for w in WAVES[:-1]) and WAVES[-1][1].size == 7
    x = np.concatenate([w[1] for w in WAVES])
    y = np.concatenate([w[2] for w in WAVES])
    wave = np.arange(x.size) // LANES
    assert x.size <= MAX_VALUES and x.size % LANES == 7
    return x.copy(), y.copy(), wave


@functools.lru_cache(maxsize=None)
def _expected():
    x, y, _ = arrays()
    on = np.array([R.on_integer_path(float(a), float(b)) for a, b in zip(x, y)])
    want = np.array([R.glossy_power(float(a), int(b)) if m else np.nan for a, b, m in zip(x, y, on)])
    on.setflags(write=False)
    want.setflags(write=False)
    return on, want


def expected():
    """(on_integer_path mask, the rule's value where the mask holds -- NaN elsewhere); read-only, computed once"""
    return _expected()
