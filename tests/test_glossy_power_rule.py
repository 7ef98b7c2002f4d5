"""CPU: the rule the glossy lobe's power is held to (tests/glossy_power_rule.py) and the wave-shaped arrays of its GPU test.

The rule restates drt_pow_shininess's double-double loop with every operation exact and rounded once. Checked here, without a GPU:
  * it is the nearest double of x^n wherever x^n >= 2^-969 -- the property tests/test_gpu_parity.py holds the device to -- within
    1 ulp down to 2^-1022 and within one unit of 2^-1074 below (the same test's other two bounds), on the GPU test's own arrays and
    on more bases per exponent than those hold;
  * its zeros: +0 for x = +-0 and n >= 1, 1 for n = 0;
  * the arrays have the shapes the GPU test says they have, lane by lane.
tests/golden holds no recorded device powers (the oracle's power table is filled from the device at test time,
cases.oracle_render_device_pow), so there is nothing recorded for the rule to reproduce; the GPU test compares it with the device.
"""
import numpy as np

import glossy_power_cases as G
import glossy_power_rule as R

MORE_EXPONENTS = (0, 1, 2, 3, 7, 8, 12, 16, 20, 32, 50, 100, 255, 511, 1000, 1023)


def _check_against_nearest(x, n, got):
    """the three bounds of tests/test_gpu_parity.py's test_glossy_power_against_exact_arithmetic; returns which band x^n is in"""
    want = R.nearest_power(x, n)
    off = abs(int(np.float64(got).view(np.int64)) - int(np.float64(want).view(np.int64)))  # both >= +0: units in the last place
    assert not np.signbit(got)
    if want >= 2.0 ** -969:
        assert off == 0, "x %r, n %d: the rule gives %r, the nearest double is %r" % (x, n, got, want)
        return 0
    assert off <= 1, "x %r, n %d: the rule gives %r, the nearest double is %r" % (x, n, got, want)
    return 1 if want >= 2.0 ** -1022 else 2


def test_the_rule_is_the_nearest_double_on_the_gpu_tests_arrays():
    x, y, _ = G.arrays()
    on, want = G.expected()
    bands = [0, 0, 0]
    for a, b, v in zip(x[on], y[on], want[on]):
        bands[_check_against_nearest(float(a), int(b), float(v))] += 1
    print("%d pairs: %d with x^n >= 2^-969 (the nearest double), %d down to 2^-1022, %d below" % (int(on.sum()), *bands))
    assert bands[0] > 1000 and bands[1] > 200 and bands[2] > 400


def test_the_rule_is_the_nearest_double_on_more_bases():
    rng = np.random.default_rng(77)
    bands = [0, 0, 0]
    for n in MORE_EXPONENTS:
        xs = [rng.uniform(0.0, 1.0, 24), 1.0 - rng.uniform(0.0, 1e-6, 8), 1.0 - np.arange(1, 9) * 2.0 ** -53]
        if n >= 1:
            xs += [2.0 ** (-e / n) * (1.0 + rng.uniform(-2e-3, 2e-3, 8)) for e in (900.0, 969.0, 1022.0, 1074.0)]
        for a in np.concatenate(xs):
            if 0.0 <= a <= 1.0:
                bands[_check_against_nearest(float(a), n, R.glossy_power(float(a), n))] += 1
    print("more bases: %d / %d / %d pairs in the three bands" % tuple(bands))
    assert bands[0] > 700 and bands[1] > 50 and bands[2] > 50


def test_the_rules_zeros_and_ones():
    for n in (0, 1, 2, 3, 100, 1023):
        for z in (0.0, -0.0):
            v = R.glossy_power(z, n)
            assert v == (1.0 if n == 0 else 0.0) and not np.signbit(v)
        assert R.glossy_power(1.0, n) == 1.0
    assert R.glossy_power(0.5, 10) == 2.0 ** -10 and R.glossy_power(0.5, 1023) == 2.0 ** -1023
    assert R.glossy_power(5e-324, 1) == 5e-324 and R.glossy_power(5e-324, 2) == 0.0
    # the guard: what goes to pow() is not the rule's
    assert R.on_integer_path(0.5, 100.0) and R.on_integer_path(-0.0, 0.0) and R.on_integer_path(1.0, 1023.0)
    for x, y in ((0.5, 2.5), (0.5, 1024.0), (0.5, -1.0), (1.5, 2.0), (-0.25, 2.0), (np.nan, 2.0), (0.5, np.nan), (0.5, 1e6)):
        assert not R.on_integer_path(x, y)


def test_the_arrays_have_the_wave_shapes_the_gpu_test_names():
    x, y, wave = G.arrays()
    on, _ = G.expected()
    assert x.size == y.size <= G.MAX_VALUES and x.size % 64 == 7 and wave[-1] == len(G.WAVES) - 1
    names = [w[0] for w in G.WAVES]
    distinct = lambda w: len(set(y[(wave == w) & on].tolist()))
    for n in G.SINGLE_EXPONENTS:  # one exponent per wave
        ws = [k for k, name in enumerate(names) if name.startswith("one exponent %d," % n)]
        assert len(ws) == 2 and all(np.all(y[wave == w] == n) and on[wave == w].all() for w in ws)
    assert sorted(distinct(k) for k, name in enumerate(names) if name.startswith("two exponents")) == [2, 2]
    assert sorted(distinct(k) for k, name in enumerate(names) if name.startswith("three exponents")) == [3, 3]
    assert [distinct(k) for k, name in enumerate(names) if name.startswith("64 exponents")] == [64, 64]
    w0 = names.index("three exponents, the first lane's is 0")
    assert y[64 * w0] == 0.0 and on[64 * w0]
    behind = [k for k, name in enumerate(names) if name.startswith("lane")]
    assert len(behind) == 4
    for k in behind:  # lane 0 on the pow() path, integer-path lanes behind it
        assert not on[64 * k] and on[64 * k + 3:64 * k + 9].all()
    reasons = {(bool(y[64 * k] != int(y[64 * k])), bool(y[64 * k] >= 1024.0), bool(x[64 * k] > 1.0)) for k in behind}
    assert {(True, False, False), (False, True, False), (False, False, True)} <= reasons
    assert int((wave == wave[-1]).sum()) == 7 and on[wave == wave[-1]].all()
    # the bases the issue lists are all there, on the integer path
    xs = x[on]
    for v in (1.0, 1.0 - 2.0 ** -53, 5e-324):
        assert (xs == v).any()
    assert ((xs == 0.0) & np.signbit(xs)).any() and ((xs == 0.0) & ~np.signbit(xs)).any()
