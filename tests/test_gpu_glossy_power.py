"""GPU: drt_pow_shininess, wave shape by wave shape, against its rule bit for bit.

The glossy lobe's power (csrc/drt_device.h) reads the exponent of the first active lane of its integer path into a scalar register,
runs the lanes that hold that exponent on scalar branches -- only the products the exponent's bits call for -- and the other lanes
through the plain per-lane loop. Which lanes share a wave therefore decides which code a lane runs, and must not decide its value.

drt_selftest_arith(7, x, y) puts element i in lane i % 64 of wave i // 64 (blocks of 256 threads, thread t of block b on element
256 b + t; tests/glossy_power_cases.py), so the arrays are laid out as waves: one exponent per wave (0, 1, 2, 3, 16, 32, 100, 255,
1023), two and three exponents interleaved, 64 different exponents, lane 0 on the pow() path with integer-path lanes behind it, and
a last wave of 7 lanes; bases +-0, 1, 1 - 2^-53, 5e-324, uniform values and values whose power falls near 2^-1022, 2^-1075 and
2^-969. Every integer-path lane must give tests/glossy_power_rule.py's value, every other lane ocml's pow, bit for bit.
"""
import numpy as np
import pytest

import cases
import glossy_power_cases as G
import pydrt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_powers():
    x, y, wave = G.arrays()
    got = pydrt.selftest_arith(7, x, y)
    got.setflags(write=False)
    return x, y, wave, got


def test_every_integer_path_lane_gives_the_rules_bits(device_powers):
    x, y, wave, got = device_powers
    on, want = G.expected()
    bad = np.flatnonzero(on & (got.view(np.uint64) != want.view(np.uint64)))
    print("%d values in %d waves, %d on the integer path, %d differ from the rule" % (x.size, len(G.WAVES), int(on.sum()), bad.size))
    for i in bad[:10]:
        print("  wave %d (%s) lane %d: %r ^ %d = %r, the rule gives %r" % (wave[i], G.WAVES[wave[i]][0], i % 64, x[i], int(y[i]),
                                                                           got[i], want[i]))
    assert bad.size == 0, "waves %s" % sorted({G.WAVES[w][0] for w in wave[bad]})
    assert not np.signbit(got[on]).any()


def test_every_other_lane_gives_pows_bits(device_powers):
    x, y, wave, got = device_powers
    on, _ = G.expected()
    assert 10 <= int((~on).sum()) <= 20
    general = pydrt.selftest_arith(3, x, y)  # ocml's pow on every lane
    assert cases.same_bits(got[~on], general[~on])


def test_a_lanes_value_does_not_depend_on_its_waves_other_lanes(device_powers):
    """the mixed waves again with their lanes reversed -- another first lane, so another split between the two loops: the same bits
    per (x, y). With the arrays above that is under 64 x 40 values in all."""
    x, y, wave, got = device_powers
    mixed = np.flatnonzero(np.isin(wave, [k for k, w in enumerate(G.WAVES) if len(set(w[2].tolist())) > 1]))
    xr, yr = x[mixed][::-1].copy(), y[mixed][::-1].copy()
    assert xr.size % 64 == 0 and x.size + xr.size <= G.MAX_VALUES
    assert cases.same_bits(pydrt.selftest_arith(7, xr, yr)[::-1], got[mixed])
