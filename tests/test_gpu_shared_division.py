"""The two forms that stand where the trace kernel's path loop had a division (csrc/drt_device.h), on the device through
drt_selftest_division, beside the division itself on the same operands:

  v_div_shared   x / f, y / f, z / f from ONE refined reciprocal where the three scaled denominators are the same bits, else the three
                 plain divisions -- decided per wave. Contract: the IEEE quotients, bit for bit, for every input.
  drt_rng        the draw's n / (2^31 - 1) as n 2^-31 corrected once by a fused multiply-add (csrc/drt_const_rule.h; all 2^31 arguments
                 are swept on the host by tests/test_const_rule_cpu.py). Contract: the IEEE quotient, bit for bit.

`/` on gfx950 is correctly rounded (tests/test_gpu_parity.py holds it to the host's), so the device's own `/` in the next output
slots is the reference; it is compared with numpy's division as well.

v_div_shared takes the shared path only in a wave whose every record has equal scales. The records therefore run twice: once as they
come -- mixed waves, mostly the plain path -- and once sorted by the kernel's own answer "this record's scales are equal", so that
such records fill whole waves; the kernel reports which way each wave went, and the test insists that the shared path really ran for
(nearly) all of them. About 2 * 10^5 records:
  - the vectors of tests/golden/unit_geometry.npz over their own lengths (what v_normalise does),
  - random vectors whose components' exponents are spread over +-600 binades, over their own length and over an unrelated divisor,
  - hand-made ones: the zero vector, one non-zero component, |x| equal to the length, subnormal lengths, lengths near the overflow and
    the underflow of 1 / len, a component 600 binades below the length, +-0, +-inf and NaN in every slot."""
import itertools
import os

import numpy as np
import pytest

import pydrt

U64 = np.uint64


def _length(v):
    """v_length: sqrt(x x + y y + z z), each operation rounded on its own"""
    with np.errstate(all="ignore"):
        return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def _spread(rng, n, lo=-600, hi=600):
    """n x 3 doubles, mantissas in [1, 2), signs and exponents independent per component"""
    m = rng.uniform(1.0, 2.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    return np.ldexp(m, rng.integers(lo, hi + 1, (n, 3)))


def hand_made():
    nan, inf = float("nan"), float("inf")
    tiny, sub, big = 2.2250738585072014e-308, 5e-324, 1.7976931348623157e308
    rows = [
        [0, 0, 0, 0], [0.0, -0.0, 0.0, 0.0], [0, 0, 0, 1], [-0.0, 0.0, -0.0, 2.5],  # 0 / 0 and 0 / f
        [3, 0, 0, 3], [0, -7, 0, 7], [0, 0, 1e-300, 1e-300], [-0.0, 2, 0.0, 2],      # one non-zero component: |x| equal to the length
        [1, 1, 1, 3 ** 0.5], [3, 4, 12, 13], [1, 2, 2, 3],
        [sub, 0, 0, sub], [3 * sub, 4 * sub, 0, 5 * sub], [tiny, tiny, 0, tiny * 2 ** 0.5], [tiny / 4, tiny / 8, tiny / 2, tiny / 2],  # subnormal lengths
        [1, 1, 1, sub], [1, 1, 1, tiny], [1e-300, 1e-310, 1e-320, 1e-300],
        [big, big / 2, big / 4, big], [big, 0, 0, big], [1, 2, 3, big], [1e300, 1e300, 1e300, inf],  # near the overflow of the length ...
        [2.0 ** 1022, 2.0 ** 1021, 1, 2.0 ** 1023], [2.0 ** 1023, 1, 1, 2.0 ** 1023], [1, 1, 1, 2.0 ** 1022], [1, 1, 1, 2.0 ** 1023],  # ... 1 / len subnormal
        [1, 1, 1, 2.0 ** -1022], [1, 1, 1, 2.0 ** -1023], [1, 1, 1, 2.0 ** -1074],                                                    # ... 1 / len overflows
        [1, 2.0 ** -600, 2.0 ** -1000, 1], [2.0 ** 300, 2.0 ** -300, 1, 2.0 ** 300], [2.0 ** 400, 2.0 ** -200, 0, 2.0 ** 400],        # 600 binades below the length
        [2.0 ** 500, 2.0 ** -560, 2.0 ** -574, 2.0 ** 500], [2.0 ** -400, 2.0 ** -1000, 2.0 ** -1074, 2.0 ** -400],                   # quotients that underflow
        [2.0 ** 1000, 2.0 ** -60, 1, 2.0 ** -30], [1, 2, 3, 1e-310], [2.0 ** 900, 1, 1, 2.0 ** -200],                                  # quotients that overflow
    ]
    # +-0, +-inf and NaN in any slot, alone and together
    special = [0.0, -0.0, inf, -inf, nan]
    for slot in range(4):
        for s in special:
            for base in ([1.0, -2.0, 0.5, 3.0], [1e200, 1e-200, 1.0, 1e100]):
                r = list(base)
                r[slot] = s
                rows.append(r)
    for a, b in itertools.product(special, special):
        rows.append([a, 1.5, b, 2.0])
        rows.append([a, b, 1.0, a])
        rows.append([1.0, a, 2.0, b])
    return np.array(rows, dtype=np.float64)


@pytest.fixture(scope="module")
def records(golden_dir):
    g = np.load(os.path.join(golden_dir, "unit_geometry.npz"), allow_pickle=False)
    geo = np.vstack([g["sph_d"], g["sph_o"] - g["sph_c"], g["pl_d"], g["pl_n"], g["pl_u"], g["pl_v"], g["pl_pu"], g["pl_pv"], g["pl_p"] - g["pl_o"],
                     g["rf_v"], g["rf_n"], g["rf_v"] + g["rf_reflect"], g["rot_w"]])
    rng = np.random.default_rng(355)
    own = np.vstack([_spread(rng, 40000), _spread(rng, 30000, -40, 40), _spread(rng, 10000, -1074, -900), _spread(rng, 10000, 480, 530)])
    same_scale = np.ldexp(rng.uniform(-2.0, 2.0, (40000, 3)), rng.integers(-1060, 1000, (40000, 1)))  # ordinary directions at every scale
    parts = [np.hstack([v, _length(v).reshape(-1, 1)]) for v in (geo, own, same_scale)]
    other = _spread(rng, 50000)
    parts.append(np.hstack([other, np.ldexp(rng.uniform(1.0, 2.0, 50000), rng.integers(-1074, 1024, 50000)).reshape(-1, 1)]))
    parts.append(hand_made())
    rec = np.ascontiguousarray(np.vstack(parts))
    assert 190000 <= rec.shape[0] <= 210000
    return rec


def _check_quotients(rec, out):
    shared, plain = out[:, 0:3].view(U64), out[:, 3:6].view(U64)
    bad = np.nonzero((shared != plain).any(axis=1))[0]
    assert bad.size == 0, "v_div_shared differs from the three divisions for %d of %d records, first: %r -> %r, `/` gives %r" % (
        bad.size, rec.shape[0], rec[bad[0]].tolist(), out[bad[0], 0:3].tolist(), out[bad[0], 3:6].tolist())
    with np.errstate(all="ignore"):
        want = rec[:, 0:3] / rec[:, 3:4]
    same = (plain == want.view(U64)) | (np.isnan(out[:, 3:6]) & np.isnan(want))  # a NaN's sign and payload are not the contract
    assert same.all(), "the device's `/` differs from the host's at record %r" % rec[np.nonzero(~same.all(axis=1))[0][0]].tolist()


@pytest.mark.gpu
def test_shared_reciprocal_division_is_the_division(records):
    rec = records
    out = pydrt.selftest_division(pydrt.DIVISION_SHARED, rec)
    _check_quotients(rec, out)
    equal = out[:, 6] == 1.0
    assert set(np.unique(out[:, 6])) <= {0.0, 1.0} and set(np.unique(out[:, 7])) <= {0.0, 1.0}
    print("records %d, with equal scales %d, in a wave that shared the reciprocal as they come %d" % (rec.shape[0], equal.sum(), (out[:, 7] == 1.0).sum()))
    # the cases are really there: records the shared form must hand to `/` (a zero or far smaller component), and ordinary ones
    assert equal.sum() >= 50000 and (~equal).sum() >= 1000
    # a wave shares exactly when all its records have equal scales (64 consecutive records to a wave)
    n_full = rec.shape[0] // 64 * 64
    wave_all = equal[:n_full].reshape(-1, 64).all(axis=1)
    assert np.array_equal(np.repeat(wave_all, 64), out[:n_full, 7] == 1.0)
    # again, the records with equal scales packed into waves of their own: now they take the shared path, all but a last partial wave
    order = np.argsort(~equal, kind="stable")
    rec2 = np.ascontiguousarray(rec[order])
    out2 = pydrt.selftest_division(pydrt.DIVISION_SHARED, rec2)
    _check_quotients(rec2, out2)
    assert np.array_equal(out2[:, 6], out[order, 6])
    n_eq = int(equal.sum())
    assert (out2[:n_eq // 64 * 64, 7] == 1.0).all() and (out2[(n_eq + 63) // 64 * 64:, 7] == 0.0).all()
    # and both runs gave every record the same answer, whichever path its wave took
    assert np.array_equal(out2[:, 0:3].view(U64), out[order, 0:3].view(U64))
    hm = hand_made()
    with np.errstate(all="ignore"):
        q = hm[:, 0:3] / hm[:, 3:4]
    assert np.isnan(q).any() and np.isinf(q).any() and ((q != 0.0) & (np.abs(q) < 2.3e-308)).any() and (q == 0.0).any()


def _xorshift(x):
    x = x ^ (x << U64(13))
    x = x ^ (x >> U64(7))
    return x ^ (x << U64(17))


def _state_before(after):
    """the state whose next xorshift64 step gives `after` (Python integers)"""
    mask = (1 << 64) - 1

    def undo(y, k, left):
        x, t = y, y
        for _ in range(64 // k):
            t = (t << k) & mask if left else t >> k
            x ^= t
        return x
    return undo(undo(undo(after, 17, True), 7, False), 13, True)


@pytest.mark.gpu
def test_the_draw_is_the_division():
    rng = np.random.default_rng(950)
    crafted = []
    for top in (0, 2 ** 31 - 1, 2 ** 31 - 2, 1, 2, 2 ** 30, 2 ** 30 - 1, 2 ** 30 + 1):
        for low in (1, 2 ** 33 - 1, 0x155555555, int(rng.integers(1, 2 ** 33))):
            crafted.append(_state_before((top << 33) | low))
    states = np.concatenate([np.array(crafted, dtype=U64), rng.integers(1, 2 ** 64, 200000 - len(crafted), dtype=U64)])
    after = _xorshift(states)
    tops = after >> U64(33)
    assert {0, 2 ** 31 - 1, 2 ** 31 - 2} <= set(int(t) for t in tops[:len(crafted)])
    out = pydrt.selftest_division(pydrt.DIVISION_DRAW, states.view(np.float64))
    assert np.array_equal(out[:, 2].view(U64), after)
    want = tops.astype(np.float64) / np.float64(2147483647.0)
    assert np.array_equal(out[:, 1].view(U64), want.view(U64))  # the device's division is the host's
    bad = np.nonzero(out[:, 0].view(U64) != want.view(U64))[0]
    assert bad.size == 0, "drt_rng differs from the division for %d states, first: n = %d gives %r, n / (2^31 - 1) = %r" % (
        bad.size, int(tops[bad[0]]), out[bad[0], 0], want[bad[0]])
    assert out[:, 0].min() == 0.0 and out[:, 0].max() == 1.0  # rng()'s range, both ends included


@pytest.mark.gpu
def test_division_entry_refuses_narrow_records():
    with pytest.raises(RuntimeError):
        pydrt.selftest_division(pydrt.DIVISION_SHARED, np.zeros((4, 3)))
