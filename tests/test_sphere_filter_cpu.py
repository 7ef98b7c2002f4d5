"""The inputs of tests/test_gpu_sphere_filter.py are worth running: checked with the oracle and the numpy restatement of the filter
(tests/sphere_filter_cases.py) alone, no GPU. The restatement vets inputs; the device is held to the oracle, never to it."""
import numpy as np
import pytest

import oracle_py as O
import sphere_filter_cases as SC


def test_batch_entry_is_the_oracles_line_sphere():
    rec = SC.family("ends")["rec"][::997]
    L = O.oracle_lib()
    O.set_math_mode(O.MATH_DEVICE)
    one = np.array([L.drt_oracle_line_sphere(O._v3(r[0:3]), O._v3(r[3:6]), O._v3(r[6:9]), float(r[9])) for r in rec])
    assert np.array_equal(one.view(np.uint64), SC.rule_distance(rec).view(np.uint64))


@pytest.mark.parametrize("name", SC.FAMILIES)
def test_family_has_hits_and_misses(name):
    f = SC.family(name)
    rec, need = f["rec"], f["need"]
    assert rec.shape[1] == 12 and (1 << 17) < len(rec) <= (1 << 18)
    assert sorted(set(rec[np.isfinite(rec[:, 10]), 10])) == sorted(SC.EXTENTS)
    share = need.mean()
    print("%s: %d records, %.3f with a hit below the limit" % (name, len(rec), share))
    assert 0.25 <= share <= 0.75


@pytest.mark.parametrize("name", SC.UNIT_FAMILIES)
def test_directions_are_of_unit_length(name):
    d = SC.family(name)["rec"][:, 3:6]
    ok = np.isfinite(d).all(axis=1)
    assert np.abs((d[ok] * d[ok]).sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -52


def test_families_hold_what_they_are_for():
    t = SC.family("tangent")["rec"]
    assert t[:, 9].min() < 2e-7 * t[:, 10].min() * 1.0 and (t[:, 9] / t[:, 10]).max() > 0.5
    assert np.isinf(t[:, 11]).any() and np.isfinite(t[:, 11]).any()
    s = SC.family("sizes")["rec"]
    assert (s[:, 9] == 0.0).any() and (s[:, 9] < 0.0).any() and (s[:, 9] == s[:, 10]).any()
    assert ((s[:, 9] > 0.0) & (s[:, 9] < 2.0 ** -24 * s[:, 10])).any()
    for part, label in (((s[:, 9] == 0.0), "r = 0"), ((s[:, 9] < 0.0), "r < 0"), ((s[:, 9] == s[:, 10]), "r = E")):
        assert SC.family("sizes")["need"][part].any(), label
    c = SC.family("components")["rec"]
    d = c[:, 3:6]
    assert ((d == 0.0) & np.signbit(d)).any() and ((d == 0.0) & ~np.signbit(d)).any()
    assert ((d != 0.0) & (np.abs(d) < 2.3e-308)).any()                                   # subnormal doubles
    assert ((d != 0.0) & (d.astype(np.float32) == 0.0)).any()                            # flush to zero in f32
    assert ((d.astype(np.float32) != 0.0) & (np.abs(d) < 1.1e-38)).any()                 # f32 subnormals
    bad = ~np.isfinite(c[:, :11])
    assert bad.any(axis=0).all() and np.isnan(c[:, :11]).any() and np.isinf(c[:, :11]).any()
    k = SC.length_k(SC.family("length")["rec"])
    assert sorted(set(k)) == sorted(SC.LENGTH_K) and SC.LENGTH_K[-1] == 1 << 20
    first = SC.family("length")["rec"][k == 0]
    for kk in SC.LENGTH_K:
        rows = SC.family("length")["rec"][k == kk]
        assert np.array_equal(rows[:, 3:6], first[:, 3:6] * (1.0 + kk * 2.0 ** -53))
        assert np.array_equal(np.delete(rows, [3, 4, 5, 11], axis=1), np.delete(first, [3, 4, 5, 11], axis=1))


@pytest.mark.parametrize("name", SC.UNIT_FAMILIES)
def test_restated_filter_rejects_no_hit(name):
    """not an assertion about the device: were the restatement to reject hits, the families (or the restatement) would be suspect"""
    assert int(SC.false_rejections(name).sum()) == 0


@pytest.mark.parametrize("name", ["tangent", "ends"])
def test_inputs_bite_without_the_pad(name):
    n = int(SC.false_rejections(name, pad=0.0).sum())
    print("%s: without the pad the restated filter rejects %d hits of %d records" % (name, n, len(SC.family(name)["rec"])))
    assert n > 0


def test_effectiveness_margin_is_the_smallest_that_the_restatement_meets():
    left = {}
    for m in range(1, SC.EFFECTIVENESS_PADS + 1):
        left[m] = 0
        for name in SC.UNIT_FAMILIES:
            rec = SC.family(name)["rec"]
            must = SC.must_be_flagged(rec, m)
            assert must.sum() >= 1000, (name, m)  # the bound has records to hold for in every family
            left[m] += int((must & ~SC.filter32(rec)).sum())
        print("m = %d: %d records beyond the margin that the restated filter does not flag" % (m, left[m]))
    assert left[SC.EFFECTIVENESS_PADS] == 0
    assert all(left[m] > 0 for m in range(1, SC.EFFECTIVENESS_PADS))
    # each of the three clauses has records of its own at the margin
    rec = np.concatenate([SC.family(n)["rec"] for n in SC.UNIT_FAMILIES])
    p, t = SC.exact_geometry(rec)
    reach = np.abs(rec[:, 9]) + SC.EFFECTIVENESS_PADS * SC.PAD * rec[:, 10]
    fin = np.isfinite(rec[:, :11]).all(axis=1)
    with np.errstate(invalid="ignore"):
        assert (fin & (p > reach)).any() and (fin & (p <= reach) & (t + reach < 0.0)).any() and (fin & (p <= reach) & (t - reach > rec[:, 11])).any()


def test_drift_figures_are_the_recorded_ones():
    got = SC.direction_drift()
    print("largest | |d|^2 - 1 | in units of 2^-52:", got)
    for key, ulps in SC.DRIFT_ULPS.items():
        assert got[key] <= ulps and got[key] > ulps / 2.0, key


def test_restated_length_tolerance():
    """the restatement's own k_ok: printed for DESIGN.md's comparison with the device's, asserted only to exist"""
    f = SC.family("length")
    k = SC.length_k(f["rec"])
    bad = SC.filter32(f["rec"]) & f["need"]
    counts = {kk: int(bad[k == kk].sum()) for kk in SC.LENGTH_K}
    print("length family, false rejections of the restated filter per k:", counts)
    assert counts[0] == 0
