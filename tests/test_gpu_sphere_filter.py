"""The hierarchy's f32 sphere filter, sphere_certainly_missed (csrc/drt_kernels.h), one record at a time on the device through
drt_selftest_unit's function 14, against THE RULE: the oracle's drt_oracle_line_sphere in device arithmetic. The walk asks the filter
whether the f64 intersector needs to run at all, so what the filter owes the walk is

    wherever the rule's distance is below the limit, the filter does not say "missed".

The families of tests/sphere_filter_cases.py (2^18 records each, one launch) put rays where a filter that is slightly too eager
breaks that: along tangents within a few f32 ulps of the extent, spheres ending at the origin or at the limit, radii of 0 and of the
whole extent, direction components that vanish in f32, inputs that are not finite. So that a filter that never rejects does not
pass either, unit-direction rays that clear their sphere by EFFECTIVENESS_PADS pads must be flagged. Nothing is asserted against the
numpy restatement of the filter.

test_length_tolerance_covers_the_paths_drift measures k_ok, the largest k of the length family (d times 1 + k 2^-53) up to which no hit
is rejected: the filter -- like the walk's distance pruning -- is derived for |d| = 1, and the rule is not the geometric answer
otherwise. On the device (MI355X): false rejections per k = 0 for every k up to 16384, 50 at 65536, 246 at 2^18, 519 at 2^20, so
k_ok = 16384, i.e. | |d|^2 - 1 | up to 3.6e-12, against a drift of at most 280.5 x 2^-52 = 6.2e-14 along 524 reflections.
"""
import numpy as np
import pytest

import pydrt
import sphere_filter_cases as SC

_device = {}


def device(name):
    """(flag, distance) of every record of a family: one launch, shared by the tests"""
    if name not in _device:
        out = pydrt.selftest_unit(pydrt.UNIT_BVH_SPHERE, SC.family(name)["rec"])
        assert set(np.unique(out[:, 0])) <= {0.0, 1.0}
        _device[name] = (out[:, 0] == 1.0, out[:, 1])
    return _device[name]


def _show(rec, i):
    return "record %d: %s" % (i, ", ".join(float(x).hex() for x in rec[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.FAMILIES)
def test_distance_is_the_rules(name):
    """the entry's second output: line_sphere on the device, the oracle's bits (a NaN where the oracle has a NaN)"""
    f = SC.family(name)
    _, dist = device(name)
    same = (dist.view(np.uint64) == f["dist"].view(np.uint64)) | (np.isnan(dist) & np.isnan(f["dist"]))
    bad = np.flatnonzero(~same)
    assert bad.size == 0, "%d of %d distances differ from the oracle's, first %s: device %r oracle %r" % (
        bad.size, len(dist), _show(f["rec"], bad[0]), dist[bad[0]], f["dist"][bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.UNIT_FAMILIES)
def test_filter_rejects_no_hit_below_the_limit(name):
    f = SC.family(name)
    flag, _ = device(name)
    bad = np.flatnonzero(flag & f["need"])
    print("%s: %d records, %d with a hit below the limit, %d flagged, %d hits flagged" % (name, len(flag), f["need"].sum(), flag.sum(), bad.size))
    assert bad.size == 0, "the filter skips %d hits below the limit, first %s: the rule's distance %r" % (
        bad.size, _show(f["rec"], bad[0]), f["dist"][bad[0]])


@pytest.mark.gpu
def test_records_that_are_not_finite_are_never_missed():
    """A NaN, +inf or -inf in one of o, d, c, r, or a NaN or +inf extent: never "missed". The limit is not among the poisoned inputs:
    +inf is its ordinary value at the start of every walk, and the walk never makes a NaN limit (it is +inf or a distance that
    compared below it); with one the filter could still say "missed" through its first clause, which no comparison `dist < NaN`
    of the walk would contradict."""
    rec = SC.family("components")["rec"]
    flag, _ = device("components")
    odd = ~np.isfinite(rec[:, :11]).all(axis=1)
    bad = np.flatnonzero(flag & odd)
    print("components: %d records with a NaN or an infinity, %d of them flagged" % (odd.sum(), bad.size))
    assert odd.sum() > 1000
    assert bad.size == 0, "%d records with a NaN or an infinity come back \"missed\", first %s" % (bad.size, _show(rec, bad[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.UNIT_FAMILIES)
def test_filter_rejects_what_clears_the_sphere(name):
    rec = SC.family(name)["rec"]
    flag, _ = device(name)
    must = SC.must_be_flagged(rec, SC.EFFECTIVENESS_PADS)
    bad = np.flatnonzero(must & ~flag)
    print("%s: %d records clear their sphere by %d pads, %d of them not flagged" % (name, must.sum(), SC.EFFECTIVENESS_PADS, bad.size))
    assert must.sum() >= 1000
    assert bad.size == 0, "%d records beyond the margin are not flagged, first %s" % (bad.size, _show(rec, bad[0]))


@pytest.mark.gpu
def test_length_tolerance_covers_the_paths_drift():
    f = SC.family("length")
    flag, _ = device("length")
    k = SC.length_k(f["rec"])
    counts = {kk: int((flag & f["need"])[k == kk].sum()) for kk in SC.LENGTH_K}
    hits = {kk: int(f["need"][k == kk].sum()) for kk in SC.LENGTH_K}
    print("false rejections per k:", counts)
    print("hits below the limit per k:", hits)
    assert counts[0] == 0 and min(hits.values()) > 10000
    k_ok = 0
    for kk in SC.LENGTH_K:
        if counts[kk]:
            break
        k_ok = kk
    drift = SC.direction_drift()
    tolerance = (1.0 + k_ok * 2.0 ** -53) ** 2 - 1.0
    print("k_ok = %d: | |d|^2 - 1 | up to %.3g; drift %r x 2^-52, the largest %.3g" % (k_ok, tolerance, drift, max(drift.values()) * 2.0 ** -52))
    assert tolerance >= 4.0 * max(drift.values()) * 2.0 ** -52


@pytest.mark.gpu
def test_sphere_entry_refuses_narrow_records():
    with pytest.raises(RuntimeError):
        pydrt.selftest_unit(pydrt.UNIT_BVH_SPHERE, np.zeros((4, 11)))
