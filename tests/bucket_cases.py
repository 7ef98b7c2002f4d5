"""Bucket films (drt_bind_buckets): the shared cases and expected films.

The rule (tests/bucket_rule.py) needs no oracle code of its own: the contribution of sample m is the `pixels` buffer of the existing
oracle's render with spp = 1, first_sample = m onto a zero film, exactly as tests/sensor_cases.py makes them (samples_cpu for the tests
without a GPU, samples_device for the GPU tests; both are imported, shared, and nothing writes to what they return).

SHAPES lists every (case, buckets, samples, first sample) the GPU tests render. tests/test_buckets_cpu.py shows on the oracle, for
each of them, that the bucket films tell buckets apart: every two buckets differ in sum and mean, and in the variance wherever the
rule lets them -- a bucket of one sample has a variance of exactly zero (asserted there too), so only buckets of two samples or more
can differ in it. example_scene is all NaN and exempt."""
import numpy as np

import bucket_rule
import cases
import sensor_cases as SC

BASE = SC.BASE
load, params_with, assert_film, film_device, film_cpu = SC.load, SC.params_with, SC.assert_film, SC.film_device, SC.film_cpu

# the cases of test_buckets_cpu's premise: the rule with n = 1 is the oracle's own film
CPU_CASES = SC.CPU_CASES

# BASE: (buckets, samples, first sample)
BASE_SHAPES = ((1, 4, 0), (2, 8, 0), (3, 8, 0), (5, 8, 0), (8, 8, 0), (8, 7, 0), (3, 6, 5), (3, 9, 0))
# 65 and 130 samples in one pair: header windows of 64 samples that end in the middle of a cycle of 3 or 7
LONG_SHAPES = ((3, 65, 0), (7, 65, 0), (3, 130, 0), (7, 130, 0))
# every other case: (buckets, samples), two samples a bucket at least
OTHER_CASES = {"grid_10nm": (3, 6), "grid_2p5nm": (2, 4), "gold_mirror": (2, 4), "many_lights": (2, 4), "deep_paths": (2, 4), "lens": (3, 6),
               "first_scene": (4, 8), "spheres_1500": (2, 4), "example_scene": (2, 4)}
RESOLVE_BUCKETS = (2, 3, 4, 7, 8)  # at 8 samples of BASE: the resolve for every legal trim

SHAPES = [(BASE, n, spp, first) for n, spp, first in BASE_SHAPES + LONG_SHAPES]
SHAPES += [(BASE, n, 8, 0) for n in RESOLVE_BUCKETS if (n, 8, 0) not in BASE_SHAPES]
SHAPES += [(name, n, spp, 0) for name, (n, spp) in OTHER_CASES.items()]

# shapes of tests/replay_shape_cases.py: (buckets, samples). blocks_4x64: a 4 x 64 tile in four row blocks, pairs of 4 samples;
# lds_s256: S = 256, four wavelength sets and a table that does not fit LDS
REPLAY_SHAPES = {"blocks_4x64": (3, 8), "lds_s256": (2, 4)}

_expected = {}


def expected_shape_films(name, cpu=False):
    """the rule's bucket films of a replay_shape_cases shape, from that module's shared per-sample renders"""
    import replay_shape_cases as RS
    key = ("shape", name, cpu)
    if key not in _expected:
        n, spp = REPLAY_SHAPES[name]
        bundle, params = RS.load(name)
        _expected[key] = bucket_rule.bucket_films(n, RS.contributions(name, bundle, params, cpu=cpu, spp=spp))
    return _expected[key]


def changes_for(spp, first=0, **more):
    c = dict(spp=spp, first_sample=first)
    c.update(more)
    return c


def expected_films(name, n, device=True, **changes):
    """the rule's n bucket films of the case: a list of (pixels, means, variances), shared and not to be written to"""
    key = (name, n, device, tuple(sorted(changes.items())))
    if key not in _expected:
        _, params = load(name)
        p = params_with(params, **changes)
        samples = (SC.samples_device if device else SC.samples_cpu)(name, **changes)
        _expected[key] = bucket_rule.bucket_films(n, samples, first_sample=int(p.first_sample))
    return _expected[key]


def expected_resolve(name, n, t, **changes):
    return bucket_rule.resolve([f[1] for f in expected_films(name, n, **changes)], t)


def bucket_counts(n, spp, first=0):
    """samples per bucket"""
    return [len([m for m in range(first, first + spp) if m % n == b]) for b in range(n)]


def assert_bucket_films(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert_film(g, w, "%s, bucket %d of %d" % (what, b, len(want)))
