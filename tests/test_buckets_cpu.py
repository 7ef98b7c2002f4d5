"""Bucket films without a GPU (-m "not gpu"): the premise of the rule on the oracle alone, that the bucket films of every shape the GPU
tests render tell buckets apart, the resolve on hand-made means, the C-ABI as the header, the compiler and pydrt see it, bucket_pair,
and the host program's refusals.

The rule (tests/bucket_rule.py): sample m goes through the reference's film update of bucket m % n as that
bucket's sample m // n; the resolve is the mean and the squared standard error across the buckets' means, and the trimmed mean of the
means sorted by an odd-even transposition network. Its input is the existing oracle's one-sample render; the premise checked here is
that with n = 1 the rule is the oracle's own multi-sample film, all three buffers, bit for bit."""
import ctypes as C
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import bucket_cases as BC
import bucket_rule
import cases
import pydrt

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")


@pytest.mark.parametrize("name", BC.CPU_CASES)
def test_one_bucket_is_the_oracles_own_film(name):
    bundle, params = BC.load(name)
    samples = BC.SC.samples_cpu(name)
    assert samples.shape == (int(params.spp), int(params.tile_w) * int(params.tile_h), bundle.S)
    (got,) = bucket_rule.bucket_films(1, samples)
    BC.assert_film(got, BC.film_cpu(name), "%s: the rule with one bucket against the oracle's film" % name)
    assert np.array_equal(got[0][:, -1], np.full(got[0].shape[0], float(params.spp)))
    if name != "first_scene":
        assert (got[2] != 0).any(), "a film without variance tells nothing about the running mean"


@pytest.mark.parametrize("name, n, spp, first", BC.SHAPES, ids=["%s-n%d-spp%d-from%d" % s for s in BC.SHAPES])
def test_the_bucket_films_tell_buckets_apart(name, n, spp, first):
    """A kernel that ignores the bucket, or takes a sample to the wrong one, must not pass: on the oracle (device arithmetic, the
    CPU's power), every two buckets that hold samples differ in sum and mean, and in the variance where both hold two samples or more.
    A bucket of one sample has a variance of exactly zero and an empty one is all zero, by the rule."""
    if n == 1:
        return  # one bucket: the premise above
    films = BC.expected_films(name, n, device=False, **BC.changes_for(spp, first))
    assert_apart(name, films, n, spp, first)


@pytest.mark.parametrize("name", sorted(BC.REPLAY_SHAPES))
def test_the_bucket_films_of_the_replay_shapes_tell_buckets_apart(name):
    n, spp = BC.REPLAY_SHAPES[name]
    assert_apart(name, BC.expected_shape_films(name, cpu=True), n, spp, 0)


def assert_apart(name, films, n, spp, first):
    counts = BC.bucket_counts(n, spp, first)
    assert sum(counts) == spp
    for b, (px, av, va) in enumerate(films):
        assert np.array_equal(px[:, -1], np.full(px.shape[0], float(counts[b]))), "the filter column is the bucket's sample count"
        if counts[b] == 0:
            assert not px.any() and not av.any() and not va.any()
        if counts[b] == 1 and name != "example_scene":
            assert not va.any(), "one sample: the variance accumulator stays zero"
    total = films[0][0][:, -1].copy()
    for b in range(1, n):
        total = total + films[b][0][:, -1]
    assert np.array_equal(total, np.full(total.shape, float(spp))), "the filter columns of the buckets sum to the sample count"
    if name == "example_scene":
        assert all(np.isnan(f[1]).all() for f in films)  # all NaN: exempt
        return
    for a, b in itertools.combinations(range(n), 2):
        if counts[a] == 0 or counts[b] == 0:
            continue
        assert not cases.same_bits(films[a][0][:, :-1], films[b][0][:, :-1]), "buckets %d and %d hold the same sums" % (a, b)
        assert not cases.same_bits(films[a][1], films[b][1]), "buckets %d and %d hold the same means" % (a, b)
        if counts[a] >= 2 and counts[b] >= 2:
            assert not cases.same_bits(films[a][2], films[b][2]), "buckets %d and %d hold the same variances" % (a, b)


def test_the_film_update_divides_by_the_samples_number_inside_its_bucket():
    c = [np.array([[3.0, -1.0]]), np.array([[10.0, 20.0]]), np.array([[1.0, 0.5]]), np.array([[30.0, 40.0]]), np.array([[2.0, -0.25]])]
    films = bucket_rule.bucket_films(2, np.stack(c))
    (px0, av0, va0), (px1, av1, va1) = films
    # bucket 0: samples 0, 2, 4 with divisors 1, 2, 3; bucket 1: samples 1, 3 with divisors 1, 2
    assert np.array_equal(px0, [[6.0, -0.75, 3.0]]) and np.array_equal(av0, [[2.0, -0.25]]) and np.array_equal(va0, [[2.0, 1.125]])
    assert np.array_equal(px1, [[40.0, 60.0, 2.0]]) and np.array_equal(av1, [[20.0, 30.0]]) and np.array_equal(va1, [[200.0, 200.0]])
    # a render continued at sample 5 goes on in bucket 1 with divisor 3, and one that starts at sample 5 does the same on a zero film
    bucket_rule.bucket_films(2, np.array([[[5.0, 0.0]]]), first_sample=5, films=films)
    assert np.array_equal(films[1][1], [[15.0, 20.0]]) and films[1][0][0, 2] == 3.0 and films[0][0][0, 2] == 3.0
    fresh = bucket_rule.bucket_films(3, np.array([[[6.0, 9.0]]]), first_sample=5)
    assert np.array_equal(fresh[2][1], [[3.0, 4.5]]) and not fresh[0][0].any() and not fresh[1][0].any()


def by_hand(x, t):
    """steps 1 to 4 for one value per bucket, python floats, written out apart from bucket_rule"""
    n = len(x)
    mu = x[0]
    for b in range(1, n):
        mu = mu + x[b]
    mu = mu / float(n)
    q = (x[0] - mu) * (x[0] - mu)
    for b in range(1, n):
        q = q + (x[b] - mu) * (x[b] - mu)
    y = list(x)
    for r in range(n):
        i = r % 2
        while i < n - 1:
            if y[i + 1] < y[i]:
                y[i], y[i + 1] = y[i + 1], y[i]
            i += 2
    e = y[t]
    for i in range(t + 1, n - t):
        e = e + y[i]
    return e / float(n - 2 * t), q / float(n * (n - 1)), y


@pytest.mark.parametrize("n", range(2, 9))
def test_the_resolve_for_every_bucket_count_and_trim(n):
    rng = np.random.default_rng(n)
    means = rng.uniform(0.0, 4.0, size=(n, 40, 7)) * 10.0 ** rng.integers(-6, 6, size=(n, 40, 7))
    assert bucket_rule.legal_trims(n) == list(range((n + 1) // 2))
    for t in bucket_rule.legal_trims(n):
        est, err = bucket_rule.resolve(means, t)
        assert est.shape == err.shape == (40, 7)
        for p in range(0, 40, 7):
            for k in range(7):
                e, q, _ = by_hand([float(v) for v in means[:, p, k]], t)
                assert est[p, k] == e and err[p, k] == q
        # the sorted means really are sorted, and the error does not depend on t
        y = np.stack(bucket_rule.sort_network(means))
        assert (np.diff(y, axis=0) >= 0).all() and np.array_equal(np.sort(means, axis=0), y)
        assert np.array_equal(err, bucket_rule.resolve(means, 0)[1])
    # the median (n odd) and the mean of the two middle values (n even)
    t = bucket_rule.median_trim(n)
    est, _ = bucket_rule.resolve(means, t)
    s = np.sort(means, axis=0)
    want = s[n // 2] / 1.0 if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0
    assert np.array_equal(est, want)


def test_sorted_order_and_bucket_order_give_different_sums():
    # in bucket order (1 + 2^-53) + 2^-53 rounds both halves away; sorted, (2^-53 + 2^-53) + 1 keeps them
    x = [1.0, 2.0 ** -53, 2.0 ** -53]
    est, err = bucket_rule.resolve([np.array([v]) for v in x], 0)
    mu = ((x[0] + x[1]) + x[2]) / 3.0
    assert mu == 1.0 / 3.0 and est[0] == (1.0 + 2.0 ** -52) / 3.0 and est[0] != mu
    # the error is made from the mean in BUCKET order
    d = [v - mu for v in x]
    assert err[0] == ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / 6.0


@pytest.mark.parametrize("n", range(3, 9))
def test_a_planted_outlier_is_left_out_by_every_trim_but_zero(n):
    for at in range(n):
        x = [1.0 + 0.01 * k for k in range(n)]
        x[at] = 1e6
        means = [np.array([v]) for v in x]
        with_it, _ = bucket_rule.resolve(means, 0)
        assert with_it[0] > 1e6 / n
        for t in bucket_rule.legal_trims(n)[1:]:
            est, err = bucket_rule.resolve(means, t)
            assert 1.0 <= est[0] <= 1.0 + 0.01 * n, "n = %d, trim %d: the outlier at bucket %d is in the estimate" % (n, t, at)
            assert err[0] > 1e9  # the error is of the plain mean, whatever t is


def test_nan_infinities_and_signed_zeros_end_up_where_the_network_puts_them():
    nan, inf = np.nan, np.inf

    def run(x, t):
        est, err = bucket_rule.resolve([np.array([v]) for v in x], t)
        y = [float(v[0]) for v in bucket_rule.sort_network([np.array([v]) for v in x])]
        return float(est[0]), float(err[0]), y

    def same(a, b):
        return cases.same_bits(np.array(a), np.array(b))

    # infinities sort as numbers: -inf first, +inf last, and a trim of 1 leaves both out
    est, err, y = run([inf, 2.0, -inf, 1.0, 3.0], 1)
    assert same(y, [-inf, 1.0, 2.0, 3.0, inf]) and est == 2.0 and np.isnan(err)  # (inf + -inf in the mean)
    est, err, y = run([inf, 2.0, 5.0, 1.0], 0)
    assert same(y, [1.0, 2.0, 5.0, inf]) and est == inf and np.isnan(err)  # (inf - inf in d_0)
    # a NaN never changes places: n = 3, rounds (0,1) (1,2) (0,1)
    #   [3, NaN, 1]: 3 | NaN stays, NaN | 1 stays, 3 | NaN stays -> as it came: the NaN is a wall, and 3 and 1 never meet
    est, err, y = run([3.0, nan, 1.0], 1)
    assert same(y, [3.0, nan, 1.0]) and np.isnan(est) and np.isnan(err)
    #   [NaN, 3, 1]: round 0 nothing, round 1 exchanges 3 and 1, round 2 nothing -> [NaN, 1, 3]; the median is 1
    est, err, y = run([nan, 3.0, 1.0], 1)
    assert same(y, [nan, 1.0, 3.0]) and est == 1.0 and np.isnan(err)
    #   [3, 1, NaN]: round 0 exchanges 3 and 1 -> [1, 3, NaN]; the median is 3
    est, err, y = run([3.0, 1.0, nan], 1)
    assert same(y, [1.0, 3.0, nan]) and est == 3.0
    #   n = 4, [2, NaN, 1, 0]: rounds (0,1)(2,3) | (1,2) | (0,1)(2,3) | (1,2): only 1 and 0 ever change places
    est, err, y = run([2.0, nan, 1.0, 0.0], 1)
    assert same(y, [2.0, nan, 0.0, 1.0]) and np.isnan(est)
    # -0 < +0 is false: zeros keep the order they came in, and the sum of the trimmed range shows which came first
    est, err, y = run([0.0, -0.0], 0)
    assert same(y, [0.0, -0.0]) and same([est], [0.0]) and same([err], [0.0])
    est, err, y = run([-0.0, 0.0, -0.0], 1)
    assert same(y, [-0.0, 0.0, -0.0]) and same([est], [0.0])
    est, err, y = run([-0.0, -0.0, 0.0], 1)
    assert same(y, [-0.0, -0.0, 0.0]) and same([est], [-0.0])
    est, err, y = run([-0.0, -0.0], 0)
    assert same([est], [-0.0]) and same([err], [0.0])  # mu = -0, d = -0 - -0 = +0
    # a negative number passes the zeros
    est, err, y = run([0.0, -0.0, -1.0], 1)
    assert same(y, [-1.0, 0.0, -0.0]) and same([est], [0.0])


def test_bucket_pair_is_the_plain_mean_of_each_half():
    rng = np.random.default_rng(3)
    for n in range(2, 9):
        m = rng.uniform(0.0, 2.0, size=(n, 6, 5))
        even, odd = pydrt.bucket_pair(m)
        we, wo = m[0].copy(), m[1].copy()
        for k in range(2, n, 2):
            we = we + m[k]
        for k in range(3, n, 2):
            wo = wo + m[k]
        assert np.array_equal(even, we / float((n + 1) // 2)) and np.array_equal(odd, wo / float(n // 2))
        assert even.shape == odd.shape == (6, 5)
    a, b = pydrt.bucket_pair([[1.0, 2.0], [3.0, 5.0]])
    assert np.array_equal(a, [1.0, 2.0]) and np.array_equal(b, [3.0, 5.0])
    before = m.copy()
    pydrt.bucket_pair(m)
    assert np.array_equal(m, before)
    for bad in (np.zeros((1, 4)), np.zeros(()), []):
        with pytest.raises(ValueError, match="bucket_pair"):
            pydrt.bucket_pair(bad)


CALLS = {
    "drt_bind_buckets": "int (*%s)(drt_context *, uint32_t)",
    "drt_read_bucket_film": "int (*%s)(drt_context *, uint32_t, double *, double *, double *)",
    "drt_bucket_film_device_ptrs": "int (*%s)(drt_context *, uint32_t, void **, void **, void **)",
    "drt_resolve_buckets": "int (*%s)(drt_context *, uint32_t)",
    "drt_read_bucket_resolve": "int (*%s)(drt_context *, double *, double *)",
    "drt_bucket_resolve_device_ptrs": "int (*%s)(drt_context *, void **, void **)",
    "drt_read_bucket_resolve_xyz": "int (*%s)(drt_context *, double *)",
    "drt_read_bucket_resolve_bgra": "int (*%s)(drt_context *, uint8_t *)",
    "drt_group_bind_buckets": "int (*%s)(drt_group *, uint32_t)",
    "drt_group_read_bucket_film": "int (*%s)(drt_group *, uint32_t, double *, double *, double *)",
    "drt_group_resolve_buckets": "int (*%s)(drt_group *, uint32_t)",
    "drt_group_read_bucket_resolve": "int (*%s)(drt_group *, double *, double *)",
}


def test_the_header_the_compiler_and_pydrt_agree_on_the_calls(tmp_path):
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for call in CALLS:
        assert re.search(r"\bint %s\(" % call, plain) and call in pydrt.HIP_SYMBOLS, call
    assert re.search(r"#define DRT_MAX_BUCKETS\s+8\b", header) and pydrt.MAX_BUCKETS == 8 and bucket_rule.MAX_BUCKETS == 8
    src = tmp_path / "buckets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "drt_hip.h"\n'
                   + "".join("%s = %s;\n" % (proto % ("f%d" % k), call) for k, (call, proto) in enumerate(CALLS.items()))
                   + 'int main(void) { printf("%d\\n", DRT_MAX_BUCKETS); return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "buckets.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = pydrt.hip_lib()
    f64p, vpp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_uint8)
    assert L.drt_bind_buckets.argtypes == [C.c_void_p, C.c_uint32]
    assert L.drt_read_bucket_film.argtypes == [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
    assert L.drt_bucket_film_device_ptrs.argtypes == [C.c_void_p, C.c_uint32, vpp, vpp, vpp]
    assert L.drt_resolve_buckets.argtypes == [C.c_void_p, C.c_uint32]
    assert L.drt_read_bucket_resolve.argtypes == [C.c_void_p, f64p, f64p]
    assert L.drt_bucket_resolve_device_ptrs.argtypes == [C.c_void_p, vpp, vpp]
    assert L.drt_read_bucket_resolve_xyz.argtypes == [C.c_void_p, f64p]
    assert L.drt_read_bucket_resolve_bgra.argtypes == [C.c_void_p, u8p]
    assert L.drt_group_bind_buckets.argtypes == [C.c_void_p, C.c_uint32]
    assert L.drt_group_read_bucket_film.argtypes == [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
    assert L.drt_group_resolve_buckets.argtypes == [C.c_void_p, C.c_uint32]
    assert L.drt_group_read_bucket_resolve.argtypes == [C.c_void_p, f64p, f64p]
    # a null context or group is refused with a message, without a device
    assert L.drt_bind_buckets(None, 0) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_read_bucket_film(None, 0, None, None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_bucket_film_device_ptrs(None, 0, None, None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_resolve_buckets(None, 0) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_read_bucket_resolve(None, None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_bucket_resolve_device_ptrs(None, None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_read_bucket_resolve_xyz(None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_read_bucket_resolve_bgra(None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_group_bind_buckets(None, 0) != 0 and b"null group" in L.drt_last_error()
    assert L.drt_group_read_bucket_film(None, 0, None, None, None) != 0 and b"null group" in L.drt_last_error()
    assert L.drt_group_resolve_buckets(None, 0) != 0 and b"null group" in L.drt_last_error()
    assert L.drt_group_read_bucket_resolve(None, None, None) != 0 and b"null group" in L.drt_last_error()


def test_pydrt_signatures_and_the_checks_it_alone_can_make():
    for cls in (pydrt.Renderer, pydrt.Group):
        assert list(inspect.signature(cls.bind_buckets).parameters) == ["self", "n"]
        assert list(inspect.signature(cls.read_bucket_film).parameters) == ["self", "b"]
        assert list(inspect.signature(cls.resolve_buckets).parameters) == ["self", "trim"]
        assert inspect.signature(cls.resolve_buckets).parameters["trim"].default is None
        assert list(inspect.signature(cls.read_bucket_resolve).parameters) == ["self"]
    assert list(inspect.signature(pydrt.Renderer.bucket_film_device_ptrs).parameters) == ["self", "b"]
    for name in ("bucket_resolve_device_ptrs", "read_bucket_resolve_xyz", "read_bucket_resolve_bgra"):
        assert list(inspect.signature(getattr(pydrt.Renderer, name)).parameters) == ["self"]
    assert list(inspect.signature(pydrt.bucket_pair).parameters) == ["means"]
    # what ctypes would wrap around is refused before the call; nine buckets pass here: the count is the library's to refuse
    assert pydrt._u32(9, "n") == 9 and pydrt._u32(np.uint32(3), "n") == 3
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="bind_buckets: n"):
            pydrt._u32(bad, "bind_buckets: n")


@pytest.mark.parametrize("env, message", [
    ({"DRT_BUCKETS": ""}, "n or n,trim in whole numbers"),
    ({"DRT_BUCKETS": "four"}, "n or n,trim in whole numbers"),
    ({"DRT_BUCKETS": "4,"}, "n or n,trim in whole numbers"),
    ({"DRT_BUCKETS": "4,1,0"}, "n or n,trim in whole numbers"),
    ({"DRT_BUCKETS": "4;1"}, "n or n,trim in whole numbers"),
    ({"DRT_BUCKETS": "-2"}, "n or n,trim in whole numbers"),
    ({"DRT_BUCKETS": "0"}, "DRT_BUCKETS: 0 buckets: from 1 to 8"),
    ({"DRT_BUCKETS": "9"}, "DRT_BUCKETS: 9 buckets: from 1 to 8"),
    ({"DRT_BUCKETS": "4,2"}, "a trim of 2 leaves nothing of 4 buckets"),
    ({"DRT_BUCKETS": "3,2"}, "a trim of 2 leaves nothing of 3 buckets"),
    ({"DRT_BUCKETS": "1,0"}, "one bucket has nothing to resolve, and so no trim"),
    ({"DRT_BUCKETS": "8", "SAMPLES": "7"}, "8 buckets of num_pixel_samples = 7 samples"),
    ({"DRT_BUCKETS": "2", "LONG_NAME": "1"}, "an output name with .bucket1.spd or .robust.spd behind it is longer than 63 characters"),
    ({"DRT_BUCKETS": "2", "DRT_ADAPTIVE_ERROR": "0.1"}, "DRT_BUCKETS cannot be combined with DRT_ADAPTIVE_ERROR"),
    ({"DRT_BUCKETS": "2", "DRT_CHECKPOINT_SPP": "1"}, "DRT_BUCKETS cannot be combined with DRT_CHECKPOINT_SPP"),
    ({"DRT_BUCKETS": "2", "DRT_RESUME": "1"}, "DRT_BUCKETS cannot be combined with DRT_RESUME"),
    ({"DRT_BUCKETS": "2", "DRT_TURNTABLE": "2"}, "DRT_BUCKETS cannot be combined with DRT_TURNTABLE"),
    ({"DRT_BUCKETS": "2", "DRT_LIGHT_LEVELS": "1,2"}, "DRT_BUCKETS cannot be combined with DRT_LIGHT_LEVELS"),
    ({"DRT_BUCKETS": "2", "DRT_DEPTH_CUTS": "1,2"}, "DRT_BUCKETS cannot be combined with DRT_DEPTH_CUTS"),
    ({"DRT_BUCKETS": "2", "DRT_SENSOR": "r.csv"}, "DRT_BUCKETS cannot be combined with DRT_SENSOR"),
    ({"DRT_BUCKETS": "2", "DRT_REGIONS": "0,0,4,4:8"}, "DRT_BUCKETS cannot be combined with DRT_REGIONS"),
])
def test_the_host_refuses_bad_buckets_before_any_device_call(tmp_path, env, message):
    """Exit status nonzero, the reason on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run that got as
    far as the launcher would fail there with the launcher's message instead."""
    cfg = open(os.path.join(REPO, "config.cfg")).read()
    env = dict(env)
    if env.pop("LONG_NAME", None):
        cfg, k = re.subn(r"(?m)^variance_spd\s+\S+", "variance_spd      output/" + "v" * 44 + ".spd", cfg)  # fits by itself, not with .robust
        assert k == 1
    samples = env.pop("SAMPLES", None)
    if samples:
        cfg, k = re.subn(r"(?m)^num_pixel_samples\s+\S+", "num_pixel_samples %s" % samples, cfg)
        assert k == 1
    (tmp_path / "config.cfg").write_text(cfg)
    os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
    os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    (tmp_path / "r.csv").write_text("wavelength,value\n380,0\n600,1\n720,0.5\n")
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout
