"""GPU (-m gpu): bucket films and their resolve (drt_bind_buckets, drt_resolve_buckets).

The rule is tests/bucket_rule.py: sample m goes through the reference's film update of bucket m % n as that bucket's sample m // n; the
resolve is the mean and squared standard error across the buckets' means and the trimmed mean of the means sorted by the odd-even
transposition network. Its input is the oracle's one-sample render of every sample (sensor_cases.samples_device). Every test compares
all three buffers of every bucket film with cases.same_bits, and the main film against the oracle; there is no tolerance anywhere.
tests/test_buckets_cpu.py shows on the oracle alone that with one bucket the rule is the oracle's own film, and that in every shape
rendered here the buckets differ from one another. Cases are at most 32 x 32 pixels (one replay shape is 4 x 64)."""
import contextlib
import gc
import os
import subprocess

import numpy as np
import pytest

import bucket_cases as BC
import bucket_rule
import cases
import oracle_py as O
import pydrt

pytestmark = pytest.mark.gpu

BASE = BC.BASE


@contextlib.contextmanager
def environment(**knobs):
    saved = {k: os.environ.get(k) for k in knobs}
    try:
        for k, v in knobs.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def read_buckets(r, n):
    return [r.read_bucket_film(b) for b in range(n)]


def render_with_buckets(bundle, params, n, calls=None, before_render=None, after=None):
    """(main film, [bucket films], stats, batch_spp) of a fresh context bound to n buckets; after(r): more to do before it closes"""
    r = pydrt.Renderer(bundle, params)
    try:
        if before_render:
            before_render(r)
        r.bind_buckets(n)
        for first, count in (calls or [(None, None)]):
            r.render(first, count)
        out = r.read_film(), read_buckets(r, n), r.stats(), r.batch_spp()
        if after:
            after(r)
        return out
    finally:
        r.close()


def check_case(name, n, what, calls=None, before_render=None, after=None, **changes):
    bundle, params = BC.load(name)
    p = BC.params_with(params, **changes)
    main, films, st, batch = render_with_buckets(bundle, p, n, calls=calls, before_render=before_render, after=after)
    oracle = {k: v for k, v in changes.items() if k != "batch_spp"}
    BC.assert_film(main, BC.film_device(name, **oracle)[:3], "%s: %s, the main film against the oracle" % (what, name))
    BC.assert_bucket_films(films, BC.expected_films(name, n, **oracle), "%s: %s" % (what, name))
    return main, films, st, batch


# ------------------------------------------------------------------------------------------------ plane_light_16
def test_one_bucket_is_the_main_film():
    main, films, _, _ = check_case(BASE, 1, "one bucket")
    BC.assert_film(films[0], main, "the bucket film against the main film from the device alone")
    assert (main[2] != 0).any()


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_eight_samples_in_n_buckets(n):
    _, films, _, _ = check_case(BASE, n, "8 samples in %d buckets" % n, **BC.changes_for(8))
    for b, count in enumerate(BC.bucket_counts(n, 8)):
        assert np.array_equal(films[b][0][:, -1], np.full(films[b][0].shape[0], float(count)))


def test_seven_samples_in_eight_buckets_leave_one_empty_and_nothing_to_resolve():
    def after(r):
        before = r.read_film(), read_buckets(r, 8), cases.stat_counts(r.stats())
        with pytest.raises(RuntimeError, match="holds 7 samples, fewer than its 8 buckets"):
            r.resolve_buckets(0)
        with pytest.raises(RuntimeError, match="nothing is resolved yet"):
            r.read_bucket_resolve()
        BC.assert_film(r.read_film(), before[0], "the main film across the refusal")
        BC.assert_bucket_films(read_buckets(r, 8), before[1], "across the refusal")
        assert cases.stat_counts(r.stats()) == before[2]
        # the eighth sample fills the last bucket
        r.render(7, 1)
        r.resolve_buckets(0)
        est, err = r.read_bucket_resolve()
        want = BC.expected_resolve(BASE, 8, 0, **BC.changes_for(8))
        assert cases.same_bits(est, want[0]) and cases.same_bits(err, want[1])

    _, films, _, _ = check_case(BASE, 8, "7 samples in 8 buckets", after=after, **BC.changes_for(7))
    assert not any(a.any() for a in films[7]), "the empty bucket stays all zero"
    assert all(f[0][:, -1].all() for f in films[:7])


def test_a_launch_that_starts_in_the_middle_of_a_cycle():
    """first_sample = 5, 6 samples, 3 buckets: the first sample belongs to bucket 2 as its sample 1"""
    _, films, st, _ = check_case(BASE, 3, "samples 5..10 in 3 buckets", **BC.changes_for(6, 5))
    assert st.launches == 1
    assert [float(f[0][0, -1]) for f in films] == [2.0, 2.0, 2.0]


@pytest.mark.parametrize("batch", [1, 3])
def test_several_calls_and_small_batches_continue_every_bucket(batch):
    """render(0, 3); render(3, 5); render(8, 1) in pairs of 1 and of 3 samples: every launch starts where the last one stopped"""
    _, _, st, got = check_case(BASE, 3, "three calls, batch_spp %d" % batch, calls=[(0, 3), (3, 5), (8, 1)], **BC.changes_for(9, batch_spp=batch))
    assert got == batch and st.launches == {1: 9, 3: 4}[batch]


@pytest.mark.parametrize("n", [3, 7])
@pytest.mark.parametrize("spp", [65, 130])
def test_header_windows_that_end_in_the_middle_of_a_cycle(spp, n):
    """one pair of 65 or 130 samples: windows of 64 headers, and 64 is no multiple of 3 or 7"""
    _, _, st, batch = check_case(BASE, n, "%d samples in one pair, %d buckets" % (spp, n), **BC.changes_for(spp))
    assert batch >= spp and st.launches == 1, "one kernel pair is meant to take all %d samples (batch_spp %d, %d pairs)" % (spp, batch, st.launches)


@pytest.mark.parametrize("n", [3, 7])
def test_a_second_call_of_65_samples_starts_at_sample_65(n):
    _, _, st, _ = check_case(BASE, n, "two calls of 65 samples, %d buckets" % n, calls=[(0, 65), (65, 65)], **BC.changes_for(130))
    assert st.launches == 2


# ------------------------------------------------------------------------------------------------ the other cases
@pytest.mark.parametrize("name", sorted(BC.OTHER_CASES))
def test_every_case_against_the_rule(name):
    n, spp = BC.OTHER_CASES[name]
    bundle, _ = BC.load(name)
    _, films, st, _ = check_case(name, n, "%d buckets" % n, **BC.changes_for(spp))
    if name == "grid_2p5nm":
        assert bundle.S == 137  # three wavelength sets
    # (many_lights: 12 lights, vertex records of 128 words, so light blocks beyond the 64 words a wave fetches)
    if name == "spheres_1500":
        assert st.path_flags & pydrt.PATH_BVH, "spheres_1500 is meant to go through the hierarchy pipeline"
    if name == "example_scene":
        for b, count in enumerate(BC.bucket_counts(n, spp)):
            assert np.isnan(films[b][0][:, :-1]).all() and np.isnan(films[b][1]).all()
            assert np.array_equal(films[b][0][:, -1], np.full(films[b][0].shape[0], float(count)))
    else:
        assert cases.stat_counts(st) == cases.stat_counts(BC.film_device(name, **BC.changes_for(spp))[4])


# ------------------------------------------------------------------------------------------------ configurations
def test_a_record_pool_that_runs_out_is_rendered_again_bucket_films_included(monkeypatch):
    """DRT_POOL_BLOCKS=1: the launches that ran out leave the bucket films untouched, as the main film, and are rendered again"""
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    _, _, st, _ = check_case(BASE, 3, "tiny record pool", **BC.changes_for(8))
    assert st.redone_launches > 0, "no launch ran out of record blocks"


def test_behind_a_forced_hierarchy():
    with environment(DRT_FORCE_BVH="1"):
        _, _, st, _ = check_case(BASE, 3, "DRT_FORCE_BVH", **BC.changes_for(8))
    assert st.path_flags & pydrt.PATH_BVH


def shape_case(name):
    import replay_shape_cases as RS
    n, spp = BC.REPLAY_SHAPES[name]
    bundle, params = RS.load(name)
    p = RS.params_with(params, spp=spp)
    main, films, st, batch = render_with_buckets(bundle, p, n)
    RS.assert_film(main, RS.oracle_film(name, bundle, params, spp=spp), "%s: the main film against the oracle" % name)
    BC.assert_bucket_films(films, BC.expected_shape_films(name), name)
    return bundle, p, st, batch


def test_a_4_x_64_tile_in_row_blocks():
    """four row blocks of 16 rows, each in pairs of 4 samples: the bucket films start at the block's first pixel, and a block's second
    pair starts at sample 4, in bucket 1 of 3"""
    import replay_shape_cases as RS
    with environment(DRT_NO_ROW_BLOCKS=None, DRT_POOL_BLOCKS=None):
        _, p, st, _ = shape_case("blocks_4x64")
    plan = RS.BLOCK_PLANS["blocks_4x64"]
    assert (int(p.tile_w), int(p.tile_h)) == (4, 64) and st.launches == plan["blocks"] * len(plan["pairs"]) and st.redone_launches == 0


def test_a_table_outside_lds_and_four_wavelength_sets():
    """S = 256: drt_bucket_kernel<2, false>, four items per pixel"""
    import replay_shape_cases as RS
    bundle, _, _, _ = shape_case("lds_s256")
    assert bundle.S == 256 and RS.table_bytes(bundle) > RS.LDS_BYTES


def test_a_ray_table_of_the_cameras_centre_rays():
    import ray_film_cases as R
    bundle, params = BC.load(BASE)
    table = R.centre_rays(bundle, int(params.width), int(params.height))
    _, _, st, _ = check_case(BASE, 3, "ray table", before_render=lambda r: r.bind_rays(*table), **BC.changes_for(8, pixel_scheme=pydrt.FILM_SAMPLE_CENTER))
    assert st.path_flags & pydrt.PATH_RAYS


def test_after_update_materials_and_reset_film_the_bucket_films_are_a_fresh_contexts():
    bundle, params = BC.load(BASE)
    p = BC.params_with(params, spp=8)
    text = open(cases.scene_path(cases.RENDER_CASES[BASE][0])).read()
    assert "shininess 100.0" in text
    after = pydrt.load_scene_text(text.replace("shininess 100.0", "shininess 30.0"), int(params.width), int(params.height))
    fresh_main, fresh_films, _, _ = render_with_buckets(after, p, 3)
    r = pydrt.Renderer(bundle, p)
    try:
        r.bind_buckets(3)
        r.render()
        before = read_buckets(r, 3)
        r.resolve_buckets(1)
        r.reset_film()
        with pytest.raises(RuntimeError, match="the film has changed since the last resolve"):
            r.read_bucket_resolve()
        with pytest.raises(RuntimeError, match="holds 0 samples"):
            r.resolve_buckets(1)
        r.update_materials(after.materials())
        assert not any(a.any() for f in read_buckets(r, 3) for a in f), "drt_reset_film zeroes the bucket films"
        r.render()
        main, films = r.read_film(), read_buckets(r, 3)
    finally:
        r.close()
    BC.assert_film(main, fresh_main, "updated context against a fresh one, main film")
    BC.assert_bucket_films(films, fresh_films, "updated context against a fresh one")
    BC.assert_bucket_films(before, BC.expected_films(BASE, 3, **BC.changes_for(8)), "before the update")
    assert not cases.same_bits(before[0][0], films[0][0]), "the update changes the film"


def test_a_groups_assembled_bucket_films_and_resolve_are_a_single_contexts():
    bundle, params = BC.load(BASE)
    p = BC.params_with(params, spp=8)
    want = BC.expected_films(BASE, 3, **BC.changes_for(8))
    g = pydrt.Group(bundle, p, devices=[0, 0, 0])
    try:
        with pytest.raises(RuntimeError, match="no buckets are bound"):
            g.read_bucket_film(0)
        with pytest.raises(RuntimeError, match="9 buckets, at most 8"):
            g.bind_buckets(9)
        g.bind_buckets(3)
        with pytest.raises(RuntimeError, match="holds 0 samples"):
            g.resolve_buckets(1)
        g.render()
        main, films = g.read_film(), [g.read_bucket_film(b) for b in range(3)]
        with pytest.raises(RuntimeError, match="bucket 3 of 3"):
            g.read_bucket_film(3)
        with pytest.raises(RuntimeError, match="nothing is resolved yet"):
            g.read_bucket_resolve()
        with pytest.raises(RuntimeError, match="trim = 2 leaves nothing of 3 buckets"):
            g.resolve_buckets(2)
        g.resolve_buckets()  # the median's trim
        est, err = g.read_bucket_resolve()
        with pytest.raises(RuntimeError, match="drt_reset_film first"):
            g.bind_buckets(2)
        with pytest.raises(RuntimeError, match="buckets are bound"):
            g.bind_depth_cuts([1])
        with pytest.raises(RuntimeError, match="buckets are bound"):
            g.bind_sensor(np.ones((1, bundle.S)))
        BC.assert_bucket_films([g.read_bucket_film(b) for b in range(3)], films, "after the group's refusals")
        g.reset_film()
        g.bind_buckets(0)
        with pytest.raises(RuntimeError, match="no buckets are bound"):
            g.read_bucket_film(0)
    finally:
        g.close()
    BC.assert_film(main, BC.film_device(BASE, **BC.changes_for(8))[:3], "a group of three contexts, the main film")
    BC.assert_bucket_films(films, want, "a group of three contexts")
    w_est, w_err = BC.expected_resolve(BASE, 3, 1, **BC.changes_for(8))
    assert cases.same_bits(est, w_est), cases.first_difference(est, w_est)
    assert cases.same_bits(err, w_err), cases.first_difference(err, w_err)


def test_binding_buckets_changes_nothing_else():
    """the main film, the statistics' counts and the hit log: the same bits with buckets bound and without"""
    bundle, params = BC.load(BASE)
    p = BC.params_with(params, spp=8, flags=pydrt.FLAG_RECORD_HITS)
    out = []
    for n in (0, 3):
        r = pydrt.Renderer(bundle, p)
        try:
            r.bind_buckets(n)
            r.render()
            out.append((r.read_film(), r.read_hit_indices(8), r.stats(), r.read_xyz()))
            if n:
                BC.assert_bucket_films(read_buckets(r, n), BC.expected_films(BASE, n, **BC.changes_for(8)), "with DRT_FLAG_RECORD_HITS")
        finally:
            r.close()
    (film0, hits0, st0, xyz0), (film1, hits1, st1, xyz1) = out
    BC.assert_film(film1, film0, "the main film with buckets bound against without")
    assert np.array_equal(hits0, hits1) and cases.same_bits(xyz0, xyz1)
    assert np.array_equal(hits0, BC.film_device(BASE, **BC.changes_for(8))[3])
    assert cases.stat_counts(st0) == cases.stat_counts(st1) and st0.launches == st1.launches


# ------------------------------------------------------------------------------------------------ the resolve
def host_bgra(bundle, width, height, mean, tmp_path):
    """the pixel bytes host/drt_bmp.c gives a spectral film without a filter column (as tests/test_gpu_denoise.py)"""
    import ctypes as C
    H = pydrt.host_lib()
    f64p = C.POINTER(C.c_double)
    H.drt_host_spd_file_to_bmp.argtypes = [C.c_char_p, C.c_char_p, f64p]
    H.drt_host_write_spd.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, f64p]
    sc = bundle.scene
    spd, bmp = str(tmp_path / "mean.spd"), str(tmp_path / "mean.bmp")
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    assert H.drt_host_write_spd(spd.encode(), width, height, bundle.S, 0, float(sc.min_wavelength), float(sc.wavelength_interval),
                                mean.ctypes.data_as(f64p)) == 0
    rows = [int(sc.cmf_rw), int(sc.cmf_x), int(sc.cmf_y), int(sc.cmf_z)]
    cmf = np.ascontiguousarray(bundle.spds()[rows])
    assert H.drt_host_spd_file_to_bmp(spd.encode(), bmp.encode(), cmf.ctypes.data_as(f64p)) == 0
    return np.frombuffer(open(bmp, "rb").read()[54:], dtype=np.uint8).reshape(-1, 4)


@pytest.mark.parametrize("n", BC.RESOLVE_BUCKETS)
def test_estimate_and_error_for_every_legal_trim(n, tmp_path):
    bundle, params = BC.load(BASE)
    p = BC.params_with(params, spp=8)
    trims = bucket_rule.legal_trims(n)
    r = pydrt.Renderer(bundle, p)
    try:
        r.bind_buckets(n)
        r.render()
        films = read_buckets(r, n)
        got = []
        for t in trims:
            r.resolve_buckets(t)
            got.append(r.read_bucket_resolve())
        ptrs = r.bucket_resolve_device_ptrs()
        film_ptrs = [r.bucket_film_device_ptrs(b) for b in range(n)]
        assert all(ptrs) and len(set(ptrs) | {q for f in film_ptrs for q in f} | set(r.film_device_ptrs())) == 2 + 3 * n + 3
        # the readouts of the last trim, and the default trim is the median's
        xyz, bgra = r.read_bucket_resolve_xyz(), r.read_bucket_resolve_bgra()
        r.resolve_buckets()
        median = r.read_bucket_resolve()
        for bad in (trims[-1] + 1, n):
            with pytest.raises(RuntimeError, match="trim = %d leaves nothing of %d buckets" % (bad, n)):
                r.resolve_buckets(bad)
        again = r.read_bucket_resolve()  # a refused resolve leaves the last one readable
    finally:
        r.close()
    BC.assert_bucket_films(films, BC.expected_films(BASE, n, **BC.changes_for(8)), "%d buckets" % n)
    means = [f[1] for f in films]
    for t, (est, err) in zip(trims, got):
        w_est, w_err = BC.expected_resolve(BASE, n, t, **BC.changes_for(8))
        assert cases.same_bits(est, w_est), "n = %d, trim %d, estimate: %s" % (n, t, cases.first_difference(est, w_est))
        assert cases.same_bits(err, w_err), "n = %d, trim %d, error: %s" % (n, t, cases.first_difference(err, w_err))
        d_est, d_err = bucket_rule.resolve(means, t)  # and from the device's own means
        assert cases.same_bits(est, d_est) and cases.same_bits(err, d_err)
    assert (got[0][1] != 0).any() and (len(trims) == 1 or not cases.same_bits(got[0][0], got[-1][0]))
    t = bucket_rule.median_trim(n)
    assert t == trims[-1] and cases.same_bits(median[0], got[-1][0]) and cases.same_bits(median[1], got[-1][1])
    assert cases.same_bits(again[0], median[0]) and cases.same_bits(again[1], median[1])
    # the conversions: the existing kernels' rules applied to the estimate (a filter column of 1: x / 1 is x)
    est = got[-1][0]
    want_xyz = O.oracle_film_to_xyz(bundle, np.concatenate([est, np.ones((est.shape[0], 1))], axis=1))
    assert cases.same_bits(xyz, want_xyz), "XYZ of the estimate: %s" % cases.first_difference(xyz, want_xyz)
    want_bgra = host_bgra(bundle, int(p.tile_w), int(p.tile_h), est, tmp_path)
    assert np.array_equal(bgra, want_bgra) and len(np.unique(bgra[:, :3])) > 20


def test_a_resolve_then_a_render_then_a_readout_is_refused():
    bundle, params = BC.load(BASE)
    r = pydrt.Renderer(bundle, BC.params_with(params, spp=8))
    try:
        r.bind_buckets(4)
        r.render(0, 4)
        r.resolve_buckets(1)
        first = r.read_bucket_resolve()
        r.render(4, 4)
        for read in (r.read_bucket_resolve, r.bucket_resolve_device_ptrs, r.read_bucket_resolve_xyz, r.read_bucket_resolve_bgra):
            with pytest.raises(RuntimeError, match="the film has changed since the last resolve"):
                read()
        BC.assert_bucket_films(read_buckets(r, 4), BC.expected_films(BASE, 4, **BC.changes_for(8)), "after the refused readouts")
        r.resolve_buckets(1)
        est, err = r.read_bucket_resolve()
    finally:
        r.close()
    want = BC.expected_resolve(BASE, 4, 1, **BC.changes_for(8))
    assert cases.same_bits(est, want[0]) and cases.same_bits(err, want[1])
    w4 = BC.expected_resolve(BASE, 4, 1, **BC.changes_for(4))
    assert cases.same_bits(first[0], w4[0]) and cases.same_bits(first[1], w4[1]) and not cases.same_bits(first[0], est)


# ------------------------------------------------------------------------------------------------ refusals and resources
def test_every_refusal_says_why_and_leaves_the_context_as_it_was():
    bundle, params = BC.load(BASE)
    p = BC.params_with(params, spp=8)
    want = BC.expected_films(BASE, 3, **BC.changes_for(8))
    gc.collect()
    r = pydrt.Renderer(bundle, p)

    def state():
        n = getattr(r, "n_buckets", 0)
        return r.read_film(), read_buckets(r, n) if n else None, cases.stat_counts(r.stats()), pydrt.selftest_live_resources()

    def refused(call, why):
        before = state()
        with pytest.raises(RuntimeError, match=why):
            call()
        after = state()
        BC.assert_film(after[0], before[0], "main film across the refusal '%s'" % why)
        if before[1] is not None:
            BC.assert_bucket_films(after[1], before[1], "across the refusal '%s'" % why)
        assert after[2:] == before[2:], why

    try:
        for read in (lambda: r.read_bucket_film(0), lambda: r.bucket_film_device_ptrs(0), lambda: r.resolve_buckets(0), r.read_bucket_resolve,
                     r.bucket_resolve_device_ptrs, r.read_bucket_resolve_xyz, r.read_bucket_resolve_bgra):
            refused(read, "no buckets are bound")
        refused(lambda: r.bind_buckets(9), "9 buckets, at most 8")
        r.bind_depth_cuts((1, 2))
        refused(lambda: r.bind_buckets(3), "depth cuts are bound")
        r.bind_depth_cuts(None)
        r.bind_sensor(np.ones((2, bundle.S)))
        refused(lambda: r.bind_buckets(3), "a sensor is bound")
        r.bind_sensor(None)
        r.bind_buckets(1)
        refused(lambda: r.resolve_buckets(0), "one bucket has no scatter to resolve")
        r.bind_buckets(3)
        refused(lambda: r.bind_depth_cuts((1, 2)), "buckets are bound")
        refused(lambda: r.bind_sensor(np.ones((2, bundle.S))), "buckets are bound")
        refused(lambda: r.render_adaptive(2, 4, 1, 0.1), "buckets bound")
        refused(lambda: r.render_adaptive_continue(4, 1, 0.1), "buckets bound")
        refused(lambda: r.render_sample_map(np.full(r.n_pixels, 2, dtype=np.uint32)), "buckets bound")
        refused(lambda: r.resolve_buckets(0), "holds 0 samples, fewer than its 3 buckets")
        refused(lambda: r.read_bucket_film(3), "bucket 3 of 3")
        r.render(0, 2)
        refused(lambda: r.resolve_buckets(0), "holds 2 samples, fewer than its 3 buckets")
        r.render(2, 6)
        refused(lambda: r.bind_buckets(2), "already holds samples")
        r.bind_buckets(0)  # (the unbind passes on a film that holds samples; a bind after it does not)
        refused(lambda: r.bind_buckets(2), "already holds samples")
        r.reset_film()
        r.bind_buckets(3)
        r.render()
        refused(lambda: r.resolve_buckets(2), "trim = 2 leaves nothing of 3 buckets")
        refused(r.read_bucket_resolve, "nothing is resolved yet")
        refused(lambda: pydrt._check(r.L.drt_read_bucket_resolve_xyz(r.ctx, None), "drt_read_bucket_resolve_xyz"), "nothing is resolved yet")
        BC.assert_bucket_films(read_buckets(r, 3), want, "after the refusals")
        BC.assert_film(r.read_film(), BC.film_device(BASE, **BC.changes_for(8))[:3], "after the refusals, the main film")
        # unbound after a reset: adaptive sampling works again, and a film that holds an adaptive render takes no buckets
        r.reset_film()
        r.bind_buckets(0)
        r.render_adaptive(2, 4, 1, 0.1)
        refused(lambda: r.bind_buckets(3), "drt_reset_film first")
        r.reset_film()
        r.bind_buckets(3)
        r.render()
        BC.assert_bucket_films(read_buckets(r, 3), want, "bound again after an adaptive render and a reset")
    finally:
        r.close()
    x = pydrt.Renderer(bundle, BC.params_with(params, mode=pydrt.MODE_XYZ))
    try:
        with pytest.raises(RuntimeError, match="DRT_MODE_XYZ"):
            x.bind_buckets(2)
        x.render()
        assert np.isfinite(x.read_xyz()).all()
    finally:
        x.close()


def test_live_resources_after_bind_rebind_unbind_and_close():
    bundle, params = BC.load(BASE)
    p = BC.params_with(params, spp=8)
    gc.collect()
    base = pydrt.selftest_live_resources()
    now = lambda: tuple(a - b for a, b in zip(pydrt.selftest_live_resources(), base))
    r = pydrt.Renderer(bundle, p)
    try:
        r.render()
        r.read_film()
        r.read_xyz()
        r.read_bgra(1)
        r.reset_film()
        unbound = now()
        r.bind_buckets(3)
        assert now()[0] == unbound[0] + 9 and now()[1:] == unbound[1:], "three buffers per bucket"
        r.render()
        r.resolve_buckets(1)
        assert now()[0] == unbound[0] + 11, "the estimate and the error"
        r.read_bucket_resolve_xyz()
        r.read_bucket_resolve_bgra()
        assert now()[0] == unbound[0] + 12, "the estimate with a filter column, for the XYZ kernel"
        r.reset_film()
        r.bind_buckets(8)
        assert now()[0] == unbound[0] + 24, "the earlier films and the earlier resolve are released by the next bind"
        r.render()
        assert r.read_bucket_film(7)[1].shape == (r.n_pixels, bundle.S)
        r.reset_film()
        r.bind_buckets(0)
        assert now() == unbound
        r.bind_buckets(2)
        r.render()
        r.resolve_buckets()
        assert now()[0] == unbound[0] + 8
    finally:
        r.close()
    gc.collect()
    assert now() == (0, 0, 0, 0), "%s still held (device, pinned, events, streams)" % (now(),)


# ------------------------------------------------------------------------------------------------ the host program
def test_drt_render_program_with_four_buckets(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    W, H, SPP = 24, 16, 8
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("output_width      800", "output_width      %d" % W).replace("output_height     600", "output_height     %d" % H)
    import re
    cfg, k = re.subn(r"(?m)^num_pixel_samples\s+\S+", "num_pixel_samples %d" % SPP, cfg)
    assert k == 1
    depth = int(re.search(r"(?m)^max_cast_depth\s+(\d+)", cfg).group(1))

    def run(name, **env):
        d = tmp_path / name
        os.makedirs(d / "output")
        for sub in ("scenes", "spectra"):
            os.symlink(os.path.join(cases.REPO, sub), d / sub)
        (d / "config.cfg").write_text(cfg)
        full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
        full.update(env)
        r = subprocess.run([exe], cwd=d, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        return d, r.stdout

    plain, _ = run("plain")
    d, text = run("buckets", DRT_BUCKETS="4", DRT_DEVICES="0,0")
    assert "Bucket films: 4 buckets, trim 1" in text
    for f in ("output.spd", "average.spd", "variance.spd", "output.bmp", "average.bmp", "variance.bmp"):
        assert open(plain / "output" / f, "rb").read() == open(d / "output" / f, "rb").read(), f
    extra = ["%s.spd.bucket%d.spd" % (f, b) for f in ("output", "average", "variance") for b in range(4)]
    extra += ["average.spd.robust.spd", "variance.spd.robust.spd", "output.spd.robust.bmp"]
    assert sorted(os.listdir(d / "output")) == sorted(os.listdir(plain / "output") + extra)  # and no temporary file is left
    # the same render through pydrt
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, H)
    r = pydrt.Renderer(bundle, pydrt.make_params(W, H, spp=SPP, max_depth=depth, seed=1))
    try:
        r.bind_buckets(4)
        r.render()
        films = read_buckets(r, 4)
        r.resolve_buckets()
        est, err = r.read_bucket_resolve()
        picture = r.read_bucket_resolve_bgra()
    finally:
        r.close()

    def tail(f, shape):
        raw = open(d / "output" / f, "rb").read()
        size = int(np.prod(shape)) * 8
        assert len(raw) > size, f
        return np.frombuffer(raw[-size:], dtype=np.float64).reshape(shape)

    for b, (px, av, _) in enumerate(films):
        assert cases.same_bits(tail("output.spd.bucket%d.spd" % b, px.shape), px), "bucket %d, sums" % b
        assert cases.same_bits(tail("average.spd.bucket%d.spd" % b, av.shape), av), "bucket %d, means" % b
        assert np.array_equal(px[:, -1], np.full(px.shape[0], 2.0))
    assert cases.same_bits(tail("average.spd.robust.spd", est.shape), est) and cases.same_bits(tail("variance.spd.robust.spd", err.shape), err)
    assert (err != 0).any() and not cases.same_bits(films[0][1], films[1][1])
    bmp = np.frombuffer(open(d / "output" / "output.spd.robust.bmp", "rb").read()[-W * H * 4:], dtype=np.uint8).reshape(H, W, 4)
    want = picture.reshape(H, W, 4)
    assert np.array_equal(bmp, want) or np.array_equal(bmp, want[::-1]), "the picture is not drt_read_bucket_resolve_bgra's"
    assert len(np.unique(want[:, :, :3])) > 10
