"""GPU (-m gpu): adaptive sampling (drt_render_adaptive, drt_group_render_adaptive) against the rule of tests/adaptive_rule.py.

A pixel rendered over samples 0 .. n-1 in order holds, bit for bit, the film a uniform n-sample render gives it. So every test here
takes the snapshots of a uniform render after each round (the oracle's, or the HIP path's, itself pinned to the oracle), asks the
rule which count each pixel gets, and requires the adaptive counts to be those and every pixel's film rows to be its snapshot's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_rule as R
import cases
import pydrt

pytestmark = pytest.mark.gpu

MIN, STEP, MAX = 4, 4, 24


def table(bundle):
    sc = bundle.scene
    return bundle.spds(), int(sc.cmf_rw), int(sc.cmf_y), float(sc.wavelength_interval)


def oracle_snapshots(bundle, params, ns):
    """the oracle's film after each count in ns, one render per round carried over (samples n_prev .. n-1)"""
    snaps, film, prev = {}, None, 0
    for n in ns:
        p = pydrt.make_params(int(params.width), int(params.height), spp=n - prev, max_depth=int(params.max_depth),
                              seed=int(params.seed), pixel_scheme=int(params.pixel_scheme), first_sample=prev,
                              x0=int(params.x0), y0=int(params.y0), tile_w=int(params.tile_w), tile_h=int(params.tile_h),
                              row_stride=int(params.row_stride))
        px, av, va, _, _ = cases.oracle_render_device_pow(bundle, p, film=film)
        film = (px, av, va)
        snaps[n] = film
        prev = n
    return snaps


def expected(bundle, snaps, n_pix, mn, mx, st, rel, floor=0.0):
    spds, rw, cy, iv = table(bundle)
    return R.sample_counts(lambda n: snaps[n][1:], spds, rw, cy, iv, n_pix, mn, mx, st, rel, floor)


def film_at_counts(snaps, counts):
    """every pixel's rows from the snapshot at its count"""
    px, av, va = (np.empty_like(a) for a in snaps[max(snaps)])
    for n, (spx, sav, sva) in snaps.items():
        m = counts == n
        px[m], av[m], va[m] = spx[m], sav[m], sva[m]
    return px, av, va


def assert_same_film(got, want, what=""):
    for g, w, name in zip(got, want, ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s %s: %s" % (what, name, cases.first_difference(g, w))


def adaptive(bundle, params, mn, mx, st, rel, floor=0.0, devices=None):
    """(report, counts [n_pix], film, stats) of an adaptive render on a fresh context (or group)"""
    r = pydrt.Renderer(bundle, params) if devices is None else pydrt.Group(bundle, params, devices)
    try:
        rep = r.render_adaptive(mn, mx, st, rel, floor)
        counts = r.read_sample_counts().reshape(-1)
        film = r.read_film()
        stats = r.stats()
    finally:
        r.close()
    return rep, counts, film, stats


def pick_rel_error(bundle, snaps, n_pix, mn, mx, st):
    """a rel_error with pixels that stop at min, at max and in between (so that nothing here passes vacuously)"""
    spds, rw, cy, iv = table(bundle)
    Y, E = R.luminance_and_error(spds, rw, cy, iv, snaps[mn][1], snaps[mn][2], mn)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = E / np.abs(Y)
    ratio = ratio[np.isfinite(ratio) & (ratio > 0)]
    for q in (0.5, 0.35, 0.65, 0.2, 0.8, 0.1, 0.9):
        rel = float(np.quantile(ratio, q))
        counts, _ = expected(bundle, snaps, n_pix, mn, mx, st, rel)
        if (counts == mn).any() and (counts == mx).any() and ((counts > mn) & (counts < mx)).any():
            return rel, counts
    raise AssertionError("no rel_error gives pixels at min, at max and in between")


def case_params(name, spp=MAX):
    bundle, p = cases.load_case(name)
    params = pydrt.make_params(int(p.width), int(p.height), spp=spp, max_depth=int(p.max_depth), seed=int(p.seed),
                               pixel_scheme=int(p.pixel_scheme))
    return bundle, params


@pytest.mark.parametrize("name", ["plane_light_48", "gold_mirror", "large_box", "grid_2p5nm", "spheres_1500", "lens"])
def test_adaptive_film_and_counts_equal_the_oracle_snapshots(name):
    bundle, params = case_params(name)
    n_pix = int(params.tile_w) * int(params.tile_h)
    snaps = oracle_snapshots(bundle, params, R.rounds(MIN, MAX, STEP))
    rel, want_counts = pick_rel_error(bundle, snaps, n_pix, MIN, MAX, STEP)
    rep, counts, film, stats = adaptive(bundle, params, MIN, MAX, STEP, rel)
    assert np.array_equal(counts, want_counts), "%d counts differ" % int((counts != want_counts).sum())
    assert (counts == MIN).any() and (counts == MAX).any() and ((counts > MIN) & (counts < MAX)).any()
    assert_same_film(film, film_at_counts(snaps, counts), name)
    assert np.array_equal(film[0][:, -1], counts.astype(np.float64))  # the filter column is the count
    assert rep["paths"] == stats.paths == int(counts.sum(dtype=np.uint64))
    assert rep["pixels_at_max"] == int((counts == MAX).sum())
    assert rep["rounds"] == len([n for n in R.rounds(MIN, MAX, STEP) if n <= counts.max()])


@pytest.fixture(scope="module")
def plane_light_reference():
    bundle, params = case_params("plane_light_48")
    rep, counts, film, stats = adaptive(bundle, params, MIN, MAX, STEP, 0.08)
    assert (counts == MIN).any() and (counts == MAX).any() and ((counts > MIN) & (counts < MAX)).any()
    return bundle, params, counts, film


@pytest.mark.parametrize("env", [{"DRT_FORCE_BVH": "1"}, {"DRT_POOL_BLOCKS": "1"}, {"DRT_NO_SIMPLE_SHADE": "1"},
                                 {"DRT_TRACE_TAIL": "0"}, {"DRT_TRACE_TAIL": "2"}, {"DRT_DARK_SKIP": "0"}])
def test_adaptive_a_b_switches_give_the_same_film_and_counts(plane_light_reference, env, monkeypatch):
    bundle, params, counts0, film0 = plane_light_reference
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rep, counts, film, stats = adaptive(bundle, params, MIN, MAX, STEP, 0.08)
    assert np.array_equal(counts, counts0)
    assert_same_film(film, film0, str(env))
    if "DRT_POOL_BLOCKS" in env:
        assert stats.redone_launches >= 1
    if "DRT_FORCE_BVH" in env:
        assert stats.path_flags & 1


def test_adaptive_limits():
    bundle, params = case_params("gold_mirror", spp=12)
    n_pix = int(params.tile_w) * int(params.tile_h)
    # a tiny rel_error: every pixel at max -- but one whose samples were all exactly 0 (Y = E = 0), which stops at min -- and the
    # film is what drt_render(0, max) gives
    rep, counts, film, stats = adaptive(bundle, params, 4, 12, 4, 1e-300)
    r = pydrt.Renderer(bundle, params)
    r.render(0, 4)
    uniform4 = r.read_film()
    dark = uniform4[1].max(axis=1) == 0.0
    r.render(4, 8)
    uniform = r.read_film()
    r.close()
    assert np.array_equal(counts, np.where(dark, 4, 12).astype(np.uint32)) and (counts == 12).any() and rep["rounds"] == 3
    assert_same_film(tuple(a[counts == 12] for a in film), tuple(a[counts == 12] for a in uniform), "tiny rel_error, at max")
    assert_same_film(tuple(a[counts == 4] for a in film), tuple(a[counts == 4] for a in uniform4), "tiny rel_error, dark at min")
    # a huge one: every pixel at min, one round
    rep, counts, film, stats = adaptive(bundle, params, 4, 12, 4, 1e300)
    assert (counts == 4).all() and rep["rounds"] == 1 and rep["pixels_at_max"] == 0 and rep["paths"] == 4 * n_pix
    # min == max: one round, every pixel at max
    rep, counts, film, stats = adaptive(bundle, params, 6, 6, 3, 0.5)
    assert (counts == 6).all() and rep["rounds"] == 1 and rep["pixels_at_max"] == n_pix
    # a step that does not divide max - min: 3, 8, 12
    snaps = oracle_snapshots(bundle, params, R.rounds(3, 12, 5))
    rel, want = pick_rel_error(bundle, snaps, n_pix, 3, 12, 5)
    rep, counts, film, stats = adaptive(bundle, params, 3, 12, 5, rel)
    assert np.array_equal(counts, want) and set(np.unique(counts)) <= {3, 8, 12}
    assert_same_film(film, film_at_counts(snaps, counts), "step 5")


def test_adaptive_nan_film_keeps_every_pixel_to_max():
    bundle, params = case_params("example_scene", spp=8)
    snaps = oracle_snapshots(bundle, params, R.rounds(2, 8, 3))
    rep, counts, film, stats = adaptive(bundle, params, 2, 8, 3, 0.5)
    assert (counts == 8).all()
    assert_same_film(film, snaps[8], "example_scene")


def test_adaptive_on_a_strided_tile_and_over_groups():
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 40, 60)
    params = pydrt.make_params(40, 60, spp=MAX, max_depth=6, seed=3, x0=7, y0=5, tile_w=25, tile_h=18, row_stride=3)
    n_pix = 25 * 18
    snaps = oracle_snapshots(bundle, params, R.rounds(MIN, MAX, STEP))
    rel, want = pick_rel_error(bundle, snaps, n_pix, MIN, MAX, STEP)
    rep, counts, film, stats = adaptive(bundle, params, MIN, MAX, STEP, rel)
    assert np.array_equal(counts, want)
    assert_same_film(film, film_at_counts(snaps, counts), "strided tile")
    for devices in ([0, 0], [0, 0, 0]):
        grep, gcounts, gfilm, gstats = adaptive(bundle, params, MIN, MAX, STEP, rel, devices=devices)
        assert np.array_equal(gcounts, counts), devices
        assert_same_film(gfilm, film, str(devices))
        assert grep["paths"] == rep["paths"] == gstats.paths and grep["pixels_at_max"] == rep["pixels_at_max"]


def test_adaptive_refusals_and_report():
    L = pydrt.hip_lib()
    bundle, params = case_params("plane_light_48", spp=8)
    r = pydrt.Renderer(bundle, params)
    try:
        with pytest.raises(RuntimeError, match="drt_read_sample_counts"):
            r.read_sample_counts()
        for bad in [dict(min_spp=1, max_spp=8, step=2, rel_error=0.1), dict(min_spp=4, max_spp=3, step=2, rel_error=0.1),
                    dict(min_spp=4, max_spp=8, step=0, rel_error=0.1), dict(min_spp=4, max_spp=8, step=2, rel_error=0.0),
                    dict(min_spp=4, max_spp=8, step=2, rel_error=float("nan")), dict(min_spp=4, max_spp=8, step=2, rel_error=float("inf")),
                    dict(min_spp=4, max_spp=8, step=2, rel_error=0.1, floor=-1.0),
                    dict(min_spp=4, max_spp=8, step=2, rel_error=0.1, floor=float("inf"))]:
            with pytest.raises(RuntimeError, match="drt_render_adaptive"):
                r.render_adaptive(**bad)
        a = pydrt.make_adaptive(4, 8, 2, 0.1)
        a.flags = 1
        assert L.drt_render_adaptive(r.ctx, C.byref(a)) != 0
        assert r.stats().paths == 0  # nothing rendered by any refusal
        r.render(0, 2)  # a film with samples in it
        with pytest.raises(RuntimeError, match="without samples"):
            r.render_adaptive(4, 8, 2, 0.1)
        r.reset_film()
        px, av, va = r.read_film()
        r.write_film(px, av, va)
        with pytest.raises(RuntimeError, match="without samples"):
            r.render_adaptive(4, 8, 2, 0.1)
        r.reset_film()
        rep = r.render_adaptive(4, 8, 2, 0.1)
        counts = r.read_sample_counts()
        st = r.stats()
        assert rep["paths"] == st.paths == int(counts.sum(dtype=np.uint64))
        assert rep["pixels_at_max"] == int((counts == 8).sum())
        for call in (lambda: r.render(0, 2), lambda: r.write_film(px, av, va), lambda: r.render_adaptive(4, 8, 2, 0.1)):
            with pytest.raises(RuntimeError, match="adaptive render"):
                call()
        r.reset_film()
        with pytest.raises(RuntimeError, match="drt_read_sample_counts"):
            r.read_sample_counts()
        r.render(0, 2)  # usable again
    finally:
        r.close()
    for flags, mode in ((pydrt.FLAG_RECORD_HITS, pydrt.MODE_SPECTRAL), (0, pydrt.MODE_XYZ)):
        p = pydrt.make_params(16, 16, spp=8, max_depth=4, flags=flags, mode=mode)
        q = pydrt.Renderer(bundle, p)
        try:
            with pytest.raises(RuntimeError, match="drt_render_adaptive"):
                q.render_adaptive(4, 8, 2, 0.1)
        finally:
            q.close()


def test_adaptive_headline_frame_against_uniform_snapshots():
    """1024^2 at depth 8, min 16, step 16, max 128: the uniform HIP render in rounds of 16 gives the snapshots; only the rows of
    the pixels whose count is the snapshot's, and the active set's rule decisions, are kept from each."""
    W = 1024
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, W)
    params = pydrt.make_params(W, W, spp=128, max_depth=8, seed=1)
    rel = 0.05
    rep, counts, film, stats = adaptive(bundle, params, 16, 128, 16, rel)
    spds, rw, cy, iv = table(bundle)
    r = pydrt.Renderer(bundle, params)
    try:
        active = np.arange(W * W)
        want = np.zeros(W * W, dtype=np.uint32)
        for n in R.rounds(16, 128, 16):
            r.render(n - 16, 16)
            px, av, va = r.read_film()
            want[active] = n
            keep = R.stays_active(spds, rw, cy, iv, av[active], va[active], n, 128, rel, 0.0)
            m = counts == n
            assert_same_film((film[0][m], film[1][m], film[2][m]), (px[m], av[m], va[m]), "pixels at %d samples" % n)
            active = active[keep]
            del px, av, va
    finally:
        r.close()
    assert np.array_equal(counts, want), "%d counts differ" % int((counts != want).sum())
    assert rep["paths"] == stats.paths == int(counts.sum(dtype=np.uint64)) < 128 * W * W


def test_drt_render_program_with_adaptive_sampling(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    os.makedirs(tmp_path / "output")
    for d in ("scenes", "spectra"):
        os.symlink(os.path.join(cases.REPO, d), tmp_path / d)
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("num_pixel_samples 4", "num_pixel_samples 20").replace("output_width      800", "output_width      48")
    cfg = cfg.replace("output_height     600", "output_height     32").replace("max_cast_depth    4", "max_cast_depth    6")
    (tmp_path / "config.cfg").write_text(cfg)
    env = dict(os.environ, DRT_ADAPTIVE_ERROR="0.1", DRT_ADAPTIVE_MIN_SPP="4", DRT_ADAPTIVE_STEP="4")
    r = subprocess.run([exe], cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "Adaptive:" in r.stdout and "of 30720 paths traced" in r.stdout
    S = 69
    px = np.fromfile(tmp_path / "output" / "output.spd", dtype=np.float64, offset=40).reshape(-1, S + 1)
    avg = np.fromfile(tmp_path / "output" / "average.spd", dtype=np.float64, offset=40).reshape(-1, S)
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 48, 32)
    params = pydrt.make_params(48, 32, spp=20, max_depth=6, seed=1)
    rep, counts, film, stats = adaptive(bundle, params, 4, 20, 4, 0.1)
    assert np.array_equal(px[:, S], counts.astype(np.float64))
    assert (counts == 4).any() and (counts > 4).any()
    assert cases.same_bits(avg, film[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        assert cases.same_bits(px[:, :S], film[0][:, :S])


def test_the_active_list_is_the_stable_compaction_of_the_rule(monkeypatch):
    """After each of the first rounds (DRT_ADAPTIVE_ROUNDS stops the render there) the next list is np.nonzero of the rule's
    decisions, in ascending tile order: the compaction keeps the order of the list it came from."""
    bundle, params = case_params("plane_light_48", spp=MAX)
    spds, rw, cy, iv = table(bundle)
    n_pix = int(params.tile_w) * int(params.tile_h)
    prev = np.arange(n_pix)
    for k, n in enumerate(R.rounds(MIN, MAX, STEP)[:3], start=1):
        monkeypatch.setenv("DRT_ADAPTIVE_ROUNDS", str(k))
        r = pydrt.Renderer(bundle, params)
        try:
            rep = r.render_adaptive(MIN, MAX, STEP, 0.08)
            lst = r.read_active_list()
            counts = r.read_sample_counts().reshape(-1)
            px, av, va = r.read_film()
        finally:
            r.close()
        assert rep["rounds"] == k and np.all(counts[prev] == n)
        keep = R.stays_active(spds, rw, cy, iv, av[prev], va[prev], n, MAX, 0.08, 0.0)
        want = prev[np.nonzero(keep)[0]]
        assert 0 < want.size < prev.size
        assert np.array_equal(lst, want.astype(np.uint32)), "round %d: %d entries against %d" % (k, lst.size, want.size)
        prev = want
