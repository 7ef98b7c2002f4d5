"""GPU (-m gpu): continuing adaptive sampling on a held film (drt_render_adaptive_continue and its group form).

What must hold, all bit for bit: (a) after any sequence of calls pixel p's rows are the uniform n_p-sample film's and its filter sum
is n_p; (b) refining -- a tighter rel_error / floor, a larger max_spp, the same step and grid of counts -- gives the film and counts
of one fresh drt_render_adaptive with the new parameters; (c) drt_render(0, m) + continue = drt_render_adaptive(min_spp = m);
(d) a render split by max_rounds and carried through host memory into a new context = the whole; (e) any other continuation follows
the per-pixel rule of tests/adaptive_resume_rule.py. The helpers are those of tests/test_gpu_adaptive.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_resume_rule as RR
import adaptive_rule as R
import cases
import pydrt
import test_gpu_adaptive as A

pytestmark = pytest.mark.gpu

MIN, STEP, MAX, MAX2 = 4, 4, 24, 40
REL = 0.08  # plane_light_48 where no oracle is needed: pixels at min, at max and in between (tests/test_gpu_adaptive.py)

_snapshots = {}


def case(name):
    """(bundle, params, n_pix, oracle snapshots at 4, 8 .. 40, a rel_error with pixels at 4, at 24 and in between), once per case"""
    if name not in _snapshots:
        bundle, params = A.case_params(name, spp=MAX2)
        n_pix = int(params.tile_w) * int(params.tile_h)
        snaps = A.oracle_snapshots(bundle, params, R.rounds(MIN, MAX2, STEP))
        rel, _ = A.pick_rel_error(bundle, snaps, n_pix, MIN, MAX, STEP)
        _snapshots[name] = (bundle, params, n_pix, snaps, rel)
    return _snapshots[name]


def state(r):
    return r.read_sample_counts().reshape(-1), r.read_film()


def same_film_bits(a, b):
    return all(cases.same_bits(x, y) for x, y in zip(a, b))


def refine(bundle, params, p, p2, devices=None):
    """P = (min, max, step, rel) and then the continuation P' = (max, step, rel) on one context (or group):
    (report of P, counts after P, report of the continuation, counts, film, stats)"""
    r = pydrt.Renderer(bundle, params) if devices is None else pydrt.Group(bundle, params, devices)
    try:
        rep = r.render_adaptive(*p)
        before = r.read_sample_counts().reshape(-1)
        rep2 = r.render_adaptive_continue(*p2)
        counts, film = state(r)
        stats = r.stats()
    finally:
        r.close()
    return rep, before, rep2, counts, film, stats


def well_spread(before, counts):
    """the continuation is worth testing: it took pixels on from at least three counts, left some alone, took some to the cap and
    stopped some on the way"""
    grew = counts > before
    return (np.unique(before[grew]).size >= 3 and (~grew).any() and (grew & (counts == MAX2)).any()
            and (grew & (counts < MAX2)).any())


@pytest.mark.parametrize("name", ["plane_light_48", "gold_mirror", "large_box", "grid_2p5nm", "spheres_1500", "lens"])
def test_refining_equals_the_fresh_render_and_the_oracle_snapshots(name):
    bundle, params, n_pix, snaps, rel = case(name)
    for factor in (0.5, 0.7):
        rel2 = rel * factor
        rep, before, rep2, counts, film, stats = refine(bundle, params, (MIN, MAX, STEP, rel), (MAX2, STEP, rel2))
        print(name, "factor", factor, "counts after P", np.unique(before, return_counts=True), "after P'", np.unique(counts, return_counts=True))
        if well_spread(before, counts):
            break
    else:
        raise AssertionError("%s: neither rel / 2 nor 0.7 rel spreads the continuation over the counts" % name)
    assert (counts >= before).all() and rep2["still_active"] == 0
    # (b) against the existing path
    frep, fcounts, ffilm, fstats = A.adaptive(bundle, params, MIN, MAX2, STEP, rel2)
    assert np.array_equal(counts, fcounts), "%d counts differ from the fresh render's" % int((counts != fcounts).sum())
    A.assert_same_film(film, ffilm, name + " against the fresh render")
    assert rep["paths"] + rep2["paths"] == frep["paths"] == stats.paths
    assert rep2["pixels_at_max"] == frep["pixels_at_max"] == int((counts == MAX2).sum())
    assert rep2["rounds"] == int((counts - before).max()) // STEP  # every active pixel takes part in every round from the first on
    # (a) against the oracle, and the rule
    want, _ = A.expected(bundle, snaps, n_pix, MIN, MAX2, STEP, rel2)
    assert np.array_equal(counts, want), "%d counts differ from the rule's" % int((counts != want).sum())
    A.assert_same_film(film, A.film_at_counts(snaps, counts), name + " against the oracle")
    assert np.array_equal(film[0][:, -1], counts.astype(np.float64))


def test_a_uniform_start_is_a_fresh_start():
    bundle, params = A.case_params("plane_light_48")
    n_pix = int(params.tile_w) * int(params.tile_h)
    for mn, mx, st in ((MIN, MAX, STEP), (3, 12, 5)):
        frep, fcounts, ffilm, fstats = A.adaptive(bundle, params, mn, mx, st, REL)
        assert np.unique(fcounts).size >= 2 and set(np.unique(fcounts)) <= set(R.rounds(mn, mx, st))
        r = pydrt.Renderer(bundle, params)
        try:
            r.render(0, mn)
            rep = r.render_adaptive_continue(mx, st, REL)
            counts, film = state(r)
            assert r.read_active_list().size == 0 and rep["still_active"] == 0
            assert r.stats().paths == fstats.paths
        finally:
            r.close()
        assert np.array_equal(counts, fcounts)
        A.assert_same_film(film, ffilm, "uniform start (%d, %d, %d)" % (mn, mx, st))
        assert rep["rounds"] + 1 == frep["rounds"] and rep["paths"] + mn * n_pix == frep["paths"]
        assert rep["pixels_at_max"] == frep["pixels_at_max"]
    # ... round by round too: the active lists of the fresh render stopped after k rounds
    for k in (1, 2):
        os.environ["DRT_ADAPTIVE_ROUNDS"] = str(k + 1)
        try:
            f = pydrt.Renderer(bundle, params)
            try:
                f.render_adaptive(MIN, MAX, STEP, REL)
                flist, (fcounts, ffilm) = f.read_active_list(), state(f)
            finally:
                f.close()
        finally:
            del os.environ["DRT_ADAPTIVE_ROUNDS"]
        r = pydrt.Renderer(bundle, params)
        try:
            r.render(0, MIN)
            rep = r.render_adaptive_continue(MAX, STEP, REL, max_rounds=k)
            assert rep["rounds"] == k and np.array_equal(r.read_active_list(), flist) and rep["still_active"] == flist.size > 0
            counts, film = state(r)
        finally:
            r.close()
        assert np.array_equal(counts, fcounts)
        A.assert_same_film(film, ffilm, "uniform start, %d rounds" % k)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_split_through_host_memory_equals_whole(k):
    bundle, params = A.case_params("plane_light_48")
    spds, rw, cy, iv = A.table(bundle)
    n_pix = int(params.tile_w) * int(params.tile_h)
    whole = pydrt.Renderer(bundle, params)
    try:
        whole.render(0, MIN)
        wrep = whole.render_adaptive_continue(MAX, STEP, REL)
        wcounts, wfilm = state(whole)
    finally:
        whole.close()
    assert wrep["rounds"] > k
    first = pydrt.Renderer(bundle, params)
    try:
        first.render(0, MIN)
        rep1 = first.render_adaptive_continue(MAX, STEP, REL, max_rounds=k)
        lst = first.read_active_list()
        counts1, film1 = state(first)
    finally:
        first.close()
    assert rep1["rounds"] == k and rep1["still_active"] == lst.size > 0
    assert np.array_equal(film1[0][:, -1], counts1.astype(np.float64))
    keep = RR.active_of(lambda n: film1[1:], spds, rw, cy, iv, counts1, np.arange(n_pix), MAX, REL, 0.0)
    assert np.array_equal(lst, np.nonzero(keep)[0].astype(np.uint32))  # ascending tile order
    second = pydrt.Renderer(bundle, params)
    try:
        second.write_film(*film1)
        rep2 = second.render_adaptive_continue(MAX, STEP, REL)
        counts2, film2 = state(second)
    finally:
        second.close()
    assert np.array_equal(counts2, wcounts)
    A.assert_same_film(film2, wfilm, "split after %d rounds" % k)
    assert rep1["paths"] + rep2["paths"] == wrep["paths"] and rep1["rounds"] + rep2["rounds"] == wrep["rounds"]
    assert rep2["pixels_at_max"] == wrep["pixels_at_max"]


def test_a_looser_bound_after_a_finished_render_renders_nothing():
    bundle, params = A.case_params("plane_light_48")
    r = pydrt.Renderer(bundle, params)
    try:
        rep = r.render_adaptive(MIN, MAX, STEP, REL / 2)
        counts, film = state(r)
        paths = r.stats().paths
        rep2 = r.render_adaptive_continue(MAX, STEP, REL * 2)
        counts2, film2 = state(r)
        assert rep2["rounds"] == 0 and rep2["paths"] == 0 and rep2["still_active"] == 0 and r.stats().paths == paths
        assert rep2["pixels_at_max"] == rep["pixels_at_max"] == int((counts == MAX).sum())
        assert np.array_equal(counts2, counts) and same_film_bits(film2, film)
    finally:
        r.close()


@pytest.mark.parametrize("name", ["plane_light_48", "gold_mirror"])
def test_a_loosened_continuation_follows_the_rule_per_pixel(name):
    """P = (4, 24, 4, rel), then P' = (40, 4, 1.5 rel): the pixels P left at 24 that fail P' go on -- all from one count, the
    same-count clause of the contract -- and the converged ones stay where they are, which is NOT what a fresh P' render gives."""
    bundle, params, n_pix, snaps, rel = case(name)
    spds, rw, cy, iv = A.table(bundle)
    rel2 = 1.5 * rel
    rep, before, rep2, counts, film, stats = refine(bundle, params, (MIN, MAX, STEP, rel), (MAX2, STEP, rel2))
    want, ran, paths, left = RR.continue_counts(lambda n: snaps[n][1:], spds, rw, cy, iv, before, MAX2, STEP, rel2, 0.0)
    grew = counts > before
    print(name, "go on", int(grew.sum()), "reach 40", int((counts == MAX2).sum()), "stop between", int((grew & (counts < MAX2)).sum()))
    assert np.array_equal(counts, want), "%d counts differ from the rule's" % int((counts != want).sum())
    assert rep2["rounds"] == ran and rep2["paths"] == paths and left.size == 0 == rep2["still_active"]
    assert grew.any() and (before[grew] == MAX).all() and (counts == MAX2).any() and (grew & (counts < MAX2)).any()
    assert ((before < MAX) == (counts < MAX)).all()
    A.assert_same_film(film, A.film_at_counts(snaps, counts), name)
    assert np.array_equal(film[0][:, -1], counts.astype(np.float64))
    fresh, _ = A.expected(bundle, snaps, n_pix, MIN, MAX2, STEP, rel2)
    frep, fcounts, ffilm, fstats = A.adaptive(bundle, params, MIN, MAX2, STEP, rel2)
    assert np.array_equal(fcounts, fresh)
    print(name, "pixels that differ from the fresh render", int((counts != fcounts).sum()))
    assert (counts != fcounts).any() and (counts >= fcounts).all()


def uniform_snapshots(bundle, params, ns):
    """the HIP path's uniform film (itself pinned to the oracle) after each count in ns"""
    snaps, prev = {}, 0
    r = pydrt.Renderer(bundle, params)
    try:
        for n in ns:
            r.render(prev, n - prev)
            snaps[n] = r.read_film()
            prev = n
    finally:
        r.close()
    return snaps


def test_the_allotment_contract():
    bundle, params = A.case_params("plane_light_48")
    spds, rw, cy, iv = A.table(bundle)
    n_pix = int(params.tile_w) * int(params.tile_h)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_adaptive(MIN, MAX, STEP, REL)
        before, film0 = state(r)
        paths = r.stats().paths
        # which pixels the first test of (40, ., REL / 2) keeps: from several counts, and 40 - n is no multiple of 5 for all of them
        keep = RR.active_of(lambda n: film0[1:], spds, rw, cy, iv, before, np.arange(n_pix), MAX2, REL / 2, 0.0)
        assert np.unique(before[keep]).size >= 3
        assert not RR.allotment_contract(before, np.nonzero(keep)[0], MAX2, 5) and RR.allotment_contract(before, np.nonzero(keep)[0], MAX2, 2)
        g = int(np.gcd.reduce(MAX2 - before[keep].astype(np.int64)))
        usable = ", ".join(str(d) for d in range(1, g + 1) if g % d == 0)
        assert g % 2 == 0 and g % 5 != 0
        with pytest.raises(RuntimeError, match=r"drt_render_adaptive_continue.*step must be one of %s$" % usable):
            r.render_adaptive_continue(MAX2, 5, REL / 2)
        counts, film = state(r)
        assert r.stats().paths == paths and np.array_equal(counts, before) and same_film_bits(film, film0)
        assert r.read_active_list().size == 0  # the finished render's list, not the refused call's
        rep = r.render_adaptive_continue(MAX2, 2, REL / 2)  # the same film with a step that divides
        counts, film = state(r)
        assert r.stats().paths == paths + rep["paths"]
    finally:
        r.close()
    snaps = uniform_snapshots(bundle, params, list(range(MIN, MAX2 + 1, 2)))
    want, ran, wpaths, left = RR.continue_counts(lambda n: snaps[n][1:], spds, rw, cy, iv, before, MAX2, 2, REL / 2, 0.0)
    assert np.array_equal(counts, want) and rep["rounds"] == ran and rep["paths"] == wpaths and left.size == 0
    assert (counts % 4 == 2).any()  # counts off P's grid: the step really was 2
    A.assert_same_film(film, A.film_at_counts(snaps, counts), "step 2")
    assert np.array_equal(film[0][:, -1], counts.astype(np.float64))


def test_refusals_leave_the_film_and_the_counters_alone():
    L = pydrt.hip_lib()
    bundle, params = A.case_params("plane_light_48", spp=8)
    r = pydrt.Renderer(bundle, params)
    try:
        with pytest.raises(RuntimeError, match="drt_render_adaptive_continue.*drt_render_adaptive renders from the start"):
            r.render_adaptive_continue(8, 2, 0.1)  # an empty film
        r.render(0, 4)
        film0 = r.read_film()
        for bad in [dict(max_spp=1, step=2, rel_error=0.1), dict(max_spp=8, step=0, rel_error=0.1), dict(max_spp=8, step=2, rel_error=0.0),
                    dict(max_spp=8, step=2, rel_error=float("nan")), dict(max_spp=8, step=2, rel_error=float("inf")),
                    dict(max_spp=8, step=2, rel_error=0.1, floor=-1.0), dict(max_spp=8, step=2, rel_error=0.1, floor=float("inf"))]:
            with pytest.raises(RuntimeError, match="drt_render_adaptive_continue"):
                r.render_adaptive_continue(**bad)
        a = pydrt.make_adaptive(4, 8, 2, 0.1)
        a.flags = 1
        assert L.drt_render_adaptive_continue(r.ctx, C.byref(a), 0, None) != 0
        a = pydrt.make_adaptive(1, 8, 2, 0.1)  # min_spp is not used, but checked as drt_render_adaptive checks it
        assert L.drt_render_adaptive_continue(r.ctx, C.byref(a), 0, None) != 0
        assert r.stats().paths == 4 * r.n_pixels and same_film_bits(r.read_film(), film0)
        with pytest.raises(RuntimeError, match="drt_read_sample_counts"):
            r.read_sample_counts()  # no refusal made the context an adaptive render's
        # filter sums that are no sample counts, in the film a caller hands over
        for value in (1.0, 2.5, float("nan"), -4.0):
            r.reset_film()
            px, av, va = (a.copy() for a in film0)
            px[100, -1] = value
            px[7, -1] = value
            r.write_film(px, av, va)
            with pytest.raises(RuntimeError, match=r"drt_render_adaptive_continue.*tile pixel 7 \(column 7, row 0"):
                r.render_adaptive_continue(8, 2, 0.1)
            assert r.stats().paths == 0 and same_film_bits(r.read_film(), (px, av, va))
        r.reset_film()
        r.write_film(*film0)
        rep = r.render_adaptive_continue(8, 2, 0.1)
        counts = r.read_sample_counts()
        assert rep["paths"] == r.stats().paths == int((counts - 4).sum(dtype=np.uint64))
        for call in (lambda: r.render(0, 2), lambda: r.write_film(*film0), lambda: r.render_adaptive(4, 8, 2, 0.1)):
            with pytest.raises(RuntimeError, match="adaptive render"):
                call()
        again = r.render_adaptive_continue(8, 2, 0.1)  # may be repeated: nothing is left to do
        assert again["rounds"] == 0 and again["paths"] == 0 and again["pixels_at_max"] == rep["pixels_at_max"]
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
            q.render(0, 4)
            with pytest.raises(RuntimeError, match="drt_render_adaptive_continue.*DRT_"):
                q.render_adaptive_continue(8, 2, 0.1)
            assert q.stats().paths == 4 * 16 * 16
        finally:
            q.close()


@pytest.fixture(scope="module")
def plane_light_refined():
    bundle, params = A.case_params("plane_light_48", spp=MAX2)
    rep, before, rep2, counts, film, stats = refine(bundle, params, (MIN, MAX, STEP, REL), (MAX2, STEP, REL / 2))
    assert well_spread(before, counts)
    return bundle, params, counts, film


@pytest.mark.parametrize("env", [{"DRT_FORCE_BVH": "1"}, {"DRT_POOL_BLOCKS": "1"}, {"DRT_NO_SIMPLE_SHADE": "1"},
                                 {"DRT_TRACE_TAIL": "0"}, {"DRT_TRACE_TAIL": "2"}, {"DRT_DARK_SKIP": "0"}])
def test_a_b_switches_give_the_same_refinement(plane_light_refined, env, monkeypatch):
    bundle, params, counts0, film0 = plane_light_refined
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rep, before, rep2, counts, film, stats = refine(bundle, params, (MIN, MAX, STEP, REL), (MAX2, STEP, REL / 2))
    assert np.array_equal(counts, counts0)
    A.assert_same_film(film, film0, str(env))
    assert rep["paths"] + rep2["paths"] == stats.paths == int(counts.sum(dtype=np.uint64))
    if "DRT_POOL_BLOCKS" in env:
        assert stats.redone_launches >= 1  # a redone round: the counts are taken again from the film, not added to
    if "DRT_FORCE_BVH" in env:
        assert stats.path_flags & 1


def test_refining_on_a_strided_tile_and_over_groups():
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 40, 60)
    params = pydrt.make_params(40, 60, spp=MAX2, max_depth=6, seed=3, x0=7, y0=5, tile_w=25, tile_h=18, row_stride=3)
    n_pix = 25 * 18
    snaps = A.oracle_snapshots(bundle, params, R.rounds(MIN, MAX2, STEP))
    rel, _ = A.pick_rel_error(bundle, snaps, n_pix, MIN, MAX, STEP)
    rep, before, rep2, counts, film, stats = refine(bundle, params, (MIN, MAX, STEP, rel), (MAX2, STEP, rel / 2))
    want, _ = A.expected(bundle, snaps, n_pix, MIN, MAX2, STEP, rel / 2)
    assert np.array_equal(counts, want) and (counts > before).any() and np.unique(before[counts > before]).size >= 2
    A.assert_same_film(film, A.film_at_counts(snaps, counts), "strided tile")
    for devices in ([0, 0], [0, 0, 0]):
        grep, gbefore, grep2, gcounts, gfilm, gstats = refine(bundle, params, (MIN, MAX, STEP, rel), (MAX2, STEP, rel / 2), devices=devices)
        assert np.array_equal(gbefore, before) and np.array_equal(gcounts, counts), devices
        A.assert_same_film(gfilm, film, str(devices))
        assert grep2 == rep2 and gstats.paths == stats.paths
        # a contract refusal renders on no device
        g = pydrt.Group(bundle, params, devices)
        try:
            g.render_adaptive(MIN, MAX, STEP, rel)
            paths, film0 = g.stats().paths, g.read_film()
            with pytest.raises(RuntimeError, match="drt_group_render_adaptive_continue.*step must be one of"):
                g.render_adaptive_continue(MAX2, 5, rel / 2)
            assert g.stats().paths == paths and same_film_bits(g.read_film(), film0)
            assert np.array_equal(g.read_sample_counts().reshape(-1), before)
        finally:
            g.close()


def test_refining_the_headline_frame_equals_the_fresh_render():
    """1024^2 at depth 8, (16, 128, 16): rel_error 0.05 and then 0.02 on the same film = 0.02 at once"""
    W = 1024
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, W)
    params = pydrt.make_params(W, W, spp=128, max_depth=8, seed=1)
    frep, fcounts, ffilm, fstats = A.adaptive(bundle, params, 16, 128, 16, 0.02)
    rep, before, rep2, counts, film, stats = refine(bundle, params, (16, 128, 16, 0.05), (128, 16, 0.02))
    print("paths", rep["paths"], "+", rep2["paths"], "fresh", frep["paths"])
    assert np.array_equal(counts, fcounts), "%d counts differ" % int((counts != fcounts).sum())
    assert rep["paths"] + rep2["paths"] == frep["paths"] == stats.paths and rep2["paths"] > 0
    assert np.unique(before[counts > before]).size >= 3 and (counts == before).any()
    A.assert_same_film(film, ffilm, "headline frame")


def test_drt_render_program_checkpoints_and_resumes_an_adaptive_render(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    S = 69

    def run(d, spp, **extra):
        os.makedirs(d / "output", exist_ok=True)
        for sub in ("scenes", "spectra"):
            if not os.path.exists(d / sub):
                os.symlink(os.path.join(cases.REPO, sub), d / sub)
        cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
        cfg = cfg.replace("num_pixel_samples 4", "num_pixel_samples %d" % spp).replace("output_width      800", "output_width      48")
        cfg = cfg.replace("output_height     600", "output_height     32").replace("max_cast_depth    4", "max_cast_depth    6")
        (d / "config.cfg").write_text(cfg)
        env = {k: v for k, v in os.environ.items() if not k.startswith("DRT_ADAPTIVE")}
        env.update(DRT_ADAPTIVE_ERROR="0.1", DRT_ADAPTIVE_MIN_SPP="4", DRT_ADAPTIVE_STEP="4", **extra)
        r = subprocess.run([exe], cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        return r.stdout

    whole, parts = tmp_path / "whole", tmp_path / "parts"
    run(whole, 20)
    out = run(parts, 12, DRT_ADAPTIVE_CHECKPOINT_ROUNDS="1")
    assert "Adaptive checkpoint after 2 rounds" in out
    manifest = open(parts / "output" / "output.spd.ckpt").read()
    assert manifest.startswith("drt-checkpoint 3\nsamples 12\n") and "\nadaptive min_spp 4 max_spp 12 step 4 rel_error " in manifest
    px12 = np.fromfile(parts / "output" / "output.spd", dtype=np.float64, offset=40).reshape(-1, S + 1)
    assert set(np.unique(px12[:, S])) == {4.0, 8.0, 12.0}
    out = run(parts, 20, DRT_ADAPTIVE_RESUME="1")
    assert "Resuming an adaptive render: 1536 pixels hold %d samples, 12 at most" % int(px12[:, S].sum()) in out
    assert not os.path.exists(parts / "output" / "output.spd.ckpt")  # a final write outside checkpoint mode retires the checkpoint
    for name in ("output.spd", "average.spd"):
        assert open(parts / "output" / name, "rb").read() == open(whole / "output" / name, "rb").read(), name
    px = np.fromfile(whole / "output" / "output.spd", dtype=np.float64, offset=40).reshape(-1, S + 1)
    assert (px[:, S] > 12).any() and (px[:, S] == 4).any()
