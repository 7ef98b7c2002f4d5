"""GPU (-m gpu): sensor films (drt_bind_sensor).

The rule is tests/sensor_rule.py: per sample, the spectrum times each curve, summed by pairs inside every set of 64 wavelengths and over
the sets in order, through the reference's film update. Its input is the oracle's one-sample render of every sample
(sensor_cases.samples_device: cases.oracle_render_device_pow with spp = 1, first_sample = m). Every test compares all three buffers
of the sensor film with cases.same_bits, and the main film against the oracle. tests/test_sensor_cpu.py shows, on the oracle alone,
that delta curves turn the rule into the oracle's own film update, and that the rule's sum is not a left-to-right one. Sizes, samples
and depths are those of tests/cases.py: at most 32 x 32 pixels and 4 samples."""
import contextlib
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import cases
import pydrt
import sensor_cases as SC
import sensor_rule

pytestmark = pytest.mark.gpu

BASE = SC.BASE


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


def render_with_sensor(bundle, params, curves, calls=None, before_render=None):
    """(main film, sensor film, stats) of a fresh context bound to `curves`"""
    r = pydrt.Renderer(bundle, params)
    try:
        if before_render:
            before_render(r)
        r.bind_sensor(curves)
        for first, n in (calls or [(None, None)]):
            r.render(first, n)
        return r.read_film(), r.read_sensor_film(), r.stats()
    finally:
        r.close()


def assert_main_film(name, main, what, **changes):
    SC.assert_film(main, SC.film_device(name, **changes)[:3], "%s: %s, the main film against the oracle" % (what, name))


def check_case(name, curves, what, **kw):
    bundle, params = SC.load(name)
    main, sensor, st = render_with_sensor(bundle, params, curves, **kw)
    assert_main_film(name, main, what)
    SC.assert_film(sensor, SC.expected_film(name, curves), "%s: %s, the sensor film against the rule" % (what, name))
    return main, sensor, st


@pytest.mark.parametrize("n", [1, 3, 8])
def test_seeded_curves_with_negative_values(n):
    bundle, _ = SC.load(BASE)
    _, sensor, _ = check_case(BASE, SC.seeded_curves(n, bundle.S), "%d channels" % n)
    assert sensor[0].shape[1] == n + 1 and (sensor[1] != 0).any() and (sensor[2] != 0).any()


@pytest.mark.parametrize("name", [c for c in SC.GPU_CASES if c != BASE])
def test_every_case_against_the_rule(name):
    bundle, params = SC.load(name)
    main, sensor, st = check_case(name, SC.seeded_curves(3, bundle.S), "three channels")
    if name == "spheres_1500":
        assert st.path_flags & pydrt.PATH_BVH, "spheres_1500 is meant to go through the hierarchy pipeline"
    if name == "example_scene":
        assert np.isnan(sensor[0][:, :-1]).all() and np.isnan(sensor[1]).all()
        assert np.array_equal(sensor[0][:, -1], np.full(sensor[0].shape[0], float(params.spp)))
    else:
        assert cases.stat_counts(st) == cases.stat_counts(SC.film_device(name)[4])


@pytest.mark.parametrize("name", [BASE, "grid_10nm", "grid_2p5nm"])
def test_delta_curves_give_the_main_films_own_columns(name):
    bundle, params = SC.load(name)
    S = bundle.S
    w = SC.delta_wavelengths(S)
    (px, av, va), sensor, _ = render_with_sensor(bundle, params, SC.delta_curves(S, w))
    want = (np.concatenate([px[:, w], px[:, S:]], axis=1), av[:, w], va[:, w])
    SC.assert_film(sensor, want, "%s: delta curves against the main film from the device alone" % name)
    assert (va[:, w] != 0).any()


def test_observer_curves_give_read_xyz():
    """sum_k / filter * (interval / n) against drt_read_xyz, per pixel and channel, rtol = 1e-12: two orders of summation of terms that
    are non-negative (but for one curve value of -1.7e-21, tests/test_sensor_cpu.py), so the first-order bound on their difference is
    about (samples + S + 4) * 2^-53 < 1e-14 relative; the two orders of margin cover what that bound leaves out"""
    bundle, params = SC.load(BASE)
    curves = pydrt.observer_curves(bundle)
    r = pydrt.Renderer(bundle, params)
    try:
        r.bind_sensor(curves)
        r.render()
        xyz, (px, _, _) = r.read_xyz(), r.read_sensor_film()
    finally:
        r.close()
    interval = float(bundle.scene.wavelength_interval)
    n = 0.0
    for v in curves[1]:
        n = n + float(v)
    n = n * interval
    got = px[:, :3] / px[:, 3:] * (interval / n)
    assert (xyz > 0).any()
    for k in range(3):
        print("channel %d: largest relative difference %.3g" % (k, np.max(np.abs(got[:, k] - xyz[:, k]) / np.where(xyz[:, k] != 0, np.abs(xyz[:, k]), 1.0))))
    assert np.array_equal(got == 0, xyz == 0), "a pixel that is exactly zero on one side is not on the other"
    assert np.allclose(got, xyz, rtol=1e-12, atol=0.0)


def test_binding_a_sensor_changes_nothing_else():
    """the main film, the statistics' counts and the hit log: the same bits with a sensor bound and without"""
    bundle, params = SC.load(BASE)
    p = SC.params_with(params, flags=pydrt.FLAG_RECORD_HITS)
    out = []
    for curves in (None, SC.seeded_curves(3, bundle.S)):
        r = pydrt.Renderer(bundle, p)
        try:
            if curves is not None:
                r.bind_sensor(curves)
            r.render()
            out.append((r.read_film(), r.read_hit_indices(int(p.spp)), r.stats(), r.read_xyz()))
            if curves is not None:
                SC.assert_film(r.read_sensor_film(), SC.expected_film(BASE, curves), "with DRT_FLAG_RECORD_HITS")
        finally:
            r.close()
    (film0, hits0, st0, xyz0), (film1, hits1, st1, xyz1) = out
    SC.assert_film(film1, film0, "the main film with a sensor bound against without")
    assert np.array_equal(hits0, hits1) and cases.same_bits(xyz0, xyz1)
    assert np.array_equal(hits0, SC.film_device(BASE)[3])
    assert cases.stat_counts(st0) == cases.stat_counts(st1) and st0.launches == st1.launches


def test_one_call_several_calls_and_small_batches_give_the_same_sensor_film():
    bundle, params = SC.load(BASE)
    spp = int(params.spp)
    assert spp == 4
    curves = SC.seeded_curves(3, bundle.S)
    ways = {
        "three calls": (params, [(0, 1), (1, 2), (3, 1)]),
        "batch_spp 1": (SC.params_with(params, batch_spp=1), None),
        "batch_spp 3": (SC.params_with(params, batch_spp=3), None),
    }
    for what, (p, calls) in ways.items():
        main, sensor, st = render_with_sensor(bundle, p, curves, calls=calls)
        if what == "batch_spp 1":
            assert st.launches == spp
        assert_main_film(BASE, main, what)
        SC.assert_film(sensor, SC.expected_film(BASE, curves), what)


def test_a_record_pool_that_runs_out_is_rendered_again_sensor_film_included(monkeypatch):
    """DRT_POOL_BLOCKS=1: the launches that ran out leave the sensor film untouched, as the main film, and are rendered again"""
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    bundle, _ = SC.load(BASE)
    _, _, st = check_case(BASE, SC.seeded_curves(3, bundle.S), "tiny record pool")
    assert st.redone_launches > 0, "no launch ran out of record blocks"


def test_behind_a_forced_hierarchy():
    bundle, _ = SC.load(BASE)
    with environment(DRT_FORCE_BVH="1"):
        _, _, st = check_case(BASE, SC.seeded_curves(3, bundle.S), "DRT_FORCE_BVH")
    assert st.path_flags & pydrt.PATH_BVH


def test_a_ray_table_of_the_cameras_centre_rays():
    import ray_film_cases as R
    bundle, params = SC.load(BASE)
    w, h = int(params.width), int(params.height)
    assert float(bundle.camera.aperture_radius) == 0.0
    curves = SC.seeded_curves(3, bundle.S)
    table = R.centre_rays(bundle, w, h)
    p = SC.params_with(params, pixel_scheme=pydrt.FILM_SAMPLE_CENTER)
    main, sensor, st = render_with_sensor(bundle, p, curves, before_render=lambda r: r.bind_rays(*table))
    assert st.path_flags & pydrt.PATH_RAYS
    assert_main_film(BASE, main, "ray table", pixel_scheme=pydrt.FILM_SAMPLE_CENTER)
    SC.assert_film(sensor, SC.expected_film(BASE, curves, pixel_scheme=pydrt.FILM_SAMPLE_CENTER), "ray table")


def test_after_update_materials_and_reset_film_the_sensor_film_is_a_fresh_contexts():
    bundle, params = SC.load(BASE)
    curves = SC.seeded_curves(3, bundle.S)
    text = open(cases.scene_path(cases.RENDER_CASES[BASE][0])).read()
    assert "shininess 100.0" in text
    after = pydrt.load_scene_text(text.replace("shininess 100.0", "shininess 30.0"), int(params.width), int(params.height))
    fresh_main, fresh_sensor, _ = render_with_sensor(after, params, curves)
    r = pydrt.Renderer(bundle, params)
    try:
        r.bind_sensor(curves)
        r.render()
        before = r.read_sensor_film()
        r.reset_film()
        r.update_materials(after.materials())
        assert not any(a.any() for a in r.read_sensor_film()), "drt_reset_film zeroes the sensor film"
        r.render()
        main, sensor = r.read_film(), r.read_sensor_film()
    finally:
        r.close()
    SC.assert_film(main, fresh_main, "updated context against a fresh one, main film")
    SC.assert_film(sensor, fresh_sensor, "updated context against a fresh one, sensor film")
    SC.assert_film(before, SC.expected_film(BASE, curves), "before the update")
    assert not cases.same_bits(before[0], sensor[0]), "the update changes the film"


def test_a_strided_tile():
    bundle, params = SC.load(BASE)
    curves = SC.seeded_curves(3, bundle.S)
    tile = dict(x0=3, y0=1, tile_w=11, tile_h=5, row_stride=3)
    main, sensor, _ = render_with_sensor(bundle, SC.params_with(params, **tile), curves)
    assert sensor[1].shape == (55, 3)
    assert_main_film(BASE, main, "strided tile", **tile)
    SC.assert_film(sensor, SC.expected_film(BASE, curves, **tile), "strided tile")


def test_a_groups_assembled_sensor_film_is_a_single_contexts():
    bundle, params = SC.load(BASE)
    curves = SC.seeded_curves(3, bundle.S)
    g = pydrt.Group(bundle, params, devices=[0, 0, 0])
    try:
        with pytest.raises(RuntimeError, match="no sensor is bound"):
            g.read_sensor_film()
        with pytest.raises(RuntimeError, match="9 channels, at most 8"):
            g.bind_sensor(np.zeros((9, bundle.S)))
        g.bind_sensor(curves)
        g.render()
        main, sensor = g.read_film(), g.read_sensor_film()
        with pytest.raises(RuntimeError, match="drt_reset_film first"):
            g.bind_sensor(curves[:1])
        with pytest.raises(RuntimeError, match="a sensor is bound"):
            g.bind_depth_cuts([1])
        SC.assert_film(g.read_sensor_film(), sensor, "after the group's refusals")
        g.reset_film()
        g.bind_sensor(None)
        with pytest.raises(RuntimeError, match="no sensor is bound"):
            g.read_sensor_film()
    finally:
        g.close()
    assert_main_film(BASE, main, "a group of three contexts")
    SC.assert_film(sensor, SC.expected_film(BASE, curves), "a group of three contexts")


def test_read_sensor_bgra_gives_the_rules_bytes():
    bundle, params = SC.load(BASE)
    rng = np.random.default_rng(5)
    curves = pydrt.observer_curves(bundle) / 20.0
    five = np.concatenate([curves, SC.seeded_curves(2, bundle.S)])
    for cv, matrix in ((curves, np.array([[2.3706743, -0.9000405, -0.4706338], [-0.5138850, 1.4253036, 0.0885814], [0.0052982, -0.0146949, 1.0093968]])),
                       (five, rng.uniform(-0.5, 1.0, size=(3, 5)))):
        r = pydrt.Renderer(bundle, params)
        try:
            r.bind_sensor(cv)
            r.render()
            film = r.read_sensor_film()
            got = [r.read_sensor_bgra(w, matrix) for w in (0, 1)]
            ptrs = r.sensor_film_device_ptrs()
            assert all(ptrs) and len(set(ptrs) | set(r.film_device_ptrs())) == 6
            with pytest.raises(RuntimeError, match="which = 2"):
                r.read_sensor_bgra(2, matrix)
        finally:
            r.close()
        for w in (0, 1):
            want = sensor_rule.bgra(film, w, matrix)
            assert np.array_equal(got[w], want), "which = %d: %d bytes differ" % (w, int((got[w] != want).sum()))
            assert len(np.unique(want[:, :3])) > 20, "a picture of one colour tells nothing"


def test_every_refusal_says_why_and_leaves_the_context_as_it_was():
    bundle, params = SC.load(BASE)
    S = bundle.S
    curves = SC.seeded_curves(3, S)
    want = SC.expected_film(BASE, curves)
    gc.collect()
    r = pydrt.Renderer(bundle, params)
    L = r.L

    def state():
        return r.read_film(), r.read_sensor_film() if getattr(r, "n_sensor", 0) else None, cases.stat_counts(r.stats()), pydrt.selftest_live_resources()

    def refused(call, why):
        before = state()
        with pytest.raises(RuntimeError, match=why):
            call()
        after = state()
        SC.assert_film(after[0], before[0], "main film across the refusal '%s'" % why)
        if before[1] is not None:
            SC.assert_film(after[1], before[1], "sensor film across the refusal '%s'" % why)
        assert after[2:] == before[2:], why

    try:
        for read in (r.read_sensor_film, r.sensor_film_device_ptrs, lambda: r.read_sensor_bgra(0, np.eye(3))):
            refused(read, "no sensor is bound")
        refused(lambda: r.bind_sensor(np.zeros((9, S))), "9 channels, at most 8")
        refused(lambda: pydrt._check(L.drt_bind_sensor(r.ctx, None, 2), "drt_bind_sensor"), "null curves")
        for bad in (np.nan, np.inf, -np.inf):
            c = curves.copy()
            c[1, 7] = bad
            refused(lambda: r.bind_sensor(c), "curve 1 is not finite at wavelength 7")
        r.bind_depth_cuts((1, 2))
        refused(lambda: r.bind_sensor(curves), "depth cuts are bound")
        r.bind_depth_cuts(None)
        r.bind_sensor(curves)
        refused(lambda: r.bind_depth_cuts((1, 2)), "a sensor is bound")
        refused(lambda: r.render_adaptive(2, 4, 1, 0.1), "a sensor bound")
        refused(lambda: r.render_adaptive_continue(4, 1, 0.1), "a sensor bound")
        refused(lambda: r.render_sample_map(np.full(r.n_pixels, 2, dtype=np.uint32)), "a sensor bound")
        r.render()
        refused(lambda: r.bind_sensor(curves[:2]), "already holds samples")
        refused(lambda: pydrt._check(L.drt_read_sensor_bgra(r.ctx, 0, None, None), "drt_read_sensor_bgra"), "null argument")
        SC.assert_film(r.read_sensor_film(), want, "after the refusals")
        assert_main_film(BASE, r.read_film(), "after the refusals")
        # unbound after a reset: adaptive sampling works again, and a film that holds an adaptive render takes no sensor
        r.reset_film()
        r.bind_sensor(None)
        r.render_adaptive(2, 4, 1, 0.1)
        refused(lambda: r.bind_sensor(curves), "drt_reset_film first")
        r.reset_film()
        r.bind_sensor(curves)
        r.render()
        SC.assert_film(r.read_sensor_film(), want, "bound again after an adaptive render and a reset")
    finally:
        r.close()
    x = pydrt.Renderer(bundle, SC.params_with(params, mode=pydrt.MODE_XYZ))
    try:
        with pytest.raises(RuntimeError, match="DRT_MODE_XYZ"):
            x.bind_sensor(curves)
        x.render()
        assert np.isfinite(x.read_xyz()).all()
    finally:
        x.close()


def test_live_resources_after_bind_rebind_unbind_and_close():
    bundle, params = SC.load(BASE)
    S = bundle.S
    gc.collect()
    base = pydrt.selftest_live_resources()
    now = lambda: tuple(a - b for a, b in zip(pydrt.selftest_live_resources(), base))
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        r.read_film()
        r.reset_film()
        unbound = now()
        r.bind_sensor(SC.seeded_curves(3, S))
        assert now()[0] == unbound[0] + 4 and now()[1:] == unbound[1:], "the curves and three film buffers"
        r.render()
        r.read_sensor_film()
        r.reset_film()
        r.bind_sensor(SC.seeded_curves(8, S))
        assert now()[0] == unbound[0] + 4, "the earlier film is released by the next bind"
        r.render()
        assert r.read_sensor_film()[1].shape[1] == 8
        r.reset_film()
        r.bind_sensor(None)
        assert now() == unbound
        r.bind_sensor(SC.seeded_curves(2, S))
        r.render()
        assert now()[0] > 0
    finally:
        r.close()
    gc.collect()
    assert now() == (0, 0, 0, 0), "%s still held (device, pinned, events, streams)" % (now(),)


def test_drt_render_program_with_three_curves(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    W, H = 24, 16
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("output_width      800", "output_width      %d" % W).replace("output_height     600", "output_height     %d" % H)
    tables = {"r.csv": [(380, 0.0), (560, 0.02), (610, 0.06), (720, 0.01)], "g.csv": [(380, 0.0), (540, 0.07), (720, 0.0)],
              "b.csv": [(380, 0.03), (450, 0.08), (550, 0.0), (720, 0.0)]}

    def run(name, **env):
        d = tmp_path / name
        os.makedirs(d / "output")
        for sub in ("scenes", "spectra"):
            os.symlink(os.path.join(cases.REPO, sub), d / sub)
        (d / "config.cfg").write_text(cfg)
        for f, rows in tables.items():
            (d / f).write_text("wavelength,value\n" + "".join("%d,%g\n" % row for row in rows))
        full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
        full.update(env)
        r = subprocess.run([exe], cwd=d, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        return d, r.stdout

    plain, _ = run("plain")
    d, text = run("sensor", DRT_SENSOR="r.csv,g.csv,b.csv", DRT_DEVICES="0,0")
    assert "Sensor film: 3 channels" in text
    standard = ("output.spd", "average.spd", "variance.spd", "output.bmp", "average.bmp", "variance.bmp")
    for f in standard:
        assert open(plain / "output" / f, "rb").read() == open(d / "output" / f, "rb").read(), f
    extra = ["output.spd.sensor.spd", "average.spd.sensor.spd", "variance.spd.sensor.spd", "output.spd.sensor.bmp"]
    assert sorted(os.listdir(d / "output")) == sorted(os.listdir(plain / "output") + extra)  # and no temporary file is left
    # the same render through pydrt, with the curves resampled by the same function
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, H)
    S = bundle.S
    curves = np.zeros((3, S))
    for k, f in enumerate(("r.csv", "g.csv", "b.csv")):
        assert pydrt.host_lib().drt_host_csv_to_spectrum(str(d / f).encode(), 380.0, 5.0, S, curves[k].ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert (curves > 0).any(axis=1).all()
    r = pydrt.Renderer(bundle, pydrt.make_params(W, H, spp=4, max_depth=4, seed=1))
    try:
        r.bind_sensor(curves)
        r.render()
        px, av, va = r.read_sensor_film()
        picture = r.read_sensor_bgra(0, np.eye(3))
    finally:
        r.close()
    P = W * H
    for f, a in (("output.spd.sensor.spd", px), ("average.spd.sensor.spd", av)):
        raw = open(d / "output" / f, "rb").read()
        assert len(raw) > a.size * 8 and cases.same_bits(np.frombuffer(raw[-a.size * 8:], dtype=np.float64).reshape(a.shape), a), f
    raw = open(d / "output" / "variance.spd.sensor.spd", "rb").read()
    assert len(raw) > P * 3 * 8
    bmp = np.frombuffer(open(d / "output" / "output.spd.sensor.bmp", "rb").read()[-P * 4:], dtype=np.uint8).reshape(H, W, 4)
    want = picture.reshape(H, W, 4)
    assert np.array_equal(bmp, want) or np.array_equal(bmp, want[::-1]), "the picture is not drt_read_sensor_bgra's through the identity"
    assert len(np.unique(want[:, :, :3])) > 10
