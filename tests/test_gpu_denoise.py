"""GPU (-m gpu): the variance-guided denoiser (drt_denoise_film, drt_denoise_buffers, drt_group_denoise, the drt_render program's
DRT_DENOISE_K) against the rule of tests/denoise_rule.py, bit for bit: mean', var' and the number of unusable pixels. Every film a
bitwise test filters is first shown to take no subnormal quotient in the rule (there the device's division may be one unit off,
DESIGN.md section 2): a condition on the input, not a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import denoise_rule as D
import pydrt

pytestmark = pytest.mark.gpu

SCENES = ["plane_light_48", "gold_mirror", "grid_2p5nm", "grid_10nm", "lens", "spheres_1500", "first_scene"]
# (radius, patch, k): the corners of the ranges and the suggested values, two values of k and more
SETTINGS = [(0, 0, 1.0), (1, 0, 0.6), (5, 1, 1.0), (10, 3, 1.5)]


def cmf_rows(bundle):
    sc = bundle.scene
    return (int(sc.cmf_rw), int(sc.cmf_x), int(sc.cmf_y), int(sc.cmf_z))


def rule(bundle, params, film, R, F, k, alpha=1.0):
    """(mean', var', unusable) by the numpy rule; the film must take no subnormal quotient"""
    mean, var, unusable, subnormal = D.denoise(bundle.spds(), cmf_rows(bundle), float(bundle.scene.wavelength_interval), int(params.tile_w),
                                               int(params.tile_h), film[0], film[1], film[2], R, F, k, alpha)
    assert subnormal == 0, "%d quotients of the rule are subnormal on this film" % subnormal
    return mean, var, unusable


def assert_denoised(got_mean, got_var, got_unusable, want, what):
    assert got_unusable == want[2], "%s: %d unusable pixels, the rule has %d" % (what, got_unusable, want[2])
    assert cases.same_bits(got_mean, want[0]), "%s mean': %s" % (what, cases.first_difference(got_mean, want[0]))
    assert cases.same_bits(got_var, want[1]), "%s var': %s" % (what, cases.first_difference(got_var, want[1]))


def check_session(r, bundle, params, film, R, F, k, alpha=1.0, what=""):
    rep = r.denoise(R, F, k, alpha)
    mean, var = r.read_denoised()
    assert rep["kernel_ms"] > 0.0
    assert_denoised(mean, var, rep["unusable"], rule(bundle, params, film, R, F, k, alpha), "%s R %d F %d k %g" % (what, R, F, k))
    return mean, var


@pytest.mark.parametrize("name", SCENES)
def test_the_device_equals_the_rule_on_rendered_films(name):
    bundle, params = cases.load_case(name)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        film = r.read_film()
        changed = 0
        for R, F, k in SETTINGS:
            mean, _ = check_session(r, bundle, params, film, R, F, k, what=name)
            changed += int(not cases.same_bits(mean, film[1]))
        assert changed >= 2  # (radius 0 returns the mean itself; the others must not, or nothing was filtered)
    finally:
        r.close()


def test_a_radius_larger_than_the_tile():
    bundle, _ = cases.load_case("plane_light_48")
    params = pydrt.make_params(48, 48, spp=4, max_depth=8, seed=1, x0=20, y0=9, tile_w=7, tile_h=5)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        film = r.read_film()
        for R, F, k in [(10, 3, 1.0), (8, 0, 2.0), (10, 1, 0.5)]:
            check_session(r, bundle, params, film, R, F, k, alpha=0.5, what="7 x 5 tile")
    finally:
        r.close()


def test_an_adaptive_film_and_its_continuation():
    bundle, p = cases.load_case("plane_light_48")
    params = pydrt.make_params(int(p.width), int(p.height), spp=32, max_depth=int(p.max_depth), seed=int(p.seed))
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_adaptive(4, 24, 4, 0.08)
        counts = r.read_sample_counts()
        assert len(np.unique(counts)) >= 3
        film = r.read_film()
        paths = r.stats().paths
        assert np.array_equal(film[0][:, -1], counts.reshape(-1).astype(np.float64))
        for R, F, k in [(5, 1, 1.0), (2, 2, 0.8)]:
            check_session(r, bundle, params, film, R, F, k, what="adaptive")
        # no film bit, no count and no render state has changed
        after = r.read_film()
        for a, b in zip(film, after):
            assert cases.same_bits(a, b)
        assert np.array_equal(r.read_sample_counts(), counts) and r.stats().paths == paths
        rep = r.render_adaptive_continue(32, 4, 0.05)
        assert rep["paths"] > 0
        with pytest.raises(RuntimeError, match="the film has changed since drt_denoise_film"):
            r.read_denoised()
        film2 = r.read_film()
        assert len(np.unique(film2[0][:, -1])) >= 3
        check_session(r, bundle, params, film2, 5, 1, 1.0, what="continued")
    finally:
        r.close()
    # the continuation after a denoise is the continuation without one
    q = pydrt.Renderer(bundle, params)
    try:
        q.render_adaptive(4, 24, 4, 0.08)
        q.render_adaptive_continue(32, 4, 0.05)
        for a, b in zip(film2, q.read_film()):
            assert cases.same_bits(a, b)
    finally:
        q.close()


def test_the_hand_made_film_through_write_film():
    bundle, _ = cases.load_case("grid_10nm")
    px, av, va, w, h = D.hand_made_film(bundle.S)
    params = pydrt.make_params(w, h, spp=2, max_depth=2)
    r = pydrt.Renderer(bundle, params)
    try:
        r.write_film(px, av, va)
        for R, F, k, alpha in [(2, 1, 1.0, 1.0), (3, 0, 0.7, 0.5), (1, 2, 2.0, 0.0), (0, 0, 1.0, 1.0), (10, 3, 1.0, 1.0)]:
            check_session(r, bundle, params, (px, av, va), R, F, k, alpha, what="hand-made")
        assert r.denoise(2, 1)["unusable"] == 9
    finally:
        r.close()


def test_the_film_is_untouched_and_drt_render_continues():
    bundle, p = cases.load_case("gold_mirror")
    params = pydrt.make_params(int(p.width), int(p.height), spp=6, max_depth=int(p.max_depth), seed=int(p.seed))
    r = pydrt.Renderer(bundle, params)
    whole = pydrt.Renderer(bundle, params)
    try:
        r.render(0, 3)
        before, paths = r.read_film(), r.stats().paths
        r.denoise(5, 1)
        r.read_denoised()
        r.read_denoised_bgra()
        for a, b in zip(before, r.read_film()):
            assert cases.same_bits(a, b)
        assert r.stats().paths == paths
        r.render(3, 3)
        whole.render(0, 6)
        for a, b in zip(r.read_film(), whole.read_film()):
            assert cases.same_bits(a, b)
        assert r.stats().paths == whole.stats().paths
    finally:
        r.close()
        whole.close()


def test_the_one_shot_and_the_group_forms_equal_the_session_form():
    bundle, params = cases.load_case("lens")
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        film = r.read_film()
        rep = r.denoise(5, 1, 0.9, 1.0)
        mean, var = r.read_denoised()
    finally:
        r.close()
    m1, v1, rep1 = pydrt.denoise_buffers(bundle, params, *film, radius=5, patch=1, k=0.9, alpha=1.0)
    assert_denoised(m1, v1, rep1["unusable"], (mean, var, rep["unusable"]), "drt_denoise_buffers")
    for devices in ([0], [0, 0], [0, 0, 0]):
        g = pydrt.Group(bundle, params, devices)
        try:
            g.render()
            gm, gv, grep = g.denoise(5, 1, 0.9, 1.0)
            for a, b in zip(film, g.read_film()):
                assert cases.same_bits(a, b)
        finally:
            g.close()
        assert_denoised(gm, gv, grep["unusable"], (mean, var, rep["unusable"]), "group %s" % devices)


def host_bgra(bundle, width, height, mean, tmp_path):
    """the pixel bytes host/drt_bmp.c gives a spectral film without a filter column"""
    H = pydrt.host_lib()
    f64p = C.POINTER(C.c_double)
    H.drt_host_spd_file_to_bmp.argtypes = [C.c_char_p, C.c_char_p, f64p]
    H.drt_host_write_spd.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, f64p]
    sc = bundle.scene
    spd, bmp = str(tmp_path / "mean.spd"), str(tmp_path / "mean.bmp")
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    assert H.drt_host_write_spd(spd.encode(), width, height, bundle.S, 0, float(sc.min_wavelength), float(sc.wavelength_interval),
                                mean.ctypes.data_as(f64p)) == 0
    rw = int(sc.cmf_rw)
    assert cmf_rows(bundle) == (rw, rw + 1, rw + 2, rw + 3)
    cmf = np.ascontiguousarray(bundle.spds()[rw:rw + 4])
    assert H.drt_host_spd_file_to_bmp(spd.encode(), bmp.encode(), cmf.ctypes.data_as(f64p)) == 0
    return np.frombuffer(open(bmp, "rb").read()[54:], dtype=np.uint8).reshape(-1, 4)


def test_read_denoised_bgra_is_the_hosts_conversion_of_the_denoised_mean(tmp_path):
    bundle, params = cases.load_case("plane_light_48")
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        r.denoise(5, 1)
        mean, _ = r.read_denoised()
        got = r.read_denoised_bgra()
        plain = r.read_bgra(1)
    finally:
        r.close()
    want = host_bgra(bundle, int(params.tile_w), int(params.tile_h), mean, tmp_path)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, plain) and len(np.unique(got)) > 50  # a picture, and not the noisy one


def test_refusals_each_with_its_message():
    bundle, p = cases.load_case("plane_light_16")
    w, h = int(p.width), int(p.height)

    def ctx(**kw):
        return pydrt.Renderer(bundle, pydrt.make_params(w, h, spp=4, max_depth=4, **kw))

    r = ctx(mode=pydrt.MODE_XYZ)
    try:
        r.render()
        with pytest.raises(RuntimeError, match="needs the spectral film"):
            r.denoise()
    finally:
        r.close()
    r = ctx(row_stride=2, tile_h=h // 2)
    try:
        r.render()
        with pytest.raises(RuntimeError, match="row_stride = 2"):
            r.denoise()
    finally:
        r.close()
    r = ctx()
    try:
        r.render()
        film = r.read_film()
        with pytest.raises(RuntimeError, match="no denoised film: drt_denoise_film first"):
            r.read_denoised()
        with pytest.raises(RuntimeError, match="no denoised film: drt_denoise_film first"):
            r.read_denoised_bgra()
        for kw, word in [(dict(radius=11), "radius"), (dict(patch=4), "patch"), (dict(k=0.0), "k ="), (dict(alpha=-1.0), "alpha")]:
            with pytest.raises(RuntimeError, match=word):
                r.denoise(**kw)
        with pytest.raises(RuntimeError, match="no denoised film"):  # a refused call has done nothing
            r.read_denoised()
        for change in (lambda: r.render(4, 2), lambda: r.write_film(*film), lambda: r.reset_film()):
            r.denoise()
            r.read_denoised()
            change()
            with pytest.raises(RuntimeError, match="the film has changed since drt_denoise_film"):
                r.read_denoised()
            with pytest.raises(RuntimeError, match="the film has changed since drt_denoise_film"):
                r.read_denoised_bgra()
    finally:
        r.close()


def test_drt_render_program_with_the_denoiser(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("num_pixel_samples 4", "num_pixel_samples 8").replace("output_width      800", "output_width      48")
    cfg = cfg.replace("output_height     600", "output_height     32").replace("max_cast_depth    4", "max_cast_depth    6")

    def run(name, **env):
        d = tmp_path / name
        os.makedirs(d / "output")
        for sub in ("scenes", "spectra"):
            os.symlink(os.path.join(cases.REPO, sub), d / sub)
        (d / "config.cfg").write_text(cfg)
        full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_DENOISE")}
        full.update(env)
        r = subprocess.run([exe], cwd=d, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        return d / "output", r.stdout

    plain, _ = run("plain")
    out, text = run("denoised", DRT_DENOISE_K="0.9", DRT_DENOISE_RADIUS="4", DRT_DENOISE_VAR_SPD="output/dv.spd")
    assert "Denoised: radius 4, patch 1, k 0.9, alpha 1" in text
    for f in ("output.spd", "average.spd", "variance.spd", "output.bmp", "average.bmp", "variance.bmp"):
        assert open(plain / f, "rb").read() == open(out / f, "rb").read(), f
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain) + ["output.spd.denoised.spd", "dv.spd"])  # and no temporary file is left
    S = 69
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 48, 32)
    params = pydrt.make_params(48, 32, spp=8, max_depth=6, seed=1)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        r.denoise(4, 1, 0.9, 1.0)
        mean, var = r.read_denoised()
    finally:
        r.close()
    head = open(out / "average.spd", "rb").read()[:40]
    for f, want in (("output.spd.denoised.spd", mean), ("dv.spd", var)):
        assert open(out / f, "rb").read()[:40] == head, f  # the average file's header: no filter column
        got = np.fromfile(out / f, dtype=np.float64, offset=40).reshape(-1, S)
        assert cases.same_bits(got, want), "%s: %s" % (f, cases.first_difference(got, want))
    assert not cases.same_bits(mean, np.fromfile(out / "average.spd", dtype=np.float64, offset=40).reshape(-1, S))
