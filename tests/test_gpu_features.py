"""GPU (-m gpu): the first-hit feature buffers (drt_render_features, drt_read_features, drt_read_feature_bgra, drt_group_render_features,
the drt_render program's DRT_FEATURES) against the rule of tests/feature_rule.py, bit for bit: mean, m2, ids and the number of empty
pixels. Every case a bitwise test runs is first shown to take no subnormal quotient in the rule (there the device's division may be
one unit off): a condition on the input, not a tolerance."""
import os
import subprocess

import numpy as np
import pytest

import cases
import feature_rule as F
import pydrt

pytestmark = pytest.mark.gpu

CASES = ["plane_light_16", "plane_light_center", "lights", "lens", "downward", "spheres_1500", "example_scene"]

_rule = {}


def rule(bundle, params, n_samples=None, first_sample=0, counts=None, key=None):
    """(mean, m2, ids, empty pixels) by the rule (computed once per key); the case must take no subnormal quotient"""
    if key is None or key not in _rule:
        mean, m2, ids, empty, subnormal = F.features(bundle, params, n_samples=n_samples, first_sample=first_sample, counts=counts)
        assert subnormal == 0, "%d quotients of the rule are subnormal on this case" % subnormal
        if key is None:
            return mean, m2, ids, empty
        _rule[key] = (mean, m2, ids, empty)
    return _rule[key]


def assert_features(got, empty, want, what):
    assert cases.same_bits(got[0], want[0]), "%s mean: %s" % (what, cases.first_difference(got[0], want[0]))
    assert cases.same_bits(got[1], want[1]), "%s m2: %s" % (what, cases.first_difference(got[1], want[1]))
    assert np.array_equal(got[2], want[2]), "%s ids: %d differ" % (what, int((got[2] != want[2]).sum()))
    assert empty == want[3], "%s: %d empty pixels, the rule has %d" % (what, empty, want[3])


def session(bundle, params, n_samples, first_sample=0):
    r = pydrt.Renderer(bundle, params)
    try:
        rep = r.render_features(n_samples, first_sample)
        got = r.read_features()
    finally:
        r.close()
    assert rep["kernel_ms"] > 0.0 and rep["rays"] == r.n_pixels * n_samples
    return got, rep


@pytest.mark.parametrize("name", CASES)
def test_the_device_equals_the_rule(name):
    bundle, params = cases.load_case(name)
    spp = int(params.spp)
    got, rep = session(bundle, params, spp)
    assert_features(got, rep["empty_pixels"], rule(bundle, params, n_samples=spp, key=name), name)


def test_a_tile_that_is_no_multiple_of_a_wave():
    bundle, _ = cases.load_case("plane_light_48")
    params = pydrt.make_params(48, 48, spp=4, max_depth=8, seed=1, x0=20, y0=9, tile_w=7, tile_h=5)
    got, rep = session(bundle, params, 4)
    want = rule(bundle, params, n_samples=4)
    assert_features(got, rep["empty_pixels"], want, "7 x 5 tile")
    assert (want[2] >= 0).any()


def test_a_row_stride_and_a_first_sample():
    bundle, p = cases.load_case("lights")
    params = pydrt.make_params(32, 32, spp=4, max_depth=6, seed=5, x0=3, y0=1, tile_w=29, tile_h=15, row_stride=2)
    got, rep = session(bundle, params, 3)
    assert_features(got, rep["empty_pixels"], rule(bundle, params, n_samples=3), "row_stride 2")
    bundle, params = cases.load_case("plane_light_16")
    got3, rep3 = session(bundle, params, 4, first_sample=3)
    want3 = rule(bundle, params, n_samples=4, first_sample=3)
    assert_features(got3, rep3["empty_pixels"], want3, "first_sample 3")
    assert not cases.same_bits(want3[0], rule(bundle, params, n_samples=4, key="plane_light_16")[0])


@pytest.mark.parametrize("name", ["plane_light_16", "lens", "spheres_1500"])
def test_ids_are_the_renders_own_first_hits(name):
    bundle, p = cases.load_case(name)
    params = pydrt.make_params(int(p.width), int(p.height), spp=int(p.spp), max_depth=int(p.max_depth), seed=int(p.seed),
                               pixel_scheme=int(p.pixel_scheme), flags=pydrt.FLAG_RECORD_HITS)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        hits = r.read_hit_indices(int(p.spp))
        r.render_features(int(p.spp))
        ids = r.read_features()[2]
    finally:
        r.close()
    assert np.array_equal(ids, hits[:r.n_pixels, 0])  # paths are ordered (sample, tile row, tile column)
    assert (ids >= 0).any() and (ids < 0).any()


def test_an_adaptive_film_gives_every_pixel_its_own_count():
    bundle, p = cases.load_case("plane_light_48")
    params = pydrt.make_params(int(p.width), int(p.height), spp=32, max_depth=int(p.max_depth), seed=int(p.seed))
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_adaptive(4, 24, 4, 0.08)
        counts = r.read_sample_counts()
        assert len(np.unique(counts)) >= 3
        film = r.read_film()
        paths = r.stats().paths
        rep = r.render_features(0)
        got = r.read_features()
        assert rep["rays"] == int(counts.sum())
        assert_features(got, rep["empty_pixels"], rule(bundle, params, counts=counts.reshape(-1)), "adaptive")
        # no film bit, no count and no render state has changed
        for a, b in zip(film, r.read_film()):
            assert cases.same_bits(a, b)
        assert np.array_equal(r.read_sample_counts(), counts) and r.stats().paths == paths
        cont = r.render_adaptive_continue(32, 4, 0.05)
        assert cont["paths"] > 0
        with pytest.raises(RuntimeError, match="the film has changed since drt_render_features"):
            r.read_features()
        with pytest.raises(RuntimeError, match="the film has changed since drt_render_features"):
            r.read_feature_bgra(pydrt.FEATURE_COVERAGE, 0.0, 1.0)
        film2 = r.read_film()
    finally:
        r.close()
    # the continuation after a feature pass is the continuation without one
    q = pydrt.Renderer(bundle, params)
    try:
        q.render_adaptive(4, 24, 4, 0.08)
        q.render_adaptive_continue(32, 4, 0.05)
        for a, b in zip(film2, q.read_film()):
            assert cases.same_bits(a, b)
    finally:
        q.close()


def hierarchy_renderer(bundle, params):
    """a context behind the hierarchy whatever the scene's size (DRT_FORCE_BVH is read when the context is created)"""
    saved = os.environ.get("DRT_FORCE_BVH")
    os.environ["DRT_FORCE_BVH"] = "1"
    try:
        r = pydrt.Renderer(bundle, params)
    finally:
        os.environ.pop("DRT_FORCE_BVH", None)
        if saved is not None:
            os.environ["DRT_FORCE_BVH"] = saved
    assert r.stats().path_flags & pydrt.PATH_BVH
    return r


def test_behind_the_hierarchy_lanes_of_one_wave_hold_different_counts():
    """drt_feature_bvh_kernel's whole-wave loop with lanes that are done while others go on: an adaptive film's counts. Forcing the
    hierarchy changes no hit, so the rule is the LDS form's."""
    bundle, p = cases.load_case("plane_light_48")
    params = pydrt.make_params(int(p.width), int(p.height), spp=32, max_depth=int(p.max_depth), seed=int(p.seed))
    r = hierarchy_renderer(bundle, params)
    try:
        r.render_adaptive(4, 24, 4, 0.08)
        counts = r.read_sample_counts().reshape(-1)
        assert any(len(np.unique(counts[k:k + 64])) >= 2 for k in range(0, counts.size, 64))  # mixed counts in one wave
        rep = r.render_features(0)
        got = r.read_features()
    finally:
        r.close()
    assert rep["rays"] == int(counts.sum())
    assert_features(got, rep["empty_pixels"], rule(bundle, params, counts=counts), "adaptive, behind the hierarchy")


def test_behind_the_hierarchy_a_tile_that_leaves_lanes_without_a_pixel():
    """35 pixels: one wave with 29 lanes that never have a ray, and three waves with none at all"""
    bundle, _ = cases.load_case("plane_light_48")
    params = pydrt.make_params(48, 48, spp=4, max_depth=8, seed=1, x0=20, y0=9, tile_w=7, tile_h=5)
    r = hierarchy_renderer(bundle, params)
    try:
        rep = r.render_features(4)
        got = r.read_features()
    finally:
        r.close()
    want = rule(bundle, params, n_samples=4)
    assert rep["rays"] == 35 * 4
    assert_features(got, rep["empty_pixels"], want, "7 x 5 tile behind the hierarchy")
    assert (want[2] >= 0).any()


def test_a_render_goes_on_as_if_the_features_had_not_run():
    bundle, p = cases.load_case("lens")
    params = pydrt.make_params(int(p.width), int(p.height), spp=6, max_depth=int(p.max_depth), seed=int(p.seed))
    r = pydrt.Renderer(bundle, params)
    try:
        r.render(0, 3)
        r.render_features(0)
        got = r.read_features()
        r.render(3, 3)
        film = r.read_film()
        stats = cases.stat_counts(r.stats())
        r.render_features(2)  # (a count of its own does not depend on the film: still readable after a render)
        fixed = r.read_features()
        r.render(6, 1)
        assert cases.same_bits(r.read_features()[0], fixed[0])
    finally:
        r.close()
    assert_features(got, int((got[0][:, 4] == 0.0).sum()), rule(bundle, params, n_samples=3, key="lens"), "between two renders")
    q = pydrt.Renderer(bundle, params)
    try:
        q.render(0, 6)
        for a, b in zip(film, q.read_film()):
            assert cases.same_bits(a, b)
        assert cases.stat_counts(q.stats()) == stats
    finally:
        q.close()


def test_the_group_form_gives_the_sessions_bits_for_any_device_list():
    bundle, params = cases.load_case("lights")
    spp = int(params.spp)
    want = rule(bundle, params, n_samples=spp, key="lights")
    for devices in ([0], [0, 0], [0, 0, 0]):
        g = pydrt.Group(bundle, params, devices)
        try:
            mean, m2, ids, rep = g.render_features(spp)
            assert_features((mean, m2, ids), rep["empty_pixels"], want, "group %s" % devices)
            assert rep["rays"] == g.n_pixels * spp and rep["kernel_ms"] > 0.0
            # counts from the devices' films: a uniform render, then every pixel at 3
            g.render(0, 3)
            film = g.read_film()
            mean, m2, ids, rep = g.render_features(0)
            assert_features((mean, m2, ids), rep["empty_pixels"], rule(bundle, params, n_samples=3, key="lights3"), "group %s from the film" % devices)
            for a, b in zip(film, g.read_film()):
                assert cases.same_bits(a, b)
        finally:
            g.close()
    g = pydrt.Group(bundle, params, [0, 0])
    try:
        with pytest.raises(RuntimeError, match="holds the filter sum 0"):  # every device checks its film before any device renders
            g.render_features(0)
    finally:
        g.close()


def test_the_bytes_are_the_rules_mapping():
    bundle, params = cases.load_case("lights")
    spp = int(params.spp)
    mean = rule(bundle, params, n_samples=spp, key="lights")[0]
    hit = mean[:, 4] > 0.0
    zlo, zhi = float(mean[hit, 3].min()), float(mean[hit, 3].max())
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_features(spp)
        for which, lo, hi in [(pydrt.FEATURE_NORMAL, -1.0, 1.0), (pydrt.FEATURE_DEPTH, zlo, zhi), (pydrt.FEATURE_COVERAGE, 0.0, 1.0),
                              (pydrt.FEATURE_DEPTH, zlo + 0.25 * (zhi - zlo), zhi - 0.25 * (zhi - zlo)),  # clamps on both sides
                              (pydrt.FEATURE_NORMAL, -0.25, 0.25), (pydrt.FEATURE_COVERAGE, 0.25, 0.5)]:
            got = r.read_feature_bgra(which, lo, hi)
            want = F.feature_bgra(mean, which, lo, hi)
            assert np.array_equal(got, want), "which %d [%g, %g]: %d bytes differ" % (which, lo, hi, int((got != want).sum()))
            assert np.all(got[:, 3] == 255)
            assert lo in (-0.25, 0.25) or len(np.unique(got[:, 0:3])) > 2  # (the whole ranges give pictures)
        clamped = r.read_feature_bgra(pydrt.FEATURE_DEPTH, zlo + 0.25 * (zhi - zlo), zhi - 0.25 * (zhi - zlo))[hit, 0]
        assert (clamped == 0).any() and (clamped == 255).any() and ((clamped > 0) & (clamped < 255)).any()
    finally:
        r.close()


def test_refusals_each_with_its_message():
    bundle, p = cases.load_case("plane_light_16")
    w, h = int(p.width), int(p.height)

    def ctx(**kw):
        return pydrt.Renderer(bundle, pydrt.make_params(w, h, spp=4, max_depth=4, **kw))

    r = ctx(mode=pydrt.MODE_XYZ)
    try:
        r.render()
        with pytest.raises(RuntimeError, match="DRT_MODE_XYZ keeps none"):
            r.render_features(0)
        r.render_features(2)  # with a count of its own it works in both modes
        xyz_mean = r.read_features()[0]
    finally:
        r.close()
    assert cases.same_bits(xyz_mean, rule(bundle, pydrt.make_params(w, h, spp=4, max_depth=4), n_samples=2)[0])
    r = ctx()
    try:
        with pytest.raises(RuntimeError, match="no feature buffers: drt_render_features first"):
            r.read_features()
        with pytest.raises(RuntimeError, match="no feature buffers: drt_render_features first"):
            r.read_feature_bgra(0, -1.0, 1.0)
        with pytest.raises(RuntimeError, match=r"tile pixel 0 \(column 0, row 0 of the tile\) holds the filter sum 0"):
            r.render_features(0)  # an empty film
        with pytest.raises(RuntimeError, match=r"flags = 4: 0 \(reserved\)"):
            r.render_features(2, flags=4)
        with pytest.raises(RuntimeError, match="sample numbers are 32 bits"):
            r.render_features(2, first_sample=0xFFFFFFFF)
        with pytest.raises(RuntimeError, match="no feature buffers"):  # a refused call has done nothing
            r.read_features()
        r.render()
        px, av, va = r.read_film()
        r.render_features(0)
        r.read_features()
        for lo, hi in [(1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf"))]:
            with pytest.raises(RuntimeError, match="finite numbers, lo below hi"):
                r.read_feature_bgra(1, lo, hi)
        with pytest.raises(RuntimeError, match="which = 3"):
            r.read_feature_bgra(3, 0.0, 1.0)
        r.reset_film()
        px[w + 2, -1] = 2.5
        r.write_film(px, av, va)
        with pytest.raises(RuntimeError, match=r"tile pixel %d \(column 2, row 1 of the tile\) holds the filter sum 2.5" % (w + 2)):
            r.render_features(0)
        for a, b in zip((px, av, va), r.read_film()):
            assert cases.same_bits(a, b)
        for change in (lambda: r.render(4, 2), lambda: r.write_film(px, av, va), lambda: r.reset_film()):
            r.reset_film()
            r.render(0, 2)
            r.render_features(0)
            r.read_features()
            change()
            with pytest.raises(RuntimeError, match="the film has changed since drt_render_features"):
                r.read_features()
    finally:
        r.close()


def test_drt_render_program_with_the_features(tmp_path):
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
        full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_FEATURES") and not k.startswith("DRT_DENOISE")}
        full.update(env)
        r = subprocess.run([exe], cwd=d, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        return d / "output", r.stdout

    plain, _ = run("plain")
    out, text = run("features", DRT_FEATURES="1", DRT_FEATURES_M2_SPD="output/fm2.spd", DRT_DEVICES="0,0")
    assert "Features: %d camera rays" % (48 * 32 * 8) in text
    standard = ("output.spd", "average.spd", "variance.spd", "output.bmp", "average.bmp", "variance.bmp")
    for f in standard:
        assert open(plain / f, "rb").read() == open(out / f, "rb").read(), f
    extra = ["output.spd.features.spd", "fm2.spd", "output.spd.normal.bmp", "output.spd.depth.bmp", "output.spd.coverage.bmp"]
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain) + extra)  # and no temporary file is left
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 48, 32)
    params = pydrt.make_params(48, 32, spp=8, max_depth=6, seed=1)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        r.render_features(0)
        mean, m2, _ = r.read_features()
        hit = mean[:, 4] > 0.0
        zlo, zhi = float(mean[hit, 3].min()), float(mean[hit, 3].max())
        pictures = {"normal": r.read_feature_bgra(0, -1.0, 1.0), "depth": r.read_feature_bgra(1, zlo, zhi), "coverage": r.read_feature_bgra(2, 0.0, 1.0)}
    finally:
        r.close()
    head = bytearray(open(out / "average.spd", "rb").read()[:40])
    for f, want in (("output.spd.features.spd", mean), ("fm2.spd", m2)):
        got_head = open(out / f, "rb").read()[:40]
        S_at = bytes(head).index(np.uint32(69).tobytes(), 4)
        assert got_head[:S_at] == bytes(head[:S_at]) and got_head[S_at:S_at + 4] == np.uint32(8).tobytes() and got_head[S_at + 4:] == bytes(head[S_at + 4:]), f
        got = np.fromfile(out / f, dtype=np.float64, offset=40).reshape(-1, 8)
        assert cases.same_bits(got, want), "%s: %s" % (f, cases.first_difference(got, want))
    for name, want in pictures.items():
        data = open(out / ("output.spd.%s.bmp" % name), "rb").read()
        assert data[:54] == open(out / "output.bmp", "rb").read()[:54]
        assert np.array_equal(np.frombuffer(data[54:], dtype=np.uint8).reshape(-1, 4), want), name
        assert name == "coverage" or len(np.unique(want[:, 0:3])) > 2
