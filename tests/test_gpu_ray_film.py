"""GPU (-m gpu): ray films (drt_bind_rays, its group form, pydrt's bind_rays, the drt_render program's DRT_PROJECTION; DESIGN.md
section 5f). The ground truth is tests/ray_film_cases.py's: a table filled with the rays of a pinhole camera under the centre scheme
must give that camera's film -- the device's own camera render and the oracle's -- bit for bit, and tables stitched from several
cameras, by rows or by layers, must give each camera's part. tests/test_ray_film_cpu.py holds the premises. Every film comparison
is cases.same_bits on all three buffers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import pydrt
import ray_film_cases as R

pytestmark = pytest.mark.gpu

_cache = {}


def assert_same_film(got, want, what):
    for name, a, b in zip(("pixels", "avgs", "vars"), got, want):
        assert cases.same_bits(a, b), "%s %s: %s" % (what, name, cases.first_difference(a, b))


def render(bundle, params, table=None, hits=False, first_sample=None, num_samples=None):
    """one context, one drt_render call: (film, hit log or None, stats); table = (origins, dirs[, weights]) binds it first"""
    r = pydrt.Renderer(bundle, params)
    try:
        if table is not None:
            r.bind_rays(*table)
        r.render(first_sample, num_samples)
        film = r.read_film()
        log = r.read_hit_indices(int(params.spp) if num_samples is None else num_samples) if hits else None
        return film, log, r.stats()
    finally:
        r.close()


def parity_ray_film(name):
    """the ray film of a camera-parity case's own table (film, hit log, stats), rendered once"""
    if name not in _cache:
        bundle, p = R.load(name)
        _cache[name] = render(bundle, p, R.camera_table(name), hits=True)
    return _cache[name]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", R.CAMERA_PARITY)
def test_a_table_of_the_cameras_rays_gives_the_cameras_film(name):
    bundle, p = R.load(name)
    assert (int(p.spp), int(p.batch_spp)) == (5, 2) and int(p.flags) & pydrt.FLAG_RECORD_HITS
    film, log, st = parity_ray_film(name)
    cam_film, cam_log, cam_st = render(bundle, p, hits=True)
    assert st.path_flags & pydrt.PATH_RAYS and not cam_st.path_flags & pydrt.PATH_RAYS
    assert st.path_flags & ~pydrt.PATH_RAYS == cam_st.path_flags  # the same kernel family
    assert bool(st.path_flags & pydrt.PATH_BVH) == (name == "spheres_1500")
    assert_same_film(film, cam_film, name + " against the camera render")
    assert np.array_equal(log, cam_log)
    assert cases.stat_counts(st) == cases.stat_counts(cam_st)
    opx, oav, ova, olog, ost = cases.oracle_render_device_pow(bundle, p, want_hits=True)
    assert_same_film(film, (opx, oav, ova), name + " against the oracle")
    assert np.array_equal(log, olog)
    assert cases.stat_counts(st) == cases.stat_counts(ost)
    assert st.rng_draws == ost.rng_draws and np.any(opx[:, :-1] != 0.0)


# ------------------------------------------------------------------------------------------------ 1b
def test_rows_with_directions_that_are_not_of_unit_length_against_the_oracle():
    """A context scanned out of LDS takes the table's directions as given: with those of alternate rows multiplied by 2 and by 0.5 the
    film, the hit log and the counts are the oracle's, rendering from the same table, bit for bit (and not the camera's film)."""
    import oracle_py as O
    name = R.SCALED_ROWS
    bundle, p = R.load(name)
    table = R.scaled_rows()
    film, log, st = render(bundle, p, table, hits=True)
    assert st.path_flags & pydrt.PATH_RAYS and not st.path_flags & pydrt.PATH_BVH
    with O.ray_table(*table):
        opx, oav, ova, olog, ost = cases.oracle_render_device_pow(bundle, p, want_hits=True)
    assert_same_film(film, (opx, oav, ova), name + " scaled rows against the oracle")
    assert np.array_equal(log, olog)
    assert cases.stat_counts(st) == cases.stat_counts(ost)
    assert not cases.same_bits(film[0], parity_ray_film(name)[0][0])


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("scene", R.STITCH_SCENES)
def test_rows_stitched_from_three_cameras_give_each_cameras_tile(scene):
    st = R.stitch(scene)
    film, _, stats = render(st["bundle"], st["params"], st["table"])
    assert bool(stats.path_flags & pydrt.PATH_BVH) == (scene == "spheres_1500")
    W, ROWS = R.STITCH_W, R.STITCH_ROWS
    for k, (b, tp) in enumerate(zip(st["cameras"], st["tile_params"])):
        want = cases.oracle_render_device_pow(b, tp)[:3]
        got = [a[ROWS * k * W:ROWS * (k + 1) * W] for a in film]
        assert_same_film(got, want, "%s rows %d..%d" % (scene, ROWS * k, ROWS * k + ROWS - 1))


# ------------------------------------------------------------------------------------------------ 3
def test_layers_take_the_ray_of_sample_modulo_layers():
    ly = R.layers()
    want = R.render_by_samples(lambda b, q, film: cases.oracle_render_device_pow(b, q, film=film), ly["cameras"], ly["params"])
    film, _, _ = render(ly["bundle"], ly["params"], ly["table"])
    assert_same_film(film, want, "two layers")
    # and the two cameras really differ: one layer alone gives another film
    alone, _, _ = render(ly["bundle"], ly["params"], tuple(a[0] for a in ly["table"]))
    assert not cases.same_bits(alone[0], film[0])
    # more layers than samples: layers 0 .. 4 of eight are read, camera s % 2 each
    eight = tuple(np.ascontiguousarray(np.concatenate([a] * 4)) for a in ly["table"])
    assert eight[0].shape[0] == 8 > int(ly["params"].spp)
    film8, _, _ = render(ly["bundle"], ly["params"], eight)
    assert_same_film(film8, want, "eight layers")
    # a render in two calls reads the layer of the ABSOLUTE sample index
    r = pydrt.Renderer(ly["bundle"], ly["params"])
    try:
        r.bind_rays(*ly["table"])
        r.render(0, 3)
        r.render(3, 2)
        assert_same_film(r.read_film(), want, "two calls")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 4
def test_weights():
    name = "lights"
    bundle, p = R.load(name)
    o, d, w = R.camera_table(name)
    base = parity_ray_film(name)[0]
    none, _, _ = render(bundle, p, (o, d))
    ones, _, _ = render(bundle, p, (o, d, np.ones_like(w)))
    assert_same_film(none, ones, "weights = NULL against all ones")
    assert not cases.same_bits(none[0], base[0])  # (the camera's vignette is not 1)
    twos, _, _ = render(bundle, p, (o, d, np.full_like(w, 2.0)))
    px, av, va = ones
    want_px = px.copy()
    want_px[:, :-1] *= 2.0  # the filter column counts samples
    assert_same_film(twos, (want_px, av * 2.0, va * 4.0), "weights of 2")
    assert np.any(va != 0.0)


def test_a_nan_direction_misses_and_a_nan_weight_poisons_its_own_pixel():
    name = "first_scene"  # open: most camera rays escape
    bundle, p = R.load(name)
    o, d, w = R.camera_table(name)
    base, log, _ = parity_ray_film(name)
    W = int(p.width)
    first = log[:, 0].reshape(int(p.spp), -1)
    escaping = np.flatnonzero((first == -1).all(axis=0))
    hitting = np.flatnonzero((first >= 0).all(axis=0) & (base[0][:, :-1] != 0.0).any(axis=1))
    assert len(escaping) and len(hitting)
    q, t = int(escaping[0]), int(hitting[len(hitting) // 2])
    # pixel t gets a NaN direction in one table and pixel q's escaping ray in the other
    nan_d, esc_o, esc_d, esc_w = d.copy(), o.copy(), d.copy(), w.copy()
    nan_d[t // W, t % W] = np.nan
    esc_o[t // W, t % W], esc_d[t // W, t % W], esc_w[t // W, t % W] = o[q // W, q % W], d[q // W, q % W], w[q // W, q % W]
    f_nan, log_nan, _ = render(bundle, p, (o, nan_d, w), hits=True)
    f_esc, _, _ = render(bundle, p, (esc_o, esc_d, esc_w))
    assert_same_film(f_nan, f_esc, "a NaN direction against an escaping ray")
    assert np.all(log_nan[:, 0].reshape(int(p.spp), -1)[:, t] == -1)
    others = np.arange(base[0].shape[0]) != t
    assert_same_film([a[others] for a in f_nan], [a[others] for a in base], "the other pixels")
    assert not cases.same_bits(f_nan[0][t], base[0][t])
    # a NaN weight: its pixel is NaN in every wavelength of all three buffers, the sample count and every other pixel are untouched
    nan_w = w.copy()
    nan_w[t // W, t % W] = np.nan
    f_w, _, _ = render(bundle, p, (o, d, nan_w))
    assert np.isnan(f_w[0][t, :-1]).all() and np.isnan(f_w[1][t]).all() and np.isnan(f_w[2][t]).all()
    assert f_w[0][t, -1] == base[0][t, -1]
    assert_same_film([a[others] for a in f_w], [a[others] for a in base], "the other pixels")


# ------------------------------------------------------------------------------------------------ 5
TILE = dict(x0=3, y0=2, tile_w=20, tile_h=11, row_stride=2)  # rows 2, 4 .. 22 of 32, columns 3 .. 22


def tile_of(film, p):
    W = int(p.width)
    x, y = np.meshgrid(TILE["x0"] + np.arange(TILE["tile_w"]), TILE["y0"] + np.arange(TILE["tile_h"]) * TILE["row_stride"])
    idx = (y * W + x).reshape(-1)
    return [a[idx] for a in film]


@pytest.mark.parametrize("name", ["lights", "spheres_1500"])
def test_a_tile_takes_its_own_rows_of_the_whole_image_table(name):
    bundle, p = R.load(name)
    full = parity_ray_film(name)[0]
    film, _, _ = render(bundle, R.params_like(p, flags=0, **TILE), R.camera_table(name))
    assert_same_film(film, tile_of(full, p), name + " tile")


@pytest.mark.parametrize("scene", ["cornell_plane_light.scn", "@spheres:1500"])
def test_a_tall_tile_rendered_in_row_blocks_reads_its_own_rows(scene):
    """64 rows, 5 samples where a kernel pair takes 2 and no hit log: drt_render goes over the tile in row blocks, each launch numbering
    its pixels from its own first row (the launcher's row-block rule; the table's entries are numbered in the whole tile)."""
    W, H = 16, 64
    bundle = pydrt.synthetic_sphere_scene(1500, W, H) if scene.startswith("@") else pydrt.load_scene(cases.scene_path(scene), W, H)
    bundle.camera.aperture_radius = 0.0
    p = pydrt.make_params(W, H, spp=R.PARITY_SPP, max_depth=4, seed=3, pixel_scheme=pydrt.FILM_SAMPLE_CENTER, batch_spp=R.PARITY_BATCH)
    table = R.centre_rays(bundle, W, H)
    film, _, st = render(bundle, p, table)
    cam, _, cam_st = render(bundle, p)
    assert st.launches > 3 and st.launches == cam_st.launches  # more kernel pairs than 5 samples in twos: the blocks
    assert_same_film(film, cam, scene + " against the camera render")
    assert_same_film(film, cases.oracle_render_device_pow(bundle, p)[:3], scene + " against the oracle")
    # the same through a tile with a column offset and a row stride
    q = R.params_like(p, x0=3, tile_w=11, y0=1, tile_h=32, row_stride=2)
    x, y = np.meshgrid(3 + np.arange(11), 1 + np.arange(32) * 2)
    idx = (y * W + x).reshape(-1)
    assert_same_film(render(bundle, q, table)[0], [a[idx] for a in film], scene + " tile")


@pytest.mark.parametrize("name", ["lights", "spheres_1500"])
def test_a_group_gives_the_single_contexts_film(name):
    bundle, p = R.load(name)
    full = parity_ray_film(name)[0]
    for devices in ([0, 0], [0, 0, 0]):
        g = pydrt.Group(bundle, R.params_like(p, flags=0), devices=devices)
        try:
            g.bind_rays(*R.camera_table(name))
            assert g.stats().path_flags & pydrt.PATH_RAYS
            g.render()
            assert_same_film(g.read_film(), full, "%s group %s" % (name, devices))
            with pytest.raises(RuntimeError, match="film holds samples"):
                g.bind_rays(None)
            with pytest.raises(RuntimeError, match="camera's rays"):
                g.cast_pixels(np.array([[0, 0]]), np.array([0]))
            with pytest.raises(RuntimeError, match="camera's rays"):
                g.render_features(2)
            with pytest.raises(RuntimeError, match="camera's rays"):
                g.render_mattes(2)
            assert_same_film(g.read_film(), full, "after the refusals")
        finally:
            g.close()
    g = pydrt.Group(bundle, R.params_like(p, flags=0), devices=[0, 0])
    try:
        o, d, w = R.camera_table(name)
        t = pydrt.RayTable()
        t.origins, t.dirs, t.n_layers, t.flags = o.ctypes.data, d.ctypes.data, 1, pydrt.RAYS_DEVICE
        assert g.L.drt_group_bind_rays(g.g, C.byref(t)) != 0 and "host pointers only" in g.L.drt_last_error().decode()
        assert not g.stats().path_flags & pydrt.PATH_RAYS
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("name", ["lights", "spheres_1500"])
def test_device_mode_gives_host_modes_bits(name):
    torch = pytest.importorskip("torch")
    bundle, p = R.load(name)
    full = parity_ray_film(name)[0]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    for params, want in ((p, full), (R.params_like(p, flags=0, **TILE), tile_of(full, p))):
        r = pydrt.Renderer(bundle, params)
        try:
            with torch.cuda.stream(stream):
                r.set_stream(stream.cuda_stream)
                table = tuple(torch.from_numpy(np.array(a)).to(dev).contiguous() for a in R.camera_table(name))
                stream.synchronize()
                r.bind_rays(*table)
                del table  # the context keeps the tensors referenced
                assert r.stats().path_flags & pydrt.PATH_RAYS
                r.render()
                assert_same_film(r.read_film(), want, name + " device mode")
            with pytest.raises(ValueError):
                r.bind_rays(torch.zeros((4, 4, 3), dtype=torch.float64, device=dev), torch.zeros((4, 4, 3), dtype=torch.float64, device=dev))
        finally:
            r.close()


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("name", ["plane_light_center", "spheres_1500"])
def test_adaptive_rendering_and_continuing_equal_the_camera_modes(name):
    bundle, p = R.load(name)
    q = R.params_like(p, spp=32, flags=0, batch_spp=0)
    out = []
    for table in (None, R.camera_table(name)):
        r = pydrt.Renderer(bundle, q)
        try:
            if table is not None:
                r.bind_rays(*table)
            rep = r.render_adaptive(4, 24, 4, 0.08)
            first = (r.read_film(), r.read_sample_counts(), rep)
            cont = r.render_adaptive_continue(32, 4, 0.05)
            out.append(first + (r.read_film(), r.read_sample_counts(), cont))
        finally:
            r.close()
    cam, ray = out
    assert_same_film(ray[0], cam[0], name + " adaptive")
    assert np.array_equal(ray[1], cam[1]) and ray[2] == cam[2]
    assert_same_film(ray[3], cam[3], name + " continued")
    assert np.array_equal(ray[4], cam[4]) and ray[5] == cam[5]
    # the rounds did something: pixels stopped at different counts, and the continuation went on
    assert len(np.unique(cam[1])) > 1 and cam[2]["rounds"] > 1 and cam[5]["paths"] > 0


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("name", ["lights", "spheres_1500"])
def test_the_xyz_film_equals_the_camera_modes(name):
    bundle, p = R.load(name)
    q = R.params_like(p, flags=0, mode=pydrt.MODE_XYZ)
    out = []
    for table in (None, R.camera_table(name)):
        r = pydrt.Renderer(bundle, q)
        try:
            if table is not None:
                r.bind_rays(*table)
            r.render()
            out.append((r.read_xyz_film(), r.read_xyz()))
        finally:
            r.close()
    assert cases.same_bits(out[0][0], out[1][0]), cases.first_difference(out[1][0], out[0][0])
    assert cases.same_bits(out[0][1], out[1][1]) and np.any(out[0][1] != 0.0)


# ------------------------------------------------------------------------------------------------ 9
def test_binding_state_and_refusals():
    name = "lights"
    bundle, p = R.load(name)
    o, d, w = R.camera_table(name)
    fresh, _, _ = render(bundle, p)
    r = pydrt.Renderer(bundle, p)
    L, err = r.L, lambda: r.L.drt_last_error().decode()
    try:
        assert not r.stats().path_flags & pydrt.PATH_RAYS
        # refused with nothing done
        t = pydrt.RayTable()
        t.origins, t.dirs, t.weights, t.n_layers, t.flags = o.ctypes.data, d.ctypes.data, None, 1, 0
        for field, value, word in (("origins", None, "origins"), ("dirs", None, "dirs"), ("n_layers", 0, "n_layers"), ("flags", 2, "flags"), ("flags", 5, "flags")):
            bad = pydrt.RayTable()
            C.memmove(C.byref(bad), C.byref(t), C.sizeof(t))
            setattr(bad, field, value)
            assert L.drt_bind_rays(r.ctx, C.byref(bad)) != 0 and word in err(), (field, err())
            assert not r.stats().path_flags & pydrt.PATH_RAYS
        assert L.drt_bind_rays(None, C.byref(t)) != 0 and "ctx" in err()
        # onto a film with samples: refused, the film unchanged, the camera still in use
        r.render(0, 2)
        before = r.read_film()
        with pytest.raises(RuntimeError, match="film holds samples"):
            r.bind_rays(o, d, w)
        assert not r.stats().path_flags & pydrt.PATH_RAYS
        assert_same_film(r.read_film(), before, "after the refused binding")
        r.render(2, 3)
        assert_same_film(r.read_film(), fresh, "the camera render, continued")
        # after a reset: bound, and the camera's calls are refused while cast_rays and test_visibility work
        r.reset_film()
        r.bind_rays(o, d, w)
        assert r.stats().path_flags & pydrt.PATH_RAYS
        for call in (lambda: r.render_features(2), lambda: r.render_mattes(2), lambda: r.cast_pixels(np.array([[1, 2]]), np.array([0]))):
            with pytest.raises(RuntimeError, match="camera's rays"):
                call()
        ro, rd = o.reshape(-1, 3)[:100], d.reshape(-1, 3)[:100]
        hits = r.cast_rays(ro, rd)
        vis = r.test_visibility(ro, ro + rd)
        r.render()
        assert np.array_equal(hits["index"], r.read_hit_indices(int(p.spp))[:100, 0])  # (sample 0's rows come first)
        assert vis.shape == (100,)
        assert_same_film(r.read_film(), parity_ray_film(name)[0], "bound after a reset")
        # unbinding needs an empty film too
        with pytest.raises(RuntimeError, match="film holds samples"):
            r.bind_rays(None)
        assert r.stats().path_flags & pydrt.PATH_RAYS
        r.reset_film()
        r.bind_rays(None)
        assert not r.stats().path_flags & pydrt.PATH_RAYS
        r.render()
        assert_same_film(r.read_film(), fresh, "the camera again")
        assert r.render_features(2)["rays"] > 0  # and its calls work again
        # a written film counts as samples
        r.reset_film()
        r.write_film(*fresh)
        with pytest.raises(RuntimeError, match="film holds samples"):
            r.bind_rays(o, d, w)
    finally:
        r.close()
    # behind the hierarchy, host mode: a table with a finite, nonzero direction that is not of unit length is refused, the first such
    # layer and pixel named, nothing changed -- no film bit included; zero, NaN and infinite directions are taken
    name = "spheres_1500"
    bundle, p = R.load(name)
    o, d, w = R.camera_table(name)
    H, W = d.shape[:2]
    two = (np.stack([o, o]), np.stack([d, d]), np.stack([w, w]))
    fresh, _, st = render(bundle, p)
    assert st.path_flags & pydrt.PATH_BVH
    r = pydrt.Renderer(bundle, p)
    g = pydrt.Group(bundle, R.params_like(p, flags=0), devices=[0, 0])
    try:
        for layer, y, x, factor in ((0, 2, 3, 2.0), (1, H - 1, W - 1, 0.5), (1, 5, 0, 1.0 + 2.0 ** -40), (0, 0, 1, 1e-3)):
            bad = two[1].copy()
            bad[layer, y, x] *= factor
            bad[1, H - 1, W - 1] *= 3.0  # a later one, or the same: the FIRST is named
            for who in (r, g):
                with pytest.raises(RuntimeError, match=r"layer %d, pixel \(%d, %d\).*unit length" % (layer, x, y)):
                    who.bind_rays(two[0], bad, two[2])
                assert not who.stats().path_flags & pydrt.PATH_RAYS
        r.render()
        assert_same_film(r.read_film(), fresh, "the camera's film after the refused bindings")
        r.reset_film()
        odd = two[1].copy()
        odd[0, 0, 0] = 0.0
        odd[0, 1, 1] = np.nan
        odd[1, 2, 2, 0] = np.inf
        odd[1, 3, 3] *= 1.0 + 2.0 ** -44  # inside the tolerance
        r.bind_rays(two[0], odd, two[2])
        assert r.stats().path_flags & pydrt.PATH_RAYS
        g.bind_rays(two[0], odd, two[2])
        assert g.stats().path_flags & pydrt.PATH_RAYS
    finally:
        r.close()
        g.close()
    # out of LDS any direction is taken (test_rows_with_directions_that_are_not_of_unit_length_against_the_oracle renders it)
    bundle, p = R.load(R.SCALED_ROWS)
    r = pydrt.Renderer(bundle, p)
    try:
        r.bind_rays(*R.scaled_rows())
        assert r.stats().path_flags & pydrt.PATH_RAYS and not r.stats().path_flags & pydrt.PATH_BVH
    finally:
        r.close()
    name = "lights"
    bundle, p = R.load(name)
    o, d, w = R.camera_table(name)
    # shapes pydrt refuses before the C call
    r = pydrt.Renderer(bundle, p)
    try:
        for bad in ((o[:-1], d[:-1], None), (o, d[..., :2], None), (o, d, w[:-1]), (o[None, None], d[None, None], None)):
            with pytest.raises(ValueError):
                r.bind_rays(*bad)
        r.bind_rays(o[None], d[None], w[None])  # [1][h][w][3] is the one-layer form
        r.render()
        assert_same_film(r.read_film(), parity_ray_film(name)[0], "[1][h][w][3]")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 10
def test_drt_render_program_with_an_equirectangular_projection(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    W, H, SPP, DEPTH = 32, 16, 2, 3
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("num_pixel_samples 4", "num_pixel_samples %d" % SPP).replace("max_cast_depth    4", "max_cast_depth    %d" % DEPTH)
    cfg = cfg.replace("output_width      800", "output_width      %d" % W).replace("output_height     600", "output_height     %d" % H)
    assert "output_width      32" in cfg and "output_height     16" in cfg and "num_pixel_samples 2" in cfg and "max_cast_depth    3" in cfg

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
        return d / "output"

    out = run("equirect", DRT_PROJECTION="equirect")
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, H)
    p = pydrt.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=1)
    (px, av, va), _, _ = render(bundle, p, pydrt.equirect_rays(bundle, W, H))
    S = bundle.S
    hdr = np.fromfile(out / "output.spd", dtype=np.uint32, count=5)
    assert list(hdr[1:5]) == [W, H, S, 1]
    fpx = np.fromfile(out / "output.spd", dtype=np.float64, offset=40).reshape(-1, S + 1)
    fav = np.fromfile(out / "average.spd", dtype=np.float64, offset=40).reshape(-1, S)
    fva = np.fromfile(out / "variance.spd", dtype=np.float64, offset=40).reshape(-1, S)
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = va / np.max(np.maximum(va, 0.0), axis=1)[:, None]  # written max-normalised per pixel (host/drt_checkpoint.c)
    assert_same_film((fpx, fav, fva), (px, av, norm), "the program's files")
    assert np.all(fpx[:, -1] == SPP) and np.any(fpx[:, :-1] != 0.0)
    # another projection is another picture; two devices give the same files
    plain = run("plain")
    assert open(plain / "output.spd", "rb").read() != open(out / "output.spd", "rb").read()
    two = run("two", DRT_PROJECTION="equirect", DRT_DEVICES="0,0")
    for f in ("output.spd", "average.spd", "variance.spd"):
        assert open(two / f, "rb").read() == open(out / f, "rb").read(), f
