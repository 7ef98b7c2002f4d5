"""GPU (-m gpu): the ID mattes (drt_render_mattes, drt_read_mattes, drt_read_matte, drt_read_matte_bgra, drt_group_render_mattes, the
drt_render program's DRT_MATTES) against the rule of tests/matte_rule.py. The rule counts in integers, so ids, counts, tail and the
launch's sums are compared with ==; the one division of drt_read_matte and the preview's + * / are IEEE operations on numbers far
from the subnormal range, so those are compared with == too."""
import os
import subprocess

import numpy as np
import pytest

import cases
import matte_rule as M
import pydrt

pytestmark = pytest.mark.gpu

CASES = ["plane_light_16", "lights", "lens", "downward", "example_scene", "spheres_8x8"]

_rule = {}


def rule(bundle, params, n_samples=None, first_sample=0, counts=None, key=None):
    """(ids, counts, tail, empty pixels, overflow pixels) by the rule, computed once per key"""
    if key is None:
        return M.mattes(bundle, params, n_samples=n_samples, first_sample=first_sample, counts=counts)
    if key not in _rule:
        _rule[key] = M.mattes(bundle, params, n_samples=n_samples, first_sample=first_sample, counts=counts)
    return _rule[key]


def assert_mattes(got, rep, want, what):
    for k, part in enumerate(("ids", "counts", "tail")):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, "%s %s" % (what, part)
        assert np.array_equal(got[k], want[k]), "%s %s: %d entries differ, first at %s" % (
            what, part, int((got[k] != want[k]).sum()), np.argwhere(got[k] != want[k])[0])
    assert rep["empty_pixels"] == want[3], "%s: %d empty pixels, the rule has %d" % (what, rep["empty_pixels"], want[3])
    assert tuple(rep["overflow_pixels"]) == tuple(want[4]), "%s: overflow %s, the rule has %s" % (what, rep["overflow_pixels"], want[4])
    assert rep["rays"] == int(want[2][:, 0].sum(dtype=np.int64)), what


def session(bundle, params, n_samples, first_sample=0):
    r = pydrt.Renderer(bundle, params)
    try:
        rep = r.render_mattes(n_samples, first_sample)
        got = r.read_mattes()
    finally:
        r.close()
    assert rep["kernel_ms"] > 0.0
    return got, rep


@pytest.mark.parametrize("name", CASES)
def test_the_device_equals_the_rule(name):
    bundle, params = M.load_case(name)
    spp = int(params.spp)
    want = rule(bundle, params, n_samples=spp, key=name)
    got, rep = session(bundle, params, spp)
    assert_mattes(got, rep, want, name)
    if name == "spheres_8x8":  # behind the hierarchy, and where both layers overflow
        assert want[4] == (8, 1) and want[3] == 6


def dense_spheres_text():
    """6 x 6 small spheres side by side in front of a narrow camera, nine materials dealt so that every 3 x 3 block has them all: at
    2 x 2 pixels every pixel looks at nine spheres of nine materials. 37 surfaces: the scene stays in LDS."""
    t = "Camera\nposition 0.0, 0.0, 7.0\ntarget 0.0, 0.0, 0.0\nroll 0.0\nfov 20.0\nfdepth 6.0\nflength 0.3\naperture 0.0\n\n"
    t += "Material\nname vacuum\nrefract constant 1.0\nbase_material\n\nMaterial\nname escape\nescape_material\n\n"
    t += "Material\nname lamp\nemission constant 1.0\nis_black_body true\n\n"
    for m in range(9):
        t += "Material\nname paint%d\ndiffuse rgb 0.%d, 0.5, 0.%d\nbdsfs bp_diffuse_bdsf\ndir_func cos_weighted_sample_hemisphere\n\n" % (m, m + 1, 9 - m)
    t += "Surface\nname lamp\ntype plane\nposition -1.0, 5.0, 1.0\npointu 1.0, 5.0, 1.0\npointv -1.0, 5.0, -1.0\nmaterial lamp\n\n"
    for i in range(6):
        for j in range(6):
            t += "Surface\nname ball_%d_%d\ntype sphere\nposition %.1f, %.1f, 0.0\nradius 0.15\nmaterial paint%d\n\n" % (
                i, j, -1.0 + 0.4 * i, -1.0 + 0.4 * j, (i % 3) * 3 + j % 3)
    return t


def test_a_scene_in_lds_whose_pixels_see_more_ids_than_slots():
    bundle = pydrt.load_scene_text(dense_spheres_text(), 2, 2)
    params = pydrt.make_params(2, 2, spp=64, max_depth=4, seed=3, pixel_scheme=pydrt.FILM_SAMPLE_RANDOM)
    assert int(bundle.scene.num_surfaces) == 37  # (the launcher keeps scenes of up to 96 surfaces in LDS)
    want = rule(bundle, params, n_samples=64)
    assert (want[2][:, 2] > 0).any() and (want[2][:, 3] > 0).any() and want[4][0] > 0 and want[4][1] > 0  # more than six of each
    assert (want[2][:, 1] > 0).any()  # and gaps between the spheres
    r = pydrt.Renderer(bundle, params)
    try:
        rep = r.render_mattes(64)
        got = r.read_mattes()
    finally:
        r.close()
    assert_mattes(got, rep, want, "dense spheres")


def test_a_tile_that_is_no_multiple_of_a_wave():
    bundle, _ = cases.load_case("plane_light_48")
    params = pydrt.make_params(48, 48, spp=4, max_depth=8, seed=1, x0=20, y0=9, tile_w=7, tile_h=5)
    want = rule(bundle, params, n_samples=4)
    got, rep = session(bundle, params, 4)
    assert_mattes(got, rep, want, "7 x 5 tile")
    assert (want[0] >= 0).any()


def test_a_row_stride_and_a_first_sample():
    bundle, p = cases.load_case("lights")
    params = pydrt.make_params(32, 32, spp=4, max_depth=6, seed=5, x0=3, y0=1, tile_w=29, tile_h=15, row_stride=2)
    got, rep = session(bundle, params, 3)
    assert_mattes(got, rep, rule(bundle, params, n_samples=3), "row_stride 2")
    bundle, params = cases.load_case("plane_light_16")
    got3, rep3 = session(bundle, params, 4, first_sample=3)
    want3 = rule(bundle, params, n_samples=4, first_sample=3)
    assert_mattes(got3, rep3, want3, "first_sample 3")
    assert not np.array_equal(want3[1], rule(bundle, params, n_samples=4, key="plane_light_16")[1])


def test_an_adaptive_film_gives_every_pixel_its_own_count():
    bundle, p = cases.load_case("plane_light_48")
    params = pydrt.make_params(int(p.width), int(p.height), spp=32, max_depth=int(p.max_depth), seed=int(p.seed))
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_adaptive(4, 24, 4, 0.08)
        counts = r.read_sample_counts()
        assert len(np.unique(counts)) >= 3 and any(len(np.unique(counts.reshape(-1)[k:k + 64])) >= 2 for k in range(0, counts.size, 64))  # mixed counts in one wave
        film = r.read_film()
        paths = r.stats().paths
        rep = r.render_mattes(0)
        got = r.read_mattes()
        assert np.array_equal(got[2][:, 0], counts.reshape(-1))
        assert_mattes(got, rep, rule(bundle, params, counts=counts.reshape(-1)), "adaptive")
        # no film bit, no count and no render state has changed
        for a, b in zip(film, r.read_film()):
            assert cases.same_bits(a, b)
        assert np.array_equal(r.read_sample_counts(), counts) and r.stats().paths == paths
        cont = r.render_adaptive_continue(32, 4, 0.05)
        assert cont["paths"] > 0
        with pytest.raises(RuntimeError, match="the film has changed since drt_render_mattes"):
            r.read_mattes()
    finally:
        r.close()


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
    """drt_matte_bvh_kernel's whole-wave loop with lanes that are done while others go on: an adaptive film's counts. Forcing the
    hierarchy changes no hit, so the rule is the LDS form's."""
    bundle, p = cases.load_case("plane_light_48")
    params = pydrt.make_params(int(p.width), int(p.height), spp=32, max_depth=int(p.max_depth), seed=int(p.seed))
    r = hierarchy_renderer(bundle, params)
    try:
        r.render_adaptive(4, 24, 4, 0.08)
        counts = r.read_sample_counts().reshape(-1)
        assert any(len(np.unique(counts[k:k + 64])) >= 2 for k in range(0, counts.size, 64))  # mixed counts in one wave
        rep = r.render_mattes(0)
        got = r.read_mattes()
    finally:
        r.close()
    assert np.array_equal(got[2][:, 0], counts)
    assert_mattes(got, rep, rule(bundle, params, counts=counts), "adaptive, behind the hierarchy")


def test_behind_the_hierarchy_a_tile_that_leaves_lanes_without_a_pixel():
    """35 pixels: one wave with 29 lanes that never have a ray, and three waves with none at all"""
    bundle, _ = cases.load_case("plane_light_48")
    params = pydrt.make_params(48, 48, spp=4, max_depth=8, seed=1, x0=20, y0=9, tile_w=7, tile_h=5)
    want = rule(bundle, params, n_samples=4)
    r = hierarchy_renderer(bundle, params)
    try:
        rep = r.render_mattes(4)
        got = r.read_mattes()
    finally:
        r.close()
    assert_mattes(got, rep, want, "7 x 5 tile behind the hierarchy")
    assert (want[0] >= 0).any()


def test_a_render_goes_on_as_if_the_mattes_had_not_run():
    bundle, p = cases.load_case("lens")
    params = pydrt.make_params(int(p.width), int(p.height), spp=6, max_depth=int(p.max_depth), seed=int(p.seed))
    r = pydrt.Renderer(bundle, params)
    try:
        r.render(0, 3)
        r.render_features(0)
        features = r.read_features()
        rep = r.render_mattes(0)
        got = r.read_mattes()
        for a, b in zip(features, r.read_features()):  # the feature buffers taken before: still readable, unchanged
            assert cases.same_bits(a, b)
        r.render(3, 3)
        film = r.read_film()
        stats = cases.stat_counts(r.stats())
        r.render_mattes(2)  # (a count of its own does not depend on the film: still readable after a render)
        fixed = r.read_mattes()
        r.render(6, 1)
        assert np.array_equal(r.read_mattes()[1], fixed[1])
    finally:
        r.close()
    assert_mattes(got, rep, rule(bundle, params, n_samples=3, key="lens"), "between two renders")
    q = pydrt.Renderer(bundle, params)
    try:
        q.render(0, 6)
        for a, b in zip(film, q.read_film()):
            assert cases.same_bits(a, b)
        assert cases.stat_counts(q.stats()) == stats
    finally:
        q.close()


def test_the_group_form_gives_the_sessions_arrays_for_any_device_list():
    bundle, params = cases.load_case("lights")
    spp = int(params.spp)
    want = rule(bundle, params, n_samples=spp, key="lights")
    for devices in ([0], [0, 0], [0, 0, 0]):
        g = pydrt.Group(bundle, params, devices)
        try:
            ids, counts, tail, rep = g.render_mattes(spp)
            assert_mattes((ids, counts, tail), rep, want, "group %s" % devices)
            assert rep["kernel_ms"] > 0.0
            # counts from the devices' films: a uniform render, then every pixel at 3
            g.render(0, 3)
            film = g.read_film()
            ids, counts, tail, rep = g.render_mattes(0)
            assert_mattes((ids, counts, tail), rep, rule(bundle, params, n_samples=3, key="lights3"), "group %s from the film" % devices)
            for a, b in zip(film, g.read_film()):
                assert cases.same_bits(a, b)
        finally:
            g.close()
    g = pydrt.Group(bundle, params, [0, 0])
    try:
        with pytest.raises(RuntimeError, match="mattes: tile pixel 0 .* holds the filter sum 0"):  # every device is checked before any renders
            g.render_mattes(0)
    finally:
        g.close()
    bundle, params = M.load_case("spheres_8x8")  # the sums over devices, where every one of them is nonzero
    g = pydrt.Group(bundle, params, [0, 0, 0])
    try:
        ids, counts, tail, rep = g.render_mattes(48)
        assert_mattes((ids, counts, tail), rep, rule(bundle, params, n_samples=48, key="spheres_8x8"), "group of 3, spheres")
    finally:
        g.close()


def test_one_matte_and_the_preview_bytes():
    bundle, params = cases.load_case("lights")
    spp = int(params.spp)
    ids, counts, tail, _, _ = rule(bundle, params, n_samples=spp, key="lights")
    n_surf, n_mat = int(bundle.scene.num_surfaces), int(bundle.scene.num_materials)
    surface = int(ids[np.argmax((counts[:, 0, 1] > 0) * counts[:, 0, 0]), 0, 0])  # the top surface of a pixel that sees two
    material = int(bundle.scene.surfaces[surface].material)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_mattes(spp)
        for layer, lst in [(M.SURFACE, [surface]), (M.MATERIAL, [material]), (M.SURFACE, [surface, M.ID_MISS, 0]),
                           (M.SURFACE, list(range(n_surf)) + [M.ID_MISS]), (M.MATERIAL, [M.ID_MISS] + list(range(n_mat)) * 3)]:
            got = r.read_matte(layer, lst)
            want = M.matte_select(ids, counts, tail, layer, lst)
            assert np.array_equal(got, want), "layer %d, %s: %d differ" % (layer, lst, int((got != want).sum()))
            assert got.min() >= 0.0 and got.max() <= 1.0
        one = r.read_matte(M.SURFACE, [surface])
        assert ((one > 0.0) & (one < 1.0)).any() and (one == 1.0).any() and (one == 0.0).any()
        assert np.all(r.read_matte(M.SURFACE, list(range(n_surf)) + [M.ID_MISS]) == 1.0)  # (no pixel of this case overflows)
        for layer in (M.SURFACE, M.MATERIAL):
            got = r.read_matte_bgra(layer)
            want = M.matte_bgra(ids, counts, tail, layer)
            assert np.array_equal(got, want), "layer %d: %d bytes differ" % (layer, int((got != want).sum()))
            assert np.all(got[:, 3] == 255) and got[:, 0:3].max() <= 191 and len(np.unique(got[:, 0:3])) > 6
    finally:
        r.close()
    bundle, params = M.load_case("spheres_8x8")  # with `other`: the preview and the full list leave it out
    ids, counts, tail, _, _ = rule(bundle, params, n_samples=48, key="spheres_8x8")
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_mattes(48)
        for layer in (M.SURFACE, M.MATERIAL):
            assert np.array_equal(r.read_matte_bgra(layer), M.matte_bgra(ids, counts, tail, layer))
        full = r.read_matte(M.MATERIAL, list(range(int(bundle.scene.num_materials))) + [M.ID_MISS])
        assert np.array_equal(full, (48.0 - tail[:, 3]) / 48.0) and (full < 1.0).sum() == 1
        top = [int(v) for v in ids[:, 0, 0] if v >= 0][:40]
        assert np.array_equal(r.read_matte(M.SURFACE, top), M.matte_select(ids, counts, tail, M.SURFACE, top))
    finally:
        r.close()


def test_refusals_each_with_its_message():
    bundle, p = cases.load_case("plane_light_16")
    w, h = int(p.width), int(p.height)
    n_surf, n_mat = int(bundle.scene.num_surfaces), int(bundle.scene.num_materials)

    def ctx(**kw):
        return pydrt.Renderer(bundle, pydrt.make_params(w, h, spp=4, max_depth=4, **kw))

    r = ctx(mode=pydrt.MODE_XYZ)
    try:
        r.render()
        with pytest.raises(RuntimeError, match="mattes: n_samples = 0 .* DRT_MODE_XYZ keeps none"):
            r.render_mattes(0)
        rep = r.render_mattes(2)  # with a count of its own it works in both modes
        xyz = r.read_mattes()
    finally:
        r.close()
    assert_mattes(xyz, rep, rule(bundle, pydrt.make_params(w, h, spp=4, max_depth=4), n_samples=2), "XYZ film")
    r = ctx()
    try:
        for read in (r.read_mattes, lambda: r.read_matte(0, [0]), lambda: r.read_matte_bgra(0)):
            with pytest.raises(RuntimeError, match="no matte buffers: drt_render_mattes first"):
                read()
        with pytest.raises(RuntimeError, match=r"mattes: tile pixel 0 \(column 0, row 0 of the tile\) holds the filter sum 0"):
            r.render_mattes(0)  # an empty film
        with pytest.raises(RuntimeError, match=r"mattes: flags = 4: 0 \(reserved\)"):
            r.render_mattes(2, flags=4)
        with pytest.raises(RuntimeError, match="mattes: first_sample 4294967295 \\+ 2 samples: sample numbers are 32 bits"):
            r.render_mattes(2, first_sample=0xFFFFFFFF)
        with pytest.raises(RuntimeError, match="no matte buffers"):  # a refused call has done nothing
            r.read_mattes()
        r.render()
        px, av, va = r.read_film()
        with pytest.raises(RuntimeError, match="mattes: first_sample 4294967295 \\+ 4 samples"):  # the film's counts
            r.render_mattes(0, first_sample=0xFFFFFFFF)
        r.render_mattes(0)
        r.read_mattes()
        with pytest.raises(RuntimeError, match="layer = 2: 0 surfaces, 1 materials"):
            r.read_matte(2, [0])
        with pytest.raises(RuntimeError, match="layer = -1"):
            r.read_matte_bgra(-1)
        with pytest.raises(RuntimeError, match="n_ids = 0: 1 to 4096 ids"):
            r.read_matte(0, [])
        with pytest.raises(RuntimeError, match="n_ids = 4097: 1 to 4096 ids"):
            r.read_matte(0, [0] * 4097)
        assert np.array_equal(r.read_matte(0, [0] * 4096), r.read_matte(0, [0]))
        with pytest.raises(RuntimeError, match=r"id_list\[1\] = -2: -1 \(a miss\) or the index of a surface"):
            r.read_matte(0, [0, -2])
        with pytest.raises(RuntimeError, match=r"id_list\[0\] = %d: the scene has %d surfaces" % (n_surf, n_surf)):
            r.read_matte(0, [n_surf])
        with pytest.raises(RuntimeError, match=r"id_list\[2\] = %d: the scene has %d materials" % (n_mat, n_mat)):
            r.read_matte(1, [0, n_mat - 1, n_mat])
        r.read_matte(0, [n_surf - 1])
        r.reset_film()
        px[w + 2, -1] = 2.5
        r.write_film(px, av, va)
        with pytest.raises(RuntimeError, match=r"mattes: tile pixel %d \(column 2, row 1 of the tile\) holds the filter sum 2.5" % (w + 2)):
            r.render_mattes(0)
        for a, b in zip((px, av, va), r.read_film()):
            assert cases.same_bits(a, b)
        for change in (lambda: r.render(4, 2), lambda: r.write_film(px, av, va), lambda: r.reset_film()):
            r.reset_film()
            r.render(0, 2)
            r.render_mattes(0)
            r.read_mattes()
            change()
            for read in (r.read_mattes, lambda: r.read_matte(0, [0]), lambda: r.read_matte_bgra(1)):
                with pytest.raises(RuntimeError, match="the film has changed since drt_render_mattes"):
                    read()
    finally:
        r.close()


def test_drt_render_program_with_the_mattes(tmp_path):
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
        full = {k: v for k, v in os.environ.items() if not k.startswith(("DRT_MATTES", "DRT_FEATURES", "DRT_DENOISE"))}
        full.update(env)
        r = subprocess.run([exe], cwd=d, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        return d / "output", r.stdout

    plain, _ = run("plain", DRT_MATTES="0")
    out, text = run("mattes", DRT_MATTES="1", DRT_DEVICES="0,0")
    assert "Mattes: %d camera rays" % (48 * 32 * 8) in text
    standard = ("output.spd", "average.spd", "variance.spd", "output.bmp", "average.bmp", "variance.bmp")
    for f in standard:
        assert open(plain / f, "rb").read() == open(out / f, "rb").read(), f
    extra = ["output.spd.surface_id.spd", "output.spd.material_id.spd", "output.spd.surface_id.bmp", "output.spd.material_id.bmp",
             "output.spd.mattes.txt"]
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain) + extra)  # and no temporary file is left
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 48, 32)
    params = pydrt.make_params(48, 32, spp=8, max_depth=6, seed=1)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render()
        r.render_mattes(0)
        ids, counts, tail = r.read_mattes()
        pictures = {"surface_id": r.read_matte_bgra(M.SURFACE), "material_id": r.read_matte_bgra(M.MATERIAL)}
    finally:
        r.close()
    assert np.all(tail[:, 0] == 8) and (counts[:, 0, 1] > 0).any()
    head = bytearray(open(out / "average.spd", "rb").read()[:40])
    for layer, name in enumerate(("surface_id", "material_id")):
        f = "output.spd.%s.spd" % name
        got_head = open(out / f, "rb").read()[:40]
        S_at = bytes(head).index(np.uint32(69).tobytes(), 4)
        assert got_head[:S_at] == bytes(head[:S_at]) and got_head[S_at:S_at + 4] == np.uint32(12).tobytes() and got_head[S_at + 4:] == bytes(head[S_at + 4:]), f
        got = np.fromfile(out / f, dtype=np.float64, offset=40).reshape(-1, 12)
        assert np.array_equal(got[:, 0::2], ids[:, layer].astype(np.float64)), f
        assert np.array_equal(got[:, 1::2], counts[:, layer] / tail[:, 0:1].astype(np.float64)), f
        data = open(out / ("output.spd.%s.bmp" % name), "rb").read()
        assert data[:54] == open(out / "output.bmp", "rb").read()[:54]
        assert np.array_equal(np.frombuffer(data[54:], dtype=np.uint8).reshape(-1, 4), pictures[name]), name
        assert len(np.unique(pictures[name][:, 0:3])) > 6
    lines = open(out / "output.spd.mattes.txt").read().splitlines()
    surfaces, materials = bundle.surface_names(), bundle.material_names()
    assert lines == ["surface %d %s material %d" % (i, n, int(bundle.scene.surfaces[i].material)) for i, n in enumerate(surfaces)] + \
        ["material %d %s" % (i, n) for i, n in enumerate(materials)]
    assert len(surfaces) > 3 and all(surfaces)
