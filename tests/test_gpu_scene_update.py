"""GPU (-m gpu): scene updates of a live context (drt_set_camera, drt_update_surfaces, drt_get_update_report, their group forms, pydrt's
bindings, the drt_render program's DRT_TURNTABLE). The rule: an updated context gives bit for bit what a fresh
context on the updated scene gives. Every film comparison is cases.same_bits on all three buffers, hit logs with array_equal, the
counting statistics with ==, each against a fresh context on the "after" bundle of tests/scene_update_cases.py AND against the oracle.
tests/test_scene_update_cpu.py holds the premises (every "after" film differs from its "before" film)."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import cases
import feature_rule as F
import matte_rule as M
import pydrt
import ray_query_cases as Q
import scene_update_cases as U

pytestmark = pytest.mark.gpu

HIT_FLOATS = ("position", "normal", "out", "on_dot", "distance")
HIT_INTS = ("index", "surface_material", "incident_material", "transmit_material")
_fresh, _oracle = {}, {}


def assert_same_film(got, want, what):
    for name, a, b in zip(("pixels", "avgs", "vars"), got, want):
        assert cases.same_bits(a, b), "%s %s: %s" % (what, name, cases.first_difference(a, b))


def assert_hits(got, want, what):
    for f in HIT_INTS:
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), "%s %s: %d differ, first ray %d: %d against %d" % (what, f, len(bad), bad[0], got[f][bad[0]], want[f][bad[0]])
    for f in HIT_FLOATS:
        assert cases.same_bits(got[f], want[f]), "%s %s: %s" % (what, f, cases.first_difference(got[f], want[f]))


@contextlib.contextmanager
def forced_bvh(on):
    saved = os.environ.get("DRT_FORCE_BVH")
    os.environ.pop("DRT_FORCE_BVH", None)
    if on:
        os.environ["DRT_FORCE_BVH"] = "1"
    try:
        yield
    finally:
        os.environ.pop("DRT_FORCE_BVH", None)
        if saved is not None:
            os.environ["DRT_FORCE_BVH"] = saved


@contextlib.contextmanager
def context(name, which="before", params=None):
    """a context on a case's scene (DRT_FORCE_BVH is read when the context is created)"""
    c = U.load(name)
    with forced_bvh(c["forced"]):
        r = pydrt.Renderer(c[which], params or c["params"])
    try:
        assert bool(r.stats().path_flags & pydrt.PATH_BVH) == c["bvh"], name
        yield r
    finally:
        r.close()


def rendered(r, p):
    """(film, hit log, counting statistics) of one drt_render call"""
    r.render()
    return r.read_film(), r.read_hit_indices(int(p.spp)), cases.stat_counts(r.stats())


def fresh(name, which="after"):
    """a fresh context's (film, hit log, counts) on a case's scene, rendered once"""
    if (name, which) not in _fresh:
        with context(name, which) as r:
            _fresh[(name, which)] = rendered(r, U.load(name)["params"])
    return _fresh[(name, which)]


def oracle(name):
    if name not in _oracle:
        c = U.load(name)
        px, av, va, log, st = cases.oracle_render_device_pow(c["after"], c["params"], want_hits=True)
        _oracle[name] = ((px, av, va), log, cases.stat_counts(st))
    return _oracle[name]


def assert_is_after(got, name, what, with_oracle=True):
    """a (film, hit log, counts) triple against the fresh context on the "after" scene and against the oracle"""
    refs = [("a fresh context", fresh(name))] + ([("the oracle", oracle(name))] if with_oracle else [])
    for ref_name, (film, log, counts) in refs:
        assert_same_film(got[0], film, "%s (%s) against %s" % (name, what, ref_name))
        assert np.array_equal(got[1], log), "%s (%s): hit log against %s" % (name, what, ref_name)
        assert got[2] == counts, "%s (%s): counts against %s" % (name, what, ref_name)


def assert_is_before(got, name, what):
    film, log, counts = fresh(name, "before")
    assert_same_film(got[0], film, "%s (%s) against the scene before" % (name, what))
    assert np.array_equal(got[1], log) and got[2] == counts


def apply(r, name, device=False, **kw):
    """what takes a context of the case's "before" scene to its "after" scene"""
    c = U.load(name)
    rows = pydrt.surface_rows(c["after"])
    if device:
        import torch
        rows = torch.from_numpy(rows).to("cuda:0")
    r.update_surfaces(rows, **kw)
    if name in U.CAMERA or name == "spheres_1500_far":
        r.set_camera(c["after"])


def query_check(r, bundle, ro, rd, p0, p1, what):
    hits, vis = r.cast_rays(ro, rd), r.test_visibility(p0, p1)
    want = Q.oracle_hits(bundle, ro, rd)
    want["distance"] = Q.oracle_distances(bundle, ro, rd, want["index"])
    assert_hits(hits, want, what)
    assert (want["index"] >= 0).any() and (want["index"] < 0).any()
    assert np.array_equal(vis, Q.oracle_visible(bundle, p0, p1)), what
    assert set(np.unique(vis)) == {0, 1}


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", U.CAMERA)
def test_set_camera_gives_the_new_cameras_film_and_the_old_one_again(name):
    c = U.load(name)
    p = c["params"]
    with context(name) as r:
        first = rendered(r, p)
        assert_is_before(first, name, "before any call")
        r.reset_film()
        r.set_camera(c["after"])
        assert_is_after(rendered(r, p), name, "set_camera")
        r.reset_film()
        r.set_camera(c["before"].camera)
        back = rendered(r, p)
        assert_same_film(back[0], first[0], name + ": the first camera again")
        assert np.array_equal(back[1], first[1]) and back[2] == first[2]
        rep = r.update_report()
        assert rep["updates"] == 2 and rep["refits_since_build"] == (2 if c["bvh"] else 0)


# ------------------------------------------------------------------------------------------------ 2, 3
@pytest.mark.parametrize("name", U.LDS_SURFACES + U.BVH_SURFACES)
def test_update_surfaces_in_host_mode_gives_a_fresh_contexts_bits(name):
    c = U.load(name)
    p = c["params"]
    with context(name) as r:
        assert_is_before(rendered(r, p), name, "before the update")
        r.reset_film()
        apply(r, name)
        assert_is_after(rendered(r, p), name, "host mode")
        rep = r.update_report()
        assert rep["updates"] == 1 and rep["refits_since_build"] == (1 if c["bvh"] else 0) and rep["kernel_ms"] > 0.0
        if name == "spheres_1500":  # a box that is too small shows here first
            query_check(r, c["after"], *U.seeded_rays(name), name + " after the update")


# ------------------------------------------------------------------------------------------------ 4
def test_the_extent_grows_and_shrinks_with_the_scene():
    name = "spheres_1500_far"
    c = U.load(name)
    p = c["params"]
    with context(name) as r:
        e0 = r.update_report()["extent"]
        assert 30.0 <= e0 < 100.0
        apply(r, name)
        e1 = r.update_report()["extent"]
        assert 16.0 * 40.0 <= e1 < 1000.0
        assert_is_after(rendered(r, p), name, "sixteen extents away")
        for centre in ((640.0, 0.0, -10.0), (0.0, 0.0, -20.0)):  # origins around both places
            query_check(r, c["after"], *U.seeded_rays(name, n=2048, seed=int(centre[0]) + 3, centre=centre), "%s around %s" % (name, centre))
        r.reset_film()
        r.update_surfaces(pydrt.surface_rows(c["before"]))
        r.set_camera(c["before"])
        assert r.update_report()["extent"] == e0
        assert_is_before(rendered(r, p), name, "and back")
        query_check(r, c["before"], *U.seeded_rays(name, n=2048, seed=5, centre=(0.0, 0.0, -20.0)), name + " back")


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("name", ["lights_all", "lights_all_bvh"])
def test_ranges_and_history(name):
    c = U.load(name)
    p = c["params"]
    rows = pydrt.surface_rows(c["after"])
    with context(name) as r:
        r.update_surfaces(rows[2:5], first=2)  # first > 0, count < n: the three lights
        assert_is_after(rendered(r, p), name, "surfaces 2..4 only")
        r.reset_film()
        # two updates in a row equal the second alone: first another scene altogether, then the case's
        other = pydrt.surface_rows(c["before"])
        other[:, U.ROW_POS] += 0.25
        other[5, U.ROW_RADIUS] = 0.3
        r.update_surfaces(other)
        r.update_surfaces(rows)
        assert_is_after(rendered(r, p), name, "two updates in a row", with_oracle=False)
        r.reset_film()
        n = r.update_report()["updates"]
        r.update_surfaces(rows[0:0])  # count == 0: a successful no-op
        r.update_surfaces(rows[0:0], first=int(c["after"].scene.num_surfaces))
        assert r.update_report()["updates"] == n
        assert_is_after(rendered(r, p), name, "after count == 0", with_oracle=False)


# ------------------------------------------------------------------------------------------------ 6
def test_rebuild_gives_the_refits_bits():
    name = "spheres_1500"
    c = U.load(name)
    p = c["params"]
    with context(name) as r:
        apply(r, name)
        assert r.update_report()["refits_since_build"] == 1
        refit = rendered(r, p)
        r.reset_film()
        apply(r, name, rebuild=True)
        assert r.update_report()["refits_since_build"] == 0 and r.update_report()["updates"] == 2
        built = rendered(r, p)
        assert_same_film(built[0], refit[0], "rebuild against refit")
        assert np.array_equal(built[1], refit[1]) and built[2] == refit[2]
        assert_is_after(built, name, "rebuild")
        query_check(r, c["after"], *U.seeded_rays(name, n=1024, seed=11), name + " after the rebuild")
    with context("lights_all") as r:  # without the hierarchy the flag changes nothing
        apply(r, "lights_all", rebuild=True)
        assert_is_after(rendered(r, U.load("lights_all")["params"]), "lights_all", "rebuild without a hierarchy", with_oracle=False)


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("name", ["lights_plane", "lights_sphere", "lights_point", "lights_all", "lights_all_bvh", "spheres_1500"])
def test_device_mode_gives_host_modes_bits(name):
    pytest.importorskip("torch")
    c = U.load(name)
    p = c["params"]
    with context(name) as r:
        assert_is_before(rendered(r, p), name, "before the update")
        r.reset_film()
        apply(r, name, device=True)
        assert_is_after(rendered(r, p), name, "device mode")
        if name == "spheres_1500":
            query_check(r, c["after"], *U.seeded_rays(name, n=1024, seed=13), name + " after the device-mode update")
            # a host-mode update of a part after it starts from the device's copy
            r.reset_film()
            rows = pydrt.surface_rows(c["before"])
            r.update_surfaces(rows[:700])
            r.update_surfaces(pydrt.surface_rows(c["after"])[:700])
            assert_is_after(rendered(r, p), name, "host mode after device mode", with_oracle=False)


def test_device_mode_reports_an_extent_beyond_2_27_at_the_next_synchronisation():
    torch = pytest.importorskip("torch")
    name = "spheres_1500"
    c = U.load(name)
    p = c["params"]
    with context(name) as r:
        bad = pydrt.surface_rows(c["before"])[:1].copy()
        bad[0, U.ROW_POS] = (2.0 ** 28, 0.0, 0.0)
        r.update_surfaces(torch.from_numpy(bad).to("cuda:0"))  # enqueued: the call itself cannot know
        for call in (r.synchronize, r.read_film, r.stats):
            with pytest.raises(RuntimeError, match="2\\^27"):
                call()
        apply(r, name, device=True)  # a good update clears it
        r.synchronize()
        assert_is_after(rendered(r, p), name, "after the violation was mended")
        assert r.update_report()["extent"] < 100.0
    with context("lights_all") as r:  # no hierarchy, no extent to hold
        far = pydrt.surface_rows(U.load("lights_all")["before"])[3:4].copy()
        far[0, U.ROW_POS] = (2.0 ** 28, 0.0, 0.0)
        r.update_surfaces(torch.from_numpy(far).to("cuda:0"), first=3)
        r.synchronize()


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("name", ["lights_all", "spheres_1500"])
def test_refusals_change_nothing(name):
    torch = pytest.importorskip("torch")
    c = U.load(name)
    p = c["params"]
    L = pydrt.hip_lib()
    rows = pydrt.surface_rows(c["after"])
    n = rows.shape[0]
    with context(name) as r:
        def refused(match, call):
            with pytest.raises(RuntimeError, match=match):
                call()
        # a film with samples
        r.render()
        refused("film holds samples", lambda: r.update_surfaces(rows))
        refused("film holds samples", lambda: r.set_camera(c["after"]))
        refused("film holds samples", lambda: r.update_surfaces(torch.from_numpy(rows).to("cuda:0")))
        r.reset_film()
        # a type and a material mismatch: the message names the surface
        wrong = pydrt.surfaces_from_rows(rows)
        wrong[3].type = pydrt.GEO_POINT if int(wrong[3].type) != pydrt.GEO_POINT else pydrt.GEO_SPHERE
        refused("surface 3: type", lambda: r.update_surfaces(wrong))
        part = pydrt.surfaces_from_rows(rows[4:])
        part[1].material = int(part[1].material) + 1  # the scene's surface 5
        refused("surface 5: material", lambda: r.update_surfaces(part, first=4))
        # first + count too large, null with count > 0, unknown flags, rebuild with device mode
        refused("surfaces \\[1, %d\\) of %d" % (n + 1, n), lambda: r.update_surfaces(rows, first=1))
        assert L.drt_update_surfaces(r.ctx, None, 0, 1, 0) != 0 and b"null" in L.drt_last_error()
        assert L.drt_update_surfaces(r.ctx, rows.ctypes.data, 0, n, 4) != 0 and b"unknown flags" in L.drt_last_error()
        assert L.drt_update_surfaces(r.ctx, rows.ctypes.data, 0, n, 8 | pydrt.SURFACES_REBUILD) != 0 and b"unknown flags" in L.drt_last_error()
        refused("DRT_SURFACES_REBUILD", lambda: r.update_surfaces(torch.from_numpy(rows).to("cuda:0"), rebuild=True))
        assert L.drt_set_camera(r.ctx, None) != 0 and b"null" in L.drt_last_error()
        if c["bvh"]:  # 2^27 in host mode, surfaces and camera: drt_create's refusal
            far = rows.copy()
            far[7, U.ROW_POS] = (0.0, -(2.0 ** 27), 0.0)
            refused("2\\^27", lambda: r.update_surfaces(far))
            refused("2\\^27", lambda: r.update_surfaces(far, rebuild=True))
            refused("2\\^27", lambda: r.set_camera(U.sphere_camera((2.0 ** 27, 0.0, 30.0), (2.0 ** 27, 0.0, -20.0), int(p.width), int(p.height))))
        assert r.update_report()["updates"] == 0
        assert_is_before(rendered(r, p), name, "after every refusal")


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("name", ["lights_all", "spheres_1500"])
def test_the_other_passes_see_the_new_scene(name):
    c = U.load(name)
    p = c["params"]
    after = c["after"]
    with context(name) as r:
        r.render_features(n_samples=2)
        r.render_mattes(n_samples=2)
        r.read_features()
        r.read_mattes()
        apply(r, name)
        with pytest.raises(RuntimeError, match="no feature buffers"):  # a pass taken before the update describes the old scene
            r.read_features()
        with pytest.raises(RuntimeError):
            r.read_mattes()
        r.render_features(n_samples=3, first_sample=1)
        mean, m2, ids = r.read_features()
        wmean, wm2, wids, _, _ = F.features(after, p, n_samples=3, first_sample=1)
        assert cases.same_bits(mean, wmean) and cases.same_bits(m2, wm2) and np.array_equal(ids, wids)
        r.render_mattes(n_samples=3)
        got = r.read_mattes()
        for a, b in zip(got, M.mattes(after, p, n_samples=3)):
            assert np.array_equal(a, b)
        film, log, _ = rendered(r, p)
        x, y = F.tile_pixels(p)
        _, _, hits = r.cast_pixels(np.stack([x, y], axis=1), np.zeros(len(x), dtype=np.uint32))
        assert np.array_equal(hits["index"], log[:len(x), 0])  # sample 0's paths come first in the log
        assert np.array_equal(log, fresh(name)[1])


def test_render_adaptive_after_an_update():
    name = "lights_all"
    c = U.load(name)
    q = U._params(c["params"], hits=False)
    q.flags = 0
    args = (2, 5, 2, 0.05)
    with context(name, "after", params=q) as r:
        want_report = r.render_adaptive(*args)
        want = r.read_film(), r.read_sample_counts(), cases.stat_counts(r.stats())
    with context(name, params=q) as r:
        apply(r, name)
        report = r.render_adaptive(*args)
        assert report == want_report
        assert_same_film(r.read_film(), want[0], "adaptive after an update")
        assert np.array_equal(r.read_sample_counts(), want[1]) and cases.stat_counts(r.stats()) == want[2]
        assert len(np.unique(want[1])) > 1  # the rounds really told pixels apart


def test_set_camera_under_a_bound_ray_table_changes_no_film_bit():
    name = "cam_plane_light_16"
    c = U.load(name)
    p = c["params"]
    w, h = int(p.width), int(p.height)
    table = pydrt.equirect_rays(c["before"], w, h)
    with context(name) as r:
        r.bind_rays(*table)
        first = rendered(r, p)
        r.reset_film()
        r.set_camera(c["after"])
        assert r.stats().path_flags & pydrt.PATH_RAYS
        again = rendered(r, p)
        assert_same_film(again[0], first[0], "the same table under another camera")
        assert np.array_equal(again[1], first[1]) and again[2] == first[2]
        with pytest.raises(RuntimeError):  # refused as before: it asks for the camera's rays
            r.render_features(n_samples=1)
        r.reset_film()
        r.bind_rays(None)
        assert_is_after(rendered(r, p), name, "unbound again", with_oracle=False)


# ------------------------------------------------------------------------------------------------ 10
@pytest.mark.parametrize("name", ["lights_all", "spheres_1500"])
def test_the_group_forms(name):
    torch = pytest.importorskip("torch")
    c = U.load(name)
    q = U._params(c["params"], hits=False)
    q.flags = 0  # (hit recording is per context)
    rows = pydrt.surface_rows(c["after"])
    cam = U.load("cam_spheres_1500" if c["bvh"] else "cam_plane_light_16")["after"].camera
    with context(name, params=q) as r:
        r.update_surfaces(rows)
        r.set_camera(cam)
        r.render()
        want = r.read_film(), cases.stat_counts(r.stats())
    with context(name, params=q) as r:
        r.render()
        before = r.read_film()
    g = pydrt.Group(c["before"], q, devices=[0, 0, 0])
    try:
        g.render()
        assert_same_film(g.read_film(), before, "the group before")
        # one context must refuse: all stay as they were
        rc = g.L.drt_group_update_surfaces(g.g, rows.ctypes.data, 0, rows.shape[0], 0)
        assert rc != 0 and b"film holds samples" in g.L.drt_last_error()
        g.reset_film()
        with pytest.raises(ValueError):
            g.update_surfaces(torch.zeros((1, 14), dtype=torch.float64))  # device mode is per context
        wrong = pydrt.surfaces_from_rows(rows)
        wrong[2].material = int(wrong[2].material) + 1
        with pytest.raises(RuntimeError, match="surface 2: material"):
            g.update_surfaces(wrong)
        g.render()
        assert_same_film(g.read_film(), before, "the group after two refusals")
        g.reset_film()
        g.update_surfaces(rows)
        g.set_camera(cam)
        g.render()
        assert_same_film(g.read_film(), want[0], "the group after the update")
        assert cases.stat_counts(g.stats()) == want[1]
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 11
def test_drt_render_program_with_a_turntable(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    W, H, SPP, DEPTH, FRAMES = 16, 16, 2, 3, 3
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("num_pixel_samples 4", "num_pixel_samples %d" % SPP).replace("max_cast_depth    4", "max_cast_depth    %d" % DEPTH)
    cfg = cfg.replace("output_width      800", "output_width      %d" % W).replace("output_height     600", "output_height     %d" % H)
    assert "output_width      16" in cfg and "output_height     16" in cfg and "num_pixel_samples 2" in cfg and "max_cast_depth    3" in cfg

    def run(name, ok=True, **env):
        d = tmp_path / name
        os.makedirs(d / "output")
        for sub in ("scenes", "spectra"):
            os.symlink(os.path.join(cases.REPO, sub), d / sub)
        (d / "config.cfg").write_text(cfg)
        full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
        full.update(env)
        r = subprocess.run([exe], cwd=d, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stdout[-2000:]
        return d / "output" if ok else r.stdout

    out = run("turntable", DRT_TURNTABLE=str(FRAMES))
    plain = run("plain")
    names = ("output", "average", "variance")
    assert sorted(os.listdir(out)) == sorted("%s.%04d.%s" % (n, k, e) for n in names for k in range(FRAMES) for e in ("spd", "bmp"))
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, H)
    p = pydrt.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=1)
    S = bundle.S
    r = pydrt.Renderer(bundle, p)
    try:
        for k in range(FRAMES):
            r.reset_film()
            r.set_camera(pydrt.turntable_camera(bundle, W, H, k, FRAMES))
            r.render()
            px, av, va = r.read_film()
            fpx = np.fromfile(out / ("output.%04d.spd" % k), dtype=np.float64, offset=40).reshape(-1, S + 1)
            fav = np.fromfile(out / ("average.%04d.spd" % k), dtype=np.float64, offset=40).reshape(-1, S)
            fva = np.fromfile(out / ("variance.%04d.spd" % k), dtype=np.float64, offset=40).reshape(-1, S)
            with np.errstate(invalid="ignore", divide="ignore"):
                norm = va / np.max(np.maximum(va, 0.0), axis=1)[:, None]  # written max-normalised per pixel (host/drt_checkpoint.c)
            assert_same_film((fpx, fav, fva), (px, av, norm), "frame %d" % k)
            assert np.all(fpx[:, -1] == SPP) and np.any(fpx[:, :-1] != 0.0)
    finally:
        r.close()
    for n in names:  # frame 0 is the plain run, byte for byte; frame 1 is another picture
        for e in ("spd", "bmp"):
            assert open(out / ("%s.0000.%s" % (n, e)), "rb").read() == open(plain / ("%s.%s" % (n, e)), "rb").read(), (n, e)
    assert open(out / "output.0001.spd", "rb").read() != open(out / "output.0000.spd", "rb").read()
    two = run("two", DRT_TURNTABLE=str(FRAMES), DRT_DEVICES="0,0")
    for f in sorted(os.listdir(out)):
        assert open(two / f, "rb").read() == open(out / f, "rb").read(), f
    # refused with a message, before any device call
    for env in ({"DRT_CHECKPOINT_SPP": "1"}, {"DRT_RESUME": "1"}, {"DRT_PROJECTION": "equirect"}):
        text = run("refused_" + list(env)[0], ok=False, DRT_TURNTABLE="2", **env)
        assert "DRT_TURNTABLE cannot be combined with " + list(env)[0] in text
    assert "DRT_TURNTABLE" in run("refused_zero", ok=False, DRT_TURNTABLE="0")
