"""GPU (-m gpu): ray queries (drt_cast_rays, drt_test_visibility, drt_cast_pixels, their group forms, the drt_render program's
DRT_PICK) against the oracle's find_ray_intersection and points_mutually_visible, ray by ray and bit for bit, on the LDS scans and
through the hierarchy walk. The inputs are those of tests/ray_query_cases.py, which tests/test_ray_query_cpu.py shows to hold no
subnormal quotient (there the device's division may be one unit off): a condition on the input, not a tolerance.
No ray and no pair is skipped."""
import contextlib
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import pydrt
import ray_query_cases as Q

pytestmark = pytest.mark.gpu

HIT_FLOATS = ("position", "normal", "out", "on_dot", "distance")
HIT_INTS = ("index", "surface_material", "incident_material", "transmit_material")
GUARD = 0xA5


@contextlib.contextmanager
def renderer(name, bvh=False, chunk=None, params=None):
    """a context on the scene; bvh: behind the hierarchy whatever its size (DRT_FORCE_BVH); chunk: host-mode staging chunk
    (DRT_RAY_CHUNK). Both are read when the context is created."""
    bundle, p = Q.load(name)
    knobs = {"DRT_FORCE_BVH": "1" if bvh else None, "DRT_RAY_CHUNK": str(chunk) if chunk else None}
    saved = {k: os.environ.get(k) for k in knobs}
    for k, v in knobs.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    try:
        r = pydrt.Renderer(bundle, params or p)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    try:
        yield r
    finally:
        r.close()


def assert_hits(got, want, what):
    for f in HIT_INTS:
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), "%s %s: %d differ, first ray %d: %d against %d" % (what, f, len(bad), bad[0], got[f][bad[0]], want[f][bad[0]])
    for f in HIT_FLOATS:
        assert cases.same_bits(got[f], want[f]), "%s %s: %s" % (what, f, cases.first_difference(got[f], want[f]))


def as_records(t):
    """a device-mode [n][104] uint8 tensor as a record array"""
    return np.ascontiguousarray(t.cpu().numpy()).view(pydrt.RAY_HIT_DTYPE).reshape(-1)


def expect_bvh(name, forced):
    return forced or name in ("spheres_1500", "fuzz_101")


@pytest.mark.parametrize("name, forced", Q.ALL_SCENES, ids=["%s%s" % (n, "-bvh" if f else "") for n, f in Q.ALL_SCENES])
def test_closest_hits_and_visibility_equal_the_oracle_ray_by_ray(name, forced):
    s, e = Q.ray_sets(name), Q.expected(name)
    ro, rd = s["rays"]
    with renderer(name, bvh=forced) as r:
        assert bool(r.stats().path_flags & pydrt.PATH_BVH) == expect_bvh(name, forced)
        hits = r.cast_rays(ro, rd)
        vis = r.test_visibility(*s["pairs"])
    want = e["hits"]
    assert_hits(hits, want, name)
    miss = want["index"] < 0
    assert miss.any() and (~miss).any()
    bundle = Q.load(name)[0]
    assert np.all(hits["surface_material"][miss] == int(bundle.scene.escape_material))
    for f in HIT_FLOATS + ("incident_material", "transmit_material"):
        assert not hits[f][miss].any(), f
        assert not np.signbit(hits[f][miss]).any() if f in HIT_FLOATS else True
    # position = (o + d * fudge) + d * distance, recomputed here
    on = ~miss
    with np.errstate(all="ignore"):
        again = Q.moved_origins(ro, rd)[on] + rd[on] * hits["distance"][on][:, None]
    assert cases.same_bits(again, hits["position"][on]), cases.first_difference(again, hits["position"][on])
    assert cases.same_bits(-rd[on], hits["out"][on])
    bad = np.flatnonzero(vis != e["visible"])
    assert not len(bad), "%s visibility: %d of %d pairs differ, first %d" % (name, len(bad), len(vis), bad[0])
    assert set(np.unique(vis)) == {0, 1}


# ------------------------------------------------------------------------------------------------
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000]


def guarded_calls(r, ro, rd, p0, p1, xy, smp, n, pad=40):
    """the three calls through the C-ABI in host mode with n queries into buffers `pad` elements longer, prefilled with a guard"""
    L = r.L
    hits = np.full((n + pad) * 104, GUARD, dtype=np.uint8)
    vis = np.full(n + pad, GUARD, dtype=np.uint8)
    phits = np.full((n + pad) * 104, GUARD, dtype=np.uint8)
    po = np.full((n + pad, 3), -7.25)
    pd = np.full((n + pad, 3), -7.25)
    pydrt._check(L.drt_cast_rays(r.ctx, ro.ctypes.data, rd.ctypes.data, n, hits.ctypes.data, 0), "drt_cast_rays")
    pydrt._check(L.drt_test_visibility(r.ctx, p0.ctypes.data, p1.ctypes.data, n, vis.ctypes.data, 0), "drt_test_visibility")
    pydrt._check(L.drt_cast_pixels(r.ctx, xy.ctypes.data, smp.ctypes.data, n, po.ctypes.data, pd.ctypes.data, phits.ctypes.data, 0), "drt_cast_pixels")
    assert np.all(hits[n * 104:] == GUARD) and np.all(vis[n:] == GUARD) and np.all(phits[n * 104:] == GUARD)
    assert np.all(po[n:] == -7.25) and np.all(pd[n:] == -7.25)
    return hits[:n * 104].view(pydrt.RAY_HIT_DTYPE), vis[:n], phits[:n * 104].view(pydrt.RAY_HIT_DTYPE), po[:n], pd[:n]


@pytest.mark.parametrize("name, chunk", [("lights", None), ("spheres_1500", None), ("lights", 100), ("spheres_1500", 64)])
def test_every_list_length_gives_the_same_bits_and_writes_nothing_past_its_end(name, chunk):
    s, e = Q.ray_sets(name), Q.expected(name)
    ro, rd = (np.ascontiguousarray(a[:1000]) for a in s["rays"])
    pick = np.arange(1000) % len(e["visible"])  # (a scene's pair set may be shorter than the longest list: taken round and round)
    p0, p1 = (np.ascontiguousarray(a[pick]) for a in s["pairs"])
    want_vis = e["visible"][pick]
    xy, smp = (np.ascontiguousarray(a[:1000]) for a in s["camera"])
    assert len(ro) == len(p0) == len(xy) == 1000
    with renderer(name, chunk=chunk) as r:
        for n in SIZES:
            hits, vis, phits, po, pd = guarded_calls(r, ro, rd, p0, p1, xy, smp, n)
            assert_hits(hits, e["hits"][:n], "%s n=%d" % (name, n))
            assert np.array_equal(vis, want_vis[:n]), n
            assert_hits(phits, e["hits"][:n], "%s pixels n=%d" % (name, n))  # (the first rays of the set are the camera rays)
            assert cases.same_bits(po, ro[:n]) and cases.same_bits(pd, rd[:n])


@pytest.mark.parametrize("name", ["lights", "spheres_1500"])
def test_device_mode_gives_host_modes_bits_and_writes_nothing_past_its_end(name):
    torch = pytest.importorskip("torch")
    s, e = Q.ray_sets(name), Q.expected(name)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    ro, rd = s["rays"]
    p0, p1 = s["pairs"]
    xy, smp = s["camera"]
    with renderer(name) as r, torch.cuda.stream(stream):
        r.set_stream(stream.cuda_stream)
        t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt).contiguous()
        hits = r.cast_rays(t(ro), t(rd))
        vis = r.test_visibility(t(p0), t(p1))
        po, pd, phits = r.cast_pixels(t(xy.astype(np.int32), torch.int32), t(smp.astype(np.int32), torch.int32))
        hits, vis, phits, po, pd = as_records(hits), vis.cpu().numpy(), as_records(phits), po.cpu().numpy(), pd.cpu().numpy()
        cam = s["parts"]["camera"]
        assert_hits(hits, e["hits"], name + " device mode")
        assert np.array_equal(vis, e["visible"])
        assert_hits(phits, e["hits"][cam], name + " device mode pixels")
        assert cases.same_bits(po, ro[cam]) and cases.same_bits(pd, rd[cam])
        # the kernels' own stores, at every list length: guard bytes behind element n - 1, odd byte offsets for the visibility words
        pick = np.arange(1000) % len(e["visible"])
        d_ro, d_rd, d_p0, d_p1 = t(ro[:1000]), t(rd[:1000]), t(p0[pick]), t(p1[pick])
        for n in SIZES:
            for off in (0, 3):
                g_hits = torch.full(((n + 8) * 104,), GUARD, dtype=torch.uint8, device=dev)
                g_vis = torch.full((n + 72,), GUARD, dtype=torch.uint8, device=dev)
                pydrt._check(r.L.drt_cast_rays(r.ctx, d_ro.data_ptr(), d_rd.data_ptr(), n, g_hits.data_ptr(), pydrt.RAYS_DEVICE), "drt_cast_rays")
                pydrt._check(r.L.drt_test_visibility(r.ctx, d_p0.data_ptr(), d_p1.data_ptr(), n, g_vis.data_ptr() + off, pydrt.RAYS_DEVICE), "drt_test_visibility")
                h, v = g_hits.cpu().numpy(), g_vis.cpu().numpy()
                assert np.all(h[n * 104:] == GUARD) and np.all(v[:off] == GUARD) and np.all(v[off + n:] == GUARD), (n, off)
                assert_hits(h[:n * 104].view(pydrt.RAY_HIT_DTYPE), e["hits"][:n], "%s device n=%d" % (name, n))
                assert np.array_equal(v[off:off + n], e["visible"][pick][:n]), (n, off)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plane_light_16", "lens", "spheres_1500"])
def test_cast_pixels_gives_the_paths_own_rays_and_first_hits(name):
    bundle, p = Q.load(name)
    spp = 2
    params = pydrt.make_params(int(p.width), int(p.height), spp=spp, max_depth=int(p.max_depth), seed=int(p.seed),
                               pixel_scheme=int(p.pixel_scheme), flags=pydrt.FLAG_RECORD_HITS)
    s, e = Q.ray_sets(name), Q.expected(name)
    xy, smp = s["camera"]
    cam = s["parts"]["camera"]
    P = int(p.width) * int(p.height)
    with renderer(name, params=params) as r:
        po, pd, hits = r.cast_pixels(xy, smp)
        r.render(0, spp)
        log = r.read_hit_indices(spp)
        r.render_features(1, first_sample=1)
        ids = r.read_features()[2]
    assert cases.same_bits(po, s["rays"][0][cam]), cases.first_difference(po, s["rays"][0][cam])
    assert cases.same_bits(pd, s["rays"][1][cam]), cases.first_difference(pd, s["rays"][1][cam])
    assert_hits(hits, e["hits"][cam], name)
    assert np.array_equal(hits["index"], log[:, 0])  # paths are ordered (sample, tile row, tile column), as the camera set is
    assert np.array_equal(hits["index"][P:2 * P], ids)  # sample `first` = 1 of render_features
    # a focus distance for the thin lens: the hit's depth along the camera's forward axis
    on = hits["index"] >= 0
    cam_s = bundle.camera
    depth = ((hits["position"][on] - np.array(list(cam_s.aperture_position))) * np.array(list(cam_s.forward))).sum(axis=1)
    assert on.any() and np.all(depth > 0.0)


def test_a_tile_context_answers_for_any_pixel_of_the_image():
    bundle, p = Q.load("lights")
    params = pydrt.make_params(int(p.width), int(p.height), spp=2, max_depth=int(p.max_depth), seed=int(p.seed), x0=5, y0=3, tile_w=7, tile_h=4, row_stride=3)
    s, e = Q.ray_sets("lights"), Q.expected("lights")
    cam = s["parts"]["camera"]
    with renderer("lights", params=params) as r:
        po, pd, hits = r.cast_pixels(*s["camera"])
    assert cases.same_bits(po, s["rays"][0][cam]) and cases.same_bits(pd, s["rays"][1][cam])
    assert_hits(hits, e["hits"][cam], "tile context")


# ------------------------------------------------------------------------------------------------
def all_queries(r, s):
    return r.cast_rays(*s["rays"]), r.test_visibility(*s["pairs"]), r.cast_pixels(*s["camera"])


def test_a_query_between_two_renders_on_a_stream_changes_nothing():
    torch = pytest.importorskip("torch")
    name = "lights"
    bundle, p = Q.load(name)
    params = pydrt.make_params(int(p.width), int(p.height), spp=6, max_depth=int(p.max_depth), seed=int(p.seed), flags=pydrt.FLAG_RECORD_HITS)
    s, e = Q.ray_sets(name), Q.expected(name)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with renderer(name, params=params) as r, torch.cuda.stream(stream):
        d_ro, d_rd, d_p0, d_p1 = t(s["rays"][0]), t(s["rays"][1]), t(s["pairs"][0]), t(s["pairs"][1])
        stream.synchronize()
        r.set_stream(stream.cuda_stream)
        r.render(0, 3)
        hits = r.cast_rays(d_ro, d_rd)  # enqueued behind the first render, no wait
        vis = r.test_visibility(d_p0, d_p1)
        r.render(3, 3)
        film, stats, log = r.read_film(), cases.stat_counts(r.stats()), r.read_hit_indices(3)
        assert_hits(as_records(hits), e["hits"], "between two renders")
        assert np.array_equal(vis.cpu().numpy(), e["visible"])
    with renderer(name, params=params) as q:
        q.render(0, 3)
        q.render(3, 3)
        for a, b in zip(film, q.read_film()):
            assert cases.same_bits(a, b)
        assert cases.stat_counts(q.stats()) == stats
        assert np.array_equal(q.read_hit_indices(3), log)


def test_nothing_else_moves():
    name = "lights"
    s = Q.ray_sets(name)
    with renderer(name) as r:
        r.render()
        r.render_features(0)
        r.render_mattes(0)

        def state():
            return r.read_film() + r.read_features() + r.read_mattes(), cases.stat_counts(r.stats())
        before, stats = state()
        all_queries(r, s)
        after, stats2 = state()  # (read_features at the film's counts is still accepted: the film generation is unchanged)
        assert stats == stats2
        for a, b in zip(before, after):
            assert a.dtype == b.dtype and (cases.same_bits(a, b) if a.dtype.kind == "f" else np.array_equal(a, b))


def test_refusals_each_with_its_message():
    s = Q.ray_sets("lights")
    ro, rd = (np.ascontiguousarray(a[:8]) for a in s["rays"])
    xy, smp = (np.ascontiguousarray(a[:8]) for a in s["camera"])
    hits = np.zeros(8, dtype=pydrt.RAY_HIT_DTYPE)
    vis = np.zeros(8, dtype=np.uint8)
    a, b, h, v, x, sm = ro.ctypes.data, rd.ctypes.data, hits.ctypes.data, vis.ctypes.data, xy.ctypes.data, smp.ctypes.data
    with renderer("lights") as r:
        L, c = r.L, r.ctx
        err = lambda: L.drt_last_error().decode()
        refused = [
            (L.drt_cast_rays(c, None, b, 8, h, 0), "origins"), (L.drt_cast_rays(c, a, None, 8, h, 0), "dirs"), (L.drt_cast_rays(c, a, b, 8, None, 0), "hits"),
            (L.drt_cast_rays(c, a, b, 8, h, 2), "flags"), (L.drt_cast_rays(c, a, b, 8, h, 3), "flags"), (L.drt_cast_rays(c, a, b, 0, h, 4), "flags"),
            (L.drt_cast_rays(c, a, b, (1 << 31) + 1, h, pydrt.RAYS_DEVICE), "n = "),
            (L.drt_test_visibility(c, None, b, 8, v, 0), "p0"), (L.drt_test_visibility(c, a, None, 8, v, 0), "p1"),
            (L.drt_test_visibility(c, a, b, 8, None, 0), "visible"), (L.drt_test_visibility(c, a, b, 8, v, 8), "flags"),
            (L.drt_test_visibility(c, a, b, (1 << 31) + 1, v, pydrt.RAYS_DEVICE), "n = "),
            (L.drt_cast_pixels(c, None, sm, 8, None, None, h, 0), "xy"), (L.drt_cast_pixels(c, x, None, 8, None, None, h, 0), "samples"),
            (L.drt_cast_pixels(c, x, sm, 8, None, None, None, 0), "hits"), (L.drt_cast_pixels(c, x, sm, 8, None, None, h, 16), "flags"),
            (L.drt_cast_pixels(c, x, sm, (1 << 31) + 1, None, None, h, pydrt.RAYS_DEVICE), "n = "),
        ]
        # (each tuple's call ran in order, but its message has been overwritten by the next: call again one by one for the text)
        assert all(rc != 0 for rc, _ in refused)
        assert L.drt_cast_rays(c, None, b, 8, h, 0) != 0 and "drt_cast_rays" in err() and "origins" in err()
        assert L.drt_cast_rays(c, a, None, 8, h, 0) != 0 and "dirs" in err()
        assert L.drt_cast_rays(c, a, b, 8, None, 0) != 0 and "hits" in err()
        assert L.drt_cast_rays(c, a, b, 8, h, 2) != 0 and "flags" in err()
        assert L.drt_cast_rays(c, a, b, (1 << 31) + 1, h, pydrt.RAYS_DEVICE) != 0 and "n = 2147483649" in err()
        assert L.drt_test_visibility(c, None, b, 8, v, 0) != 0 and "drt_test_visibility" in err() and "p0" in err()
        assert L.drt_test_visibility(c, a, None, 8, v, 0) != 0 and "p1" in err()
        assert L.drt_test_visibility(c, a, b, 8, None, 0) != 0 and "visible" in err()
        assert L.drt_test_visibility(c, a, b, 8, v, 8) != 0 and "flags" in err()
        assert L.drt_cast_pixels(c, None, sm, 8, None, None, h, 0) != 0 and "drt_cast_pixels" in err() and "xy" in err()
        assert L.drt_cast_pixels(c, x, None, 8, None, None, h, 0) != 0 and "samples" in err()
        assert L.drt_cast_pixels(c, x, sm, 8, None, None, None, 0) != 0 and "hits" in err()
        w, hgt = int(r.params.width), int(r.params.height)
        for bad in ((w, 0), (0, hgt), (0xFFFFFFFF, 0)):
            xy2 = xy.copy()
            xy2[5] = bad
            assert L.drt_cast_pixels(c, xy2.ctypes.data, sm, 8, None, None, h, 0) != 0
            assert "xy[5]" in err() and "outside" in err(), err()
        assert not hits.view(np.uint8).any() and not vis.any()  # nothing was written
        # n = 0 is a successful no-op, whatever the pointers
        assert L.drt_cast_rays(c, None, None, 0, None, 0) == 0 and L.drt_test_visibility(c, None, None, 0, None, 0) == 0
        assert L.drt_cast_pixels(c, None, None, 0, None, None, None, pydrt.RAYS_DEVICE) == 0
        # origins and dirs of drt_cast_pixels are optional
        assert L.drt_cast_pixels(c, x, sm, 8, None, None, h, 0) == 0
        assert np.array_equal(hits["index"], Q.expected("lights")["hits"]["index"][:8])
        assert L.drt_cast_rays(None, a, b, 8, h, 0) != 0 and "ctx" in err()
    g = pydrt.Group(*Q.load("lights"), devices=[0, 0])
    try:
        assert g.L.drt_group_cast_rays(g.g, None, b, 8, h) != 0 and "origins" in err()
        xy2 = xy.copy()
        xy2[7] = (0, int(g.params.height))
        assert g.L.drt_group_cast_pixels(g.g, xy2.ctypes.data, sm, 8, None, None, h) != 0 and "xy[7]" in err()
        assert g.L.drt_group_test_visibility(g.g, a, b, 0, None) == 0
    finally:
        g.close()


def test_the_group_forms_give_the_sessions_bits_in_list_order():
    for name in ("lights", "spheres_1500"):
        s, e = Q.ray_sets(name), Q.expected(name)
        cam = s["parts"]["camera"]
        for devices in ([0], [0, 0], [0, 0, 0]):
            g = pydrt.Group(*Q.load(name), devices=devices)
            try:
                assert_hits(g.cast_rays(*s["rays"]), e["hits"], "%s group %s" % (name, devices))
                assert np.array_equal(g.test_visibility(*s["pairs"]), e["visible"])
                po, pd, hits = g.cast_pixels(*s["camera"])
                assert_hits(hits, e["hits"][cam], "%s group %s pixels" % (name, devices))
                assert cases.same_bits(po, s["rays"][0][cam]) and cases.same_bits(pd, s["rays"][1][cam])
                # a list shorter than the device list
                assert_hits(g.cast_rays(s["rays"][0][:2], s["rays"][1][:2]), e["hits"][:2], "short list")
            finally:
                g.close()


# ------------------------------------------------------------------------------------------------
def test_drt_render_program_with_picks(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("num_pixel_samples 4", "num_pixel_samples 2").replace("output_width      800", "output_width      48")
    cfg = cfg.replace("output_height     600", "output_height     32")
    assert "output_width      48" in cfg and "output_height     32" in cfg

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
        return d / "output", r.stdout

    picks = [(0, 0, 0), (24, 16, 0), (47, 31, 1), (10, 2, 5), (24, 30, 0), (3, 29, 2)]
    plain, text0 = run("plain")
    out, text = run("picks", DRT_PICK=";".join("%d,%d" % (x, y) if s == 0 else "%d,%d,%d" % (x, y, s) for x, y, s in picks), DRT_DEVICES="0,0")
    assert "pick " not in text0
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain))
    for f in os.listdir(plain):
        assert open(plain / f, "rb").read() == open(out / f, "rb").read(), f
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 48, 32)
    params = pydrt.make_params(48, 32, spp=2, max_depth=4, seed=1)
    r = pydrt.Renderer(bundle, params)
    try:
        _, _, hits = r.cast_pixels(np.array([p[:2] for p in picks]), np.array([p[2] for p in picks]))
    finally:
        r.close()
    lines = [l for l in text.splitlines() if l.startswith("pick ")]
    assert len(lines) == len(picks)
    surfaces, materials = bundle.surface_names(), bundle.material_names()
    seen_hit = False
    for line, (x, y, s), h in zip(lines, picks, hits):
        if h["index"] < 0:
            assert line == "pick %d %d %d miss" % (x, y, s)
            continue
        m = re.fullmatch(r"pick (\d+) (\d+) (\d+) surface (-?\d+) (.*) material (\d+) (.*) distance (\S+) position (\S+) (\S+) (\S+)", line)
        assert m, line
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (x, y, s)
        assert int(m.group(4)) == h["index"] and m.group(5) == surfaces[int(h["index"])]
        assert int(m.group(6)) == h["surface_material"] and m.group(7) == materials[int(h["surface_material"])]
        assert float(m.group(8)) == h["distance"]  # %.17g round-trips
        assert [float(m.group(k)) for k in (9, 10, 11)] == list(h["position"])
        seen_hit = True
    assert seen_hit
