"""GPU (-m gpu): sample maps (drt_render_sample_map, drt_group_render_sample_map) against the rule of tests/sample_map_rule.py.

A pixel rendered over samples 0 .. n-1 in order holds, bit for bit, the film a uniform n-sample render gives it. So the expected film
of a map is, per pixel, the oracle's snapshot at the pixel's count (test_gpu_adaptive's helpers), and the expected report is the plan's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_resume_rule as RR
import cases
import pydrt
import ray_film_cases as RF
import sample_map_rule as SM
import test_gpu_adaptive as A

pytestmark = pytest.mark.gpu

VALUES = (0, 1, 2, 3, 5, 8, 13, 21, 40)
COUNTS = [v for v in VALUES if v]
REL = 0.08  # plane_light_48: an adaptive render with pixels at min, at max and in between (tests/test_gpu_adaptive.py)

_snaps = {}


def make_map(P, seed=11):
    """The test map over P >= 400 tile pixels, values from VALUES: seeded noise, then the shapes at which a ballot word, a block count,
    the scan or the scatter can go wrong (checked by check_map)."""
    rng = np.random.default_rng(seed)
    m = rng.choice(np.array(VALUES, dtype=np.uint32), size=P)
    m[64:128] = 40                       # a whole wave kept
    end = 512 if P >= 512 else P         # block 1 (a partial last block below 512 pixels) holds one nonzero pixel
    m[256:end] = 0
    if P >= 512:
        m[300] = 5
    m[0], m[P - 1] = 13, 21
    return m


def runs_of(mask, n):
    """is there a run of n consecutive true entries"""
    c = np.concatenate(([0], np.cumsum(mask)))
    return bool(mask.size >= n and ((c[n:] - c[:-n]) == n).any())


def check_map(m):
    P = m.size
    assert set(np.unique(m)) == set(VALUES)
    assert m[0] != 0 and m[P - 1] != 0
    assert runs_of(m == 0, 64) and runs_of(m == 40, 64)
    assert any(int((m[b:b + 256] != 0).sum()) == 1 for b in range(0, P, 256))


def snapshots(name, bundle, params):
    """the oracle's film at every count of VALUES (0: the film nothing was rendered into), once per case"""
    if name not in _snaps:
        snaps = A.oracle_snapshots(bundle, params, COUNTS)
        snaps[0] = tuple(np.zeros_like(a) for a in snaps[COUNTS[-1]])
        for film in snaps.values():
            for a in film:
                a.setflags(write=False)
        _snaps[name] = snaps
    return _snaps[name]


def render_map(bundle, params, maps, add=False, devices=None, before=None):
    """(reports, counts [P], film, stats) of the maps rendered one after the other on a fresh context (or group)"""
    r = pydrt.Renderer(bundle, params) if devices is None else pydrt.Group(bundle, params, devices)
    try:
        if before:
            before(r)
        reps = [r.render_sample_map(m, add=add and k > 0) for k, m in enumerate(maps)]
        counts = r.read_sample_counts().reshape(-1)
        film = r.read_film()
        stats = r.stats()
    finally:
        r.close()
    return reps, counts, film, stats


def check_against(name, M, rep, counts, film, stats, snaps):
    assert np.array_equal(counts, M), "%s: %d counts differ" % (name, int((counts != M).sum()))
    assert np.array_equal(film[0][:, -1], counts.astype(np.float64))  # the filter column is the count
    A.assert_same_film(film, A.film_at_counts(snaps, M), name)
    want = SM.plan(np.zeros_like(M), M)
    assert rep == want["report"], (rep, want["report"])
    assert stats.paths == int(M.sum(dtype=np.uint64)) == rep["paths"]
    zero = M == 0
    assert all(not a[zero].any() for a in film)


@pytest.mark.parametrize("name", ["plane_light_48", "gold_mirror", "grid_2p5nm", "spheres_1500", "lens"])
def test_a_map_on_a_fresh_context_gives_every_pixel_its_snapshot(name):
    bundle, params = A.case_params(name, spp=40)
    M = make_map(int(params.tile_w) * int(params.tile_h))
    check_map(M)
    snaps = snapshots(name, bundle, params)
    (rep,), counts, film, stats = render_map(bundle, params, [M.reshape(int(params.tile_h), int(params.tile_w))])
    check_against(name, M, rep, counts, film, stats, snaps)


@pytest.mark.parametrize("n", [1, 7, 40])
def test_a_uniform_map_is_the_uniform_render(n):
    bundle, params = A.case_params("plane_light_48", spp=40)
    P = int(params.tile_w) * int(params.tile_h)
    (rep,), counts, film, stats = render_map(bundle, params, [np.full(P, n, dtype=np.int64)])
    r = pydrt.Renderer(bundle, params)
    try:
        r.render(0, n)
        want = r.read_film()
    finally:
        r.close()
    assert (counts == n).all() and rep["rounds"] == bin(n).count("1") and rep["paths"] == n * P == stats.paths
    assert rep["pixels_rendered"] == P and rep["pixels_above"] == 0 and rep["max_count"] == n
    A.assert_same_film(film, want, "uniform %d" % n)


def test_two_maps_in_a_row():
    bundle, params = A.case_params("plane_light_48", spp=40)
    P = int(params.tile_w) * int(params.tile_h)
    snaps = snapshots("plane_light_48", bundle, params)
    M1, M2 = make_map(P), make_map(P, seed=12)[::-1].copy()
    top = np.maximum(M1, M2)
    reps, counts, film, stats = render_map(bundle, params, [M1, M2])
    assert np.array_equal(counts, top)
    assert reps[0] == SM.plan(np.zeros(P), M1)["report"] and reps[1] == SM.plan(M1, M2)["report"]
    assert reps[1]["pixels_above"] == int((M1 > M2).sum()) > 0
    (rep,), counts1, film1, _ = render_map(bundle, params, [top])
    A.assert_same_film(film, film1, "two maps against one")
    A.assert_same_film(film, A.film_at_counts(snaps, top), "two maps against the snapshots")
    assert stats.paths == int(top.sum(dtype=np.uint64))
    # DRT_MAP_ADD: the second map on top of the first
    reps, counts, film, stats = render_map(bundle, params, [M1, M2], add=True)
    both = M1 + M2
    assert np.array_equal(counts, both) and np.array_equal(film[0][:, -1], both.astype(np.float64))
    assert reps[1] == SM.plan(M1, M2, add=True)["report"] and reps[1]["pixels_above"] == 0
    (rep,), counts1, film1, _ = render_map(bundle, params, [both])
    A.assert_same_film(film, film1, "added maps against one")


def test_a_map_tops_up_a_uniform_render_and_an_adaptive_one():
    bundle, params = A.case_params("plane_light_48", spp=40)
    P = int(params.tile_w) * int(params.tile_h)
    M = make_map(P)
    # the oracle's snapshots hold 4 samples nowhere: the HIP path's uniform film (itself pinned to the oracle) at 4
    snaps = dict(snapshots("plane_light_48", bundle, params))
    r = pydrt.Renderer(bundle, params)
    try:
        r.render(0, 4)
        snaps[4] = r.read_film()
        rep = r.render_sample_map(M)
        counts, film = r.read_sample_counts().reshape(-1), r.read_film()
    finally:
        r.close()
    want = np.maximum(M, 4)
    assert np.array_equal(counts, want) and rep == SM.plan(np.full(P, 4), M)["report"] and rep["pixels_above"] == int((M < 4).sum())
    A.assert_same_film(film, A.film_at_counts(snaps, want), "topped up from 4")
    # after an adaptive render: three more samples of every odd tile pixel
    add = np.zeros(P, dtype=np.uint32)
    add[1::2] = 3
    spds, rw, cy, iv = A.table(bundle)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_adaptive(A.MIN, A.MAX, A.STEP, REL)
        before = r.read_sample_counts().reshape(-1)
        assert np.unique(before).size >= 3
        rep = r.render_sample_map(add, add=True)
        counts, film = r.read_sample_counts().reshape(-1), r.read_film()
        assert np.array_equal(counts, before + add) and rep == SM.plan(before, add, add=True)["report"]
        assert r.read_active_list().size == 0
        # the continuation afterwards, under its own contract
        keep = RR.active_of(lambda n: film[1:], spds, rw, cy, iv, counts, np.arange(P), 40, REL / 2, 0.0)
        ok = RR.allotment_contract(counts, np.nonzero(keep)[0], 40, 4)
        if ok:
            r.render_adaptive_continue(40, 4, REL / 2)
        else:
            with pytest.raises(RuntimeError, match="drt_render_adaptive_continue.*step must be one of"):
                r.render_adaptive_continue(40, 4, REL / 2)
            assert np.array_equal(r.read_sample_counts().reshape(-1), counts)
    finally:
        r.close()
    import test_gpu_adaptive_resume as AR
    uni = AR.uniform_snapshots(bundle, params, sorted(set(int(c) for c in np.unique(counts))))
    A.assert_same_film(film, A.film_at_counts(uni, counts), "three more after an adaptive render")


def test_a_device_tensor_gives_the_same_film_and_report():
    import torch
    bundle, params = A.case_params("plane_light_48", spp=40)
    P = int(params.tile_w) * int(params.tile_h)
    M = make_map(P)
    (rep0,), counts0, film0, _ = render_map(bundle, params, [M])
    # made on the device: the values 0 .. 8 of VALUES by index, never a host copy of the map
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    table = torch.tensor(VALUES, dtype=torch.int32, device="cuda:0")
    t = table[torch.randint(0, len(VALUES), (int(params.tile_h), int(params.tile_w)), generator=g, device="cuda:0")].contiguous()
    r = pydrt.Renderer(bundle, params)
    try:
        rep = r.render_sample_map(t)
        counts, film = r.read_sample_counts().reshape(-1), r.read_film()
    finally:
        r.close()
    host = t.cpu().numpy().reshape(-1).astype(np.uint32)
    (rep1,), counts1, film1, _ = render_map(bundle, params, [host])
    assert rep == rep1 and np.array_equal(counts, counts1) and np.array_equal(counts, host)
    A.assert_same_film(film, film1, "device tensor against its host copy")
    # and the test map itself through a tensor on the device and one on the host
    for tensor in (torch.from_numpy(M.astype(np.int32)).to("cuda:0"), torch.from_numpy(M.astype(np.int32))):
        (rep2,), counts2, film2, _ = render_map(bundle, params, [tensor])
        assert rep2 == rep0 and np.array_equal(counts2, counts0)
        A.assert_same_film(film2, film0, "tensor on %s" % tensor.device)


@pytest.mark.parametrize("env", [{"DRT_FORCE_BVH": "1"}, {"DRT_POOL_BLOCKS": "1"}, {"DRT_NO_SIMPLE_SHADE": "1"},
                                 {"DRT_NO_FIXED_LISTS": "1"}, {"DRT_NO_CLOSED_SHADE": "1"}])
def test_a_b_switches_give_the_same_bits(env, monkeypatch):
    bundle, params = A.case_params("plane_light_48", spp=40)
    M = make_map(int(params.tile_w) * int(params.tile_h))
    snaps = snapshots("plane_light_48", bundle, params)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    (rep,), counts, film, stats = render_map(bundle, params, [M])
    check_against(str(env), M, rep, counts, film, stats, snaps)
    if "DRT_POOL_BLOCKS" in env:
        assert stats.redone_launches > 0
    if "DRT_FORCE_BVH" in env:
        assert stats.path_flags & 1


def test_a_bound_ray_table_of_the_centre_rays_gives_the_camera_film():
    name = "plane_light_center"
    bundle, p = RF.load(name)
    params = RF.params_like(p, flags=0, spp=40)
    M = make_map(int(params.tile_w) * int(params.tile_h))
    (rep0,), counts0, film0, _ = render_map(bundle, params, [M])
    (rep,), counts, film, _ = render_map(bundle, params, [M], before=lambda r: r.bind_rays(*RF.camera_table(name)))
    assert rep == rep0 and np.array_equal(counts, counts0) and np.array_equal(counts, M)
    A.assert_same_film(film, film0, "ray table against the camera")


def test_a_strided_tile_and_a_group():
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), 40, 60)
    params = pydrt.make_params(40, 60, spp=40, max_depth=6, seed=3, x0=7, y0=5, tile_w=25, tile_h=18, row_stride=3)
    M = make_map(25 * 18)
    check_map(M)
    snaps = snapshots("strided", bundle, params)
    (rep,), counts, film, stats = render_map(bundle, params, [M])
    check_against("strided tile", M, rep, counts, film, stats, snaps)
    (grep,), gcounts, gfilm, gstats = render_map(bundle, params, [M], devices=[0, 0, 0])
    assert np.array_equal(gcounts, counts) and grep == rep and gstats.paths == stats.paths
    A.assert_same_film(gfilm, film, "group of three")


def state_of(r):
    return r.read_film(), cases.stat_counts(r.stats()), pydrt.selftest_live_resources()


def same_state(a, b):
    return all(cases.same_bits(x, y) for x, y in zip(a[0], b[0])) and a[1:] == b[1:]


def test_refusals_leave_everything_as_it_was():
    L = pydrt.hip_lib()
    bundle, params = A.case_params("plane_light_48", spp=8)
    P = int(params.tile_w) * int(params.tile_h)
    M = make_map(P)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render(0, 4)
        film0 = r.read_film()
        # a filter sum that is no count, in a film the caller hands over
        r.reset_film()
        px, av, va = (a.copy() for a in film0)
        px[100, -1] = 2.5
        px[7, -1] = 2.5
        r.write_film(px, av, va)
        s0 = state_of(r)
        with pytest.raises(RuntimeError, match=r"drt_render_sample_map.*tile pixel 7 \(column 7, row 0 of the tile\) holds the filter sum 2\.5"):
            r.render_sample_map(M)
        assert same_state(state_of(r), s0)
        with pytest.raises(RuntimeError, match="drt_read_sample_counts"):
            r.read_sample_counts()  # no refusal made the context an adaptive render's
        # DRT_MAP_ADD past 2^32 - 1: every pixel holds 4
        r.reset_film()
        r.write_film(*film0)
        s0 = state_of(r)
        big = np.zeros(P, dtype=np.uint64)
        big[9] = big[300] = 2 ** 32 - 2
        with pytest.raises(RuntimeError, match=r"drt_render_sample_map.*tile pixel 9 \(column 9, row 0 of the tile\) holds 4 samples"):
            r.render_sample_map(big, add=True)
        assert same_state(state_of(r), s0)
        m = pydrt.SampleMap()
        # undefined flag bits, null pointers
        keep = M.copy()
        m.targets, m.flags = keep.ctypes.data, 4
        assert L.drt_render_sample_map(r.ctx, C.byref(m)) != 0 and b"flags" in L.drt_last_error()
        m.targets, m.flags = None, 0
        assert L.drt_render_sample_map(r.ctx, C.byref(m)) != 0 and b"null" in L.drt_last_error()
        assert L.drt_render_sample_map(r.ctx, None) != 0 and L.drt_render_sample_map(None, C.byref(m)) != 0
        assert same_state(state_of(r), s0)
        # depth cuts bound
        r.reset_film()
        r.bind_depth_cuts([1, 2])
        s0 = state_of(r)
        with pytest.raises(RuntimeError, match="drt_render_sample_map.*depth cuts"):
            r.render_sample_map(M)
        assert same_state(state_of(r), s0)
        r.bind_depth_cuts(None)
        # a map that asks for nothing
        before = pydrt.selftest_live_resources()
        rep = r.render_sample_map(np.zeros(P, dtype=np.uint32))
        assert rep == {"rounds": 0, "paths": 0, "pixels_rendered": 0, "pixels_above": 0, "max_count": 0}
        assert not r.read_sample_counts().any() and r.read_active_list().size == 0 and r.stats().paths == 0
        for call in (lambda: r.render(0, 2), lambda: r.write_film(*film0)):
            with pytest.raises(RuntimeError, match="adaptive render"):
                call()
        assert pydrt.selftest_live_resources() != before  # the buffers of a call that went through stay with the context
        r.reset_film()
        r.render(0, 2)  # usable again
    finally:
        r.close()
    for flags, mode in ((pydrt.FLAG_RECORD_HITS, pydrt.MODE_SPECTRAL), (0, pydrt.MODE_XYZ)):
        p = pydrt.make_params(16, 16, spp=8, max_depth=4, flags=flags, mode=mode)
        q = pydrt.Renderer(bundle, p)
        try:
            q.render(0, 4)
            paths, live = q.stats().paths, pydrt.selftest_live_resources()
            with pytest.raises(RuntimeError, match="drt_render_sample_map.*DRT_"):
                q.render_sample_map(np.full(256, 8))
            assert q.stats().paths == paths == 4 * 256 and pydrt.selftest_live_resources() == live
        finally:
            q.close()


def test_downstream_denoiser_features_and_bgra(tmp_path):
    bundle, params = A.case_params("plane_light_48", spp=40)
    W, H = int(params.tile_w), int(params.tile_h)
    M = make_map(W * H)
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_sample_map(M)
        d = r.denoise(radius=2)
        assert d["unusable"] == int((M < 2).sum()) > 0
        with pytest.raises(RuntimeError, match="drt_render_features"):
            r.render_features(0)  # some pixels hold no sample
        rep = r.render_sample_map(np.ones(W * H, dtype=np.uint8), add=True)
        assert rep["rounds"] == 1 and rep["paths"] == W * H
        f = r.render_features(0)
        assert f["rays"] > 0
        film = r.read_film()
        assert np.array_equal(film[0][:, -1], (M + 1).astype(np.float64))
        # the device's BMP bytes against the host conversion of the film that was read
        Hl = pydrt.host_lib()
        f64p = C.POINTER(C.c_double)
        Hl.drt_host_spd_file_to_bmp.argtypes = [C.c_char_p, C.c_char_p, f64p]
        Hl.drt_host_write_spd.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, f64p]
        Hl.drt_host_write_bmp_bgra.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8)]
        sc = bundle.scene
        cmf = np.ascontiguousarray(bundle.spds()[int(sc.cmf_rw):int(sc.cmf_rw) + 4])
        for which, buf, has_filter in ((0, film[0], 1), (1, film[1], 0)):
            spd, host_bmp, dev_bmp = (str(tmp_path / ("%d.%s" % (which, e))).encode() for e in ("spd", "host.bmp", "dev.bmp"))
            buf = np.ascontiguousarray(buf)
            assert Hl.drt_host_write_spd(spd, W, H, int(sc.num_wavelengths), has_filter, float(sc.min_wavelength),
                                         float(sc.wavelength_interval), buf.ctypes.data_as(f64p)) == 0
            assert Hl.drt_host_spd_file_to_bmp(spd, host_bmp, cmf.ctypes.data_as(f64p)) == 0
            bgra = np.ascontiguousarray(r.read_bgra(which))
            assert Hl.drt_host_write_bmp_bgra(dev_bmp, W, H, bgra.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
            assert open(dev_bmp, "rb").read() == open(host_bmp, "rb").read(), which
    finally:
        r.close()


def test_live_resources_return_after_close():
    bundle, params = A.case_params("plane_light_16", spp=8)
    before = pydrt.selftest_live_resources()
    r = pydrt.Renderer(bundle, params)
    try:
        r.render_sample_map(np.arange(256) % 9)
        r.render_sample_map(np.full(256, 2), add=True)
        assert pydrt.selftest_live_resources() != before
    finally:
        r.close()
    assert pydrt.selftest_live_resources() == before
    g = pydrt.Group(bundle, params, [0, 0])
    try:
        g.render_sample_map(np.arange(256) % 9)
    finally:
        g.close()
    assert pydrt.selftest_live_resources() == before


def test_drt_render_program_with_regions(tmp_path):
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    W, H, S, BASE = 32, 24, 69, 3
    regions = [(4, 3, 12, 10, 8), (10, 8, 30, 30, 21)]  # overlapping; the second runs out of the image
    cfg = open(os.path.join(cases.REPO, "config.cfg")).read()
    cfg = cfg.replace("num_pixel_samples 4", "num_pixel_samples %d" % BASE).replace("output_width      800", "output_width      %d" % W)
    cfg = cfg.replace("output_height     600", "output_height     %d" % H).replace("max_cast_depth    4", "max_cast_depth    6")
    bundle = pydrt.load_scene(cases.scene_path("cornell_plane_light.scn"), W, H)
    params = pydrt.make_params(W, H, spp=BASE, max_depth=6, seed=1)
    want = pydrt.region_map(W, H, BASE, regions).reshape(-1)
    assert set(np.unique(want)) == {3, 8, 21} and np.array_equal(want, SM.region_map(W, H, BASE, regions).reshape(-1))
    snaps = A.oracle_snapshots(bundle, params, [3, 8, 21])

    def run(where, env):
        os.makedirs(where / "output")
        for d in ("scenes", "spectra"):
            os.symlink(os.path.join(cases.REPO, d), where / d)
        (where / "config.cfg").write_text(cfg)
        full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
        full.update(env)
        r = subprocess.run([exe], cwd=where, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        out = where / "output"
        return (r.stdout, np.fromfile(out / "output.spd", dtype=np.float64, offset=40).reshape(-1, S + 1),
                np.fromfile(out / "average.spd", dtype=np.float64, offset=40).reshape(-1, S),
                np.fromfile(out / "variance.spd", dtype=np.float64, offset=40).reshape(-1, S))

    spec = ";".join("%d,%d,%d,%d:%d" % r for r in regions)
    text, px, avg, var = run(tmp_path / "a", {"DRT_REGIONS": spec})
    assert "Sample map: 2 regions" in text and "%d paths traced" % int(want.sum()) in text
    epx, eav, eva = A.film_at_counts(snaps, want)
    assert np.array_equal(px[:, S], want.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = eva / np.max(np.maximum(eva, 0.0), axis=1)[:, None]  # the variance is written max-normalised per pixel (host/drt_checkpoint.c)
    A.assert_same_film((px, avg, var), (epx, eav, norm), "DRT_REGIONS")
    bmp = open(tmp_path / "a" / "output" / "output.spd.counts.bmp", "rb").read()
    grey = np.floor(255.0 * want.astype(np.float64) / 21.0 + 0.5).astype(np.uint8)
    bgra = np.frombuffer(bmp[54:], dtype=np.uint8).reshape(-1, 4)
    assert len(bmp) == 54 + W * H * 4 and (bgra[:, :3] == grey[:, None]).all() and (bgra[:, 3] == 255).all()
    assert set(np.unique(grey)) == {36, 97, 255}
    for name in ("output.bmp", "average.bmp", "variance.bmp"):
        assert os.path.getsize(tmp_path / "a" / "output" / name) == 54 + W * H * 4
    # without the variable: the plain render of num_pixel_samples, and no picture of the counts
    text, px, avg, var = run(tmp_path / "b", {})
    assert "Sample map" not in text and not os.path.exists(tmp_path / "b" / "output" / "output.spd.counts.bmp")
    r = pydrt.Renderer(bundle, params)
    try:
        r.render(0, BASE)
        film = r.read_film()
    finally:
        r.close()
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = film[2] / np.max(np.maximum(film[2], 0.0), axis=1)[:, None]
    A.assert_same_film((px, avg, var), (film[0], film[1], norm), "without DRT_REGIONS")
    A.assert_same_film(film, snaps[3], "the plain render against the oracle")
