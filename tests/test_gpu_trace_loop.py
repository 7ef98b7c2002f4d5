"""GPU (-m gpu): the trace kernel's path loop, after it stopped loading anything back behind its record stores (csrc/drt_kernels.h).

What moved: a carried path's vignette -- in ray mode its weight -- is kept in a row of the wave's LDS area from the path's start to
its end instead of being loaded back from the header; the block of the current four vertices and the lanes' statistics (scans,
shaded vertices, draws) live in LDS lane rows (TRACE_LW_*), paths are counted per wave, shadow scans are shaded vertices x lights
and record blocks are what the pool handed out less the spares still held; the scene point carries one swap bit instead of the two
media indices (TraceHit). None of it changes a floating-point operation, so every case here is the oracle's
(cases.oracle_render_device_pow) bit for bit: the three film buffers, the hit log and the five statistics. The cases are the
smallest shapes at which each of these can go wrong; each names what it is there for."""
import numpy as np
import pytest

import cases
import oracle_py as O
import pydrt
import ray_film_cases as R

pytestmark = pytest.mark.gpu

HEADLINE = "cornell_plane_light.scn"
IMAGE = (96, 64)                                       # the tiles below are cut from this image
TILE = dict(x0=24, y0=16, tile_w=48, tile_h=32)        # 1536 pixels: 24 waves' worth of paths per sample
TILE_SPP = 6
ENV = ("DRT_TRACE_TAIL", "DRT_TAIL_RESUME", "DRT_POOL_BLOCKS")

_oracle = {}


def params(spp, depth, seed=5, batch_spp=0, flags=pydrt.FLAG_RECORD_HITS, **tile):
    return pydrt.make_params(IMAGE[0], IMAGE[1], spp=spp, max_depth=depth, seed=seed, batch_spp=batch_spp, flags=flags, **tile)


def headline():
    return pydrt.load_scene(cases.scene_path(HEADLINE), *IMAGE)


def oracle(key, bundle, p, table=None):
    """the oracle's (pixels, means, variances, hit log, statistics) of a case, rendered once and never written to"""
    if key not in _oracle:
        if table is None:
            _oracle[key] = cases.oracle_render_device_pow(bundle, p, want_hits=True, num_threads=16)
        else:
            with O.ray_table(*table):
                _oracle[key] = cases.oracle_render_device_pow(bundle, p, want_hits=True, num_threads=16)
    return _oracle[key]


def device(bundle, p, table=None, sample_map=None):
    r = pydrt.Renderer(bundle, p)
    try:
        if table is not None:
            r.bind_rays(*table)
        if sample_map is not None:
            r.render_sample_map(sample_map)
        else:
            r.render()
        log = None if sample_map is not None else r.read_hit_indices(int(p.spp))
        return r.read_film(), log, r.stats()
    finally:
        r.close()


def check(what, got, want):
    film, log, st = got
    opx, oav, ova, olog, ost = want
    print("%s: device %s oracle %s" % (what, cases.stat_counts(st), cases.stat_counts(ost)))
    for g, w, name in zip(film, (opx, oav, ova), ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s, %s: %s" % (what, name, cases.first_difference(g, w))
    if log is not None:
        assert np.array_equal(log, olog), "%s: the hit log" % what
    assert cases.stat_counts(st) == cases.stat_counts(ost), "%s: statistics" % what
    return st


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def test_a_tile_of_six_pixels_at_one_sample():
    """3 x 2 pixels, 1 spp: six lanes of one wave start a path, the other 58 never write or read their vignette row or their lane words"""
    bundle = headline()
    p = params(1, 8, x0=47, y0=31, tile_w=3, tile_h=2)
    st = check("3 x 2", device(bundle, p), oracle("3x2", bundle, p))
    assert st.paths == 6 and st.path_flags & pydrt.PATH_TRACE_TAIL


WAYS = {"default": {}, "DRT_TRACE_TAIL=0": {"DRT_TRACE_TAIL": "0"}, "DRT_TRACE_TAIL=2": {"DRT_TRACE_TAIL": "2"},
        "DRT_TAIL_RESUME=0": {"DRT_TAIL_RESUME": "0"}}


@pytest.mark.parametrize("way", sorted(WAYS))
@pytest.mark.parametrize("depth", [1, 3, 8])
def test_the_headline_tile(depth, way, monkeypatch):
    """48 x 32 pixels at 6 spp of the headline scene: plastic, mirror, glass and gold, so one wave holds paths that are carried to
    their end, paths that stop being carried (resumed by the tail pass, or with DRT_TAIL_RESUME=0 replayed whole) and, with
    DRT_TRACE_TAIL=0 or 2, the instantiation without the tail rows. Depth 1: every path ends in its first iteration."""
    for var, val in WAYS[way].items():
        monkeypatch.setenv(var, val)
    bundle = headline()
    p = params(TILE_SPP, depth, batch_spp=4, **TILE)
    want = oracle(("tile", depth), bundle, p)
    assert want[4].shaded_vertices > 0 and (depth == 1 or want[4].shaded_vertices > want[4].paths)
    st = check("tile, depth %d, %s" % (depth, way), device(bundle, p), want)
    assert bool(st.path_flags & pydrt.PATH_TRACE_TAIL) == (way in ("default", "DRT_TAIL_RESUME=0"))
    assert st.shadow_scans == st.shaded_vertices  # one light


def test_the_closed_box_at_depth_20():
    """cornell_large_box.scn is closed: paths reach their 13th vertex and take the table-block branch of path_open_vertex, whose
    block ids are read back from the lane's LDS word"""
    bundle = pydrt.load_scene(cases.scene_path("cornell_large_box.scn"), *IMAGE)
    p = params(2, 20, seed=6, x0=40, y0=24, tile_w=16, tile_h=16)
    want = oracle("box20", bundle, p)
    deepest = int((want[3] >= 0).sum(axis=1).max())
    print("closed box: the longest path hits %d surfaces" % deepest)
    assert deepest >= 14, "no path reaches its 13th vertex"
    check("closed box, depth 20", device(bundle, p), want)


def test_many_lights():
    """tests/cases.py's 12-light scene: the instantiation without TAIL; shadow scans = shaded vertices x lights"""
    bundle, q = cases.load_case("many_lights")
    p = R.params_like(q, flags=pydrt.FLAG_RECORD_HITS)
    st = check("many lights", device(bundle, p), oracle("many_lights", bundle, p))
    n_lights = st.shadow_scans // st.shaded_vertices
    assert n_lights > 1 and st.shadow_scans == st.shaded_vertices * n_lights and not st.path_flags & pydrt.PATH_TRACE_TAIL


def test_a_lens():
    """aperture > 0: camera_ray draws for the lens, so a path's draws start before its first vertex"""
    bundle, q = cases.load_case("lens")
    assert float(bundle.camera.aperture_radius) > 0.0
    p = R.params_like(q, flags=pydrt.FLAG_RECORD_HITS)
    check("lens", device(bundle, p), oracle("lens", bundle, p))


def test_the_camera_inside_a_sphere():
    """the camera stands inside the glass ball: the first hit is the ball's inside, where the media are swapped"""
    text = cases.degenerate_scenes()["camera_inside_the_glass_ball"]
    bundle = pydrt.load_scene_text(text, 24, 24)
    p = pydrt.make_params(24, 24, spp=3, max_depth=6, seed=2, flags=pydrt.FLAG_RECORD_HITS)
    want = oracle("inside", bundle, p)
    first = want[3][:, 0]
    ball = int(np.bincount(first[first >= 0]).argmax())
    assert (first == ball).mean() > 0.9 and int(bundle.scene.surfaces[ball].type) == pydrt.GEO_SPHERE
    check("camera inside the glass ball", device(bundle, p), want)


def test_a_ray_film_whose_weights_are_odd_numbers():
    """ray mode: the LDS row holds the ray's weight. -0, a subnormal, +inf and NaN go through the arithmetic as they are"""
    name = "plane_light_center"
    bundle, p = R.load(name)
    o, d, w = R.camera_table(name)
    w = w.copy()
    H, W = w.shape
    odd = {(H // 2, W // 2): -0.0, (H // 2, W // 2 + 1): 5e-324, (H // 2 + 1, W // 2): np.inf, (H // 2 + 1, W // 2 + 1): np.nan, (2, 3): -1.5}
    for at, v in odd.items():
        w[at] = v
    table = (o, d, w)
    want = oracle("odd weights", bundle, p, table)
    film, log, st = device(bundle, p, table)
    assert st.path_flags & pydrt.PATH_RAYS and st.path_flags & pydrt.PATH_TRACE_TAIL
    check("odd weights", (film, log, st), want)
    t = (H // 2 + 1) * W + W // 2 + 1
    assert np.isnan(film[0][t, :-1]).all()


def test_a_sample_map_of_the_tile():
    """the LIST instantiations (slots by list position): a uniform map of 6 is rendered in rounds of 2 and 4 samples and gives the
    uniform film and its counts (a map render keeps no hit log: the library refuses the flag, so none is compared here)"""
    bundle = headline()
    want = oracle(("tile", 8), bundle, params(TILE_SPP, 8, batch_spp=4, **TILE))
    m = np.full((TILE["tile_h"], TILE["tile_w"]), TILE_SPP, dtype=np.uint32)
    check("sample map", device(bundle, params(TILE_SPP, 8, batch_spp=4, flags=0, **TILE), sample_map=m), want)


def test_a_tiny_record_pool(monkeypatch):
    """DRT_POOL_BLOCKS=1: launches run out of record blocks, their paths are cut short (HDR_TERM_NOT_DONE) and rendered again in
    worst-case-sized launches: the film without it, and the statistics -- a launch's counts join the totals only when it was complete"""
    bundle = headline()
    p = params(TILE_SPP, 8, batch_spp=6, **TILE)
    want = oracle(("tile", 8), bundle, params(TILE_SPP, 8, batch_spp=4, **TILE))
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    st = check("tiny pool", device(bundle, p), want)
    assert st.redone_launches >= 1, "no launch ran out of record blocks"
