"""GPU (-m gpu): the trace kernel's ray stash (csrc/drt_kernels.h, csrc/drt_stash_rule.h).

drt_trace_kernel makes the starts of a wave's next 64 path ids in one go -- pixel and sample, generator state, camera ray, vignette --
and an idle lane picks its entry up; drt_trace_direct_kernel (DRT_NO_RAY_STASH=1, or a block without room for the stash) computes a
start in the lane that falls idle, as before. Same ids to the same lanes, the same operations on the same values: every case here is
the oracle's (cases.oracle_render_device_pow) bit for bit -- the three film buffers, the hit log and the five statistics -- in both
forms, and the reported flag (PATH_RAY_STASH) says which form ran. The cases are the smallest shapes at which a fill, a pick-up or
the hand-out between them can go wrong, on test_gpu_trace_loop's image and tiles; each names what it is there for."""
import numpy as np
import pytest

import cases
import oracle_py as O
import pydrt
import ray_film_cases as R

pytestmark = pytest.mark.gpu

HEADLINE = "cornell_plane_light.scn"
IMAGE = (96, 64)
TILE = dict(x0=24, y0=16, tile_w=48, tile_h=32)  # 1536 pixels
TILE_SPP = 6
ENV = ("DRT_NO_RAY_STASH", "DRT_TRACE_CHUNK", "DRT_TRACE_TAIL", "DRT_POOL_BLOCKS")
FORMS = {"stash": None, "direct": "1"}  # DRT_NO_RAY_STASH

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


def check(what, got, want, stats=True):
    film, log, st = got
    opx, oav, ova, olog, ost = want
    print("%s: device %s oracle %s, path flags %#x" % (what, cases.stat_counts(st), cases.stat_counts(ost), st.path_flags))
    for g, w, name in zip(film, (opx, oav, ova), ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s, %s: %s" % (what, name, cases.first_difference(g, w))
    if log is not None:
        assert np.array_equal(log, olog), "%s: the hit log" % what
    if stats:
        assert cases.stat_counts(st) == cases.stat_counts(ost), "%s: statistics" % what
    return st


def ran(st, form, stash_possible=True):
    """the reported flag names the form that ran"""
    assert bool(st.path_flags & pydrt.PATH_RAY_STASH) == (form == "stash" and stash_possible), "%s: path flags %#x" % (form, st.path_flags)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


@pytest.fixture(params=sorted(FORMS))
def form(request, monkeypatch):
    if FORMS[request.param] is not None:
        monkeypatch.setenv("DRT_NO_RAY_STASH", FORMS[request.param])
    return request.param


# name: (tile, spp, depth, what it is there for)
SHAPES = {
    "3x2 at 1 spp": (dict(x0=47, y0=31, tile_w=3, tile_h=2), 1, 8, "one fill with 6 valid entries and 58 lanes that store nothing"),
    "64 paths": (dict(x0=40, y0=24, tile_w=8, tile_h=8), 1, 8, "one full fill, then the counter is used up"),
    "65 paths": (dict(x0=40, y0=24, tile_w=13, tile_h=5), 1, 8, "a second fill of one entry"),
    "127 paths": (dict(x0=47, y0=31, tile_w=1, tile_h=1), 127, 8, "a full fill and a short last one (two launches of at most 65 samples); one pixel, more samples than lanes"),
    "3 spp": (TILE, 3, 3, "a fill spans 22 pixels"),
    "65 spp on 4x2": (dict(x0=46, y0=30, tile_w=4, tile_h=2), 65, 4, "a pixel boundary inside a fill, more samples than lanes"),
    "depth 1": (TILE, TILE_SPP, 1, "every lane ends every iteration: the stash is emptied 64 at a time"),
    "depth 8": (TILE, TILE_SPP, 8, "the steady state of a few pick-ups per iteration"),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_a_shape_of_fills_and_pick_ups(name, form):
    tile, spp, depth, why = SHAPES[name]
    bundle = headline()
    p = params(spp, depth, batch_spp=min(spp, 65) if tile is not TILE else 4, **tile)
    st = check("%s (%s), %s" % (name, why, form), device(bundle, p), oracle((name,), bundle, p))
    assert st.paths == tile["tile_w"] * tile["tile_h"] * spp
    ran(st, form)


def test_a_new_chunk_at_every_fill(form, monkeypatch):
    """DRT_TRACE_CHUNK=64 on the 48 x 32 tile at 6 spp: every fill draws from the work counter first"""
    monkeypatch.setenv("DRT_TRACE_CHUNK", "64")
    bundle = headline()
    p = params(TILE_SPP, 8, batch_spp=4, **TILE)
    ran(check("chunks of 64, %s" % form, device(bundle, p), oracle(("depth 8",), bundle, p)), form)


def test_without_tail_rows(form, monkeypatch):
    """DRT_TRACE_TAIL=0: the instantiation without tail rows, the stash right behind the lane rows"""
    monkeypatch.setenv("DRT_TRACE_TAIL", "0")
    bundle = headline()
    p = params(TILE_SPP, 8, batch_spp=4, **TILE)
    st = check("no tail rows, %s" % form, device(bundle, p), oracle(("depth 8",), bundle, p))
    assert not st.path_flags & pydrt.PATH_TRACE_TAIL
    ran(st, form)


def test_a_lens(form):
    """test_lens.scn, aperture 0.05: the lens sampler rejects, so draw counts differ per entry; they are counted at pick-up"""
    bundle, q = cases.load_case("lens")
    assert float(bundle.camera.aperture_radius) > 0.0
    p = R.params_like(q, flags=pydrt.FLAG_RECORD_HITS)
    ran(check("lens, %s" % form, device(bundle, p), oracle("lens", bundle, p)), form)


def test_the_centre_pixel_scheme(form):
    """no draw before the first vertex: the stashed generator state is the key's"""
    bundle, q = cases.load_case("plane_light_center")
    assert int(q.pixel_scheme) == pydrt.FILM_SAMPLE_CENTER
    p = R.params_like(q, flags=pydrt.FLAG_RECORD_HITS)
    ran(check("centre scheme, %s" % form, device(bundle, p), oracle("centre", bundle, p)), form)


def test_a_sample_map_with_two_counts(form):
    """the LIST instantiations: the left half of the tile to 3 samples, the right half to 6, in rounds, so a round's fill reads
    pixel_list and a per-pixel sample_base. A pixel rendered over samples 0 .. n-1 holds the film a uniform n-sample render gives
    it (a map render keeps no hit log and its statistics are the map's, so films only)"""
    bundle = headline()
    three = oracle(("3 spp at depth 8",), bundle, params(3, 8, batch_spp=4, **TILE))
    six = oracle(("depth 8",), bundle, params(TILE_SPP, 8, batch_spp=4, **TILE))
    m = np.full((TILE["tile_h"], TILE["tile_w"]), 3, dtype=np.uint32)
    m[:, TILE["tile_w"] // 2:] = 6
    film, _, st = device(bundle, params(TILE_SPP, 8, batch_spp=4, flags=0, **TILE), sample_map=m)
    right = (m.reshape(-1) == 6)
    for g, a, b, name in zip(film, three[:3], six[:3], ("pixels", "means", "variances")):
        want = np.where(right[:, None], b, a)
        assert cases.same_bits(g, want), "sample map, %s, %s: %s" % (form, name, cases.first_difference(g, want))
    assert st.paths == int(m.sum())
    ran(st, form)


def test_a_bound_ray_table_keeps_the_direct_start(form):
    """ray mode: table_ray is three loads, drt_trace_rays_kernel starts its paths directly whatever the switch says (one kernel text
    for both forms of the context: the flags without PATH_RAYS are the camera render's, as test_gpu_ray_film holds them)"""
    name = "plane_light_center"
    bundle, p = R.load(name)
    table = R.camera_table(name)
    st = check("ray table, %s" % form, device(bundle, p, table), oracle("table", bundle, p, table))
    assert st.path_flags & pydrt.PATH_RAYS  # which says the ray-mode kernel ran; the stash flag stays the context's, as PATH_TRACE_TAIL does
    ran(st, form)


def test_a_record_pool_that_runs_out(form, monkeypatch):
    """DRT_POOL_BLOCKS=1: launches run out of record blocks with entries in the stash, their paths are cut short and rendered
    again: the film and the hit log without it, and the statistics -- a launch's counts join the totals only when it was complete"""
    bundle = headline()
    p = params(TILE_SPP, 8, batch_spp=6, **TILE)
    want = oracle(("depth 8",), bundle, params(TILE_SPP, 8, batch_spp=4, **TILE))
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    st = check("tiny pool, %s" % form, device(bundle, p), want)
    assert st.redone_launches >= 1, "no launch ran out of record blocks"
    ran(st, form)


def crowded_headline(n_balls):
    """the headline scene with n_balls small plastic and mirror balls more on a grid above the floor: one light still, so the tail
    rows stay, and the surface tables grow by 256 bytes of LDS a ball"""
    text = open(cases.scene_path(HEADLINE)).read()
    mats = ("white_plastic", "teal_plastic", "mirror", "red_plastic")
    for k in range(n_balls):
        x, y, z = -2.5 + 0.55 * (k % 10), -2.7 + 0.6 * (k // 30), -2.0 + 1.2 * ((k // 10) % 3)
        text += "\nSurface\nname extra%d\ntype sphere\nposition %.3f, %.3f, %.3f\nradius 0.2\nmaterial %s\n" % (k, x, y, z, mats[k % 4])
    return text


def test_a_scene_whose_block_has_no_room_for_the_stash(form):
    """69 surfaces: scanned out of LDS with the tail rows (scene_in_lds and the tail rule are defined on what they were), but
    the block with 20 KB of stash would be over 64 KB, so the launcher keeps the direct form and says so"""
    bundle = pydrt.load_scene_text(crowded_headline(60), *IMAGE)
    p = params(2, 6, seed=9, x0=32, y0=24, tile_w=32, tile_h=16)
    st = check("crowded, %s" % form, device(bundle, p), oracle("crowded", bundle, p))
    assert not st.path_flags & pydrt.PATH_BVH and st.path_flags & pydrt.PATH_TRACE_TAIL
    ran(st, form, stash_possible=False)
