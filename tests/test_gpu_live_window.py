"""GPU (-m gpu): the live window (include/drt_hip.h, drt_live_window). Dense renders trace and shade the window's
pixels only and fill the rest; nothing a caller can read may change. Every case is at most 96 x 96, 8 samples a call, depth 4, and is
compared bit for bit -- film (sum + filter, mean, variance: cases.same_bits), the counting statistics (==) and the wrap-around
checksums bench.py takes of a frame -- three ways: against the same calls under DRT_NO_LIVE_WINDOW=1, against the oracle, and against
a fresh context that renders the same samples in one call.

DRT_MODE_XYZ folds the spectrum per kernel pair, which the oracle does not restate: that case compares its eight accumulators bit for
bit with the window off and with a fresh context, and its XYZ with the oracle's to 1e-9 relative, the bound tests/test_gpu_parity.py
holds that mode to. drt_render_tile goes out in row blocks only from 2^18 pixels on: at 64 x 48 the one-shot case runs the plain
path, and test_one_shot_call_in_row_blocks, the one case above 96 x 96 (512 x 512, 2 M paths), is the row blocks' own. Row blocks of
drt_render at the small size: the batch_spp = 2 case; with a record pool that runs out under them: test_tiny_pool_redoes_windowed_row_blocks,
at the 96 x 200, 23 samples and depth 7 of tests/test_gpu_parity.py's row-block case."""
import contextlib
import os

import numpy as np
import pytest

import cases
import live_window_cases as W
import pydrt

pytestmark = pytest.mark.gpu

SPP, DEPTH = 8, 4


def params_of(w, h, spp=SPP, **kw):
    return pydrt.make_params(w, h, spp=spp, max_depth=DEPTH, seed=5, **kw)


@contextlib.contextmanager
def environment(**env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def checksums(film):
    return tuple(int(np.ascontiguousarray(a).view(np.int64).sum()) for a in film)


def run(bundle, params, calls=((0, SPP),), window=True, preload=None, move_to=None, want_window=None, env=None):
    """(film, counts, window, stats) of a context that renders `calls` (first_sample, n); preload: a film written first; move_to: a
    camera set on the live context before anything is rendered. The variables in `env` are read when the context is created."""
    with environment(DRT_NO_LIVE_WINDOW="0" if window else "1", **(env or {})):
        r = pydrt.Renderer(bundle, params)
    try:
        if move_to is not None:
            r.set_camera(move_to)
        if preload is not None:
            r.write_film(*preload)
        win = r.live_window()
        if want_window is not None and window:
            assert win == want_window, "the context's window %s, drt_live_window_of %s" % (win, want_window)
        for first, n in calls:
            r.render(first, n)
        film = (r.read_xyz_film(),) if int(params.mode) == pydrt.MODE_XYZ else r.read_film()
        st = r.stats()
        return film, cases.stat_counts(st), win, st
    finally:
        r.close()


def assert_same(got, want, what):
    for name, a, b in zip(("pixels", "avgs", "vars"), got[0], want[0]):
        assert cases.same_bits(a, b), "%s, %s: %s" % (what, name, cases.first_difference(a, b))
    assert checksums(got[0]) == checksums(want[0]) or any(np.isnan(a).any() for a in got[0]), what + ": checksums"
    assert got[1] == want[1], "%s: counts %s against %s" % (what, got[1], want[1])


def three_ways(bundle, params, calls=((0, SPP),), preload=None, start=None, want_part=True, env=None):
    """the scenario with the window, without it, as the oracle renders it, and in a fresh context; returns the windowed run.
    start: the bundle the live context is created on before its camera is moved to `bundle`'s."""
    total = sum(n for _, n in calls)
    first = calls[0][0]
    win_of = pydrt.live_window_of(bundle, params)
    part = win_of != W.whole_tile(params)
    assert part == want_part, "window %s of tile %s" % (win_of, W.whole_tile(params))
    kw = dict(calls=calls, preload=preload, env=env)
    if start is not None:
        kw["move_to"] = bundle.camera
    on = run(start or bundle, params, want_window=win_of, **kw)
    off = run(start or bundle, params, window=False, **kw)
    assert off[2] == W.whole_tile(params)
    assert_same(on, off, "against DRT_NO_LIVE_WINDOW=1")
    po = params_of(int(params.width), int(params.height), spp=total, x0=int(params.x0), y0=int(params.y0), tile_w=int(params.tile_w),
                   tile_h=int(params.tile_h), row_stride=int(params.row_stride), first_sample=first, pixel_scheme=int(params.pixel_scheme))
    opx, oav, ova, _, ost = cases.oracle_render_device_pow(bundle, po, film=preload, num_threads=8)
    assert_same(on, ((opx, oav, ova), cases.stat_counts(ost)), "against the oracle")
    fresh = run(bundle, params, calls=((first, total),), preload=preload)
    assert_same(on, fresh, "against a fresh context")
    return on


def test_headline_scene():
    p = params_of(96, 96)
    on = three_ways(W.load("cornell_plane_light.scn", 96, 96), p)
    assert on[1][0] == 96 * 96 * SPP


def test_gold_mirror_scene():
    three_ways(W.load("cornell_gold_mirror.scn", 64, 48), params_of(64, 48))


def test_rolled_camera():
    three_ways(W.load("cornell_plane_light.scn", 64, 48, "rolled30"), params_of(64, 48))


def test_camera_inside_the_box():
    three_ways(W.load("cornell_plane_light.scn", 48, 48, "inside"), params_of(48, 48), want_part=False)


def test_scene_off_screen():
    bundle = W.load("cornell_plane_light.scn", 48, 48, "off_screen")
    win = pydrt.live_window_of(bundle, params_of(48, 48))
    assert win[0] == win[1]
    on = three_ways(bundle, params_of(48, 48))
    assert on[1] == (48 * 48 * SPP, 48 * 48 * SPP, 0, 0, 2 * 48 * 48 * SPP)  # fill only: a path, a scan and two draws each
    assert not on[0][0][:, :-1].any() and (on[0][0][:, -1] == SPP).all()


def test_offset_tile_with_row_stride():
    p = params_of(96, 96, x0=4, y0=3, tile_w=60, tile_h=40, row_stride=2)
    bundle = W.load("cornell_plane_light.scn", 96, 96)
    win = pydrt.live_window_of(bundle, p)
    assert 4 < win[0] and win[1] == 64 and 3 < win[2] and win[3] < 3 + 39 * 2 + 1, win  # cut on three sides, by the tile on the fourth
    three_ways(bundle, p)


def test_two_render_calls():
    three_ways(W.load("cornell_plane_light.scn", 64, 48), params_of(64, 48), calls=((0, SPP), (SPP, SPP)))


def test_row_blocks():
    """two samples a pair and 96 rows: drt_render goes out in row blocks, each between its own two copies of its part of the window"""
    three_ways(W.load("cornell_plane_light.scn", 96, 96), params_of(96, 96, batch_spp=2))


def test_center_scheme():
    """(the RANDOM scheme is every other case's: there a dead path counts its two pixel draws, here none)"""
    three_ways(W.load("cornell_plane_light.scn", 64, 48), params_of(64, 48, pixel_scheme=pydrt.FILM_SAMPLE_CENTER))


def test_preloaded_film():
    """a film the caller wrote: outside the window its rows get the update of eight samples worth +0, as the reference leaves them"""
    bundle = W.load("cornell_plane_light.scn", 64, 48)
    rng = np.random.default_rng(11)
    n, S = 64 * 48, bundle.S
    px, av, va = rng.uniform(0.5, 1.5, (n, S + 1)), rng.uniform(0.5, 1.5, (n, S)), rng.uniform(0.5, 1.5, (n, S))
    px[:, S] = rng.integers(1, 5, n)  # the filter sum is a count: the kernels add a pair's samples to it at once, the reference one by one
    av[::7, ::3] = -0.0  # zeros of either sign among them: x + (+0) makes -0 a +0
    px[::5, :S:4] = 0.0
    on = three_ways(bundle, params_of(64, 48), preload=(px, av, va))
    assert not cases.same_bits(on[0][1][0], av[0])  # (a corner pixel, outside the window: its mean has moved towards 0)


def test_xyz_film():
    bundle = W.load("cornell_plane_light.scn", 64, 48)
    p = params_of(64, 48, mode=pydrt.MODE_XYZ)
    assert pydrt.live_window_of(bundle, p) != W.whole_tile(p)
    on, off, fresh = run(bundle, p, calls=((0, 4), (4, 4))), run(bundle, p, calls=((0, 4), (4, 4)), window=False), run(bundle, p, calls=((0, 4), (4, 4)))
    for other, what in ((off, "DRT_NO_LIVE_WINDOW=1"), (fresh, "a fresh context")):
        assert cases.same_bits(on[0][0], other[0][0]), "%s: %s" % (what, cases.first_difference(on[0][0], other[0][0]))
        assert on[1] == other[1] and checksums(on[0]) == checksums(other[0])
    opx, _, _, _, ost = cases.oracle_render_device_pow(bundle, params_of(64, 48), num_threads=8)
    assert on[1] == cases.stat_counts(ost)
    import oracle_py as O
    want = O.oracle_film_to_xyz(bundle, opx)
    with environment(DRT_NO_LIVE_WINDOW="0"):
        r = pydrt.Renderer(bundle, p)
    try:
        r.render(0, SPP)
        got = r.read_xyz()
    finally:
        r.close()
    assert cases.xyz_rel_err(got, want) <= 1e-9


def test_set_camera_moves_the_window():
    start = W.load("cornell_plane_light.scn", 64, 48)
    moved = W.load("cornell_plane_light.scn", 64, 48, "off_axis")
    p = params_of(64, 48)
    assert pydrt.live_window_of(start, p) != pydrt.live_window_of(moved, p)
    three_ways(moved, p, start=start)
    # ... and into the box: the window is the whole tile from then on
    three_ways(W.load("cornell_plane_light.scn", 64, 48, "inside"), p, start=start, want_part=False)


def test_hierarchy_scene():
    bundle = pydrt.synthetic_sphere_scene(1500, 48, 48)
    far = W.with_camera(bundle, W.camera_variant(bundle, 48, 48, "twice_distance"))
    p = params_of(48, 48)
    on = three_ways(far, p)
    assert on[3].path_flags & pydrt.PATH_BVH


def test_tiny_pool_redoes_windowed_pairs():
    bundle = W.load("cornell_plane_light.scn", 96, 96)
    on = three_ways(bundle, params_of(96, 96), env={"DRT_POOL_BLOCKS": "1"})
    assert on[3].redone_launches >= 1, "the pool of %d blocks did not run out (peak %d)" % (on[3].record_pool_blocks, on[3].record_pool_peak)


def test_tiny_pool_redoes_windowed_row_blocks():
    """The three at once: a window that is a proper part of the tile, a drt_render call that goes out in row blocks (the shape of
    test_render_in_row_blocks_is_the_same_film: 12 blocks of 17 rows, 12 + 11 samples each) and a record pool that runs out, so that
    pairs over a block's rows are rendered again as windowed pairs -- the rows window_copy stages, the rows the pair's kernels see and
    the rows the fill pass takes must be the same rows."""
    bundle = W.load("cornell_plane_light.scn", 96, 200)
    p = pydrt.make_params(96, 200, spp=23, max_depth=7, seed=2, batch_spp=3)
    win = pydrt.live_window_of(bundle, p)
    assert win != W.whole_tile(p) and win[0] < win[1] and win[2] < win[3], win
    on = run(bundle, p, calls=((0, 23),), want_window=win, env={"DRT_POOL_BLOCKS": "1"})
    opx, oav, ova, _, ost = cases.oracle_render_device_pow(bundle, p, num_threads=16)
    assert_same(on, ((opx, oav, ova), cases.stat_counts(ost)), "against the oracle")
    assert on[3].paths == 96 * 200 * 23
    assert on[3].redone_launches > 0, "the pool of %d blocks did not run out (peak %d)" % (on[3].record_pool_blocks, on[3].record_pool_peak)


def test_one_shot_call():
    bundle = W.load("cornell_plane_light.scn", 64, 48)
    p = params_of(64, 48)
    want = run(bundle, p, window=False)
    for flags in (pydrt.FLAG_FILM_ZERO, 0):
        p1 = params_of(64, 48, flags=flags)
        px, av, va, st = pydrt.render_tile(bundle, p1)
        assert_same(((px, av, va), cases.stat_counts(st)), want, "drt_render_tile flags %d" % flags)
    opx, oav, ova, _, ost = cases.oracle_render_device_pow(bundle, p, num_threads=8)
    assert_same(want, ((opx, oav, ova), cases.stat_counts(ost)), "against the oracle")


def test_one_shot_call_in_row_blocks():
    """drt_render_tile goes out in row blocks from 2^18 tile pixels on (the one case far above the 96 x 96 of the others): each block stages
    and returns its own part of the window, and its film rows are fetched when its event fires. With the window against without it;
    the oracle holds three bands of rows (above the window, across its upper edge, through its middle)."""
    size = 512
    bundle = W.load("cornell_plane_light.scn", size, size)
    p = params_of(size, size, batch_spp=4, flags=pydrt.FLAG_FILM_ZERO)
    win = pydrt.live_window_of(bundle, p)
    assert win != W.whole_tile(p) and win[2] > 8
    films = {}
    for window in (True, False):
        with environment(DRT_NO_LIVE_WINDOW="0" if window else "1"):
            px, av, va, st = pydrt.render_tile(bundle, p)
        assert st.redone_launches == 0
        films[window] = ((px, av, va), cases.stat_counts(st))
    assert_same(films[True], films[False], "drt_render_tile in row blocks against DRT_NO_LIVE_WINDOW=1")
    for y0 in (0, win[2] - 4, size // 2):
        band = params_of(size, size, y0=y0, tile_h=8)
        o = cases.oracle_render_device_pow(bundle, band, num_threads=16)
        rows = slice(y0 * size, (y0 + 8) * size)
        for name, a, b in zip(("pixels", "avgs", "vars"), films[True][0], o[:3]):
            assert cases.same_bits(a[rows], b), "rows %d.. %s: %s" % (y0, name, cases.first_difference(a[rows], b))
