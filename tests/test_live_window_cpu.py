"""CPU: the live window's rule (csrc/drt_window_rule.h through the host-only drt_live_window_of). No GPU.

Conservative: no camera ray of a tile pixel outside the window hits anything -- the four film-corner rays and the centre ray of every
such pixel through the CPU oracle's ray tables, and the oracle's own render with its hit log. Tight: the headline window is the
geometry's 651.7 (of 1024) pixels, rounding and one guard pixel a side on top. Off: the cameras and materials for which the rule must
answer the whole tile, and the empty window of a scene wholly off screen."""
import numpy as np
import pytest

import live_window_cases as W
import oracle_py as O
import pydrt

CASES = [(s, w, h, c) for s in W.SCENES for (w, h) in W.SIZES for c in W.CAMERAS]


def params_of(w, h, spp=1, depth=1, **kw):
    return pydrt.make_params(w, h, spp=spp, max_depth=depth, seed=3, **kw)


@pytest.mark.parametrize("scene,w,h,camera", CASES, ids=["%s-%dx%d-%s" % (s.replace(".scn", ""), w, h, c) for s, w, h, c in CASES])
def test_conservative(scene, w, h, camera):
    bundle = W.load(scene, w, h, camera)
    win = pydrt.live_window_of(bundle, params_of(w, h))
    outside = W.outside_mask(win, params_of(w, h))
    if camera == "inside":
        assert win == (0, w, 0, h)
    if camera == "shipped" and scene in ("cornell_plane_light.scn", "cornell_gold_mirror.scn"):  # (cornell_large_box's camera is inside its box)
        assert outside.sum() > outside.size // 4, "the shipped camera of %s leaves no pixel outside its window %s" % (scene, win)
    if not outside.any():
        return
    # the four corner rays and the centre ray of every pixel: sample l of the oracle's ray-mode render is table layer l
    o, d = W.corner_ray_tables(bundle.camera, w, h)
    with O.ray_table(o, d):
        hits = O.oracle_render_tile(bundle, params_of(w, h, spp=5), want_hits=True, math_mode=O.MATH_DEVICE)[3]
    hits = hits.reshape(5, h, w)
    bad = np.argwhere((hits != -1) & outside[None])
    assert not len(bad), "window %s: %d corner / centre rays outside it hit, first (layer, y, x) %s" % (win, len(bad), bad[0])
    # the render's own camera rays, four random samples a pixel
    hits = O.oracle_render_tile(bundle, params_of(w, h, spp=4), want_hits=True, math_mode=O.MATH_DEVICE)[3].reshape(4, h, w)
    bad = np.argwhere((hits != -1) & outside[None])
    assert not len(bad), "window %s: %d camera rays outside it hit, first (sample, y, x) %s" % (win, len(bad), bad[0])


@pytest.mark.parametrize("size,limit", [(1024, 656), (96, 66)])
def test_tight(size, limit):
    bundle = W.load("cornell_plane_light.scn", size, size)
    x_lo, x_hi, y_lo, y_hi = pydrt.live_window_of(bundle, params_of(size, size))
    assert 0 < x_hi - x_lo <= limit and 0 < y_hi - y_lo <= limit, (x_lo, x_hi, y_lo, y_hi)
    # ... and it is centred: the camera looks down the box's axis
    assert x_lo + x_hi == size and y_lo + y_hi == size


def test_tile_clips_the_window():
    bundle = W.load("cornell_plane_light.scn", 96, 96)
    whole = pydrt.live_window_of(bundle, params_of(96, 96))
    p = params_of(96, 96, x0=20, y0=5, tile_w=40, tile_h=30, row_stride=2)
    win = pydrt.live_window_of(bundle, p)
    assert win == (max(whole[0], 20), min(whole[1], 60), max(whole[2], 5), min(whole[3], 5 + 29 * 2 + 1))


def test_off():
    w = h = 96
    p = params_of(w, h)
    bundle = W.load("cornell_plane_light.scn", w, h)
    assert pydrt.live_window_of(bundle, p) != W.whole_tile(p)
    lens = pydrt.Camera.from_buffer_copy(bundle.camera)
    lens.aperture_radius = 0.1
    assert pydrt.live_window_of(bundle, p, camera=lens) == W.whole_tile(p), "a lens camera"

    def emissive(mats, sc):
        mats[sc.escape_material].is_emissive = 1
    assert pydrt.live_window_of(W.with_materials(bundle, emissive), p) == W.whole_tile(p), "an emissive escape material"

    def no_black_body(mats, sc):
        mats[sc.escape_material].is_black_body = 0
    assert pydrt.live_window_of(W.with_materials(bundle, no_black_body), p) == W.whole_tile(p), "an escape material that is no black body"
    assert pydrt.live_window_of(W.load("cornell_plane_light.scn", w, h, "inside"), p) == W.whole_tile(p), "a camera inside the box"
    assert pydrt.live_window_of(W.load("cornell_plane_light.scn", w, h, "sideways"), p) == W.whole_tile(p), "a scene corner behind the pinhole"
    nan = pydrt.Camera.from_buffer_copy(bundle.camera)
    nan.forward[1] = float("nan")
    assert pydrt.live_window_of(bundle, p, camera=nan) == W.whole_tile(p), "a coordinate that is not finite"
    tile = params_of(w, h, x0=8, y0=3, tile_w=50, tile_h=20, row_stride=3)
    assert pydrt.live_window_of(bundle, tile, camera=lens) == W.whole_tile(tile) == (8, 58, 3, 61)


def test_empty():
    w = h = 96
    bundle = W.load("cornell_plane_light.scn", w, h, "off_screen")
    win = pydrt.live_window_of(bundle, params_of(w, h))
    assert win[0] == win[1] and win[2] == win[3], win
    hits = O.oracle_render_tile(bundle, params_of(w, h, spp=4), want_hits=True, math_mode=O.MATH_DEVICE)[3]
    assert (hits == -1).all()
