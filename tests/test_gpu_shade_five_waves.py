"""GPU (-m gpu): the closed shade kernel's form with window headers and one record slot in the wave's LDS region, five waves per SIMD
(csrc/drt_kernels.h, drt_shade_kernel_closed_lds) -- against the CPU oracle, the closed kernel with headers in registers and the
general instantiation.

Every film here is bit for bit the oracle's (cases.oracle_render_device_pow) and bit for bit the film of the same render with
DRT_NO_CLOSED_LDS=1 (the closed kernel with headers in registers, two slots, four waves) and with DRT_NO_CLOSED_SHADE=1 (the general
instantiation). Renderer.shade_closed_lds() says which closed kernel a context launches.

The shapes are the smallest at which the new paths can go wrong: a 16 x 8 tile of cornell_plane_light and of cornell_gold_mirror in a
64 x 64 image, at the lower right corner of the box, where 63 of the 128 pixels see nothing at all and the others see plastic walls, the
mirror, the glass and the gold -- every list the closed kernel has a body for, at vertex indices up to 19 when the depth is 20.
  - samples per launch 1, 2, 63, 64, 65, 129: the edges of the 64-sample header window, and a last window of one sample;
  - max depth 8 and 20: vertices 8 and up take header word 3, which the window no longer loads, vertices 16 and up the block table;
  - DRT_DARK_SKIP forced on and off: a window that is skipped whole must not leave a header or a slot behind for the next one;
  - one workgroup for the whole launch (DRT_RESERVE_BLOCKS): a wave then takes a tail item directly after a main-pass piece and the
    reverse, in the one LDS region both passes use;
  - DRT_TAIL_RESUME=0 once: the tail pass replays every path from its first vertex.
The oracle's own counts say that no case passes empty."""
import numpy as np
import pytest

import cases
import pydrt
import test_gpu_fixed_lists as FL

pytestmark = pytest.mark.gpu

SCENES = ("cornell_plane_light.scn", "cornell_gold_mirror.scn")
SIZE, TILE = 64, dict(x0=40, y0=48, tile_w=16, tile_h=8)
SAMPLES = (1, 2, 63, 64, 65, 129)
DEPTHS = (8, 20)
KNOBS = ("DRT_NO_CLOSED_SHADE", "DRT_NO_CLOSED_LDS", "DRT_DARK_SKIP", "DRT_RESERVE_BLOCKS", "DRT_TAIL_RESUME")

_bundles, _oracles = {}, {}


def bundle_of(scene):
    if scene not in _bundles:
        _bundles[scene] = pydrt.load_scene(cases.scene_path(scene), SIZE, SIZE)
    return _bundles[scene]


def params(n, depth):
    """one launch of n samples of the tile's pixels"""
    return pydrt.make_params(SIZE, SIZE, spp=n, max_depth=depth, seed=5, batch_spp=n, **TILE)


def oracle(scene, n, depth):
    """the oracle's film, hit log and statistics of a case, rendered once and shared (never written to)"""
    key = (scene, n, depth)
    if key not in _oracles:
        _oracles[key] = cases.oracle_render_device_pow(bundle_of(scene), params(n, depth), want_hits=True, num_threads=16)
    return _oracles[key]


def render(scene, n, depth, want, lds):
    """`want`: the instantiation the context must say it launches; `lds`: ... and whether in the form with headers in LDS"""
    r = pydrt.Renderer(bundle_of(scene), params(n, depth))
    try:
        assert r.shade_instantiation() == want, "the context launches the %s instantiation, not the %s one" % (r.shade_instantiation(), want)
        assert r.shade_closed_lds() == lds
        r.render()
        return r.read_film(), r.stats()
    finally:
        r.close()


def assert_is_the_oracles(scene, n, depth, got, what):
    film, st = got
    opx, oav, ova, _, ost = oracle(scene, n, depth)
    assert cases.stat_counts(st) == cases.stat_counts(ost), what
    for g, w, name in zip(film, (opx, oav, ova), ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s against the oracle, %s: %s" % (what, name, cases.first_difference(g, w))


def assert_same(a, b, what):
    for x, y, name in zip(a[0], b[0], ("pixels", "means", "variances")):
        assert cases.same_bits(x, y), "%s, %s: %s" % (what, name, cases.first_difference(x, y))
    assert cases.stat_counts(a[1]) == cases.stat_counts(b[1]), what


def clear(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def closed_and_general(scene, n, depth, monkeypatch, what):
    """the film of the closed kernel with headers in LDS: the oracle's, the other closed kernel's, and the general instantiation's"""
    monkeypatch.delenv("DRT_NO_CLOSED_SHADE", raising=False)
    monkeypatch.delenv("DRT_NO_CLOSED_LDS", raising=False)
    closed = render(scene, n, depth, "closed", True)
    assert_is_the_oracles(scene, n, depth, closed, what)
    for name, want in (("DRT_NO_CLOSED_LDS", "closed"), ("DRT_NO_CLOSED_SHADE", "general")):
        monkeypatch.setenv(name, "1")
        other = render(scene, n, depth, want, False)
        monkeypatch.delenv(name)
        assert_same(closed, other, "%s, default against %s=1" % (what, name))
    return closed


@pytest.mark.parametrize("scene", SCENES)
def test_the_tile_holds_what_the_cases_are_there_for(scene):
    """pixels nothing reaches beside pixels that are hit, every list of the closed kernel, and both deep bands at depth 20"""
    opx, _, _, ohits, ost = oracle(scene, 65, 20)
    dark = int((opx[:, :-1] == 0).all(axis=1).sum())
    assert 32 <= dark <= 96, "%d of %d pixels stay dark" % (dark, opx.shape[0])
    classes, n_shaded = FL.vertex_classes(bundle_of(scene), ohits)
    assert n_shaded == ost.shaded_vertices
    gold = FL.GGX if scene == SCENES[0] else FL.CONDUCTOR
    for lst in (FL.PLASTIC, FL.MIRROR, FL.GLASS, gold):
        v = classes.get(lst, np.zeros(0))
        print("%s: %s: %d vertices, %d at index >= 8, %d at index >= 16" % (scene, lst, len(v), int((v >= 8).sum()), int((v >= 16).sum())))
        assert len(v) >= 200 and int((v >= 8).sum()) >= 50 and int((v >= 16).sum()) >= 5, (scene, lst)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("n", SAMPLES)
@pytest.mark.parametrize("scene", SCENES)
def test_window_edges_and_deep_vertices(scene, n, depth, monkeypatch):
    clear(monkeypatch)
    closed_and_general(scene, n, depth, monkeypatch, "%s, %d samples, depth %d" % (scene, n, depth))


@pytest.mark.parametrize("skip", ("1", "0"))
@pytest.mark.parametrize("n", (2, 65, 129))
@pytest.mark.parametrize("scene", SCENES)
def test_dark_pixels_beside_hit_ones(scene, n, skip, monkeypatch):
    """DRT_DARK_SKIP=1: the instantiation that passes over whole windows and single samples worth nothing in a pixel that is still
    dark; 0: the one that replays them all. The same film"""
    clear(monkeypatch)
    monkeypatch.setenv("DRT_DARK_SKIP", skip)
    closed_and_general(scene, n, 8, monkeypatch, "%s, %d samples, DRT_DARK_SKIP=%s" % (scene, n, skip))


@pytest.mark.parametrize("skip", ("1", "0"))
@pytest.mark.parametrize("scene", SCENES)
def test_four_waves_take_every_item(scene, skip, monkeypatch):
    """all but one workgroup held back: four waves draw the launch's 40-odd items -- main-pass pieces of four pixels and the groups'
    tail passes, mixed -- so each runs both passes by turns in its one LDS region"""
    clear(monkeypatch)
    monkeypatch.setenv("DRT_RESERVE_BLOCKS", "1000000")
    monkeypatch.setenv("DRT_DARK_SKIP", skip)
    closed_and_general(scene, 65, 20, monkeypatch, "%s, one workgroup, DRT_DARK_SKIP=%s" % (scene, skip))


def test_without_the_resumed_tails(monkeypatch):
    """DRT_TAIL_RESUME=0: the tail pass replays every path it is left from vertex 0, in windows of the closed form's size"""
    clear(monkeypatch)
    monkeypatch.setenv("DRT_TAIL_RESUME", "0")
    closed_and_general(SCENES[0], 65, 20, monkeypatch, "DRT_TAIL_RESUME=0")
