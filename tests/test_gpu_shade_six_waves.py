"""GPU (-m gpu): the closed shade kernel in workgroups of 512 lanes, one SPD table for eight waves, six waves per SIMD
(csrc/drt_kernels.h, drt_shade_kernel_closed_lds6) -- against the CPU oracle and the five-wave and four-wave closed kernels.

Every film here is bit for bit the oracle's (cases.oracle_render_device_pow) and bit for bit the film of the same render with
DRT_CLOSED_WAVES=5 (drt_shade_kernel_closed_lds, workgroups of 256 lanes) and with DRT_NO_CLOSED_LDS=1 (drt_shade_kernel_closed, four
waves). Renderer.shade_closed_waves() says which of the three a context's dense launches run, so no case passes on a fallback.

What differs from the five-wave kernel, and so what the shapes are chosen for: eight waves stage one table and stride eight regions
behind it; a pixel's film rows are scalar addresses with the lane's offset made at the read and at the write; the tail pass's cursor
reads the vignette, block word 2 and light 0's emission back from LDS and fetches a general vertex's dir_pdf behind its lights.
The shapes, S = 69, a 16 x 16 tile of cornell_plane_light and of cornell_gold_mirror in a 64 x 64 image at the lower right corner of
the box (pixels nothing reaches beside plastic, mirror, glass and both golds: all four fixed lists):
  - samples per launch 1, 63, 64, 65, 130: the edges of the 64-sample header window, the header slots' wrap, a third window of two;
  - max depth 1, 8, 16: no bounce at all, the last prefetched record, vertices 8-15 through header word 3 (past its three blocks);
  - DRT_DARK_SKIP 1 and 0: both DARK instantiations;
  - DRT_NO_LIVE_WINDOW set and not;
  - a tile of 2 x 2 pixels: one pixel group, fewer work items than a workgroup has waves, so some of its waves draw nothing (they
    still stage the table and meet the others at the barrier);
  - DRT_POOL_BLOCKS=1: launches run out of record blocks, leave the film alone and are rendered again."""
import pytest

import cases
import pydrt

pytestmark = pytest.mark.gpu

SCENES = ("cornell_plane_light.scn", "cornell_gold_mirror.scn")
SIZE = 64
TILE = dict(x0=40, y0=48, tile_w=16, tile_h=16)
SMALL = dict(x0=46, y0=58, tile_w=2, tile_h=2)
SAMPLES = (1, 63, 64, 65, 130)
DEPTHS = (1, 8, 16)
KNOBS = ("DRT_NO_CLOSED_SHADE", "DRT_NO_CLOSED_LDS", "DRT_CLOSED_WAVES", "DRT_DARK_SKIP", "DRT_RESERVE_BLOCKS", "DRT_NO_LIVE_WINDOW", "DRT_POOL_BLOCKS",
         "DRT_SHADE_BLOCKS_PER_CU")
# the switch that selects a kernel, and the waves per SIMD the context must then report
FORMS = ((None, 6), ("DRT_CLOSED_WAVES=5", 5), ("DRT_NO_CLOSED_LDS=1", 4))

_bundles, _oracles = {}, {}


def bundle_of(scene):
    if scene not in _bundles:
        _bundles[scene] = pydrt.load_scene(cases.scene_path(scene), SIZE, SIZE)
    return _bundles[scene]


def params(n, depth, tile, batch=None):
    return pydrt.make_params(SIZE, SIZE, spp=n, max_depth=depth, seed=5, batch_spp=batch or n, **tile)


def oracle(scene, n, depth, tile=None):
    """the oracle's film and statistics of a case, rendered once and shared (never written to)"""
    tile = tile or TILE
    key = (scene, n, depth, tuple(sorted(tile.items())))
    if key not in _oracles:
        _oracles[key] = cases.oracle_render_device_pow(bundle_of(scene), params(n, depth, tile), num_threads=16)
    return _oracles[key]


def render(scene, p, waves):
    r = pydrt.Renderer(bundle_of(scene), p)
    try:
        assert r.shade_instantiation() == "closed", "the context launches the %s instantiation" % r.shade_instantiation()
        assert r.shade_closed_waves() == waves, "the context runs the %d-wave closed kernel, not the %d-wave one" % (r.shade_closed_waves(), waves)
        assert r.shade_closed_lds() == (waves >= 5)
        r.render()
        return r.read_film(), r.stats()
    finally:
        r.close()


def clear(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def three_kernels(scene, n, depth, monkeypatch, what, tile=None, batch=None):
    """the six-wave kernel's film is the oracle's, and the five-wave and four-wave kernels' films are the six-wave kernel's"""
    tile = tile or TILE
    opx, oav, ova, _, ost = oracle(scene, n, depth, tile)
    films = []
    for switch, waves in FORMS:
        if switch:
            monkeypatch.setenv(*switch.split("="))
        films.append(render(scene, params(n, depth, tile, batch), waves))
        if switch:
            monkeypatch.delenv(switch.split("=")[0])
    six = films[0]
    assert cases.stat_counts(six[1]) == cases.stat_counts(ost), what
    for g, w, name in zip(six[0], (opx, oav, ova), ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s, six waves against the oracle, %s: %s" % (what, name, cases.first_difference(g, w))
    for other, (switch, _) in zip(films[1:], FORMS[1:]):
        for x, y, name in zip(six[0], other[0], ("pixels", "means", "variances")):
            assert cases.same_bits(x, y), "%s, six waves against %s, %s: %s" % (what, switch, name, cases.first_difference(x, y))
        assert cases.stat_counts(six[1]) == cases.stat_counts(other[1]), what
    return six


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("n", SAMPLES)
@pytest.mark.parametrize("scene", SCENES)
def test_window_edges_and_depths(scene, n, depth, monkeypatch):
    clear(monkeypatch)
    three_kernels(scene, n, depth, monkeypatch, "%s, %d samples, depth %d" % (scene, n, depth))


@pytest.mark.parametrize("skip", ("1", "0"))
@pytest.mark.parametrize("n", (1, 65, 130))
@pytest.mark.parametrize("scene", SCENES)
def test_both_dark_forms(scene, n, skip, monkeypatch):
    """DRT_DARK_SKIP=1: the instantiation that passes over windows and samples worth nothing in a pixel still dark; 0: the other"""
    clear(monkeypatch)
    monkeypatch.setenv("DRT_DARK_SKIP", skip)
    three_kernels(scene, n, 8, monkeypatch, "%s, %d samples, DRT_DARK_SKIP=%s" % (scene, n, skip))


@pytest.mark.parametrize("scene", SCENES)
def test_without_the_live_window(scene, monkeypatch):
    """(every other case here runs with it)"""
    clear(monkeypatch)
    monkeypatch.setenv("DRT_NO_LIVE_WINDOW", "1")
    three_kernels(scene, 65, 16, monkeypatch, "%s, DRT_NO_LIVE_WINDOW=1" % scene)


@pytest.mark.parametrize("skip", ("1", "0"))
@pytest.mark.parametrize("scene", SCENES)
def test_fewer_items_than_a_workgroup_has_waves(scene, skip, monkeypatch):
    """four pixels: one group, at most four main-pass pieces and a tail pass for eight waves"""
    clear(monkeypatch)
    monkeypatch.setenv("DRT_DARK_SKIP", skip)
    three_kernels(scene, 65, 16, monkeypatch, "%s, 2 x 2 tile, DRT_DARK_SKIP=%s" % (scene, skip), tile=SMALL)


@pytest.mark.parametrize("scene", SCENES)
def test_one_workgroup_takes_every_item(scene, monkeypatch):
    """all but one workgroup held back: eight waves draw the launch's items -- main-pass pieces and tail passes, mixed -- so each runs
    both passes by turns in its one LDS region"""
    clear(monkeypatch)
    monkeypatch.setenv("DRT_RESERVE_BLOCKS", "1000000")
    three_kernels(scene, 65, 16, monkeypatch, "%s, one workgroup" % scene)


def test_a_record_pool_that_runs_out(monkeypatch):
    """DRT_POOL_BLOCKS=1: a launch that ran out leaves the film untouched (the kernel's first test) and is rendered again"""
    clear(monkeypatch)
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    film, st = three_kernels(SCENES[0], 16, 8, monkeypatch, "tiny record pool", batch=8)
    assert st.redone_launches > 0, "no launch ran out of record blocks"
