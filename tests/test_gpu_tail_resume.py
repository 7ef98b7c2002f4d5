"""GPU (-m gpu): the shade kernel's tail pass resumed from the prefix the trace kernel carried.

The trace kernel carries a path's tail wavelengths (the S mod 64 beyond the 64 lanes) while its vertices are two-lobe plastic or
mirror. At the first vertex k of any other material it stops; with k in 1..15 it leaves (throughput, dst) after vertex k - 1 in
tail_resume / tail_stage and k in the header, and the tail pass replays the path from vertex k instead of vertex 0
(csrc/drt_kernels.h). DRT_TAIL_RESUME=0 replays such paths whole, DRT_TRACE_TAIL=0 carries nothing in the trace kernel at all. Every
case here is rendered the three ways: the three film buffers, XYZ and the statistics bit for bit the same, and with resume on bit for
bit the oracle's (cases.oracle_render_device_pow, the comparison of tests/test_gpu_fixed_lists.py).

So that no case passes empty, the oracle's hit log is walked on the CPU (resume_vertices) and every case asserts how many paths are
resumed at which k. Scenes are written here as .scn text (the box and its materials are tests/test_gpu_fixed_lists.py's); cameras and
sizes were chosen on the CPU so that the oracle alone meets the counts."""
import numpy as np
import pytest

import cases
import oracle_py as O
import pydrt
import test_gpu_fixed_lists as FL

pytestmark = pytest.mark.gpu

REF_XYZ_TOL = FL.REF_XYZ_TOL  # 1e-9: DRT_MODE_XYZ sums in another order than the oracle's fold

GRIDS = dict(FL.GRIDS)
GRIDS.update({72: (380.0, 735.0, 5.0), 65: (380.0, 700.0, 5.0), 73: (380.0, 740.0, 5.0)})  # tails of 8, of 1, and of 9 (not carried)

WAYS = (("resume on", {}), ("DRT_TAIL_RESUME=0", {"DRT_TAIL_RESUME": "0"}), ("DRT_TRACE_TAIL=0", {"DRT_TRACE_TAIL": "0"}))


def load(text, size, S=69):
    g = GRIDS[S]
    b = pydrt.load_scene_text(text, size, size, min_wl=g[0], max_wl=g[1], wl_interval=g[2])
    assert b.S == S
    return b


def resume_vertices(bundle, hits):
    """From the oracle's hit log [paths][max_depth]: per path, the index k of its first shaded vertex that is neither two-lobe
    plastic nor {mirror_bdsf} (-1: it has none, the trace kernel carries the path to its end), and whether a mirror vertex lies
    before k. A path with k >= 0 is replayed by the tail pass: from vertex k where 1 <= k <= 15, from vertex 0 otherwise."""
    mats = bundle.materials()
    surf_mat = np.array([bundle.scene.surfaces[i].material for i in range(int(bundle.scene.num_surfaces))])
    black = np.array([bool(m.is_black_body) for m in mats])
    names = [tuple(pydrt.BDSF_NAMES[m.bdsfs[j]] for j in range(int(m.num_bdsfs))) for m in mats]
    carried = np.array([n == FL.PLASTIC or n == FL.MIRROR for n in names])
    is_mirror = np.array([n == FL.MIRROR for n in names])
    hit = hits >= 0
    mat = np.where(hit, surf_mat[np.where(hit, hits, 0)], 0)
    shaded = np.cumprod(hit & ~black[mat], axis=1).astype(bool)  # the path ends at the first depth that is not shaded
    other = shaded & ~carried[mat]
    k = np.where(other.any(axis=1), other.argmax(axis=1), -1)
    before = np.arange(hits.shape[1])[None, :] < k[:, None]
    mirror_before = (shaded & is_mirror[mat] & before).any(axis=1)
    return k, mirror_before, int(shaded.sum())


def band(k, lo, hi):
    return int(((k >= lo) & (k <= hi)).sum())


def assert_counts(key, k, need):
    """need: {(lo, hi): at least this many paths whose first other-material vertex is in lo..hi}"""
    for (lo, hi), n in need.items():
        got = band(k, lo, hi)
        print("%s: %d paths with k in %d..%d (need %d)" % (key, got, lo, hi, n))
        assert got >= n, "%s: only %d paths with k in %d..%d" % (key, got, lo, hi)


def render(bundle, p):
    r = pydrt.Renderer(bundle, p)
    try:
        r.render()
        film = (r.read_xyz_film(),) if int(p.mode) == pydrt.MODE_XYZ else r.read_film()
        return film, r.read_xyz(), r.stats()
    finally:
        r.close()


def three_ways(monkeypatch, what, run, same_stats=True):
    """run() under the three settings; every result after the first must be the first's, bit for bit. run() returns
    (tuple of arrays, stats or None, path_flags). Returns the resume-on result."""
    out = []
    for name, env in WAYS:
        for var in ("DRT_TAIL_RESUME", "DRT_TRACE_TAIL"):
            monkeypatch.delenv(var, raising=False)
        for var, val in env.items():
            monkeypatch.setenv(var, val)
        out.append(run())
    for var in ("DRT_TAIL_RESUME", "DRT_TRACE_TAIL"):
        monkeypatch.delenv(var, raising=False)
    for (name, _), got in zip(WAYS[1:], out[1:]):
        assert len(got[0]) == len(out[0][0])
        for n, (a, b) in enumerate(zip(out[0][0], got[0])):
            assert cases.same_bits(a, b), "%s, resume on against %s, buffer %d: %s" % (what, name, n, cases.first_difference(a, b))
        if same_stats and got[1] is not None:
            assert cases.stat_counts(out[0][1]) == cases.stat_counts(got[1]), "%s: statistics, resume on against %s" % (what, name)
    return out


def plain(bundle, p):
    def run():
        film, xyz, st = render(bundle, p)
        return tuple(film) + (xyz,), st, int(st.path_flags)
    return run


_oracle_cache = {}


def oracle(key, bundle, p):
    """the oracle's film and hit log of a case, rendered once and shared (never written to)"""
    if key not in _oracle_cache:
        _oracle_cache[key] = cases.oracle_render_device_pow(bundle, p, want_hits=True, num_threads=16)
    return _oracle_cache[key]


def check(key, text, size, spp, depth, monkeypatch, need, S=69, mode="spectral", seed=3, mirror_prefix=0, carried=True, batch=4):
    bundle = load(text, size, S)
    p = pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=seed, batch_spp=batch)
    opx, oav, ova, ohits, ost = oracle((key, S, size, spp, depth, seed), bundle, p)
    k, mirror_before, n_shaded = resume_vertices(bundle, ohits)
    assert n_shaded == ost.shaded_vertices, "the walk of the hit log and the oracle disagree about what is shaded"
    assert_counts(key, k, need)
    if mirror_prefix:
        n = int((mirror_before & (k >= 1) & (k <= 15)).sum())
        print("%s: %d resumed paths with a mirror vertex in the prefix" % (key, n))
        assert n >= mirror_prefix
    if mode == "xyz":
        p = pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=seed, batch_spp=batch, mode=pydrt.MODE_XYZ)
    out = three_ways(monkeypatch, key, plain(bundle, p))
    flags = [o[2] & pydrt.PATH_TRACE_TAIL for o in out]
    assert (bool(flags[0]), bool(flags[1]), bool(flags[2])) == (carried, carried, False), "which way carried tails in the trace kernel"
    got, st = out[0][0], out[0][1]
    assert cases.stat_counts(st) == cases.stat_counts(ost)
    want_xyz = O.oracle_film_to_xyz(bundle, opx)
    if mode == "xyz":
        ok = np.isfinite(want_xyz).all(axis=1)
        assert np.array_equal(ok, np.isfinite(got[-1]).all(axis=1)) and cases.xyz_rel_err(got[-1][ok], want_xyz[ok]) <= REF_XYZ_TOL
    else:
        for g, w, name in zip(got, (opx, oav, ova, want_xyz), ("pixels", "means", "variances", "XYZ")):
            assert cases.same_bits(g, w), "%s against the oracle, %s: %s" % (key, name, cases.first_difference(g, w))
    return bundle, p


BOX = dict(size=48, spp=16, depth=8)
BOX_NEED = {(1, 1): 500, (2, 3): 500, (4, 7): 500, (0, 0): 200}


def test_box_one_plane_light(monkeypatch):
    """plastic walls, a glass sphere, a mirror plane, a smooth-gold and a GGX-gold sphere: resumed at k = 1, 2-3 and 4-7 (k = 4 opens
    a new record block), replayed whole at k = 0, and resumed behind a mirror vertex"""
    check("box", FL.box_scene(), monkeypatch=monkeypatch, need=BOX_NEED, mirror_prefix=200, **BOX)


@pytest.mark.parametrize("S,carried", [(72, True), (65, True), (64, False), (73, False)])
def test_box_on_other_grids(S, carried, monkeypatch):
    """a tail of 8 (the most the trace kernel carries), of 1, none at all (S = 64: no tail pass), and of 9: the trace kernel carries
    nothing, so no resume array is allocated and the three ways are one"""
    check("box", FL.box_scene(), monkeypatch=monkeypatch, need=BOX_NEED, S=S, carried=carried, **BOX)


def test_box_xyz_film(monkeypatch):
    check("box", FL.box_scene(), monkeypatch=monkeypatch, need=BOX_NEED, mode="xyz", **BOX)


DEEP = dict(size=40, spp=12, depth=20, seed=6)


def deep_room():
    """a closed box, the left and the right wall mirrors facing each other, the camera looking along them at a glass sphere and a
    GGX-gold sphere at the far end: paths bounce between the mirrors and off the plastic walls before they meet either"""
    return (FL._camera(position=(0.0, 0.0, 2.6), target=(-3.0, -0.4, -1.0)) + FL._materials() + FL._walls(left="mirror", right="mirror", front="white")
            + FL._sphere("glass_ball", (1.2, -2.2, -1.8), 0.8, "glass") + FL._sphere("ggx_ball", (-1.4, -2.4, -2.0), 0.6, "rough_gold")
            + FL.PLANE_LIGHT)


def test_deep_paths(monkeypatch):
    """k in 8-11: no visibility bit in the header, the vertex in the header's third block; k in 12-15: through the table block;
    k >= 16 does not fit the header's field: replayed from vertex 0"""
    check("deep", deep_room(), monkeypatch=monkeypatch, need={(8, 11): 50, (12, 15): 50, (16, 19): 50, (1, 7): 500}, **DEEP)


def test_adaptive_round_and_continuation(monkeypatch):
    """the LIST instantiations: slots are indexed by list position. One adaptive render to 12 samples, continued to 20"""
    import test_gpu_adaptive as A
    bundle = load(FL.box_scene(), 48)
    p = pydrt.make_params(48, 48, spp=20, max_depth=8, seed=3, batch_spp=4)
    snaps = A.oracle_snapshots(bundle, p, [4, 8, 12, 16, 20])
    k, _, _ = resume_vertices(bundle, oracle(("box", 69, 48, 16, 8, 3), bundle, pydrt.make_params(48, 48, spp=16, max_depth=8, seed=3, batch_spp=4))[3])
    assert_counts("adaptive (the uniform film's first 16 samples)", k, {(1, 7): 1500})
    rel, _ = A.pick_rel_error(bundle, snaps, 48 * 48, 4, 20, 4)

    def run():
        r = pydrt.Renderer(bundle, p)
        try:
            r.render_adaptive(4, 12, 4, rel)
            c0 = r.read_sample_counts().reshape(-1).copy()
            rep = r.render_adaptive_continue(20, 4, rel)
            c1 = r.read_sample_counts().reshape(-1).copy()
            assert rep["rounds"] >= 1
            return r.read_film() + (c0.astype(np.float64), c1.astype(np.float64)), None, int(r.stats().path_flags)
        finally:
            r.close()
    out = three_ways(monkeypatch, "adaptive", run)
    film, c1 = out[0][0][:3], out[0][0][4].astype(np.int64)
    assert (c1 == 4).any() and (c1 == 20).any() and ((c1 > 4) & (c1 < 20)).any()
    A.assert_same_film(film, A.film_at_counts(snaps, c1), "adaptive, resume on, against the oracle's snapshots")


def test_ray_film(monkeypatch):
    """a ray film of the box: the ray-mode entry points of the trace kernel. The table is the oracle camera's own rays (centre
    scheme), so the film is the camera's and the oracle's"""
    import ray_film_cases as R
    bundle = load(FL.box_scene(), 48)
    p = pydrt.make_params(48, 48, spp=16, max_depth=8, seed=3, batch_spp=4, pixel_scheme=pydrt.FILM_SAMPLE_CENTER)
    opx, oav, ova, ohits, ost = oracle(("box_centre",), bundle, p)
    k, _, _ = resume_vertices(bundle, ohits)
    assert_counts("ray film", k, {(1, 7): 1500, (0, 0): 200})
    assert float(bundle.camera.aperture_radius) == 0.0
    table = R.centre_rays(bundle, 48, 48)

    def run():
        r = pydrt.Renderer(bundle, p)
        try:
            r.bind_rays(*table)
            r.render()
            st = r.stats()
            assert st.path_flags & pydrt.PATH_RAYS
            return r.read_film() + (r.read_xyz(),), st, int(st.path_flags)
        finally:
            r.close()
    out = three_ways(monkeypatch, "ray film", run)
    for g, w, name in zip(out[0][0], (opx, oav, ova), ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "ray film against the oracle, %s: %s" % (name, cases.first_difference(g, w))


def test_context_after_update_materials(monkeypatch):
    """a live context whose plastic walls are given another shininess: the prefix the trace kernel carries holds the new glossy terms"""
    before = load(FL.box_scene(), 48)
    after = load(FL.box_scene().replace("shininess 100.0", "shininess 30.0"), 48)
    p = pydrt.make_params(48, 48, spp=16, max_depth=8, seed=3, batch_spp=4)
    opx, oav, ova, ohits, ost = oracle(("box_shiny30",), after, p)
    k, _, _ = resume_vertices(after, ohits)
    assert_counts("after update_materials", k, {(1, 7): 1500})
    assert not cases.same_bits(opx, oracle(("box", 69, 48, 16, 8, 3), before, p)[0]), "the update changes the film"

    def run():
        r = pydrt.Renderer(before, p)
        try:
            r.update_materials(after.materials())
            r.render()
            st = r.stats()
            return r.read_film() + (r.read_xyz(),), st, int(st.path_flags)
        finally:
            r.close()
    out = three_ways(monkeypatch, "update_materials", run)
    for g, w, name in zip(out[0][0], (opx, oav, ova), ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "updated context against the oracle, %s: %s" % (name, cases.first_difference(g, w))


def test_tiny_record_pool_rendered_again(monkeypatch):
    """DRT_POOL_BLOCKS=1: launches run out of record blocks, their shade kernels do nothing and the samples are rendered again in
    worst-case-sized launches (tests/test_gpu_parity.py, test_record_pool_that_runs_out_is_rendered_again_not_wrong) -- the headers,
    the staging slots and the resume array of the launch that ran out are written again before they are read"""
    bundle = load(FL.box_scene(), 48)
    p = pydrt.make_params(48, 48, spp=16, max_depth=8, seed=3, batch_spp=8)
    opx, oav, ova, ohits, ost = oracle(("box", 69, 48, 16, 8, 3), bundle, p)
    monkeypatch.setenv("DRT_POOL_BLOCKS", "1")
    redone = []

    def run():
        film, xyz, st = render(bundle, p)
        redone.append(int(st.redone_launches))
        return tuple(film) + (xyz,), st, int(st.path_flags)
    out = three_ways(monkeypatch, "tiny pool", run)
    assert min(redone) >= 1, "no launch ran out of record blocks: %s" % redone
    for g, w, name in zip(out[0][0], (opx, oav, ova), ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "tiny pool against the oracle, %s: %s" % (name, cases.first_difference(g, w))
