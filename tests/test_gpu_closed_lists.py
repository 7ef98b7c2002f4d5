"""GPU (-m gpu): the shade kernel's closed instantiation, and the rough conductor's fixed-list form, against the general list.

A scene whose every material lists nothing or exactly one of {two-lobe plastic}, {mirror_bdsf}, {fs_dielectric_reflectance_bdsf,
fs_dielectric_transmittance_bdsf}, {fs_conductor_bdsf}, {ct_conductor_bdsf} is replayed by drt_shade_kernel_closed (csrc/drt_kernels.h,
shade_pixels<CLOSED>): the general BDSF list is not compiled into it, neither in the main pass nor in the tail pass's general step.
Every case here is rendered three ways -- default, DRT_NO_CLOSED_SHADE=1 (the general instantiation: the rough conductor through
the general loop) and DRT_NO_FIXED_LISTS=1 (the general instantiation, every non-plastic vertex through the general loop) -- the
three film buffers bit for bit the same, the statistics the same, and the default film bit for bit the oracle's
(cases.oracle_render_device_pow). Renderer.shade_instantiation() says which kernel a context launches.

So that no case passes empty, the oracle's hit log is walked on the CPU as tests/test_gpu_fixed_lists.py does: at least 500 shaded
rough-conductor vertices in every case that is there for them, at least 50 in each deep band (vertex index 8 and up: no visibility
bit in the header, beyond the prefetched records; 16 and up: no plastic flag). Cameras and sizes were chosen on the CPU so that the
oracle alone meets the counts."""
import numpy as np
import pytest

import cases
import pydrt
import test_gpu_fixed_lists as FL
from test_gpu_fixed_lists import CONDUCTOR, GGX, GLASS, MIRROR, PLASTIC

pytestmark = pytest.mark.gpu

SWITCHES = ("DRT_NO_CLOSED_SHADE", "DRT_NO_FIXED_LISTS")


def render(bundle, p, want):
    """one fresh context's film, XYZ and statistics; `want`: the instantiation the context must say it launches"""
    r = pydrt.Renderer(bundle, p)
    try:
        assert r.shade_instantiation() == want, "the context launches the %s instantiation, not the %s one" % (r.shade_instantiation(), want)
        r.render()
        return r.read_film(), r.read_xyz(), r.stats()
    finally:
        r.close()


def assert_same(a, b, what):
    for x, y, name in zip(a[0], b[0], ("pixels", "means", "variances")):
        assert cases.same_bits(x, y), "%s, %s: %s" % (what, name, cases.first_difference(x, y))
    assert cases.same_bits(a[1], b[1]), "%s, XYZ: %s" % (what, cases.first_difference(a[1], b[1]))
    assert cases.stat_counts(a[2]) == cases.stat_counts(b[2]), what


def three_ways(bundle, p, monkeypatch, what, default="closed"):
    """default, DRT_NO_CLOSED_SHADE=1, DRT_NO_FIXED_LISTS=1: the same film, XYZ and statistics; returns the default render"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    on = render(bundle, p, default)
    for name in SWITCHES:
        monkeypatch.setenv(name, "1")
        off = render(bundle, p, "general")
        monkeypatch.delenv(name)
        assert_same(on, off, "%s, default against %s=1" % (what, name))
    return on


def check(key, text, size, spp, depth, monkeypatch, need, S=69, deep=(), seed=3, default="closed"):
    """`need`: the lists the case is there for (>= 500 vertices each); `deep`: (list(s), first vertex index) bands (>= 50 each)"""
    bundle = FL.load(text, size, S)
    p = pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=seed, batch_spp=4)
    opx, oav, ova, ohits, ost = FL.oracle((key, S), bundle, p)  # (shared with tests/test_gpu_fixed_lists.py where the case is the same)
    classes, n_shaded = FL.vertex_classes(bundle, ohits)
    assert n_shaded == ost.shaded_vertices, "the walk of the hit log and the oracle disagree about what is shaded"
    counts = {k: len(v) for k, v in classes.items()}
    print("%s S=%d: shaded vertices by list %s" % (key, S, counts))
    for lst in need:
        assert counts.get(lst, 0) >= 500, "%s: only %d vertices of %s" % (key, counts.get(lst, 0), lst)
    for lists, first in deep:
        n = sum(int((classes.get(lst, np.zeros(0)) >= first).sum()) for lst in lists)
        print("%s: %d vertices of %s at index >= %d" % (key, n, lists, first))
        assert n >= 50, "%s: only %d vertices of %s at index >= %d" % (key, n, lists, first)
    film, xyz, st = three_ways(bundle, p, monkeypatch, key, default)
    assert cases.stat_counts(st) == cases.stat_counts(ost)
    for g, w, name in zip(film, (opx, oav, ova), ("pixels", "means", "variances")):
        assert cases.same_bits(g, w), "%s against the oracle, %s: %s" % (key, name, cases.first_difference(g, w))


@pytest.mark.parametrize("S", [69, 64, 2])
def test_one_box_one_plane_light(S, monkeypatch):
    """glass sphere, mirror plane, smooth-gold sphere, GGX-gold sphere, plastic walls, depth 8: tails of 5, 0 and 2 wavelengths"""
    check("box", FL.box_scene(), 48, 16, 8, monkeypatch, need=(MIRROR, GLASS, CONDUCTOR, GGX, PLASTIC), S=S)


def test_three_register_sets_keep_the_general_instantiation(monkeypatch):
    """S = 171 is three wavelength sets per lane: the closed instantiation exists for one set only"""
    check("box", FL.box_scene(), 48, 16, 8, monkeypatch, need=(GGX,), S=171, default="general")


def ggx_corridor():
    """tests/test_gpu_fixed_lists.py's corridor of two facing mirrors with a GGX-gold sphere beside the glass one"""
    return FL.mirror_corridor() + FL._sphere("ggx_ball", (-0.8, -2.0, 1.2), 1.0, "rough_gold")


def test_deep_paths_between_two_mirrors(monkeypatch):
    """depth 20 in the closed corridor: vertices 8 and up (no visibility bit, beyond the prefetch) and 16 and up (no plastic flag)"""
    check("corridor_20", FL.mirror_corridor(), 32, 8, 20, monkeypatch, need=(MIRROR, GLASS), deep=[((MIRROR, GLASS), 8), ((MIRROR, GLASS), 16), ((PLASTIC,), 16)],
          seed=6)


def test_deep_rough_conductor_vertices(monkeypatch):
    """the same corridor with a GGX-gold sphere in it: rough-conductor vertices in both deep bands"""
    check("ggx_corridor_20", ggx_corridor(), 32, 8, 20, monkeypatch, need=(GGX,), deep=[((GGX,), 8), ((GGX,), 16)], seed=6)


def test_two_lights(monkeypatch):
    """a plane and a sphere light: the header's visibility bits cover light 0 only, and no leading-run loop"""
    check("lights_plane_sphere", FL.box_scene(lights=FL.PLANE_LIGHT + FL.SPHERE_LIGHT), 40, 12, 6, monkeypatch, need=(MIRROR, GLASS, CONDUCTOR, GGX))


def test_a_list_outside_the_covered_ones_takes_the_general_instantiation(monkeypatch):
    """the mirror plane's material lists {bp_diffuse_bdsf} alone: one such material in the scene, and the general instantiation runs"""
    lst = ("bp_diffuse_bdsf",)
    check("closed_uncovered", FL.box_scene(mirror_bdsfs=lst), 48, 16, 8, monkeypatch, need=(lst, GGX), default="general")


BARE = ()  # a material that is no black body and lists no BDSF


def bare_scene():
    """the box with one more sphere whose material gives a refraction spectrum only (as the base material does): no black body and
    no BDSF, so a hit on it is a shaded vertex whose BDSF sum is zero"""
    bare = "\nMaterial\nname bare\nrefract constant 1.2\ndir_func cos_weighted_sample_hemisphere\n"
    text = FL.box_scene(extra=FL._sphere("bare_ball", (1.2, -2.2, 1.6), 0.8, "bare"))
    return text.replace("\nMaterial\nname light\n", bare + "\nMaterial\nname light\n", 1)


def test_a_shaded_material_that_lists_nothing_takes_the_general_instantiation(monkeypatch):
    """every list of the scene is covered, but one surface's material is no black body and lists nothing: its vertices sum to zero
    in the general list, the closed code has no form for them, so the launcher must not take it"""
    check("closed_bare", bare_scene(), 48, 16, 8, monkeypatch, need=(BARE, GGX, GLASS), default="general")


def test_a_live_context_keeps_its_instantiation_through_material_updates(monkeypatch):
    """A material update changes shininess and roughness and refuses every other change, a list's among them: so no update can turn a
    covered list into an uncovered one, the getter says so before and after, and the film after an update is a fresh context's"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    text = FL.box_scene()
    assert "roughness 0.1" in text
    before, after = FL.load(text, 32), FL.load(text.replace("roughness 0.1", "roughness 0.3"), 32)
    p = pydrt.make_params(32, 32, spp=8, max_depth=8, seed=3, batch_spp=4)
    fresh_before, fresh_after = render(before, p, "closed"), render(after, p, "closed")
    assert not cases.same_bits(fresh_before[0][0], fresh_after[0][0]), "the roughness changes the film"
    monkeypatch.setenv("DRT_NO_CLOSED_SHADE", "1")
    assert_same(fresh_after, render(after, p, "general"), "after the update, closed against general")
    monkeypatch.delenv("DRT_NO_CLOSED_SHADE")
    names = [tuple(pydrt.BDSF_NAMES[m.bdsfs[j]] for j in range(int(m.num_bdsfs))) for m in before.materials()]
    rough = names.index(GGX)
    r = pydrt.Renderer(before, p)
    try:
        assert r.shade_instantiation() == "closed"
        uncovered = before.materials()
        uncovered[rough].bdsfs[0] = pydrt.BDSF_NAMES.index("bp_diffuse_bdsf")
        with pytest.raises(RuntimeError, match="material %d: bdsfs\\[0\\]" % rough):
            r.update_materials(uncovered)
        assert r.shade_instantiation() == "closed"
        for to, want in ((after, fresh_after), (before, fresh_before)):
            r.reset_film()
            r.update_materials(to.materials())
            assert r.shade_instantiation() == "closed"
            r.render()
            assert_same((r.read_film(), r.read_xyz(), r.stats()), want, "updated context against a fresh one")
    finally:
        r.close()
