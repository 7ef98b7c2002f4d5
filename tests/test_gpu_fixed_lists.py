"""GPU (-m gpu): the shade kernel's straight-line bodies for mirror, glass and smooth-conductor vertices against the general list.

The main pass replays a vertex whose material lists exactly {mirror_bdsf}, {fs_dielectric_reflectance_bdsf,
fs_dielectric_transmittance_bdsf} or {fs_conductor_bdsf} through bdsf_at_wavelength's fixed-list form (csrc/drt_kernels.h,
fixed_vertex); DRT_NO_FIXED_LISTS=1, read when the context is created, sends it through the general loop. Every case here is rendered
both ways: the three film buffers bit for bit the same, the statistics the same, and the film with the bodies on bit for bit the
oracle's (cases.oracle_render_device_pow, the comparison of tests/test_gpu_parity.py).

So that no case passes empty, the oracle's hit log is walked on the CPU -- depth, surface, the surface's material, the material's
list -- and every case asserts at least 500 shaded vertices of each list it is there for, and at least 50 in each deep band (vertex
index 8 and up: no visibility bit in the header and, with one light, beyond the prefetched records; 16 and up: no plastic flag).
Scenes are written here, as .scn text; cameras and sizes were chosen on the CPU so that the oracle alone meets the counts."""
import numpy as np
import pytest

import cases
import oracle_py as O
import pydrt

pytestmark = pytest.mark.gpu

REF_XYZ_TOL = 1e-9  # DRT_MODE_XYZ against the oracle's film folded to XYZ: the sums run in another order (tests/test_gpu_parity.py)

MIRROR = ("mirror_bdsf",)
GLASS = ("fs_dielectric_reflectance_bdsf", "fs_dielectric_transmittance_bdsf")
CONDUCTOR = ("fs_conductor_bdsf",)
GGX = ("ct_conductor_bdsf",)
PLASTIC = ("bp_diffuse_bdsf", "bp_glossy_bdsf")

GRIDS = {69: (380.0, 720.0, 5.0), 64: (380.0, 695.0, 5.0), 2: (380.0, 720.0, 340.0), 171: (380.0, 720.0, 2.0)}  # 171: three register sets


def _camera(position=(0.0, 0.0, 8.0), target=(0.0, 0.0, 0.0), fov=90.0):
    return ("Camera\nposition %g, %g, %g\ntarget %g, %g, %g\nroll 0.0\nfov %g\nfdepth 6.0\nflength 0.3\naperture 0.0\n"
            % (position + target + (fov,)))


def _plastic(name, d, g):
    return ("\nMaterial\nname %s\ndiffuse rgb %s\nglossy rgb %s\nshininess 100.0\nbdsfs bp_diffuse_bdsf, bp_glossy_bdsf\n"
            "dir_func cos_weighted_sample_hemisphere\n" % (name, d, g))


def _materials(glass_bdsfs=GLASS, mirror_bdsfs=MIRROR):
    """the materials of every scene here; the glass and the mirror take the list under test"""
    return ("\nMaterial\nname vacuum\nrefract constant 1.0\nbase_material\n\nMaterial\nname escape\nescape_material\n"
            + _plastic("white", "0.55, 0.55, 0.55", "0.1, 0.1, 0.1") + _plastic("red", "0.5, 0.0, 0.0", "0.5, 0.1, 0.1")
            + _plastic("green", "0.1, 0.35, 0.1", "0.1, 0.25, 0.1") + _plastic("blue", "0.2, 0.2, 0.8", "0.2, 0.2, 0.3")
            + "\nMaterial\nname mirror\nmirror rgb 0.813, 0.837, 0.888\ndiffuse rgb 0.3, 0.3, 0.1\nbdsfs %s\ndir_func sample_specular_direction\n" % ", ".join(mirror_bdsfs)
            + "\nMaterial\nname smooth_gold\nrefract csv au_spec_n.csv\nextinct csv au_spec_k.csv\nbdsfs fs_conductor_bdsf\ndir_func sample_specular_direction\n"
            + "\nMaterial\nname rough_gold\nrefract csv au_spec_n.csv\nextinct csv au_spec_k.csv\nroughness 0.1\nbdsfs ct_conductor_bdsf\ndir_func sample_ct_direction\n"
            + "\nMaterial\nname glass\nrefract csv glass.csv\nmirror rgb 0.7, 0.8, 0.9\nglossy constant 1.0\nshininess 16.0\nbdsfs %s\n"
              "dir_func sample_reflect_or_transmit_direction\n" % ", ".join(glass_bdsfs)
            + "\nMaterial\nname water\nrefract constant 1.33\nbdsfs fs_dielectric_reflectance_bdsf, fs_dielectric_transmittance_bdsf\n"
              "dir_func sample_reflect_or_transmit_direction\n"
            + "\nMaterial\nname light\nemission constant 1.0\nis_black_body true\n"
            + "\nMaterial\nname warm_light\nemission blackbody 4000.0 scale 1.2\nis_black_body true\n")


def _plane(name, p, u, v, material):
    return cases._surface(name, "plane", "position %g, %g, %g\npointu %g, %g, %g\npointv %g, %g, %g" % (p + u + v), material)


def _sphere(name, c, r, material):
    return cases._surface(name, "sphere", "position %g, %g, %g\nradius %g" % (c + (r,)), material)


def _walls(left="red", right="green", front=None):
    s = (_plane("back_wall", (-3, 3, -3), (3, 3, -3), (-3, -3, -3), "blue") + _plane("left_wall", (-3, 3, 3), (-3, 3, -3), (-3, -3, 3), left)
         + _plane("right_wall", (3, 3, -3), (3, 3, 3), (3, -3, -3), right) + _plane("floor", (-3, -3, -3), (3, -3, -3), (-3, -3, 3), "white")
         + _plane("ceiling", (-3, 3, 3), (3, 3, 3), (-3, 3, -3), "white"))
    if front:
        s += _plane("front_wall", (3, 3, 3), (-3, 3, 3), (3, -3, 3), front)
    return s


PLANE_LIGHT = _plane("light_source", (-1, 2.9, 1), (1, 2.9, 1), (-1, 2.9, -1), "light")


def box_scene(glass_bdsfs=GLASS, mirror_bdsfs=MIRROR, lights=PLANE_LIGHT, camera=None, extra=""):
    """one box: a glass sphere, a mirror plane, a smooth-gold and a GGX-gold sphere, plastic walls"""
    return ((camera or _camera()) + _materials(glass_bdsfs, mirror_bdsfs) + _walls()
            + _sphere("gold_ball", (2.0, -2.0, -0.5), 0.75, "smooth_gold") + _sphere("ggx_ball", (0.3, -2.3, 0.8), 0.7, "rough_gold")
            + _sphere("glass_ball", (-1.5, -1.8, 2.0), 1.0, "glass")
            + _plane("mirror_plane", (-1.6, 1.4, -2.4), (-1.6, -1.4, -2.9), (1.6, 1.4, -2.4), "mirror") + lights + extra)


def mirror_corridor():
    """a closed box: the left and the right wall are mirrors facing each other, a glass sphere between them, the camera inside"""
    return (_camera(position=(0.0, 0.0, 2.5), target=(-3.0, -0.3, 0.0)) + _materials() + _walls(left="mirror", right="mirror", front="white")
            + _sphere("glass_ball", (0.5, -1.0, 0.0), 1.0, "glass") + PLANE_LIGHT)


def simple_scene():
    """plastic walls and a mirror plane, no material with a Fresnel function: the SIMPLE instantiation"""
    mats = _materials()
    keep = [m for m in mats.split("\nMaterial\n") if m and not any(w in m for w in ("fs_", "ct_conductor"))]
    return (_camera() + "\nMaterial\n" + "\nMaterial\n".join(k.strip("\n") + "\n" for k in keep) + _walls()
            + _sphere("ball", (1.5, -2.0, 0.5), 1.0, "red")
            + _plane("mirror_plane", (-2.0, 2.0, -2.4), (-2.0, -2.0, -2.9), (2.0, 2.0, -2.4), "mirror") + PLANE_LIGHT)


def load(text, size, S=69):
    g = GRIDS[S]
    b = pydrt.load_scene_text(text, size, size, min_wl=g[0], max_wl=g[1], wl_interval=g[2])
    assert b.S == S
    return b


def vertex_classes(bundle, hits):
    """{BDSF list (names): vertex indices of the shaded vertices with that list}, from the oracle's hit log [paths][max_depth]: a path
    is shaded at every depth it hits a surface whose material is no black body (cast_ray, src/daily_ray_trace.c:440-472), so the
    vertex index is the depth"""
    mats = bundle.materials()
    surf_mat = np.array([bundle.scene.surfaces[i].material for i in range(int(bundle.scene.num_surfaces))])
    black = np.array([bool(m.is_black_body) for m in mats])
    names = [tuple(pydrt.BDSF_NAMES[m.bdsfs[j]] for j in range(int(m.num_bdsfs))) for m in mats]
    hit = hits >= 0
    mat = np.where(hit, surf_mat[np.where(hit, hits, 0)], -1)
    shaded = hit & ~black[np.where(hit, mat, 0)]
    shaded = np.cumprod(shaded, axis=1).astype(bool)  # the path ends at the first depth that is not shaded
    depth = np.broadcast_to(np.arange(hits.shape[1]), hits.shape)
    out = {}
    for m in np.unique(mat[shaded]):
        out.setdefault(names[m], []).append(depth[shaded & (mat == m)])
    return {k: np.concatenate(v) for k, v in out.items()}, int(shaded.sum())


def render(bundle, p):
    r = pydrt.Renderer(bundle, p)
    r.render()
    film = (r.read_xyz_film(),) if int(p.mode) == pydrt.MODE_XYZ else r.read_film()
    xyz = r.read_xyz()
    st = r.stats()
    r.close()
    return film, xyz, st


def on_and_off(bundle, p, monkeypatch, what):
    """the case with the fixed bodies and without them: same film, same XYZ, same statistics"""
    monkeypatch.delenv("DRT_NO_FIXED_LISTS", raising=False)
    on = render(bundle, p)
    monkeypatch.setenv("DRT_NO_FIXED_LISTS", "1")
    off = render(bundle, p)
    monkeypatch.delenv("DRT_NO_FIXED_LISTS")
    for a, b, name in zip(on[0], off[0], ("pixels", "means", "variances")):
        assert cases.same_bits(a, b), "%s, fixed lists on / off, %s: %s" % (what, name, cases.first_difference(a, b))
    assert cases.same_bits(on[1], off[1]), "%s, fixed lists on / off, XYZ: %s" % (what, cases.first_difference(on[1], off[1]))
    assert cases.stat_counts(on[2]) == cases.stat_counts(off[2])
    return on


_oracle_cache = {}


def oracle(key, bundle, p):
    """the oracle's film and hit log of a case, rendered once and shared (never written to)"""
    if key not in _oracle_cache:
        _oracle_cache[key] = cases.oracle_render_device_pow(bundle, p, want_hits=True, num_threads=16)
    return _oracle_cache[key]


def check(key, text, size, spp, depth, monkeypatch, need, S=69, mode="spectral", deep=(), seed=3):
    """render `text` both ways and against the oracle; `need`: the lists the case is there for (>= 500 vertices each);
    `deep`: (list(s), first vertex index) bands that need >= 50 vertices"""
    bundle = load(text, size, S)
    p = pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=seed, batch_spp=4)
    opx, oav, ova, ohits, ost = oracle((key, S), bundle, p)
    classes, n_shaded = vertex_classes(bundle, ohits)
    assert n_shaded == ost.shaded_vertices, "the walk of the hit log and the oracle disagree about what is shaded"
    counts = {k: len(v) for k, v in classes.items()}
    print("%s S=%d: shaded vertices by list %s" % (key, S, counts))
    for lst in need:
        assert counts.get(lst, 0) >= 500, "%s: only %d vertices of %s" % (key, counts.get(lst, 0), lst)
    for lists, first in deep:
        n = sum(int((classes.get(lst, np.zeros(0)) >= first).sum()) for lst in lists)
        print("%s: %d vertices of %s at index >= %d" % (key, n, lists, first))
        assert n >= 50, "%s: only %d vertices of %s at index >= %d" % (key, n, lists, first)
    if mode == "xyz":
        p = pydrt.make_params(size, size, spp=spp, max_depth=depth, seed=seed, batch_spp=4, mode=pydrt.MODE_XYZ)
    film, xyz, st = on_and_off(bundle, p, monkeypatch, key)
    assert cases.stat_counts(st) == cases.stat_counts(ost)
    if mode == "xyz":
        want = O.oracle_film_to_xyz(bundle, opx)
        ok = np.isfinite(want).all(axis=1)
        assert np.array_equal(ok, np.isfinite(xyz).all(axis=1)) and cases.xyz_rel_err(xyz[ok], want[ok]) <= REF_XYZ_TOL
    else:
        for g, w, name in zip(film, (opx, oav, ova), ("pixels", "means", "variances")):
            assert cases.same_bits(g, w), "%s against the oracle, %s: %s" % (key, name, cases.first_difference(g, w))
        want = O.oracle_film_to_xyz(bundle, opx)
        assert cases.same_bits(xyz, want), "%s against the oracle, XYZ: %s" % (key, cases.first_difference(xyz, want))


@pytest.mark.parametrize("S,mode", [(69, "spectral"), (64, "spectral"), (2, "spectral"), (171, "spectral"), (69, "xyz")])
def test_one_box_one_plane_light(S, mode, monkeypatch):
    """glass sphere, mirror plane, smooth-gold sphere, GGX-gold sphere, plastic walls, depth 8: the reference grid (main pass + tail
    pass), 64 wavelengths (no tail), 2, and 171 (three register sets per lane); once with the XYZ film"""
    check("box", box_scene(), 48, 16, 8, monkeypatch, need=(MIRROR, GLASS, CONDUCTOR, GGX, PLASTIC), S=S, mode=mode)


REVERSED = GLASS[::-1]
NOT_MATCHING = {
    "reversed": dict(glass_bdsfs=REVERSED),
    "reflectance_alone": dict(glass_bdsfs=GLASS[:1]),
    "mirror_then_diffuse": dict(mirror_bdsfs=MIRROR + ("bp_diffuse_bdsf",)),
    "glass_then_mirror": dict(glass_bdsfs=GLASS + MIRROR),
}


@pytest.mark.parametrize("name", sorted(NOT_MATCHING))
def test_lists_that_must_not_match(name, monkeypatch):
    """a permutation, a sublist and two supersets of the fixed lists take the general loop, whose carry-over of bdsf_result from a
    function whose direction test fails (Q1) the oracle pins: {reflectance} alone leaves every transmitted direction +0, {mirror,
    diffuse} overwrites what the mirror left, {reflectance, transmittance, mirror} adds the carried term a third time"""
    kw = NOT_MATCHING[name]
    lst = kw.get("glass_bdsfs") or kw.get("mirror_bdsfs")
    check("not_matching_" + name, box_scene(**kw), 48, 16, 8, monkeypatch, need=(lst, CONDUCTOR))


SPHERE_LIGHT = _sphere("bulb", (-2.0, 1.0, 0.0), 0.3, "warm_light")
POINT_LIGHT = cases._surface("spark", "point", "position 2.0, 1.5, 1.5", "warm_light")


@pytest.mark.parametrize("name,lights", [("plane_sphere", PLANE_LIGHT + SPHERE_LIGHT), ("point_plane", POINT_LIGHT + PLANE_LIGHT),
                                         ("sphere_point_plane", SPHERE_LIGHT + POINT_LIGHT + PLANE_LIGHT)])
def test_two_and_three_lights(name, lights, monkeypatch):
    """plane, sphere and point lights, two and three of them, in every first position: the header's visibility bits cover light 0 only"""
    check("lights_" + name, box_scene(lights=lights), 40, 12, 6, monkeypatch, need=(MIRROR, GLASS, CONDUCTOR))


def test_twelve_lights_records_wider_than_a_register(monkeypatch):
    """test_many_lights.scn's twelve lights with a glass and a mirror surface added: a vertex record is wider than a 64-word register,
    no vertex is among the prefetched ones and there is no LDS slot to read from"""
    base = open(cases.scene_path("test_many_lights.scn")).read()
    text = (base + "\nMaterial\nname mirror\nmirror rgb 0.813, 0.837, 0.888\nbdsfs mirror_bdsf\ndir_func sample_specular_direction\n"
            "\nMaterial\nname glass\nrefract csv glass.csv\nbdsfs fs_dielectric_reflectance_bdsf, fs_dielectric_transmittance_bdsf\n"
            "dir_func sample_reflect_or_transmit_direction\n"
            + _sphere("glass_ball", (-1.5, -1.8, 1.5), 1.0, "glass") + _plane("mirror_plane", (1.0, 2.0, -2.5), (1.0, -2.5, -2.9), (2.9, 2.0, -1.0), "mirror"))
    check("twelve_lights", text, 48, 12, 5, monkeypatch, need=(MIRROR, GLASS), seed=4)


@pytest.mark.parametrize("depth", [12, 40])
def test_deep_paths_between_two_mirrors(depth, monkeypatch):
    """a closed box with two facing mirrors and a glass sphere: vertices 8 and up (no visibility bit in the header; fetched when they
    are replayed, lifted by v_readlane) and, at depth 40, 16 and up (no plastic flag)"""
    deep = [((MIRROR, GLASS), 8)] + ([((MIRROR, GLASS), 16)] if depth > 16 else [])
    check("corridor_%d" % depth, mirror_corridor(), 32, 8, depth, monkeypatch, need=(MIRROR, GLASS), deep=deep, seed=6)


def test_camera_inside_the_glass_sphere(monkeypatch):
    """every path starts inside the glass: total internal reflection (ts_sin_sq >= 1) and the NaN vec3_transmit leaves behind"""
    text = box_scene(camera=_camera(position=(-1.5, -1.8, 2.2), target=(0.0, 0.0, 0.0)))
    check("inside_glass", text, 40, 12, 8, monkeypatch, need=(GLASS,))


def test_glass_met_from_inside_another_medium(monkeypatch):
    """a glass sphere inside a sphere of water: its vertices are met from a medium that is not the scene's base material, so the pair
    of media has no tabulated rows (`paired` false: the divisions of the untabulated form)"""
    text = box_scene(extra=_sphere("water_ball", (-1.5, -1.8, 2.0), 1.6, "water"), camera=_camera(position=(0.0, 0.0, 7.0), target=(-1.5, -1.8, 2.0), fov=60.0))
    check("nested_media", text, 40, 12, 8, monkeypatch, need=(GLASS,))


def test_simple_instantiation_mirror_only(monkeypatch):
    """an all-plastic box with a mirror plane takes the SIMPLE instantiation, which has the mirror's body only: fixed lists on and
    off there, and both again through the general instantiation (DRT_NO_SIMPLE_SHADE=1)"""
    text = simple_scene()
    check("simple", text, 48, 16, 8, monkeypatch, need=(MIRROR, PLASTIC))
    bundle = load(text, 48)
    p = pydrt.make_params(48, 48, spp=16, max_depth=8, seed=3, batch_spp=4)
    monkeypatch.delenv("DRT_NO_SIMPLE_SHADE", raising=False)
    simple = render(bundle, p)
    monkeypatch.setenv("DRT_NO_SIMPLE_SHADE", "1")
    general = on_and_off(bundle, p, monkeypatch, "simple scene, general instantiation")
    monkeypatch.delenv("DRT_NO_SIMPLE_SHADE")
    for a, b in zip(simple[0], general[0]):
        assert cases.same_bits(a, b)
    assert cases.stat_counts(simple[2]) == cases.stat_counts(general[2])
