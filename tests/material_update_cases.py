"""Material updates (drt_update_spectra, drt_update_materials): the cases of tests/test_material_update_cpu.py
and tests/test_gpu_material_update.py. A case is a scene before, the scene after -- the same surfaces, camera, material lists and SPD
indices, other values in some SPD rows or another shininess / roughness -- and the params both are rendered with. What an updated
context must equal is a fresh context on the "after" bundle, so nothing here knows how an update works. Materials are found by their
BDSF lists and names, never by position. Each case is the smallest place where one derived thing can go stale."""
import ctypes as C

import numpy as np

import cases
import pydrt

DIFFUSE, GLOSSY, MIRROR, FS_CONDUCTOR, FS_REFLECT, FS_TRANSMIT, CT_CONDUCTOR = range(7)  # pydrt.BDSF_NAMES

_cases = {}


def with_tables(bundle, spds=None, materials=None):
    """a bundle that shares `bundle`'s surfaces and camera and has an SPD table and a material array of its own"""
    spds = np.ascontiguousarray(bundle.spds() if spds is None else spds, dtype=np.float64)
    mats = bundle.materials() if materials is None else materials
    assert spds.shape[1] == bundle.S and len(mats) == int(bundle.scene.num_materials)
    sc = pydrt.Scene()
    C.memmove(C.byref(sc), C.byref(bundle.scene), C.sizeof(pydrt.Scene))
    sc.spds, sc.num_spds = spds.ctypes.data_as(C.POINTER(C.c_double)), spds.shape[0]
    sc.materials = C.cast(mats, C.POINTER(pydrt.Material))
    b = pydrt.SceneBundle(sc, bundle.camera, keep=(spds, mats, bundle))
    b.material_names = bundle.material_names  # the names are the loaded scene's
    return b


def bdsfs_of(m):
    return [int(b) for b in list(m.bdsfs)[:int(m.num_bdsfs)]]


def material(bundle, name=None, bdsfs=None, emissive=None, nth=0):
    """the index of the nth material with this name, this BDSF list, or this is_emissive"""
    names = bundle.material_names()
    found = []
    for i in range(int(bundle.scene.num_materials)):
        m = bundle.scene.materials[i]
        if name is not None and names[i] != name:
            continue
        if bdsfs is not None and bdsfs_of(m) != list(bdsfs):
            continue
        if emissive is not None and bool(m.is_emissive) != emissive:
            continue
        found.append(i)
    return found[nth]


def base_refract_row(bundle):
    return int(bundle.scene.materials[int(bundle.scene.base_material)].refract_spd)


def _params(p, hits=True, mode=None):
    q = pydrt.Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(pydrt.Params))
    q.batch_spp = 2
    if hits:
        q.flags = int(q.flags) | pydrt.FLAG_RECORD_HITS
    if mode is not None:
        q.mode = mode
    return q


def _case(before, after, params, same_log, bvh=False, forced=False, mode=None):
    return {"before": before, "after": after, "params": _params(params, mode=mode), "same_log": same_log, "bvh": bvh or forced, "forced": forced}


def tint(row, lo=0.35, hi=0.8):
    """another spectrum of the same kind: the row times a ramp over the wavelengths (no value repeats the old one, none leaves [0, 1])"""
    return row * np.linspace(lo, hi, row.shape[0])


def _edit_rows(scene, rows_of, same_log, **kw):
    """the scene's own bundle before; after: the rows rows_of(bundle) names, each through its function"""
    b, p = cases.load_case(scene)
    spds = b.spds()
    for row, f in rows_of(b).items():
        assert row >= 0 and row not in (int(b.scene.cmf_rw), int(b.scene.cmf_x), int(b.scene.cmf_y), int(b.scene.cmf_z))
        spds[row] = f(spds[row])
    return _case(b, with_tables(b, spds=spds), p, same_log, **kw)


def _glass_and_wall(b):
    """the glass's refract row (paths change) and a wall's diffuse row (a derived / PI row)"""
    glass = b.scene.materials[material(b, bdsfs=[FS_REFLECT, FS_TRANSMIT])]
    wall = b.scene.materials[material(b, name="red_plastic")]
    return {int(glass.refract_spd): lambda r: r * 1.12 + 0.03, int(wall.diffuse_spd): tint}


def _build(name):
    mat = lambda b, **kw: b.scene.materials[material(b, **kw)]
    if name == "wall_diffuse":  # the derived / PI row; plane_light_16 is a mixed scene: the trace kernel's tail columns too
        return _edit_rows("plane_light_16", lambda b: {int(mat(b, name="red_plastic").diffuse_spd): tint}, True)
    if name == "light_emission":  # the one light's row: the row light0_em_spd names
        return _edit_rows("plane_light_16", lambda b: {int(mat(b, emissive=True).emission_spd): lambda r: tint(r, 0.2, 1.4)}, True)
    if name == "large_box_diffuse":  # all-plastic: tail_all_staged
        return _edit_rows("large_box", lambda b: {int(mat(b, name="white_plastic").diffuse_spd): tint}, True)
    if name == "many_lights_emission":  # one of the 12 lights' three emission rows
        return _edit_rows("many_lights", lambda b: {int(mat(b, emissive=True, nth=1).emission_spd): lambda r: tint(r, 0.1, 2.0)}, True)
    if name == "glass_refract":  # the dielectric pair rows and refract_i0 / refract_i1: the paths through the glass change
        return _edit_rows("plane_light_16", lambda b: {int(mat(b, bdsfs=[FS_REFLECT, FS_TRANSMIT]).refract_spd): lambda r: r * 1.12 + 0.03}, False)
    if name in ("gold_mirror_conductor", "ggx_gold_conductor"):  # cA, cB; a conductor's n and k weigh a path and steer none
        scene, lobe = ("gold_mirror", FS_CONDUCTOR) if name == "gold_mirror_conductor" else ("plane_light_16", CT_CONDUCTOR)
        return _edit_rows(scene, lambda b: {int(mat(b, bdsfs=[lobe]).refract_spd): lambda r: r * 1.3 + 0.1,
                                            int(mat(b, bdsfs=[lobe]).extinct_spd): lambda r: tint(r, 0.6, 1.2)}, True)
    if name == "base_refract":  # the base material's refract row feeds every pair row
        return _edit_rows("plane_light_16", lambda b: {base_refract_row(b): lambda r: r * np.linspace(1.02, 1.2, r.shape[0])}, False)
    if name == "shared_row":  # two materials name one diffuse row: one derived row, shared
        b, p = cases.load_case("plane_light_16")
        mats = b.materials()
        shared = int(mats[material(b, name="white_plastic")].diffuse_spd)
        mats[material(b, name="red_plastic")].diffuse_spd = shared
        before = with_tables(b, materials=mats)
        spds = b.spds()
        spds[shared] = tint(spds[shared])
        return _case(before, with_tables(before, spds=spds), p, True)
    if name == "glossy_and_mirror":
        return _edit_rows("plane_light_16", lambda b: {int(mat(b, name="white_plastic").glossy_spd): tint,
                                                       int(mat(b, bdsfs=[MIRROR]).mirror_spd): lambda r: tint(r, 0.5, 0.95)}, True)
    if name in ("shininess", "roughness"):
        b, p = cases.load_case("plane_light_16")
        mats = b.materials()
        if name == "shininess":  # new drt_pow_shininess pairs; the lobe's power weighs a path and steers none
            mats[material(b, name="white_plastic")].shininess = 37.5
        else:  # the GGX sampler's roughness: paths change
            mats[material(b, bdsfs=[CT_CONDUCTOR])].roughness = 0.35
        return _case(b, with_tables(b, materials=mats), p, name == "shininess")
    if name in ("grid_10nm", "grid_4nm", "grid_2p5nm"):  # S = 35: no tail; 86: two sets, a tail too long for the trace kernel; 137: three sets
        return _edit_rows(name, _glass_and_wall, False)
    if name == "grid_2p5nm_60_rows":  # a table that cannot fit 64 KiB of LDS whatever the derived rows add: 60 * 137 * 8 > 65536
        b, p = cases.load_case("grid_2p5nm")
        spds = b.spds()
        extra = np.random.default_rng(60).uniform(0.0, 1.0, (60 - spds.shape[0], spds.shape[1]))
        before = with_tables(b, spds=np.concatenate([spds, extra]))
        assert int(before.scene.num_spds) == 60 and 60 * before.S * 8 > 65536
        spds = before.spds()
        for row, f in _glass_and_wall(b).items():
            spds[row] = f(spds[row])
        spds[59] = spds[59] * 0.5  # an unused row: it must arrive, and change nothing
        return _case(before, with_tables(before, spds=spds), p, False)
    if name == "spheres_1500":  # the hierarchy's kernels
        # (its spheres are plastic, mirror and GGX gold: a derived / PI row and a conductor's pair rows, and no edit that steers a path)
        return _edit_rows("spheres_1500", lambda b: {int(mat(b, bdsfs=[CT_CONDUCTOR]).refract_spd): lambda r: r * 1.3 + 0.1,
                                                     int(mat(b, bdsfs=[DIFFUSE, GLOSSY]).diffuse_spd): tint}, True, bvh=True)
    if name == "lights_bvh":  # test_lights.scn forced behind the tree: three kinds of light, thin glass
        return _edit_rows("lights", lambda b: {int(mat(b, bdsfs=[FS_TRANSMIT]).refract_spd): lambda r: r * 1.2 + 0.05,
                                               int(mat(b, name="warm_light").emission_spd): lambda r: tint(r, 0.2, 1.4)}, False, forced=True)
    if name == "xyz":
        return _edit_rows("plane_light_16", _glass_and_wall, False, mode=pydrt.MODE_XYZ)
    if name == "nan_and_zero":  # a NaN in the glass's refract row; a zero there and in the base material's at the same wavelength: 0 / 0 in both pair rows
        def rows(b):
            def holes(r):
                r = r.copy()
                r[3], r[7] = 0.0, np.nan
                return r

            def zero(r):
                r = r.copy()
                r[3] = 0.0
                return r
            return {int(mat(b, bdsfs=[FS_REFLECT, FS_TRANSMIT]).refract_spd): holes, base_refract_row(b): zero}
        return _edit_rows("plane_light_16", rows, True)  # (neither hole is at the two samples around 630 nm, which alone steer a path)
    raise KeyError(name)


SPECTRA = ["wall_diffuse", "light_emission", "large_box_diffuse", "many_lights_emission", "glass_refract", "gold_mirror_conductor",
           "ggx_gold_conductor", "base_refract", "shared_row", "glossy_and_mirror", "grid_10nm", "grid_4nm", "grid_2p5nm",
           "grid_2p5nm_60_rows", "spheres_1500", "lights_bvh", "xyz", "nan_and_zero"]
MATERIALS = ["shininess", "roughness"]
ALL = SPECTRA + MATERIALS


def load(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def light_level_rows(bundle, k):
    """what DRT_LIGHT_LEVELS gives drt_group_update_spectra for level k: (first_row, rows) -- the scene's own rows from the first to the
    last row an emissive material names as its emission, those rows times k (one multiplication per sample), the others as they are"""
    spds = bundle.spds()
    em = sorted({int(bundle.scene.materials[i].emission_spd) for i in range(int(bundle.scene.num_materials))
                 if bundle.scene.materials[i].is_emissive and int(bundle.scene.materials[i].emission_spd) >= 0})
    if not em:
        return 0, spds[0:0]
    rows = spds[em[0]:em[-1] + 1].copy()
    for r in em:
        rows[r - em[0]] = spds[r] * k
    return em[0], rows
