"""Lobe films (drt_bind_lobes): the shared cases and expected films.

Expected films need no oracle code of their own. They are the existing oracle's renders of bundles whose material lists are edited in
Python: restricted() drops list entries and keeps dir_func and everything else, so no path changes -- the BDSF list never steers a
path -- and hit logs and draw counts stay what they are (asserted wherever a restricted render is made).

  - direct layers (test 2): film 0 of class_direct_map(K) at the case's own depth is the oracle's render at max_depth = 1 of the bundle
    with EVERY list restricted to K, wherever restriction_is_exact holds for every material;
  - direct plus indirect (test 3): film 0 of class_map(K) at max_depth = 2 is the oracle's depth-2 render of the bundle with ONLY
    material M restricted to K, on the pixels whose samples all hit M first and never hit M second (from the hit log).
Everything is made once per key and shared; nothing writes to what these functions return."""
import contextlib
import ctypes as C

import numpy as np

import cases
import lobe_rule as LR
import oracle_py as O
import pydrt
import sensor_cases as SC

BASE = SC.BASE
load, params_with, assert_film = SC.load, SC.params_with, SC.assert_film

# test 1 and test 4: every case of the all-to-one test
ALL_CASES = ("plane_light_16", "grid_10nm", "grid_2p5nm", "gold_mirror", "many_lights", "deep_paths", "lens", "lights", "first_scene", "spheres_1500",
             "example_scene")
# test 2: (case, class) wherever the restriction is exact for every material of the case
DIRECT_CASES = ("plane_light_16", "gold_mirror", "many_lights", "lights", "lens")
# test 3: case -> {material: qualifying pixels}, measured on the CPU oracle at max_depth = 2 (tests/test_lobes_cpu.py asserts them)
INDIRECT_PIXELS = {"plane_light_16": {2: 10, 3: 17, 4: 14}, "lights": {2: 302, 3: 171, 4: 43, 5: 9}, "gold_mirror": {8: 4}}

_cache = {}


def material_lists(bundle):
    return [[int(m.bdsfs[j]) for j in range(m.num_bdsfs)] for m in bundle.materials()]


def direct_pairs():
    """the (case, class) pairs of test 2"""
    out = []
    for name in DIRECT_CASES:
        lists = material_lists(load(name)[0])
        for cls in sorted(LR.CLASSES):
            if all(LR.restriction_is_exact(lst, LR.CLASSES[cls]) for lst in lists):
                out.append((name, cls))
    return out


def indirect_triples():
    """the (case, material, class) triples of test 3: the classes that keep something of the material's list, exactly"""
    out = []
    for name, mats in INDIRECT_PIXELS.items():
        lists = material_lists(load(name)[0])
        for m in sorted(mats):
            for cls in sorted(LR.CLASSES):
                if LR.restrict(lists[m], LR.CLASSES[cls]) and LR.restriction_is_exact(lists[m], LR.CLASSES[cls]):
                    out.append((name, m, cls))
    return out


@contextlib.contextmanager
def restricted(bundle, functions, only_material=None):
    """the bundle with its lists (or only material `only_material`'s) restricted to `functions`, for the time of the block. The scene's
    `materials` field is a pointer: its ADDRESS is saved and put back (reading the field gives an object that aliases it)."""
    mats = bundle.materials()
    for i, m in enumerate(mats):
        if only_material is not None and i != only_material:
            continue
        keep = LR.restrict([int(m.bdsfs[j]) for j in range(m.num_bdsfs)], functions)
        for j in range(len(m.bdsfs)):
            m.bdsfs[j] = keep[j] if j < len(keep) else 0
        m.num_bdsfs = len(keep)
    saved = C.cast(bundle.scene.materials, C.c_void_p).value
    try:
        bundle.scene.materials = C.cast(mats, C.POINTER(pydrt.Material))
        yield bundle
    finally:
        bundle.scene.materials = C.cast(C.c_void_p(saved), C.POINTER(pydrt.Material))
    assert C.cast(bundle.scene.materials, C.c_void_p).value == saved


def _render(bundle, p, device):
    if device:
        return cases.oracle_render_device_pow(bundle, p, want_hits=True, num_threads=16)
    return O.oracle_render_tile(bundle, p, want_hits=True, num_threads=16, math_mode=O.MATH_DEVICE)


def oracle_film(name, device, functions=None, only_material=None, **changes):
    """(pixels, means, variances, hits, stats) of the oracle's render of the case -- with lists restricted when `functions` is given.
    device: the glossy power from the device (GPU tests) or from glibc (CPU tests)."""
    key = (name, device, None if functions is None else tuple(sorted(functions)), only_material, tuple(sorted(changes.items())))
    if key not in _cache:
        bundle, params = load(name)
        p = params_with(params, **changes)
        if functions is None:
            _cache[key] = _render(bundle, p, device)
        else:
            with restricted(bundle, frozenset(functions), only_material):
                _cache[key] = _render(bundle, p, device)
            plain = oracle_film(name, device, **changes)
            assert np.array_equal(plain[3], _cache[key][3]), "%s: a list edit changed the hit log" % name
            assert cases.stat_counts(plain[4]) == cases.stat_counts(_cache[key][4]), "%s: a list edit changed the path statistics" % name
    return _cache[key]


def surface_materials(bundle):
    return np.array([int(bundle.scene.surfaces[i].material) for i in range(int(bundle.scene.num_surfaces))], dtype=np.int64)


# test 3's one exception to "never hit M second": test_lights' transmittance-only sphere. Every second vertex of a path that enters it
# is inside it, so no pixel passes the condition, while the issue's table counts the 43 pixels whose samples all hit it first. Its list
# lies in one class, so the bundle "with only M restricted to K" is the unedited bundle and the condition has nothing to protect.
SECOND_HIT_EXEMPT = {("lights", 4)}


def qualifying_pixels(name, material, device=False):
    """pixels (indices into the tile) whose samples at max_depth = 2 all hit `material` first and never hit it second (the second
    condition not for SECOND_HIT_EXEMPT). The hit log is sample-major: row s * P + p."""
    key = ("pixels", name, material, device)
    if key not in _cache:
        bundle, params = load(name)
        hits = oracle_film(name, device, max_depth=2)[3]
        spp = int(params.spp)
        surf = surface_materials(bundle)
        mat = np.where(hits >= 0, surf[np.clip(hits, 0, len(surf) - 1)], -1).reshape(spp, -1, 2)
        ok = (mat[:, :, 0] == material).all(axis=0)
        if (name, material) in SECOND_HIT_EXEMPT:
            lst = material_lists(bundle)[material]
            assert any(LR.restrict(lst, K) == lst for K in LR.CLASSES.values()), "the exemption holds only where no class drops anything"
        else:
            ok &= (mat[:, :, 1] != material).all(axis=0)
        _cache[key] = np.flatnonzero(ok)
    return _cache[key]


def n_lights(bundle):
    """emissive materials' surfaces: what the light fold runs over"""
    mats = bundle.materials()
    return sum(1 for i in range(int(bundle.scene.num_surfaces)) if mats[int(bundle.scene.surfaces[i].material)].is_emissive)


def gamma_for(name, n, **changes):
    bundle, params = load(name)
    p = params_with(params, **changes)
    return LR.gamma(int(p.max_depth), n_lights(bundle), int(p.spp), n)


def to_map(e):
    """a lobe_rule entries list as the pydrt.LobeMap the library takes"""
    m = pydrt.LobeMap()
    m.emission = e[0]
    for f in range(LR.NUM):
        m.direct[f] = e[1 + f]
        m.indirect[f] = e[1 + LR.NUM + f]
    return m


def assert_films(got, want, what):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert_film(g, w, "%s, film %d of %d" % (what, c, len(want)))
