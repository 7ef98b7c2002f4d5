"""Lobe films without a GPU (-m "not gpu"): the premises of tests/test_gpu_lobes.py on the oracle alone, the sum identity's bound on the
oracle's restricted renders, restriction_is_exact by hand, the map checks and presets, the C-ABI as the header, the compiler and pydrt
see it, and the host program's refusals.

The rule is DESIGN.md, section 5n, and tests/lobe_rule.py. The expected films of the GPU tests are the existing oracle's renders of
bundles whose material lists are restricted in Python (tests/lobe_cases.py). The premises checked here: such an edit changes no hit
log and no draw count; the pixels test 3 compares exist in the numbers DESIGN 5n states; the classes' films differ from one another
and from the main film, so a kernel that ignores the map cannot pass; and the restricted renders add up to the main film within the
bound gamma the GPU test holds the device to."""
import ctypes as C
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import lobe_cases as LC
import lobe_rule as LR
import pydrt

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")
F = LR.F


# ------------------------------------------------------------------------------------------------ the premises on the oracle
@pytest.mark.parametrize("name", LC.DIRECT_CASES)
def test_direct_layers_of_the_oracle_keep_the_paths_and_differ(name):
    """test 2's expected films: list edits leave hit log and statistics alone (asserted where the render is made), every class that
    receives direct light differs from the main film at depth 1, and every two such classes differ from one another"""
    lists = LC.material_lists(LC.load(name)[0])
    main = LC.oracle_film(name, False, max_depth=1)
    classes = [cls for n, cls in LC.direct_pairs() if n == name]
    assert classes, name
    films = {cls: LC.oracle_film(name, False, LR.CLASSES[cls], max_depth=1) for cls in classes}
    # (light sampled at a mirror, a smooth conductor or glass meets the one direction that reflects or refracts with probability zero:
    # those classes' direct layers are the emission alone, as the render restricted to nothing is)
    none = LC.oracle_film(name, False, (), max_depth=1)
    keeps = [cls for cls in classes if any(LR.restrict(lst, LR.CLASSES[cls]) for lst in lists) and not cases.same_bits(films[cls][0], none[0])]
    assert len(keeps) >= 2 and {"diffuse", "glossy"} <= set(keeps), "%s: fewer than two classes receive direct light" % name
    for cls in keeps:
        assert not cases.same_bits(films[cls][0], main[0]), "%s: class %s is the whole film" % (name, cls)
    for a, b in itertools.combinations(keeps, 2):
        assert not cases.same_bits(films[a][0], films[b][0]), "%s: classes %s and %s give the same film" % (name, a, b)
    for cls in classes:
        assert np.array_equal(films[cls][0][:, -1], main[0][:, -1])


def test_which_direct_pairs_are_exact():
    pairs = LC.direct_pairs()
    # the glass of the Cornell scenes lists [reflectance, transmittance]: transmittance carries reflectance's value over
    for name in ("plane_light_16", "gold_mirror", "lens"):
        assert (name, "transmission") not in pairs and {(name, c) for c in ("diffuse", "glossy", "specular")} <= set(pairs)
    # test_lights has a transmittance-only material, and test_many_lights no glass at all: every class passes
    for name in ("lights", "many_lights"):
        assert {(name, c) for c in LR.CLASSES} <= set(pairs)
    assert [F["fs_dielectric_transmittance_bdsf"]] in LC.material_lists(LC.load("lights")[0])


@pytest.mark.parametrize("name", sorted(LC.INDIRECT_PIXELS))
def test_the_pixels_of_the_depth_two_comparison(name):
    for material, count in LC.INDIRECT_PIXELS[name].items():
        pixels = LC.qualifying_pixels(name, material)
        assert len(pixels) == count and count >= 3, "%s, material %d: %d pixels" % (name, material, len(pixels))


@pytest.mark.parametrize("name, material, cls", LC.indirect_triples(), ids=["%s-m%d-%s" % t for t in LC.indirect_triples()])
def test_depth_two_layers_of_the_oracle_keep_the_paths(name, material, cls):
    """test 3's expected films; where the class drops something of the material's list the film differs from the main film on the
    pixels compared"""
    main = LC.oracle_film(name, False, max_depth=2)
    film = LC.oracle_film(name, False, LR.CLASSES[cls], only_material=material, max_depth=2)
    pixels = LC.qualifying_pixels(name, material)
    lst = LC.material_lists(LC.load(name)[0])[material]
    if LR.restrict(lst, LR.CLASSES[cls]) != lst:
        assert not cases.same_bits(film[0][pixels], main[0][pixels]), "%s, material %d, %s: nothing was dropped" % (name, material, cls)
    else:
        assert cases.same_bits(film[0], main[0])


def test_the_triples_are_the_ones_the_issue_names():
    triples = LC.indirect_triples()
    assert {(n, m) for n, m, _ in triples} == {(n, m) for n, mats in LC.INDIRECT_PIXELS.items() for m in mats}
    assert ("lights", 4, "transmission") in triples and ("lights", 5, "specular") in triples and ("gold_mirror", 8, "specular") in triples
    assert ("plane_light_16", 2, "diffuse") in triples and ("plane_light_16", 2, "glossy") in triples


# ------------------------------------------------------------------------------------------------ the sum identity
@pytest.mark.parametrize("name", ("lights", "many_lights"))
def test_the_direct_layers_add_up_to_the_depth_one_film_within_gamma(name):
    """every class is exact in these two cases, so on the pixels none of whose samples ended on an emitter (the render restricted to
    nothing is +0 there) the four classes' depth-1 renders are a partition of the depth-1 film's polynomial"""
    main = LC.oracle_film(name, False, max_depth=1)[0]
    none = LC.oracle_film(name, False, (), max_depth=1)[0]
    rows = np.flatnonzero(~none[:, :-1].any(axis=1))
    assert len(rows) >= 50
    films = [LC.oracle_film(name, False, LR.CLASSES[cls], max_depth=1)[0][rows] for cls in sorted(LR.CLASSES)]
    g = LC.gamma_for(name, len(films), max_depth=1)
    bad, worst = LR.sum_identity_violations(films, main[rows], g)
    print("%s: %d rows, worst |sum - main| / magnitude = %.3g, gamma = %.3g" % (name, len(rows), worst, g))
    assert bad == 0 and (main[rows][:, :-1] != 0).any()


@pytest.mark.parametrize("name, material", [(n, m) for n, mats in LC.INDIRECT_PIXELS.items() for m in mats])
def test_the_depth_two_layers_add_up_within_gamma(name, material):
    triples = [t for t in LC.indirect_triples() if t[:2] == (name, material)]
    pixels = LC.qualifying_pixels(name, material)
    main = LC.oracle_film(name, False, max_depth=2)[0][pixels]
    films = [LC.oracle_film(name, False, LR.CLASSES[cls], only_material=material, max_depth=2)[0][pixels] for _, _, cls in triples]
    lst = LC.material_lists(LC.load(name)[0])[material]
    assert sorted(f for _, _, cls in triples for f in LR.restrict(lst, LR.CLASSES[cls])) == sorted(lst), "the classes partition the list"
    g = LC.gamma_for(name, len(films), max_depth=2)
    bad, worst = LR.sum_identity_violations(films, main, g)
    print("%s, material %d: worst %.3g, gamma %.3g" % (name, material, worst, g))
    assert bad == 0


def test_the_bound_itself():
    assert LR.gamma(8, 1, 4, 7) == 2.0 * (40 + 3 + 17 + 4 + 7) * 2.0 ** -53
    one = np.array([[1.0, 2.0, 4.0]])
    assert LR.sum_identity_violations([one, one], np.array([[2.0, 4.0, 4.0]]), 1e-16)[0] == 0
    assert LR.sum_identity_violations([one, one], np.array([[2.0, 4.5, 4.0]]), 1e-16)[0] == 1
    # NaN for NaN, and a NaN on one side only is a violation; tiny negative values count by their magnitude
    nan = np.array([[np.nan, 1.0, 4.0]])
    assert LR.sum_identity_violations([nan], nan, 1e-16)[0] == 0 and LR.sum_identity_violations([nan], np.array([[0.0, 1.0, 4.0]]), 1e-16)[0] == 1
    assert LR.sum_identity_violations([np.array([[-8e-18, 0.0]]), np.array([[8e-18, 0.0]])], np.array([[0.0, 0.0]]), 1e-16)[0] == 0


# ------------------------------------------------------------------------------------------------ the rule's pieces
def test_restriction_is_exact_by_hand_on_the_shipped_lists():
    d, g, m, c, r, t, ct = (F[n] for n in LR.FUNCTIONS)
    plastic, glass = [d, g], [r, t]
    for K in LR.CLASSES.values():
        assert LR.restriction_is_exact(plastic, K) and LR.restriction_is_exact([m], K) and LR.restriction_is_exact([c], K)
        assert LR.restriction_is_exact([ct], K) and LR.restriction_is_exact([t], K) and LR.restriction_is_exact([], K) and LR.restriction_is_exact([d], K)
    assert LR.restriction_is_exact(glass, LR.CLASSES["specular"])          # reflectance comes first
    assert not LR.restriction_is_exact(glass, LR.CLASSES["transmission"])  # transmittance carries reflectance's value over
    assert LR.restriction_is_exact(glass, LR.CLASSES["diffuse"]) and LR.restriction_is_exact(glass, {r, t})
    # a conditional function behind one that is dropped is not exact; behind a kept one, or in front, it is
    assert not LR.restriction_is_exact([d, m], {m}) and LR.restriction_is_exact([m, d], {m}) and LR.restriction_is_exact([d, m], {d, m})
    assert LR.restriction_is_exact([d, m], {d}) and not LR.restriction_is_exact([m, t, g], {t, g}) and LR.restriction_is_exact([m, t, g], {m, g})
    assert LR.restrict([d, g, m], {g, m}) == [g, m] and LR.restrict(glass, {d}) == []
    shipped = {tuple(lst) for name in LC.ALL_CASES for lst in LC.material_lists(LC.load(name)[0])}
    assert shipped == {(), (d, g), (d,), (m,), (c,), (r, t), (t,), (ct,)}
    assert LR.ALWAYS_ASSIGN == {d, g, ct}
    assert sorted(f for K in LR.CLASSES.values() for f in K) == list(range(LR.NUM)), "the classes partition the functions"


def test_the_map_checks():
    ok = LR.all_to(0)
    assert LR.map_error(1, ok) is None and LR.map_error(0, None) is None and LR.map_error(8, LR.all_to(7)) is None
    assert "at most 8" in LR.map_error(9, ok) and LR.map_error(1, None) == "null map"
    assert "names film 1 of 1" in LR.map_error(1, LR.all_to(1)) and "names film 3 of 3" in LR.map_error(3, LR.entries(0, {0: 3}, {}))
    assert LR.map_error(1, LR.all_to(LR.NONE)) is None and LR.map_error(2, LR.entries(1, {"mirror_bdsf": 0}, {6: 1})) is None
    assert LR.films_needed(LR.all_to(LR.NONE)) == 1 and LR.films_needed(LR.entries(0, {0: 5}, {})) == 6
    e = LR.entries(2, {"bp_glossy_bdsf": 1}, {"ct_conductor_bdsf": 0}, default=3)
    assert e == [2, 3, 1, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 0] and len(LR.all_to(4)) == 15
    assert LR.class_direct_map(LR.CLASSES["glossy"]) == [0, 1, 0, 1, 1, 1, 1, 0] + [1] * 7
    assert LR.class_map(LR.CLASSES["transmission"]) == [0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1]


def test_the_presets_are_pydrts_and_the_headers():
    assert sorted(pydrt.LOBE_PRESETS) == sorted(LR.PRESETS) == ["functions", "standard"]
    for name, (want, names) in LR.PRESETS.items():
        m, got_names = pydrt.LOBE_PRESETS[name]
        assert pydrt.lobe_map_entries(m) == want and list(got_names) == names and pydrt.lobe_map_films(m) == len(names) == LR.films_needed(want)
        assert LR.map_error(len(names), want) is None and LR.NONE not in want
    want, names = LR.PRESETS["functions"]
    assert len(names) == 8 and want == [0] + list(range(1, 8)) * 2
    want, names = LR.PRESETS["standard"]
    assert len(names) == 7 and want == [0, 1, 3, 5, 5, 5, 6, 3, 2, 4, 5, 5, 5, 6, 4]
    assert tuple(pydrt.BDSF_NAMES) == LR.FUNCTIONS and pydrt.LOBE_NONE == LR.NONE == 0xFF and pydrt.MAX_LOBE_FILMS == LR.MAX_LOBE_FILMS == 8


def test_lobe_map_builds_and_refuses():
    m = pydrt.lobe_map(emission=0, direct={"bp_diffuse": 1, "mirror_bdsf": 2}, indirect={"ct_conductor": 3})
    assert pydrt.lobe_map_entries(m) == LR.entries(0, {"bp_diffuse_bdsf": 1, "mirror_bdsf": 2}, {"ct_conductor_bdsf": 3})
    assert pydrt.lobe_map_films(m) == 4 and C.sizeof(pydrt.LobeMap) == 16
    assert pydrt.lobe_map_entries(pydrt.lobe_map(default=2)) == LR.all_to(2) and pydrt.lobe_map_entries(pydrt.lobe_map()) == LR.all_to(LR.NONE)
    for bad in (dict(emission=8), dict(emission=-1), dict(direct={"bp_diffuse": 300}), dict(default=9)):
        with pytest.raises(ValueError, match="a film 0 .. 7 or LOBE_NONE"):
            pydrt.lobe_map(**bad)
    with pytest.raises(ValueError, match="unknown scattering function"):
        pydrt.lobe_map(indirect={"lambert": 0})
    assert pydrt._lobe_bind_args(None, None) == (0, None) and pydrt._lobe_bind_args("standard", None)[0] == 7
    assert pydrt._lobe_bind_args(m, None) == (4, m) and pydrt._lobe_bind_args(m, 6) == (6, m)
    with pytest.raises(ValueError, match="unknown preset"):
        pydrt._lobe_bind_args("cryptomatte", None)
    with pytest.raises(TypeError, match="bind_lobes"):
        pydrt._lobe_bind_args([0] * 15, None)
    with pytest.raises(ValueError, match="bind_lobes: n"):
        pydrt._lobe_bind_args(m, -1)


def test_the_film_level_rule_is_one_bucket():
    c = np.stack([np.array([[3.0, -1.0]]), np.array([[1.0, 0.5]]), np.array([[2.0, -0.25]])])
    px, av, va = LR.film_of_samples(c)
    assert np.array_equal(px, [[6.0, -0.75, 3.0]]) and np.array_equal(av, [[2.0, -0.25]]) and np.array_equal(va, [[2.0, 1.125]])
    # a film that starts at sample 5 divides by 6
    px, av, va = LR.film_of_samples(np.array([[[6.0, 9.0]]]), first_sample=5)
    assert np.array_equal(av, [[1.0, 1.5]]) and px[0, 2] == 1.0
    px, av, va = LR.empty_film(3, 2, [5, 6, 7])
    assert not px[:, :2].any() and not av.any() and not va.any() and np.array_equal(px[:, 2], [3.0, 3.0, 3.0])
    assert not np.signbit(px).any() and not np.signbit(av).any() and not np.signbit(va).any()


# ------------------------------------------------------------------------------------------------ the interface
CALLS = {
    "drt_bind_lobes": "int (*%s)(drt_context *, uint32_t, const drt_lobe_map *)",
    "drt_read_lobe_film": "int (*%s)(drt_context *, uint32_t, double *, double *, double *)",
    "drt_lobe_film_device_ptrs": "int (*%s)(drt_context *, uint32_t, void **, void **, void **)",
    "drt_read_lobe_xyz": "int (*%s)(drt_context *, uint32_t, double *)",
    "drt_read_lobe_bgra": "int (*%s)(drt_context *, uint32_t, int, uint8_t *)",
    "drt_group_bind_lobes": "int (*%s)(drt_group *, uint32_t, const drt_lobe_map *)",
    "drt_group_read_lobe_film": "int (*%s)(drt_group *, uint32_t, double *, double *, double *)",
}


def test_the_header_the_compiler_and_pydrt_agree_on_the_calls(tmp_path):
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for call in CALLS:
        assert re.search(r"\bint %s\(" % call, plain) and call in pydrt.HIP_SYMBOLS, call
    assert re.search(r"#define DRT_MAX_LOBE_FILMS\s+8\b", header) and re.search(r"#define DRT_LOBE_NONE\s+0xFFu", header)
    src = tmp_path / "lobes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "drt_hip.h"\n'
                   + "".join("%s = %s;\n" % (proto % ("f%d" % k), call) for k, (call, proto) in enumerate(CALLS.items()))
                   + "typedef char map_is_16_bytes[sizeof(drt_lobe_map) == 16 ? 1 : -1];\n"
                   + "typedef char rows_of_seven[sizeof(((drt_lobe_map *)0)->direct) == 7 && sizeof(((drt_lobe_map *)0)->indirect) == 7 ? 1 : -1];\n"
                   + "typedef char layout[offsetof(drt_lobe_map, emission) == 0 && offsetof(drt_lobe_map, direct) == 1 && offsetof(drt_lobe_map, indirect) == 8 ? 1 : -1];\n"
                   + 'int main(void) { drt_lobe_map m = { 0, { 0 }, { 0 }, 0 }; m.direct[DRT_NUM_BDSFS - 1] = DRT_LOBE_NONE;\n'
                   + '  printf("%d %u\\n", DRT_MAX_LOBE_FILMS, (unsigned)m.direct[6]); return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "lobes.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = pydrt.hip_lib()
    f64p, vpp, u8p, mapp = C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_uint8), C.POINTER(pydrt.LobeMap)
    assert L.drt_bind_lobes.argtypes == [C.c_void_p, C.c_uint32, mapp]
    assert L.drt_read_lobe_film.argtypes == [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
    assert L.drt_lobe_film_device_ptrs.argtypes == [C.c_void_p, C.c_uint32, vpp, vpp, vpp]
    assert L.drt_read_lobe_xyz.argtypes == [C.c_void_p, C.c_uint32, f64p]
    assert L.drt_read_lobe_bgra.argtypes == [C.c_void_p, C.c_uint32, C.c_int, u8p]
    assert L.drt_group_bind_lobes.argtypes == [C.c_void_p, C.c_uint32, mapp]
    assert L.drt_group_read_lobe_film.argtypes == [C.c_void_p, C.c_uint32, f64p, f64p, f64p]
    assert [n for n, _ in pydrt.LobeMap._fields_] == ["emission", "direct", "indirect", "pad_"]
    # a null context or group is refused with a message, without a device
    assert L.drt_bind_lobes(None, 0, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_read_lobe_film(None, 0, None, None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_lobe_film_device_ptrs(None, 0, None, None, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_read_lobe_xyz(None, 0, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_read_lobe_bgra(None, 0, 1, None) != 0 and b"null context" in L.drt_last_error()
    assert L.drt_group_bind_lobes(None, 0, None) != 0 and b"null group" in L.drt_last_error()
    assert L.drt_group_read_lobe_film(None, 0, None, None, None) != 0 and b"null group" in L.drt_last_error()


def test_pydrt_signatures_and_the_checks_it_alone_can_make():
    for cls in (pydrt.Renderer, pydrt.Group):
        assert list(inspect.signature(cls.bind_lobes).parameters) == ["self", "map_or_preset", "n"]
        assert inspect.signature(cls.bind_lobes).parameters["n"].default is None
        assert list(inspect.signature(cls.read_lobe_film).parameters) == ["self", "c"]
    assert list(inspect.signature(pydrt.Renderer.lobe_film_device_ptrs).parameters) == ["self", "c"]
    assert list(inspect.signature(pydrt.Renderer.read_lobe_xyz).parameters) == ["self", "c"]
    assert list(inspect.signature(pydrt.Renderer.read_lobe_bgra).parameters) == ["self", "c", "which"]
    assert list(inspect.signature(pydrt.lobe_map).parameters) == ["emission", "direct", "indirect", "default"]
    assert inspect.signature(pydrt.lobe_map).parameters["default"].default == pydrt.LOBE_NONE
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="read_lobe_film: c"):
            pydrt._u32(bad, "read_lobe_film: c")


# ------------------------------------------------------------------------------------------------ the host program
@pytest.mark.parametrize("env, message", [
    ({"DRT_LOBES": ""}, 'DRT_LOBES="": standard or functions'),
    ({"DRT_LOBES": "Standard"}, 'DRT_LOBES="Standard": standard or functions'),
    ({"DRT_LOBES": "standard,functions"}, "standard or functions"),
    ({"DRT_LOBES": "7"}, 'DRT_LOBES="7": standard or functions'),
    ({"DRT_LOBES": "functions", "LONG_NAME": "1"}, "an output name with .lobe7.spd or .lobes.txt behind it is longer than 63 characters"),
    ({"DRT_LOBES": "standard", "DRT_BUCKETS": "2"}, "DRT_LOBES cannot be combined with DRT_BUCKETS"),
    ({"DRT_LOBES": "standard", "DRT_ADAPTIVE_ERROR": "0.1"}, "DRT_LOBES cannot be combined with DRT_ADAPTIVE_ERROR"),
    ({"DRT_LOBES": "standard", "DRT_CHECKPOINT_SPP": "1"}, "DRT_LOBES cannot be combined with DRT_CHECKPOINT_SPP"),
    ({"DRT_LOBES": "standard", "DRT_RESUME": "1"}, "DRT_LOBES cannot be combined with DRT_RESUME"),
    ({"DRT_LOBES": "standard", "DRT_TURNTABLE": "2"}, "DRT_LOBES cannot be combined with DRT_TURNTABLE"),
    ({"DRT_LOBES": "functions", "DRT_LIGHT_LEVELS": "1,2"}, "DRT_LOBES cannot be combined with DRT_LIGHT_LEVELS"),
    ({"DRT_LOBES": "functions", "DRT_DEPTH_CUTS": "1,2"}, "DRT_LOBES cannot be combined with DRT_DEPTH_CUTS"),
    ({"DRT_LOBES": "functions", "DRT_SENSOR": "r.csv"}, "DRT_LOBES cannot be combined with DRT_SENSOR"),
    ({"DRT_LOBES": "functions", "DRT_REGIONS": "0,0,4,4:8"}, "DRT_LOBES cannot be combined with DRT_REGIONS"),
])
def test_the_host_refuses_bad_lobes_before_any_device_call(tmp_path, env, message):
    """Exit status nonzero, the reason on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run that got as
    far as the launcher would fail there with the launcher's message instead."""
    cfg = open(os.path.join(REPO, "config.cfg")).read()
    env = dict(env)
    if env.pop("LONG_NAME", None):
        cfg, k = re.subn(r"(?m)^variance_spd\s+\S+", "variance_spd      output/" + "v" * 44 + ".spd", cfg)  # fits by itself, not with .lobe7.spd
        assert k == 1
    (tmp_path / "config.cfg").write_text(cfg)
    os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
    os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    (tmp_path / "r.csv").write_text("wavelength,value\n380,0\n600,1\n720,0.5\n")
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout
