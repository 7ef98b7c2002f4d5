"""CPU (-m "not gpu"): the premises of tests/test_gpu_material_update.py, checked with the oracle. Every "after" scene of
tests/material_update_cases.py renders another film than its "before" scene, so no GPU test can pass by doing nothing. The hit log
differs where the edit steers a path -- the glass's and the base material's refract row (the refraction sampler reads the index at
630 nm), the GGX roughness -- and is equal where it only weighs one: a diffuse, emission, glossy or mirror row, shininess, and a
conductor's n and k (the specular and the GGX sampler read neither). SceneBundle.materials() round-trips byte for byte; the program
refuses what DRT_LIGHT_LEVELS cannot be combined with before any device call; its row arithmetic is numpy's."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

import cases
import material_update_cases as MU
import oracle_py as O
import pydrt


def oracle(bundle, params):
    px, av, va, hits, st = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_DEVICE)
    return (px, av, va), hits, st


def fixed_fields(m):
    return (int(m.is_black_body), int(m.is_emissive), int(m.num_bdsfs), MU.bdsfs_of(m), int(m.dir_func), int(m.emission_spd), int(m.diffuse_spd),
            int(m.glossy_spd), int(m.mirror_spd), int(m.refract_spd), int(m.extinct_spd))


@pytest.mark.parametrize("name", MU.ALL)
def test_the_after_scene_renders_another_film_and_the_hit_log_says_what_steers_a_path(name):
    c = MU.load(name)
    p = c["params"]
    assert int(p.spp) <= 4 and int(p.tile_w) <= 32 and int(p.tile_h) <= 32 and int(p.flags) & pydrt.FLAG_RECORD_HITS and int(p.batch_spp) == 2
    b, a = c["before"].scene, c["after"].scene
    # what an update fixes: the surfaces, the table's size, every material field but shininess and roughness, the observer's rows
    assert int(b.num_surfaces) == int(a.num_surfaces) and int(b.num_materials) == int(a.num_materials)
    assert (int(b.num_spds), int(b.num_wavelengths)) == (int(a.num_spds), int(a.num_wavelengths))
    assert C.string_at(b.surfaces, int(b.num_surfaces) * C.sizeof(pydrt.Surface)) == C.string_at(a.surfaces, int(a.num_surfaces) * C.sizeof(pydrt.Surface))
    for i in range(int(b.num_materials)):
        assert fixed_fields(b.materials[i]) == fixed_fields(a.materials[i]), i
    sb, sa = c["before"].spds(), c["after"].spds()
    for row in (int(b.cmf_rw), int(b.cmf_x), int(b.cmf_y), int(b.cmf_z)):
        assert np.array_equal(sb[row], sa[row])
    rows_differ = not cases.same_bits(sb, sa)
    params_differ = any((b.materials[i].shininess, b.materials[i].roughness) != (a.materials[i].shininess, a.materials[i].roughness)
                        for i in range(int(b.num_materials)))
    assert rows_differ == (name in MU.SPECTRA) and params_differ == (name in MU.MATERIALS)
    t0 = time.perf_counter()
    film_b, log_b, _ = oracle(c["before"], p)
    film_a, log_a, _ = oracle(c["after"], p)
    assert time.perf_counter() - t0 < 20.0  # both renders: a case stays a matter of seconds
    for fb, fa in zip(film_b, film_a):
        assert not cases.same_bits(fb, fa)
    assert np.array_equal(log_b, log_a) == c["same_log"]
    with np.errstate(invalid="ignore"):
        assert np.any(film_a[0][:, :-1] != 0.0)  # and the "after" film is not black


def test_the_cases_are_what_they_say():
    for name in MU.ALL:
        c = MU.load(name)
        n = int(c["before"].scene.num_surfaces)
        assert (n > 96) == (c["bvh"] and not c["forced"]), name
    assert [MU.load(n)["before"].S for n in ("grid_10nm", "grid_4nm", "grid_2p5nm", "grid_2p5nm_60_rows")] == [35, 86, 137, 137]
    c = MU.load("grid_2p5nm_60_rows")
    assert int(c["before"].scene.num_spds) >= 60 and int(c["before"].scene.num_spds) * 137 * 8 > 65536
    c = MU.load("shared_row")
    rows = [int(c["before"].scene.materials[i].diffuse_spd) for i in range(int(c["before"].scene.num_materials))]
    shared = [r for r in set(rows) if r >= 0 and rows.count(r) == 2]
    assert len(shared) == 1 and not np.array_equal(c["before"].spds()[shared[0]], c["after"].spds()[shared[0]])
    assert int(MU.load("xyz")["params"].mode) == pydrt.MODE_XYZ
    c = MU.load("nan_and_zero")
    glass = int(c["after"].scene.materials[MU.material(c["after"], bdsfs=[MU.FS_REFLECT, MU.FS_TRANSMIT])].refract_spd)
    base = MU.base_refract_row(c["after"])
    sa = c["after"].spds()
    zero = np.flatnonzero((sa[glass] == 0.0) & (sa[base] == 0.0))
    assert len(zero) == 1 and np.isnan(sa[glass]).sum() == 1  # 0 / 0 in both pair rows at one wavelength, a NaN at another
    c = MU.load("many_lights_emission")
    assert sum(1 for i in range(int(c["before"].scene.num_surfaces))
               if c["before"].scene.materials[int(c["before"].scene.surfaces[i].material)].is_emissive) == 12


@pytest.mark.parametrize("name", ["plane_light_16", "spheres_1500"])
def test_materials_round_trip_byte_for_byte(name):
    bundle, _ = cases.load_case(name)
    n = int(bundle.scene.num_materials)
    raw = C.string_at(bundle.scene.materials, n * C.sizeof(pydrt.Material))
    mats = bundle.materials()
    assert len(mats) == n and C.string_at(mats, n * C.sizeof(pydrt.Material)) == raw
    mats[2].shininess = 3.0  # a copy: the scene's own array stays
    assert C.string_at(bundle.scene.materials, n * C.sizeof(pydrt.Material)) == raw
    again = MU.with_tables(bundle, materials=bundle.materials())
    assert C.string_at(again.scene.materials, n * C.sizeof(pydrt.Material)) == raw and cases.same_bits(again.spds(), bundle.spds())


def test_the_header_and_pydrt_agree_on_the_calls(tmp_path):
    header = open(os.path.join(cases.REPO, "include", "drt_hip.h")).read()
    for call in ("drt_update_spectra", "drt_update_materials", "drt_group_update_spectra", "drt_group_update_materials"):
        assert re.search(r"\bint %s\(" % call, header) and call in pydrt.HIP_SYMBOLS, call
    assert re.search(r"#define DRT_SPECTRA_DEVICE\s+1u", header) and pydrt.SPECTRA_DEVICE == 1
    src = tmp_path / "material.c"
    src.write_text('#include <stdio.h>\n#include "drt_hip.h"\nint main(void) { printf("%zu\\n", sizeof(drt_material)); return 0; }\n')
    exe = tmp_path / "material"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(cases.REPO, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout) == C.sizeof(pydrt.Material)


def run_program(tmp_path, env, no_device=True):
    for sub in ("scenes", "spectra"):
        os.symlink(os.path.join(cases.REPO, sub), tmp_path / sub)
    os.makedirs(tmp_path / "output")
    (tmp_path / "config.cfg").write_text(open(os.path.join(cases.REPO, "config.cfg")).read())
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    if no_device:
        full["HIP_VISIBLE_DEVICES"] = "-1"  # no device call could succeed: the refusal must come first
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    return subprocess.run([exe], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


@pytest.mark.parametrize("env, message", [
    ({"DRT_LIGHT_LEVELS": "1,2", "DRT_TURNTABLE": "2"}, "DRT_LIGHT_LEVELS cannot be combined with DRT_TURNTABLE"),
    ({"DRT_LIGHT_LEVELS": "1,2", "DRT_CHECKPOINT_SPP": "1"}, "DRT_LIGHT_LEVELS cannot be combined with DRT_CHECKPOINT_SPP"),
    ({"DRT_LIGHT_LEVELS": "1,2", "DRT_RESUME": "1"}, "DRT_LIGHT_LEVELS cannot be combined with DRT_RESUME"),
    ({"DRT_LIGHT_LEVELS": "1,2", "DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_RESUME": "1"}, "DRT_LIGHT_LEVELS cannot be combined with DRT_ADAPTIVE_RESUME"),
    ({"DRT_LIGHT_LEVELS": "1,2", "DRT_PROJECTION": "equirect"}, "DRT_LIGHT_LEVELS cannot be combined with DRT_PROJECTION"),
    ({"DRT_LIGHT_LEVELS": "1,2", "DRT_MATTES": "1"}, "DRT_LIGHT_LEVELS cannot be combined with DRT_MATTES"),
    ({"DRT_LIGHT_LEVELS": "1,2", "DRT_PICK": "1,1"}, "DRT_LIGHT_LEVELS cannot be combined with DRT_PICK"),
    ({"DRT_LIGHT_LEVELS": "1,bright"}, "finite numbers separated by commas"),
    ({"DRT_LIGHT_LEVELS": ""}, "finite numbers separated by commas"),
    ({"DRT_LIGHT_LEVELS": "1,inf"}, "finite numbers separated by commas"),
    ({"DRT_LIGHT_LEVELS": ",".join(["1"] * 65)}, "64 levels at most"),
])
def test_the_program_refuses_light_levels_it_cannot_make_before_any_device_call(tmp_path, env, message):
    r = run_program(tmp_path, env)
    assert r.returncode != 0 and message in r.stdout, r.stdout[-1000:]
    assert os.listdir(tmp_path / "output") == []


@pytest.mark.parametrize("scene", ["plane_light_16", "many_lights", "lights"])
def test_light_level_rows_are_the_emission_rows_times_the_level(scene):
    """MU.light_level_rows is what the GPU test gives Renderer.update_spectra beside the program: held here to plain numpy, row by row"""
    bundle, _ = cases.load_case(scene)
    spds = bundle.spds()
    sc = bundle.scene
    em = {int(sc.materials[i].emission_spd) for i in range(int(sc.num_materials)) if sc.materials[i].is_emissive}
    assert em and min(em) >= 4  # never an observer's row
    for k in (1.0, 0.25, 3.0):
        first, rows = MU.light_level_rows(bundle, k)
        assert first == min(em) and rows.shape == (max(em) - min(em) + 1, bundle.S)
        for r in range(first, first + rows.shape[0]):
            want = spds[r] * k if r in em else spds[r]
            assert cases.same_bits(rows[r - first], want), (scene, k, r)
        if k == 1.0:
            assert cases.same_bits(rows, spds[first:first + rows.shape[0]])  # level 1 is the scene itself
