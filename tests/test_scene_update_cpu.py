"""CPU (-m "not gpu"): the premises of tests/test_gpu_scene_update.py, checked with the oracle. Every "after" scene of
tests/scene_update_cases.py renders another film and another hit log than its "before" scene, so no GPU test can pass by doing nothing;
pydrt.surface_rows round-trips bit for bit; the turntable's frame 0 is the scene's own camera."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

import cases
import oracle_py as O
import pydrt
import scene_update_cases as U


def oracle(bundle, params):
    px, av, va, hits, st = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_DEVICE)
    return (px, av, va), hits, st


@pytest.mark.parametrize("name", U.ALL)
def test_the_after_scene_renders_another_film_and_another_hit_log(name):
    c = U.load(name)
    p = c["params"]
    assert int(p.spp) <= 5 and int(p.tile_w) <= 32 and int(p.tile_h) <= 32 and int(p.flags) & pydrt.FLAG_RECORD_HITS
    b, a = c["before"].scene, c["after"].scene
    assert int(b.num_surfaces) == int(a.num_surfaces)
    for i in range(int(b.num_surfaces)):  # what an update fixes
        assert (int(b.surfaces[i].type), int(b.surfaces[i].material)) == (int(a.surfaces[i].type), int(a.surfaces[i].material)), i
    t0 = time.perf_counter()
    film_b, log_b, _ = oracle(c["before"], p)
    film_a, log_a, _ = oracle(c["after"], p)
    assert time.perf_counter() - t0 < 20.0  # both renders: a case stays a matter of seconds
    for fb, fa in zip(film_b, film_a):
        assert not cases.same_bits(fb, fa)
    # (a point light is never intersected and steers no path: moving it alone changes the film and leaves the log)
    assert np.array_equal(log_b, log_a) == (name in U.SAME_LOG)
    assert np.any(film_a[0][:, :-1] != 0.0)  # and the "after" film is not black


def test_the_forced_and_unforced_hierarchy_cases_are_what_they_say():
    for name in U.ALL:
        c = U.load(name)
        n = int(c["before"].scene.num_surfaces)
        if c["bvh"] and not c["forced"]:
            assert n > 96, name  # more than the LDS holds: behind the hierarchy unforced
        else:
            assert n <= 96, name
    assert int(U.load("spheres_96")["before"].scene.num_surfaces) == 97
    # the degenerate case: the updated plane's edges are parallel, the one it replaces had a proper parallelogram
    c = U.load("parallel_edges")
    last = int(c["after"].scene.num_surfaces) - 1
    for bundle, parallel in ((c["before"], False), (c["after"], True)):
        s = bundle.scene.surfaces[last]
        cross = np.cross(np.array(list(s.u)), np.array(list(s.v)))
        assert (np.abs(cross).max() == 0.0) == parallel


def test_the_far_case_is_sixteen_extents_away():
    c = U.load("spheres_1500_far")
    near = np.abs(pydrt.surface_rows(c["before"])[:, U.ROW_POS]).max()
    far = np.abs(pydrt.surface_rows(c["after"])[:, U.ROW_POS]).max()
    assert 16.0 * near <= far < 2.0 ** 27
    assert abs(c["after"].camera.aperture_position[0]) >= 16.0 * near


@pytest.mark.parametrize("name", ["lights", "spheres_1500"])
def test_surface_rows_round_trip_bit_for_bit(name):
    bundle, _ = cases.load_case(name)
    n = int(bundle.scene.num_surfaces)
    rows = pydrt.surface_rows(bundle)
    assert rows.shape == (n, 14) and rows.dtype == np.float64
    raw = C.string_at(bundle.scene.surfaces, n * C.sizeof(pydrt.Surface))
    assert rows.tobytes() == raw
    back = pydrt.surfaces_from_rows(rows)
    assert C.string_at(back, n * C.sizeof(pydrt.Surface)) == raw
    assert pydrt.surface_rows(back).tobytes() == raw
    head = rows[:, 0].copy().view("<u4").reshape(n, 2)  # word 0: type, material
    assert all((int(head[i, 0]), int(head[i, 1])) == (int(bundle.scene.surfaces[i].type), int(bundle.scene.surfaces[i].material)) for i in range(n))
    assert rows[0, 1:4].tolist() == list(bundle.scene.surfaces[0].position) and rows[0, 4] == bundle.scene.surfaces[0].radius
    with pytest.raises(ValueError):
        pydrt.surfaces_from_rows(np.zeros((3, 13)))


def _bytes(cam):
    return C.string_at(C.byref(cam), C.sizeof(pydrt.Camera))


@pytest.mark.parametrize("scene", ["cornell_plane_light.scn", "test_lens.scn", "cornell_downward.scn"])
def test_turntable_frame_0_is_the_scenes_camera_and_the_half_turn_looks_back(scene):
    w, h = 24, 16
    bundle = pydrt.load_scene(cases.scene_path(scene), w, h)
    for n in (1, 2, 3, 8):
        assert _bytes(pydrt.turntable_camera(bundle, w, h, 0, n)) == _bytes(bundle.camera)
        assert _bytes(pydrt.turntable_camera(bundle, w, h, n, n)) == _bytes(bundle.camera)  # frames count modulo n
    f0 = np.array(list(bundle.camera.forward))
    for n in (2, 8):
        half = pydrt.turntable_camera(bundle, w, h, n // 2, n)
        f = np.array(list(half.forward))
        # position - target is negated exactly in x and z (a half turn's cosine and sine are -1 and 0), then rounded once when the target
        # is added and once when it is subtracted again, and normalised: a few units in the last place of a unit vector's components
        assert np.allclose(f[[0, 2]], -f0[[0, 2]], rtol=0.0, atol=16 * np.finfo(np.float64).eps)
        assert abs(f[1] - f0[1]) <= 16 * np.finfo(np.float64).eps
        assert half.focal_depth == bundle.camera.focal_depth and half.aperture_radius == bundle.camera.aperture_radius
    # a quarter of the way round the camera is somewhere else -- unless it looks straight down the axis, as cornell_downward's does
    q = pydrt.turntable_camera(bundle, w, h, 1, 4)
    assert (_bytes(q) != _bytes(bundle.camera)) == (scene != "cornell_downward.scn")
    with pytest.raises(ValueError):
        pydrt.turntable_camera(bundle, w, h, 0, 0)
    with pytest.raises(ValueError):
        pydrt.turntable_camera(pydrt.synthetic_sphere_scene(1, w, h), w, h, 0, 4)


# ------------------------------------------------------------------------------------------------
REPORT_FIELDS = [("updates", 0), ("refits_since_build", 4), ("extent", 8), ("kernel_ms", 16)]
CALLS = ("drt_set_camera", "drt_update_surfaces", "drt_group_set_camera", "drt_group_update_surfaces", "drt_get_update_report", "drt_group_reset_film")


def test_the_header_the_compiler_and_pydrt_agree_on_the_report(tmp_path):
    header = open(os.path.join(cases.REPO, "include", "drt_hip.h")).read()
    for call in CALLS:
        assert re.search(r"\bint %s\(" % call, header) and call in pydrt.HIP_SYMBOLS, call
    assert re.search(r"#define DRT_SURFACES_DEVICE\s+1u", header) and re.search(r"#define DRT_SURFACES_REBUILD\s+2u", header)
    assert (pydrt.SURFACES_DEVICE, pydrt.SURFACES_REBUILD) == (1, 2)
    src = tmp_path / "report.c"
    lines = ['printf("%s %%zu\\n", offsetof(drt_update_report, %s));' % (n, n) for n, _ in REPORT_FIELDS]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "drt_hip.h"\nint main(void) {\n%s\n'
                   'printf("sizeof %%zu\\nsurface %%zu\\n", sizeof(drt_update_report), sizeof(drt_surface));\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "report"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(cases.REPO, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(pydrt.UpdateReport) == 24 and int(out["surface"]) == C.sizeof(pydrt.Surface) == 112
    assert [(n, int(out[n])) for n, _ in REPORT_FIELDS] == REPORT_FIELDS
    assert [(n, getattr(pydrt.UpdateReport, n).offset) for n, _ in pydrt.UpdateReport._fields_] == REPORT_FIELDS


@pytest.mark.parametrize("env, message", [
    ({"DRT_TURNTABLE": "2", "DRT_CHECKPOINT_SPP": "1"}, "DRT_TURNTABLE cannot be combined with DRT_CHECKPOINT_SPP"),
    ({"DRT_TURNTABLE": "2", "DRT_RESUME": "1"}, "DRT_TURNTABLE cannot be combined with DRT_RESUME"),
    ({"DRT_TURNTABLE": "2", "DRT_PROJECTION": "equirect"}, "DRT_TURNTABLE cannot be combined with DRT_PROJECTION"),
    ({"DRT_TURNTABLE": "2", "DRT_ADAPTIVE_ERROR": "0.1", "DRT_ADAPTIVE_RESUME": "1"}, "DRT_TURNTABLE cannot be combined with DRT_ADAPTIVE_RESUME"),
    ({"DRT_TURNTABLE": "2", "DRT_MATTES": "1"}, "DRT_TURNTABLE cannot be combined with DRT_MATTES"),
    ({"DRT_TURNTABLE": "0"}, "from 1 to 9999 frames"),
    ({"DRT_TURNTABLE": "three"}, "is not a whole number"),
])
def test_the_program_refuses_a_turntable_it_cannot_make_before_any_device_call(tmp_path, env, message):
    for sub in ("scenes", "spectra"):
        os.symlink(os.path.join(cases.REPO, sub), tmp_path / sub)
    os.makedirs(tmp_path / "output")
    (tmp_path / "config.cfg").write_text(open(os.path.join(cases.REPO, "config.cfg")).read())
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"  # no device call could succeed: the refusal must come first
    exe = os.path.join(cases.REPO, "daily-ray-trace_amd", "drt_render")
    r = subprocess.run([exe], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode != 0 and message in r.stdout, r.stdout[-1000:]
    assert os.listdir(tmp_path / "output") == []
