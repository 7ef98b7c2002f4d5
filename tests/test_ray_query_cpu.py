"""CPU: what the ray queries (drt_cast_rays, drt_test_visibility, drt_cast_pixels) need no device for -- the
struct's layout in the header, a C compiler's view of it and pydrt's; the drt_render host's DRT_PICK refusals; and, with the oracle
alone, that the inputs tests/ray_query_cases.py builds for the GPU tests are worth running."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import hierarchy_cases as HC
import pydrt
import ray_query_cases as Q

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")
FIELDS = [("position", 0), ("normal", 24), ("out", 48), ("on_dot", 72), ("distance", 80), ("index", 88), ("surface_material", 92),
          ("incident_material", 96), ("transmit_material", 100)]


def test_the_header_declares_the_struct_and_the_calls():
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    body = re.search(r"typedef struct drt_ray_hit[^{]*\{(.*?)\}\s*drt_ray_hit;", header, re.S).group(1)
    names = re.findall(r"\b(\w+)(?:\[3\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in FIELDS]
    assert re.search(r"#define DRT_RAYS_DEVICE 1u", header)
    for call in ("drt_cast_rays", "drt_test_visibility", "drt_cast_pixels", "drt_group_cast_rays", "drt_group_test_visibility", "drt_group_cast_pixels"):
        assert re.search(r"\bint %s\(" % call, header), call
        assert call in pydrt.HIP_SYMBOLS


def test_a_c_compiler_and_pydrt_agree_on_the_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "drt_hip.h"\nint main(void)\n{\n    printf("sizeof %zu\\n", sizeof(drt_ray_hit));\n'
                   + "".join('    printf("%s %%zu\\n", offsetof(drt_ray_hit, %s));\n' % (n, n) for n, _ in FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["sizeof"]) == 104
    assert [(n, int(out[n])) for n, _ in FIELDS] == FIELDS
    T = pydrt.RayHit
    assert C.sizeof(T) == 104
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == FIELDS
    dt = pydrt.RAY_HIT_DTYPE
    assert dt.itemsize == 104 and [(n, dt.fields[n][1]) for n in dt.names] == FIELDS
    assert pydrt.RAYS_DEVICE == 1


# ------------------------------------------------------------------------------------------------
def _run_host(tmp_path, env):
    cfg = open(os.path.join(REPO, "config.cfg")).read()
    (tmp_path / "config.cfg").write_text(cfg)
    os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
    os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full.update(env)
    full["HIP_VISIBLE_DEVICES"] = "-1"
    return subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


@pytest.mark.parametrize("value", [
    "", "10", "10,", ",10", "10,20,", "10,20,1,2", "10;20", "10,20;", ";10,20", "10,20;;30,40", "a,b", "10,-20", "10, 20", "10,20 ", "1.5,2",
    "10,20,x", "10,20,99999999999", "0x10,2",
    "800,0",  # config.cfg renders 800 x 600: the first column outside
    "0,600", "799,599;800,599", "4294967295,0",
    ";".join("%d,%d" % (k, k) for k in range(65)),  # a 65th entry
])
def test_the_host_refuses_a_bad_pick_list_before_any_device_call(tmp_path, value):
    """Exit status nonzero, the variable named on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run that got
    as far as the launcher would fail there with the launcher's message instead."""
    r = _run_host(tmp_path, {"DRT_PICK": value})
    assert r.returncode != 0
    assert "DRT_PICK" in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout and "pick " not in r.stdout


@pytest.mark.parametrize("value", ["0,0", "799,599,7", "10,20;30,40,2;5,6", ";".join("%d,%d,%d" % (k, k, k) for k in range(64))])
def test_a_good_pick_list_gets_as_far_as_the_launcher(tmp_path, value):
    r = _run_host(tmp_path, {"DRT_PICK": value})
    assert r.returncode != 0 and "DRT_PICK" not in r.stderr and "HIP launcher" in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Q.SCENE_NAMES)
def test_the_generated_sets_are_worth_running(name):
    """With the oracle alone, in DEVICE arithmetic. No ray set is left out: the GPU tests compare every ray and every pair of these
    sets, so the share a comparison may skip is zero -- which needs the sets free of subnormal quotients, asserted here."""
    s, e = Q.ray_sets(name), Q.expected(name)
    ro, rd = s["rays"]
    p0, p1 = s["pairs"]
    hits, vis = e["hits"], e["visible"]
    n = len(ro)
    assert n == len(hits) and len(p0) == len(vis) and sum(p.stop - p.start for p in s["parts"].values()) == n
    assert sum(p.stop - p.start for p in s["pair_parts"].values()) == len(p0)
    for part in ("camera", "one_zero", "two_zeros", "special"):
        assert part in s["parts"], part
    w, h = int(Q.load(name)[1].width), int(Q.load(name)[1].height)
    assert s["parts"]["camera"] == slice(0, 2 * w * h)
    # (c): exact zeros in the directions
    assert np.all((rd[s["parts"]["one_zero"]] == 0.0).sum(axis=1) == 1) and np.all((rd[s["parts"]["two_zeros"]] == 0.0).sum(axis=1) == 2)
    # (d): the four specials are what they say
    sp = s["parts"]["special"]
    assert np.isnan(rd[sp][0]).any() and not rd[sp][1].any() and np.isinf(ro[sp][2]).any()
    assert hits["index"][sp][0] == -1  # a NaN direction misses
    hit_share = float((hits["index"] >= 0).mean())
    vis_share = float(vis.mean())
    print("%s: %d rays, %.1f %% hit; %d pairs, %.1f %% visible" % (name, n, 100 * hit_share, len(vis), 100 * vis_share))
    assert hit_share >= 0.10
    if name not in Q.CLOSED_ROOMS:
        assert 1.0 - hit_share >= 0.10
    else:
        assert (hits["index"] < 0).any()
    assert vis_share >= 0.10 and 1.0 - vis_share >= 0.10
    assert "same_point" in s["pair_parts"] and "ends_on_a_surface" in s["pair_parts"] and "other_pixel" in s["pair_parts"]
    sm = s["pair_parts"]["same_point"]
    assert np.array_equal(p0[sm], p1[sm])
    assert Q.subnormal_quotients(name) == 0
    # what the oracle says of a hit is self-consistent: position = moved origin + d * distance, bit for bit
    on = hits["index"] >= 0
    mo = Q.moved_origins(ro, rd)
    with np.errstate(all="ignore"):
        again = mo[on] + rd[on] * hits["distance"][on][:, None]
    assert cases.same_bits(again, hits["position"][on]), cases.first_difference(again, hits["position"][on])
    assert not hits["distance"][~on].any() and not hits["position"][~on].any()


@pytest.mark.parametrize("name", ["spheres_1500", "spheres_20000"])
def test_the_seeded_rays_of_the_hierarchy_tests_are_worth_running(name):
    """tests/test_gpu_hierarchy.py compares every one of these 4096 rays and pairs bit for bit after a device build: the same premise,
    no subnormal quotient, and both answers of both queries occur, some hundreds of times each (the sparse 1500 spheres are hit by one
    ray in thirteen)."""
    bundle = HC.load(name)["after"]
    ro, rd, p0, p1 = HC.seeded_rays(name)
    assert len(ro) == len(p0) == 4096
    hits, vis = Q.oracle_hits(bundle, ro, rd), Q.oracle_visible(bundle, p0, p1)
    assert Q.subnormal_quotients_of(bundle, ro, rd, p0, p1, hits["normal"]) == 0
    hit_share, vis_share = float((hits["index"] >= 0).mean()), float(vis.mean())
    print("%s: %.1f %% of the rays hit, %.1f %% of the pairs are visible" % (name, 100 * hit_share, 100 * vis_share))
    assert 0.05 <= hit_share <= 0.95 and 0.05 <= vis_share <= 0.95


def test_the_restated_camera_rays_hit_what_the_paths_own_hit_log_says():
    import oracle_py as O
    for name in ("plane_light_16", "lens"):
        bundle, params = Q.load(name)
        spp, P = int(params.spp), int(params.width) * int(params.height)
        log = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_DEVICE)[3]
        first = log[:, 0].reshape(spp, P)
        cam = Q.expected(name)["hits"]["index"][Q.ray_sets(name)["parts"]["camera"]].reshape(2, P)
        assert np.array_equal(cam, first[:2])


# exempt from the assertion below, by name: a scene that loses its spheres fails instead of going unchecked. None today.
SCENES_WITHOUT_A_SPHERE = frozenset()


@pytest.mark.parametrize("name", Q.SCENE_NAMES)
def test_scaled_directions_are_not_answered_by_normalising_first(name):
    """Part (e): per factor, rays whose closest hit under the rule is another surface (or none) than their normalised ray's. Only a
    sphere can tell: line_plane's hit does not depend on |d|, so a scene without a sphere would be exempt, by name
    (SCENES_WITHOUT_A_SPHERE) -- none is: every scene of the set has one."""
    s, e = Q.ray_sets(name), Q.expected(name)
    part = s["parts"]["scaled"]
    bo, bd, factor = s["scaled"]
    ro, rd = s["rays"]
    assert len(bo) == part.stop - part.start and np.array_equal(ro[part], bo)
    off = np.abs((bd * bd).sum(axis=1) - 1.0)
    assert off.max() <= 16 * 2.0 ** -52, off.max() / 2.0 ** -52  # (a mirror direction is a reflected unit vector)
    for f in Q.SCALE_FACTORS:
        assert np.array_equal(rd[part][factor == f], bd[factor == f] * f)
    bundle = Q.load(name)[0]
    assert bool(Q.spheres_of(bundle)) == (name not in SCENES_WITHOUT_A_SPHERE)
    if name in SCENES_WITHOUT_A_SPHERE:
        return
    base = Q.oracle_hits(bundle, bo, bd)["index"]
    got = e["hits"]["index"][part]
    counts = {f: int((base != got)[factor == f].sum()) for f in Q.SCALE_FACTORS}
    print("%s: %d scaled rays; closest hit differs from the normalised ray's, per factor: %s; light directions: %d of %d" % (
        name, len(bo), counts, int((base != got)[factor == 0.0].sum()), int((factor == 0.0).sum())))
    assert all(n >= 1 for n in counts.values()), counts
