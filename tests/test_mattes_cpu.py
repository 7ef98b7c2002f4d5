"""CPU: the ID-matte rule (tests/matte_rule.py) against the path it restates -- the oracle's own hit log,
counted a second time here with collections.Counter -- and on hand-made id sequences that pin its corners down. Then what needs no
device: the struct's layout, drt_read_matte's argument checks and the drt_render host's DRT_MATTES refusals."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import feature_rule as F
import matte_rule as M
import oracle_py as O
import pydrt

REPO = cases.REPO
BIN = os.path.join(REPO, "daily-ray-trace_amd", "drt_render")
CASES = ["plane_light_16", "lights", "lens", "downward", "example_scene", "spheres_8x8"]
# counted on the oracle's hit log: pixels that see more than one surface, pixels part hit and part miss
SEEN = {"plane_light_16": (27, 15), "lights": (30, 54), "lens": (39, 41), "downward": (36, 5), "example_scene": (0, 0)}

_rule = {}


def rule_of(name):
    """(bundle, params, ids, counts, tail, empty, overflow) of a case at its own spp, computed once"""
    if name not in _rule:
        bundle, params = M.load_case(name)
        _rule[name] = (bundle, params) + M.mattes(bundle, params, n_samples=int(params.spp))
    return _rule[name]


def test_mattes_struct_matches_the_header():
    T = pydrt.Mattes
    assert C.sizeof(T) == 40
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [
        ("n_samples", 0), ("first_sample", 4), ("flags", 8), ("empty_pixels", 12), ("overflow_pixels", 16), ("rays", 24), ("kernel_ms", 32)]
    header = open(os.path.join(REPO, "include", "drt_hip.h")).read()
    body = re.search(r"typedef struct drt_mattes\s*\{(.*?)\}\s*drt_mattes;", header, re.S).group(1)
    names = re.findall(r"\b(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in T._fields_]
    assert int(re.search(r"#define DRT_MATTE_SLOTS\s+(\d+)", header).group(1)) == M.SLOTS == pydrt.MATTE_SLOTS
    assert int(re.search(r"#define DRT_MATTE_ID_MISS\s+\((-?\d+)\)", header).group(1)) == M.ID_MISS == pydrt.MATTE_ID_MISS
    enum = re.search(r"enum \{ DRT_MATTE_SURFACE = (\d), DRT_MATTE_MATERIAL = (\d), DRT_MATTE_LAYERS = (\d) \};", header)
    assert [int(v) for v in enum.groups()] == [M.SURFACE, M.MATERIAL, M.LAYERS] == [pydrt.MATTE_SURFACE, pydrt.MATTE_MATERIAL, pydrt.MATTE_LAYERS]


def counter_slots(seq):
    """the count a second time: a Counter over the first six distinct ids in order of appearance"""
    hits = [int(v) for v in seq if v >= 0]
    kept = list(dict.fromkeys(hits))[:M.SLOTS]
    n = collections.Counter(v for v in hits if v in kept)
    ranked = sorted(kept, key=lambda v: (-n[v], v))
    pad = M.SLOTS - len(ranked)
    return ranked + [-1] * pad, [n[v] for v in ranked] + [0] * pad, len(hits) - sum(n.values()), len(seq) - len(hits)


@pytest.mark.parametrize("name", CASES)
def test_the_rule_counts_the_paths_own_hit_log(name):
    bundle, params, ids, counts, tail, empty, overflow = rule_of(name)
    spp, P = int(params.spp), int(params.tile_w) * int(params.tile_h)
    hits = O.oracle_render_tile(bundle, params, want_hits=True, math_mode=O.MATH_DEVICE)[3]
    surf = hits[:, 0].reshape(spp, P).T  # the log is ordered (sample, tile row, tile column)
    material = np.array([int(bundle.scene.surfaces[i].material) for i in range(int(bundle.scene.num_surfaces))] + [-1])
    mat = material[surf]  # (a miss, -1, reads the last entry)
    seen = {"several": 0, "mixed": 0, "over": [0, 0], "tie": 0, "most": [0, 0]}
    for p in range(P):
        for layer, seq in ((M.SURFACE, surf[p]), (M.MATERIAL, mat[p])):
            want_ids, want_n, other, misses = counter_slots(seq)
            assert ids[p, layer].tolist() == want_ids and counts[p, layer].tolist() == want_n, (p, layer)
            assert (int(tail[p, 0]), int(tail[p, 1]), int(tail[p, 2 + layer])) == (spp, misses, other), (p, layer)
            assert sum(want_n) + other + misses == spp
            distinct = len(set(int(v) for v in seq if v >= 0))
            seen["most"][layer] = max(seen["most"][layer], distinct)
            seen["over"][layer] += int(distinct > M.SLOTS)
            assert (other > 0) == (distinct > M.SLOTS)
        n = counts[p, M.SURFACE]
        seen["several"] += int(n[1] > 0)
        seen["mixed"] += int(0 < tail[p, 1] < spp)
        seen["tie"] += int(any(n[k] > 0 and n[k] == n[k + 1] for k in range(M.SLOTS - 1)))
    assert empty == int((surf < 0).all(axis=1).sum()) and list(overflow) == seen["over"]
    print("%s: %s, %d empty" % (name, seen, empty))
    if name in SEEN:
        assert (seen["several"], seen["mixed"]) == SEEN[name]
    # the inputs do exercise the rule
    if name == "example_scene":
        assert empty == P and not (ids >= 0).any() and not counts.any()
    else:
        assert seen["several"] > 0 and seen["mixed"] > 0
    if name == "spheres_8x8":
        assert seen["most"] == [10, 7] and seen["over"] == [8, 1] and empty == 6 and seen["mixed"] == 58
    if name in ("plane_light_16", "spheres_8x8"):
        assert seen["tie"] > 0


def one(seq_surface, seq_material=None):
    ids, counts, tail, empty, overflow = M.mattes_of_ids([seq_surface], [seq_surface if seq_material is None else seq_material])
    return ids[0], counts[0], tail[0].tolist(), empty, overflow


def test_ranking_by_count_then_id_with_empty_slots_last():
    ids, counts, tail, empty, overflow = one([7, 3, 7, 9, 3, 5], [1, 0, 1, 2, 0, 0])
    assert ids[0].tolist() == [3, 7, 5, 9, -1, -1] and counts[0].tolist() == [2, 2, 1, 1, 0, 0]  # ties: the lower id first
    assert ids[1].tolist() == [0, 1, 2, -1, -1, -1] and counts[1].tolist() == [3, 2, 1, 0, 0, 0]
    assert tail == [6, 0, 0, 0] and empty == 0 and overflow == (0, 0)
    # surface 0 is an id like any other: it does not pass for an empty slot
    ids, counts, tail, _, _ = one([0, 0, 4])
    assert ids[0].tolist() == [0, 4, -1, -1, -1, -1] and counts[0].tolist() == [2, 1, 0, 0, 0, 0]


def test_an_id_that_comes_after_the_slots_are_full_goes_to_other():
    seq = [10, 11, 12, 13, 14, 15, 16, 10, 16, 17]
    ids, counts, tail, empty, overflow = one(seq, [0] * len(seq))
    assert ids[0].tolist() == [10, 11, 12, 13, 14, 15] and counts[0].tolist() == [2, 1, 1, 1, 1, 1]
    assert tail == [10, 0, 3, 0] and overflow == (1, 0)
    assert ids[1].tolist() == [0, -1, -1, -1, -1, -1] and counts[1].tolist() == [10, 0, 0, 0, 0, 0]


def test_a_dominant_id_that_arrives_late_lands_in_other():
    """what the fixed sample order costs: six ids seen once each fill the slots, the seventh covers the rest of the pixel unseen"""
    seq = [1, 2, 3, 4, 5, 6] + [9] * 20 + [-1, -1]
    ids, counts, tail, empty, overflow = one(seq)
    assert ids[0].tolist() == [1, 2, 3, 4, 5, 6] and counts[0].tolist() == [1] * 6
    assert tail == [28, 2, 20, 20] and overflow == (1, 1) and empty == 0
    # the same samples with the dominant id first keep it
    ids, counts, tail, _, _ = one([9] * 20 + [1, 2, 3, 4, 5, 6])
    assert ids[0].tolist() == [9, 1, 2, 3, 4, 5] and counts[0].tolist() == [20, 1, 1, 1, 1, 1] and tail == [26, 0, 1, 1]


def test_all_misses_and_a_single_sample():
    ids, counts, tail, empty, overflow = one([-1] * 5)
    assert not (ids >= 0).any() and not counts.any() and tail == [5, 5, 0, 0] and empty == 1
    ids, counts, tail, empty, _ = one([4], [2])
    assert ids[:, 0].tolist() == [4, 2] and counts[:, 0].tolist() == [1, 1] and tail == [1, 0, 0, 0] and empty == 0
    ids, counts, tail, empty, _ = one([-1])
    assert tail == [1, 1, 0, 0] and empty == 1


def test_one_matte_is_the_integer_sum_over_the_listed_ids():
    bundle, params, ids, counts, tail, empty, overflow = rule_of("spheres_8x8")
    c = tail[:, 0].astype(np.float64)
    for layer, n in ((M.SURFACE, int(bundle.scene.num_surfaces)), (M.MATERIAL, int(bundle.scene.num_materials))):
        everything = M.matte_select(ids, counts, tail, layer, list(range(n)) + [M.ID_MISS])
        assert np.array_equal(everything, (c - tail[:, 2 + layer]) / c)
        assert (everything < 1.0).any()
        assert np.array_equal(M.matte_select(ids, counts, tail, layer, [M.ID_MISS]), tail[:, 1] / c)
    top = int(ids[np.argmax(counts[:, 0, 0]), 0, 0])
    cover = M.matte_select(ids, counts, tail, M.SURFACE, [top, top])  # (a list is a set: naming an id twice counts it once)
    assert cover.max() <= 1.0 and cover.max() == counts[:, 0, 0].max() / 48.0
    ids1, counts1, tail1, _, _ = M.mattes_of_ids([[5, 5, 8, -1]], [[1, 1, 1, -1]])
    assert M.matte_select(ids1, counts1, tail1, M.SURFACE, [8])[0] == 0.25
    assert M.matte_select(ids1, counts1, tail1, M.SURFACE, [5, M.ID_MISS])[0] == 0.75
    assert M.matte_select(ids1, counts1, tail1, M.MATERIAL, [1])[0] == 0.75


def test_the_preview_bytes_for_known_ids():
    assert M.palette(-1) == (64, 64, 64)  # h = 0
    h = 0x9E3779B1 ^ (0x9E3779B1 >> 16)
    assert M.palette(0) == (64 + (h & 127), 64 + ((h >> 8) & 127), 64 + ((h >> 16) & 127)) == (64 + 6, 64 + 103, 64 + 55)
    ids, counts, tail, _, _ = M.mattes_of_ids([[0, 0, 0, 0], [0, 0, -1, -1], [-1, -1], [0, 3, 3, 3]], [[2] * 4, [2, 2, -1, -1], [-1, -1], [2] * 4])
    b = M.matte_bgra(ids, counts, tail, M.SURFACE)
    r, g, bl = M.palette(0)
    assert b[0].tolist() == [bl, g, r, 255]
    assert b[1].tolist() == [int(0.5 * bl + 0.5), int(0.5 * g + 0.5), int(0.5 * r + 0.5), 255]  # misses add nothing
    assert b[2].tolist() == [0, 0, 0, 255]
    r3, g3, b3 = M.palette(3)
    assert b[3].tolist() == [int(0.75 * b3 + 0.25 * bl + 0.5), int(0.75 * g3 + 0.25 * g + 0.5), int(0.75 * r3 + 0.25 * r + 0.5), 255]
    assert M.matte_bgra(ids, counts, tail, M.MATERIAL)[0].tolist() == [M.palette(2)[2], M.palette(2)[1], M.palette(2)[0], 255]
    assert max(max(M.palette(i)) for i in range(-1, 3000)) <= 191


@pytest.mark.parametrize("name", ["lights", "spheres_8x8", "example_scene"])
def test_the_host_programs_conversion_gives_the_rules_bytes(name):
    _, _, ids, counts, tail, _, _ = rule_of(name)
    H = pydrt.host_lib()
    for layer in (M.SURFACE, M.MATERIAL):
        out = np.zeros((ids.shape[0], 4), dtype=np.uint8)
        H.drt_host_matte_bgra(pydrt._ptr(ids, C.c_int32), pydrt._ptr(counts, C.c_uint32), pydrt._ptr(tail, C.c_uint32),
                              C.c_uint64(ids.shape[0]), C.c_int(layer), pydrt._ptr(out, C.c_uint8))
        want = M.matte_bgra(ids, counts, tail, layer)
        assert np.array_equal(out, want), "%s layer %d: %d bytes differ" % (name, layer, int((out != want).sum()))


@pytest.mark.parametrize("name", ["lights", "spheres_8x8", "example_scene"])
def test_empty_pixels_are_the_feature_rules(name):
    bundle, params, ids, counts, tail, empty, overflow = rule_of(name)
    assert empty == F.features(bundle, params, n_samples=int(params.spp))[3]
    if name == "lights":
        counts_in = 1 + (np.arange(int(params.tile_w) * int(params.tile_h)) * 7) % 5
        got = M.mattes(bundle, params, first_sample=2, counts=counts_in)
        assert got[3] == F.features(bundle, params, first_sample=2, counts=counts_in)[3] and np.array_equal(got[2][:, 0], counts_in)


# ------------------------------------------------------------------------------------------------
def test_read_matte_checks_its_arguments_before_it_looks_at_the_context():
    """without a device: the layer, the list's length and an id below -1 are refused whatever the context is, here none"""
    L = pydrt.hip_lib()
    out = np.zeros(4)
    lst = np.array([0, 1, -2], dtype=np.int32)

    def call(layer, ids, n):
        rc = L.drt_read_matte(None, layer, pydrt._ptr(ids, C.c_int32), n, pydrt._ptr(out, C.c_double))
        assert rc != 0
        return L.drt_last_error().decode()

    assert "layer = 2: 0 surfaces, 1 materials" in call(2, lst, 2)
    assert "layer = -1" in call(-1, lst, 2)
    assert "n_ids = 0: 1 to 4096 ids" in call(0, lst, 0)
    assert "n_ids = 4097: 1 to 4096 ids" in call(1, lst, 4097)
    assert "id_list[2] = -2: -1 (a miss) or the index of a surface" in call(0, lst, 3)
    assert "id_list[2] = -2: -1 (a miss) or the index of a material" in call(1, lst, 3)
    assert "null context" in call(0, lst, 2)
    rc = L.drt_read_matte_bgra(None, 0, pydrt._ptr(np.zeros(4, dtype=np.uint8), C.c_uint8))
    assert rc != 0 and "null argument" in L.drt_last_error().decode()


@pytest.mark.parametrize("value", ["2", "-1", "yes", "", "1x", "01"])
def test_the_host_refuses_bad_matte_settings_before_any_device_call(tmp_path, value):
    """Exit status nonzero, the variable named on stderr, and no device opened: HIP_VISIBLE_DEVICES hides every device, so a run
    that got as far as the launcher would fail there with the launcher's message instead."""
    cfg = open(os.path.join(REPO, "config.cfg")).read()
    (tmp_path / "config.cfg").write_text(cfg)
    os.symlink(os.path.join(REPO, "scenes"), tmp_path / "scenes")
    os.symlink(os.path.join(REPO, "spectra"), tmp_path / "spectra")
    full = {k: v for k, v in os.environ.items() if not k.startswith("DRT_")}
    full["DRT_MATTES"] = value
    full["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([BIN, "config.cfg"], cwd=tmp_path, env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0
    assert 'DRT_MATTES="%s": 0 or 1' % value in r.stderr, r.stderr
    assert "HIP launcher" not in r.stderr and "Rendering" not in r.stdout
