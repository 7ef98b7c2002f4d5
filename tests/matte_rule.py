"""The ID mattes (include/drt_hip.h, drt_mattes), restated: per tile pixel and layer -- the surface a sample's
first hit lands on, and that surface's material -- six ranked (id, count) slots, the hits no slot had room for, and the misses.
Integers only, so the device is held to this with ==. Not a test file: the matte tests import it.

The samples are the feature rule's (tests/feature_rule.py): the path's own camera ray of (x, y, sample), the oracle's
find_ray_intersection. What is new is the counting, written here one sample at a time in plain Python."""
import ctypes as C

import numpy as np

import cases
import feature_rule as F
import oracle_py as O
import pydrt

SLOTS, LAYERS, ID_MISS = 6, 2, -1  # DRT_MATTE_SLOTS, DRT_MATTE_LAYERS, DRT_MATTE_ID_MISS
SURFACE, MATERIAL = 0, 1
_f64p = C.POINTER(C.c_double)


def load_case(name):
    """tests/cases.py's cases, and "spheres_8x8": the many-sphere scene at 8 x 8 pixels, 48 spp, where pixels see more surfaces and
    more materials than a layer has slots"""
    if name == "spheres_8x8":
        return pydrt.synthetic_sphere_scene(1500, 8, 8), pydrt.make_params(8, 8, spp=48, max_depth=6, seed=9)
    return cases.load_case(name)


def first_hit_ids(bundle, ro, rd):
    """(surface id [n], material id [n]) of n rays, both -1 for a miss (a NaN ray misses)"""
    L = O.oracle_lib()
    sc = bundle.scene
    n = ro.shape[0]
    surf = np.full(n, ID_MISS, dtype=np.int64)
    mat = np.full(n, ID_MISS, dtype=np.int64)
    pt = O.Point()
    ro, rd = np.ascontiguousarray(ro), np.ascontiguousarray(rd)
    for k in range(n):
        idx = L.drt_oracle_find_ray_intersection(C.byref(sc), ro[k].ctypes.data_as(_f64p), rd[k].ctypes.data_as(_f64p), C.byref(pt))
        if idx >= 0:
            surf[k], mat[k] = idx, int(sc.surfaces[idx].material)
    return surf, mat


def sample_ids(bundle, params, n_samples=None, first_sample=0, counts=None):
    """Every tile pixel's samples in ascending order: (surface ids, material ids), two lists of P integer arrays, and counts [P]"""
    x, y = F.tile_pixels(params)
    P = len(x)
    counts = np.full(P, int(n_samples), dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64).reshape(P)
    assert counts.min() >= 1
    pix = np.repeat(np.arange(P), counts)  # every (pixel, k < count) pair, pixel-major
    k = np.concatenate([np.arange(c) for c in counts])
    sx, sy, smp = x[pix], y[pix], int(first_sample) + k
    px, py, disc = F.sample_draws(bundle, params, sx, sy, smp)
    ro, rd = F.camera_rays(bundle, sx, sy, px, py, disc)
    surf, mat = first_hit_ids(bundle, ro, rd)
    ends = np.cumsum(counts)[:-1]
    return np.split(surf, ends), np.split(mat, ends), counts


def count_slots(seq):
    """One pixel, one layer: the ids of its samples in order (-1 a miss) -> (ranked ids [6], ranked counts [6], other, misses)"""
    ids, n, other, misses = [], [], 0, 0
    for v in (int(v) for v in seq):
        if v < 0:
            misses += 1
        elif v in ids:
            n[ids.index(v)] += 1
        elif len(ids) < SLOTS:
            ids.append(v)
            n.append(1)
        else:
            other += 1
    order = sorted(range(len(ids)), key=lambda k: (-n[k], ids[k]))
    pad = SLOTS - len(ids)
    return [ids[k] for k in order] + [ID_MISS] * pad, [n[k] for k in order] + [0] * pad, other, misses


def mattes_of_ids(surf, mat):
    """The counting over per-pixel id sequences (lists of P sequences, a layer each). Returns (ids [P][2][6] int32,
    counts [P][2][6] uint32, tail [P][4] uint32 = c_p, misses, other per layer, empty pixels, overflow pixels per layer)."""
    P = len(surf)
    ids = np.empty((P, LAYERS, SLOTS), dtype=np.int32)
    counts = np.empty((P, LAYERS, SLOTS), dtype=np.uint32)
    tail = np.empty((P, 4), dtype=np.uint32)
    for p in range(P):
        assert len(surf[p]) == len(mat[p]) >= 1
        for layer, seq in ((SURFACE, surf[p]), (MATERIAL, mat[p])):
            ids[p, layer], counts[p, layer], other, misses = count_slots(seq)
            tail[p, 2 + layer] = other
        tail[p, 0], tail[p, 1] = len(surf[p]), misses
    t = tail.astype(np.int64)
    assert np.all(counts.sum(axis=2, dtype=np.int64) + t[:, 2:4] + t[:, 1:2] == t[:, 0:1])
    empty = int(np.count_nonzero(tail[:, 1] == tail[:, 0]))
    overflow = (int(np.count_nonzero(tail[:, 2])), int(np.count_nonzero(tail[:, 3])))
    return ids, counts, tail, empty, overflow


def mattes(bundle, params, n_samples=None, first_sample=0, counts=None):
    """The whole rule over the tile of `params`: n_samples of every pixel, or counts[p] of pixel p, from sample first_sample on"""
    surf, mat, _ = sample_ids(bundle, params, n_samples=n_samples, first_sample=first_sample, counts=counts)
    return mattes_of_ids(surf, mat)


def matte_select(ids, counts, tail, layer, id_list):
    """drt_read_matte: coverage [P] = (the counts of the layer's slots whose id is in id_list, plus misses if -1 is) / c_p; the sum
    in integers, one division"""
    want = set(int(v) for v in id_list)
    P = ids.shape[0]
    total = np.zeros(P, dtype=np.int64)
    for p in range(P):
        s = int(tail[p, 1]) if ID_MISS in want else 0
        for k in range(SLOTS):
            if int(ids[p, layer, k]) >= 0 and int(ids[p, layer, k]) in want:
                s += int(counts[p, layer, k])
        total[p] = s
    return total.astype(np.float64) / tail[:, 0].astype(np.float64)


def palette(i):
    """(R, G, B) of an id: h = (uint32)(id + 1) * 0x9E3779B1; h ^= h >> 16; 64 + (h & 127), 64 + ((h >> 8) & 127), 64 + ((h >> 16) & 127)"""
    h = ((int(i) + 1) * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 16
    return 64 + (h & 127), 64 + ((h >> 8) & 127), 64 + ((h >> 16) & 127)


def matte_bgra(ids, counts, tail, layer):
    """drt_read_matte_bgra's bytes [P][4]: per channel v = sum over the ranked slots, from +0, of (count / c_p) * palette(id), the
    byte (uint8)(v + 0.5); alpha 255"""
    P = ids.shape[0]
    out = np.empty((P, 4), dtype=np.uint8)
    for p in range(P):
        c = np.float64(tail[p, 0])
        v = [np.float64(0.0)] * 3
        for k in range(SLOTS):
            share = np.float64(counts[p, layer, k]) / c
            pal = palette(ids[p, layer, k])
            for ch in range(3):
                v[ch] = v[ch] + share * np.float64(pal[ch])
        out[p] = [int(v[2] + 0.5), int(v[1] + 0.5), int(v[0] + 0.5), 255]
    return out
