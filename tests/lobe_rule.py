"""Lobe films (drt_bind_lobes): the map, the presets, the classes, and what of the rule can be said without a path.

A context is bound to n films, 1 <= n <= 8, and a map of 15 entries: `emission`, `direct[f]` and `indirect[f]` for each of the seven
scattering functions f of include/bdsf_list.h. An entry is a film 0 .. n-1 or NONE. For one sample, with f_i the i-th entry of vertex
0's own list and a_i(args) the dispatcher's bdsf_result after entry i (the function's value, or the value carried over from the entry
before it when its direction test fails, 0.0 when nothing came before):
  R^c_K(args) = 0.0, then R = a_i + R over the positions i with K[f_i] == c in list order (K: the direct or the indirect row);
  C^c = 0.0, then per visible light in order C = C + R^c_direct(light), C = C * em, C = C * c_l -- for every film;
  vertex 0: dst^c = 0.0 + 1.0 * C^c, T^c = 1.0 * (R^c_indirect(sample) * dir_pdf);
  vertex v >= 1: dst^c = dst^c + T^c * C_v, T^c = T^c * (R_v * dir_pdf_v) with the main film's C_v and R_v;
  the end, on an emitter below max_depth: value^c = dst^c + T^c * spd for every film when a vertex was shaded; with none,
  value = 0.0 + 1.0 * spd for film `emission` and 0.0 for the others;
  value^c * vignette goes through the reference's film update of film c with the sample's own number + 1 as the divisor: every film
  takes every sample, zeros included.

What follows from it without tracing anything, and is what the tests use:
  - a map with all 15 entries on one film makes that film the main film; a film no entry names is the film of all-zero samples;
  - R^c_K is the dispatcher's own sum over the list restricted to the functions K sends to c, PROVIDED the carry-over sees the same
    values in the restricted list: restriction_is_exact() says when. Then the film of a class is the existing oracle's render of the
    bundle with its lists restricted in Python.
The film-level rule is bucket_rule.bucket_films(1, ...): one film, every sample, the divisor the sample's number + 1."""
import numpy as np

import bucket_rule

MAX_LOBE_FILMS = 8
NONE = 0xFF
# names and order of include/bdsf_list.h
FUNCTIONS = ("bp_diffuse_bdsf", "bp_glossy_bdsf", "mirror_bdsf", "fs_conductor_bdsf", "fs_dielectric_reflectance_bdsf",
             "fs_dielectric_transmittance_bdsf", "ct_conductor_bdsf")
F = {name: k for k, name in enumerate(FUNCTIONS)}
NUM = len(FUNCTIONS)

# functions that assign bdsf_result whatever the directions are (src/bdsf.c:105-119, :174-186); the others test the directions first
# and leave bdsf_result as it was when the test fails (quirk Q1)
ALWAYS_ASSIGN = frozenset((F["bp_diffuse_bdsf"], F["bp_glossy_bdsf"], F["ct_conductor_bdsf"]))

# the classes of the standard preset
CLASSES = {
    "diffuse": (F["bp_diffuse_bdsf"],),
    "glossy": (F["bp_glossy_bdsf"], F["ct_conductor_bdsf"]),
    "specular": (F["mirror_bdsf"], F["fs_conductor_bdsf"], F["fs_dielectric_reflectance_bdsf"]),
    "transmission": (F["fs_dielectric_transmittance_bdsf"],),
}


def entries(emission=NONE, direct=None, indirect=None, default=NONE):
    """the 15 entries of a map as a list: emission, direct[7], indirect[7]; direct / indirect: {function index or name: film}"""
    def row(d):
        out = [default] * NUM
        for f, film in (d or {}).items():
            out[F[f] if isinstance(f, str) else int(f)] = int(film)
        return out
    return [int(emission)] + row(direct) + row(indirect)


def all_to(film):
    return [film] * (1 + 2 * NUM)


def map_error(n, e):
    """why drt_bind_lobes refuses (n, entries), or None"""
    if n == 0:
        return None
    if n > MAX_LOBE_FILMS:
        return "%d films, at most %d" % (n, MAX_LOBE_FILMS)
    if e is None:
        return "null map"
    assert len(e) == 1 + 2 * NUM
    for k, v in enumerate(e):
        if not 0 <= v <= 0xFF:
            return "entry %d is no byte" % k
        if v >= n and v != NONE:
            return "entry %d names film %d of %d" % (k, v, n)
    return None


def films_needed(e):
    used = [v for v in e if v != NONE]
    return max(used) + 1 if used else 1


def preset_functions():
    """eight films: emission, then one per function, direct and indirect together"""
    both = {f: 1 + f for f in range(NUM)}
    names = ["emission"] + [n[:-len("_bdsf")] for n in FUNCTIONS]
    return entries(0, both, both), names


def preset_standard():
    """seven films: emission; diffuse direct, indirect; glossy direct, indirect; specular; transmission"""
    direct, indirect = {}, {}
    for f in CLASSES["diffuse"]:
        direct[f], indirect[f] = 1, 2
    for f in CLASSES["glossy"]:
        direct[f], indirect[f] = 3, 4
    for f in CLASSES["specular"]:
        direct[f] = indirect[f] = 5
    for f in CLASSES["transmission"]:
        direct[f] = indirect[f] = 6
    names = ["emission", "diffuse_direct", "diffuse_indirect", "glossy_direct", "glossy_indirect", "specular", "transmission"]
    return entries(0, direct, indirect), names


PRESETS = {"functions": preset_functions(), "standard": preset_standard()}


def class_direct_map(functions):
    """test 2's map: emission and the class's direct light on film 0, everything else on film 1"""
    return entries(0, {f: 0 for f in functions}, {}, default=1)


def class_map(functions):
    """test 3's map: emission, the class's direct and indirect light on film 0, everything else on film 1"""
    keep = {f: 0 for f in functions}
    return entries(0, keep, keep, default=1)


def restrict(lst, functions):
    """the list with only the entries whose function is in `functions`, in order"""
    return [f for f in lst if f in functions]


def restriction_is_exact(lst, functions):
    """True when the sum of the addends of `functions` in `lst` is the dispatcher's own sum over restrict(lst, functions) for every
    direction: every kept function either always assigns bdsf_result, or is preceded in the list only by kept functions -- then what
    it carries over when its direction test fails is what it carries over in the restricted list."""
    for i, f in enumerate(lst):
        if f not in functions or f in ALWAYS_ASSIGN:
            continue
        if any(g not in functions for g in lst[:i]):
            return False
    return True


def film_of_samples(samples, first_sample=0, film=None):
    """the film-level rule: samples [M][P][S], the contributions of samples first_sample, first_sample + 1, ... to ONE lobe film, through
    the reference's film update with the sample's own number + 1 as the divisor: bucket_rule's rule with one bucket"""
    return bucket_rule.bucket_films(1, samples, first_sample=first_sample, films=None if film is None else [film])[0]


def empty_film(P, S, sample_numbers):
    """the film no entry names: every sample is worth +0, so sums, means and variances stay +0 and the filter column counts"""
    return film_of_samples(np.zeros((len(sample_numbers), P, S)), first_sample=sample_numbers[0] if len(sample_numbers) else 0)


def gamma(max_depth, n_lights, spp, n):
    """the sum identity's bound: the depth of the two evaluation trees of the same polynomial, doubled, in units of 2^-53"""
    return 2.0 * (5 * max_depth + 3 * n_lights + 17 + spp + n) * 2.0 ** -53


def sum_identity_violations(films_px, main_px, g):
    """per element of the `pixels` buffers (filter column aside): |sum_c film_c - main| <= g * (sum_c |film_c| + |main|), NaN for NaN.
    Returns the number of elements that break it and the largest ratio seen."""
    with np.errstate(all="ignore"):
        total = films_px[0][:, :-1].copy()
        mag = np.abs(films_px[0][:, :-1])
        for px in films_px[1:]:
            total = total + px[:, :-1]
            mag = mag + np.abs(px[:, :-1])
        main = main_px[:, :-1]
        mag = mag + np.abs(main)
        nan_t, nan_m = np.isnan(total), np.isnan(main)
        diff = np.abs(total - main)
        bad = (nan_t != nan_m) | (~nan_m & ~(diff <= g * mag))
        ratio = np.where(~nan_m & (mag > 0), diff / np.where(mag > 0, mag, 1.0), 0.0)
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0
