"""The rule of drt_render_adaptive_continue (include/drt_hip.h), restated in numpy on top of tests/adaptive_rule.py: every pixel starts
from the count n_p it holds, is tested on its own rows with c = n_p, and while it is active gets min(step, max_spp - n_p) more
samples and is tested again. Not a test file: the tests of the continuation import it."""
import numpy as np

import adaptive_rule as R


def active_of(snapshot, spds, cmf_rw, cmf_y, interval, counts, pixels, max_spp, rel_error, floor):
    """bool per entry of `pixels`: the rule's decision for pixel p on the rows of snapshot(counts[p]).
    snapshot(n) -> (avgs, vars) [n_pix][S] of a uniform n-sample render."""
    pixels = np.asarray(pixels)
    keep = np.zeros(pixels.size, dtype=bool)
    for n in np.unique(counts[pixels]):
        sel = counts[pixels] == n
        if n >= max_spp:
            continue  # finished, whatever its rows say
        av, va = snapshot(int(n))
        keep[sel] = R.stays_active(spds, cmf_rw, cmf_y, interval, av[pixels[sel]], va[pixels[sel]], int(n), max_spp, rel_error, floor)
    return keep


def continue_counts(snapshot, spds, cmf_rw, cmf_y, interval, start, max_spp, step, rel_error, floor, max_rounds=0):
    """The counts a continuation from `start` ([n_pix] counts, each >= 2) ends with.
    Returns (counts, rendering rounds, samples rendered, the active pixels left, ascending)."""
    counts = np.asarray(start).astype(np.int64).reshape(-1).copy()
    active = np.arange(counts.size)
    active = active[active_of(snapshot, spds, cmf_rw, cmf_y, interval, counts, active, max_spp, rel_error, floor)]
    ran, paths = 0, 0
    while active.size and not (max_rounds and ran >= max_rounds):
        k = np.minimum(step, max_spp - counts[active])
        counts[active] += k
        paths += int(k.sum())
        ran += 1
        active = active[active_of(snapshot, spds, cmf_rw, cmf_y, interval, counts, active, max_spp, rel_error, floor)]
    return counts.astype(np.uint32), ran, paths, active


def allotment_contract(counts, active, max_spp, step):
    """what keeps a round a rectangle of pixels x samples: all active pixels hold one count, or every max_spp - n_p is a multiple of step"""
    n = np.asarray(counts)[np.asarray(active, dtype=np.int64)].astype(np.int64)
    return n.size == 0 or n.min() == n.max() or bool(((max_spp - n) % step == 0).all())
