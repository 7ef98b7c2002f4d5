"""The convergence rule of adaptive sampling (include/drt_hip.h, drt_adaptive), restated in numpy: a loop over the wavelengths in
ascending order, vectorised over pixels, so that every sum runs in the order drt_converge_kernel takes (np.sum would sum pairwise)
and every decision comes out the same. Not a test file: the adaptive tests import it."""
import numpy as np


def luminance_and_error(spds, cmf_rw, cmf_y, interval, avgs, vars_, n):
    """Y and E of pixels holding n samples. avgs / vars_: [pixels][S] film rows (vars_: the sum of products, not divided)."""
    rw, cy = spds[cmf_rw], spds[cmf_y]
    S = rw.shape[0]
    N = 0.0
    for i in range(S):
        N += cy[i] * rw[i]
    N *= interval
    c = np.float64(n)
    d = c * (c - 1.0)
    avgs = np.asarray(avgs, dtype=np.float64).reshape(-1, S)
    vars_ = np.asarray(vars_, dtype=np.float64).reshape(-1, S)
    Y = np.zeros(avgs.shape[0])
    E = np.zeros(avgs.shape[0])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(S):
            Y = Y + cy[i] * avgs[:, i] * rw[i]
            E = E + cy[i] * np.sqrt(vars_[:, i] / d) * rw[i]
        Y = Y * (interval / N)
        E = E * (interval / N)
    return Y, E


def stays_active(spds, cmf_rw, cmf_y, interval, avgs, vars_, n, max_spp, rel_error, floor):
    """bool per pixel: n < max_spp and not E <= rel_error * max(|Y|, floor) (a NaN stays)"""
    Y, E = luminance_and_error(spds, cmf_rw, cmf_y, interval, avgs, vars_, n)
    aY = np.abs(Y)
    m = np.where(aY >= floor, aY, floor)
    with np.errstate(invalid="ignore"):
        done = E <= rel_error * m
    return (n < max_spp) & ~done


def rounds(min_spp, max_spp, step):
    """the sample counts after each round, as long as some pixel is active: min_spp, then + min(step, max_spp - n) up to max_spp"""
    n = [min_spp]
    while n[-1] < max_spp:
        n.append(n[-1] + min(step, max_spp - n[-1]))
    return n


def sample_counts(snapshot, spds, cmf_rw, cmf_y, interval, n_pix, min_spp, max_spp, step, rel_error, floor):
    """The counts the rule gives. snapshot(n) -> (avgs, vars) [n_pix][S] of a uniform n-sample render (only the rows of pixels
    still active are read). Returns (counts, rounds run)."""
    counts = np.zeros(n_pix, dtype=np.uint32)
    active = np.arange(n_pix)
    ran = 0
    for n in rounds(min_spp, max_spp, step):
        if active.size == 0:
            break
        ran += 1
        av, va = snapshot(n)
        counts[active] = n
        keep = stays_active(spds, cmf_rw, cmf_y, interval, av[active], va[active], n, max_spp, rel_error, floor)
        active = active[keep]
    return counts, ran
