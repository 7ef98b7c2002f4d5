"""The variance-guided denoiser of the spectral film (include/drt_hip.h, drt_denoise), restated in numpy:
vectorised over pixels, Python loops over window, patch and wavelengths in the rule's order, so that every sum runs in the order the
device takes and every decision comes out the same. Only + - * / sqrt enter. Not a test file: the denoise tests import it.

Besides the filtered film the rule counts the quotients it takes that are subnormal and not zero: the device's division may be one
unit off there, so a bitwise test asserts that its input has none."""
import numpy as np

_TINY = np.finfo(np.float64).tiny


class _Quotients:
    """a / b, counting the results that are subnormal and not zero (where `count` says the rule takes the quotient at all)"""

    def __init__(self):
        self.subnormal = 0

    def div(self, a, b, count=True):
        q = np.asarray(a / b)
        m = (q != 0.0) & (np.abs(q) < _TINY)
        if count is not True:
            m = m & count
        self.subnormal += int(np.count_nonzero(m))
        return q


def usable_counts(c):
    """a count is a whole number in [2, 2^32)"""
    with np.errstate(invalid="ignore"):
        return (c >= 2.0) & (c < 4294967296.0) & (c == np.floor(c))


def hand_made_film(S, w=9, h=7, seed=11):
    """Positive spectra of the size 1 with mixed counts, and among them: NaN and infinite rows, the counts 0, 1, 2.5 and 2^32,
    pixels that are all zero. No value is near the subnormal range, so no quotient of the rule is."""
    rng = np.random.default_rng(seed)
    P = w * h
    counts = rng.choice([2.0, 3.0, 8.0, 17.0, 64.0], P)
    level = np.where(np.arange(P) % w < w // 2, 1.0, 1.5)[:, None]
    av = level * (0.75 + 0.5 * rng.random((P, S)))
    va = (0.05 + 0.1 * rng.random((P, S))) * (counts * (counts - 1.0))[:, None] * level * level
    counts[3], counts[10], counts[17], counts[24] = 0.0, 1.0, 2.5, 4294967296.0
    av[5, 2] = np.nan
    va[12, S // 2] = np.nan
    av[19, 0] = np.inf
    va[26, S - 1] = np.inf
    va[33, 1] = -1.0  # (the square root of a negative variance is a NaN)
    for p in (7, 8, 16, 40):
        av[p] = 0.0
        va[p] = 0.0
    px = np.empty((P, S + 1))
    px[:, :S] = av * counts[:, None]
    px[:, S] = counts
    return px, av, va, w, h


def guide(spds, cmf, interval, pixels, avgs, vars_, quot=None):
    """Step 1. cmf = (rw, x, y, z) SPD rows. Returns G [P][3], s [P][3], V [P][3], the variance of the mean var / (c (c - 1))
    [P][S] and usable [P]."""
    quot = quot or _Quotients()
    rw = spds[cmf[0]]
    S = rw.shape[0]
    pixels = np.asarray(pixels, dtype=np.float64).reshape(-1, S + 1)
    avgs = np.asarray(avgs, dtype=np.float64).reshape(-1, S)
    vars_ = np.asarray(vars_, dtype=np.float64).reshape(-1, S)
    P = avgs.shape[0]
    cy = spds[cmf[2]]
    N = 0.0
    for i in range(S):
        N += cy[i] * rw[i]
    N *= interval
    with np.errstate(all="ignore"):
        scale = quot.div(np.float64(interval), np.float64(N))
        c = pixels[:, S]
        d = c * (c - 1.0)
        G = np.zeros((P, 3))
        s = np.zeros((P, 3))
        nv = np.empty((P, S))
        for i in range(S):
            nv[:, i] = quot.div(vars_[:, i], d)
            r = np.sqrt(nv[:, i])
            for k in range(3):
                ck = spds[cmf[1 + k]]
                G[:, k] = G[:, k] + ck[i] * avgs[:, i] * rw[i]
                s[:, k] = s[:, k] + ck[i] * r * rw[i]
        G = G * scale
        s = s * scale
        V = s * s
        ok = usable_counts(c) & np.all(np.isfinite(G), axis=1) & np.all(np.isfinite(V), axis=1)
    return G, s, V, nv, ok


def _falloff(x):
    """f(x) = (x < 1) ? (1 - (x > 0 ? x : 0))^2 : 0; a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        t = 1.0 - np.where(x > 0.0, x, 0.0)
        return np.where(x < 1.0, t * t, 0.0)


def _shift(a, dy, dx, fill):
    """b[y][x] = a[y + dy][x + dx], `fill` outside"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys0, ys1 = max(0, -dy), min(H, H - dy)
    xs0, xs1 = max(0, -dx), min(W, W - dx)
    if ys0 < ys1 and xs0 < xs1:
        b[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return b


def denoise(spds, cmf, interval, tile_w, tile_h, pixels, avgs, vars_, radius=5, patch=1, k=1.0, alpha=1.0, centre_gate=True,
            want_weights=False):
    """The whole rule. Returns (mean' [P][S], var' [P][S], unusable pixels, subnormal quotients) and, with want_weights, also the
    weights [window][P] in window order. centre_gate=False leaves the gate by the centre pair's own distance out (tests only: it
    shows why the rule has it)."""
    quot = _Quotients()
    rw = spds[cmf[0]]
    S = rw.shape[0]
    H, Wd = int(tile_h), int(tile_w)
    P = H * Wd
    avgs = np.asarray(avgs, dtype=np.float64).reshape(P, S)
    vars_ = np.asarray(vars_, dtype=np.float64).reshape(P, S)
    k = np.float64(k)
    alpha = np.float64(alpha)
    G, _, V, nv, ok = guide(spds, cmf, interval, pixels, avgs, vars_, quot)
    G2, V2, ok2 = G.reshape(H, Wd, 3), V.reshape(H, Wd, 3), ok.reshape(H, Wd)
    k2 = k * k
    R, F = int(radius), int(patch)

    def pair_e(dy, dx):
        """e(a, b) for b = a + (dy, dx), at every a; valid where both are inside and usable"""
        Gb, Vb, okb = _shift(G2, dy, dx, 0.0), _shift(V2, dy, dx, 0.0), _shift(ok2, dy, dx, False)
        valid = ok2 & okb
        with np.errstate(all="ignore"):
            tot = None
            for c in range(3):
                Ga, Va = G2[:, :, c], V2[:, :, c]
                gb, vb = Gb[:, :, c], Vb[:, :, c]
                diff = Ga - gb
                num = diff * diff - alpha * (Va + np.where(vb < Va, vb, Va))
                den = k2 * (Va + vb)
                pos = valid & (den > 0.0)
                q = quot.div(num, np.where(pos, den, 1.0), pos)
                delta = np.where(den > 0.0, q, np.where(num <= 0.0, 0.0, np.inf))
                tot = delta if tot is None else tot + delta
        return tot, valid

    Wsum = np.zeros((H, Wd))
    macc = np.zeros((H, Wd, S))
    vacc = np.zeros((H, Wd, S))
    av2, nv2 = avgs.reshape(H, Wd, S), nv.reshape(H, Wd, S)
    weights = []
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            e0, valid0 = pair_e(dy, dx)
            total = np.zeros((H, Wd))
            n = np.zeros((H, Wd))
            with np.errstate(all="ignore"):
                for oy in range(-F, F + 1):
                    for ox in range(-F, F + 1):
                        # the pair (p + o, q + o): the displacement's e, read at p + o
                        eo = _shift(e0, oy, ox, 0.0)
                        vo = _shift(valid0, oy, ox, False)
                        total = np.where(vo, total + eo, total)
                        n = n + vo
                D = quot.div(total, np.where(valid0, 3.0 * n, 1.0), valid0)
                Dc = quot.div(e0, 3.0, valid0)
                w = _falloff(D)
                if centre_gate:
                    fc = _falloff(Dc)
                    w = np.where(fc < w, fc, w)
                w = np.where(valid0, w, 0.0)
                Wsum = Wsum + w
                avq = _shift(av2, dy, dx, 0.0)
                nvq = _shift(nv2, dy, dx, 0.0)
                use = (w != 0.0)[:, :, None]  # (a term of weight 0 adds a zero to a sum that is never -0: leaving it out changes no bit)
                macc = np.where(use, macc + w[:, :, None] * avq, macc)
                vacc = np.where(use, vacc + (w * w)[:, :, None] * nvq, vacc)
            if want_weights:
                weights.append(w.reshape(P).copy())
    with np.errstate(all="ignore"):
        okp = ok2[:, :, None]
        Wd3 = np.where(ok2, Wsum, 1.0)[:, :, None]
        mean = np.where(okp, quot.div(macc, Wd3, okp), av2)
        var = np.where(okp, quot.div(vacc, Wd3 * Wd3, okp), nv2)
    out = (mean.reshape(P, S), var.reshape(P, S), int(P - np.count_nonzero(ok)), quot.subnormal)
    if want_weights:
        return out + (np.array(weights),)
    return out
