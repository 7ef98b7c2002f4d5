"""Sensor films (drt_bind_sensor): the rule, in plain numpy with + - * / only.

For pixel p, sample number m (absolute), the sample's contribution c[0..S) -- what the film update of src/daily_ray_trace.c:732 takes,
vignette included -- and the curves R[k][0..S):
  1. for each wavelength set j = 0 .. ceil(S/64) - 1: q[i] = R[k][64j+i] * c[64j+i] where 64j+i < S, and +0.0 elsewhere (i = 0..63);
  2. six times q = q[0::2] + q[1::2]; then t_j = q[0];
  3. v_k = t_0, then v_k = v_k + t_j for j = 1, 2, ... in order;
  4. v_k through the reference's film update (:732-743, as oracle/drt_oracle.c:1076-1086 restates it): sum_k = sum_k + v_k, the running
     mean and the variance accumulator with the divisor (double)(m + 1), the filter column += 1.0.
numpy's float64 `+` and `*` on arrays are IEEE operations one element at a time and contract nothing."""
import numpy as np


def channel_values(curves, c):
    """steps 1 to 3: curves [n][S], c [P][S] (one sample's contributions) -> v [P][n]"""
    curves = np.asarray(curves, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    n, S = curves.shape
    P = c.shape[0]
    assert c.shape == (P, S)
    n_sets = (S + 63) // 64
    v = np.zeros((P, n))
    with np.errstate(all="ignore"):
        for k in range(n):
            vk = None
            for j in range(n_sets):
                lo, hi = 64 * j, min(64 * j + 64, S)
                q = np.zeros((P, 64))  # +0.0 where 64j+i >= S
                q[:, :hi - lo] = curves[k, lo:hi] * c[:, lo:hi]
                for _ in range(6):
                    q = q[:, 0::2] + q[:, 1::2]
                t = q[:, 0]
                vk = t if vk is None else vk + t
            v[:, k] = vk
    return v


def film_update(film, v, m):
    """step 4, in place: film = (pixels [P][n+1], means [P][n], variances [P][n]), v [P][n] the values of sample number m"""
    px, av, va = film
    n = v.shape[1]
    with np.errstate(all="ignore"):
        px[:, :n] = px[:, :n] + v
        t0 = v - av
        t1 = t0
        t0 = t0 / float(m + 1)
        av[:] = av + t0
        t0 = v - av
        t0 = t1 * t0
        va[:] = va + t0
        px[:, n] = px[:, n] + 1.0


def empty_film(P, n):
    return np.zeros((P, n + 1)), np.zeros((P, n)), np.zeros((P, n))


def sensor_film(curves, samples, first_sample=0, film=None):
    """the sensor film after samples first_sample, first_sample + 1, ...: samples [M][P][S] per-sample contributions"""
    curves = np.asarray(curves, dtype=np.float64)
    samples = np.asarray(samples)
    if film is None:
        film = empty_film(samples.shape[1], curves.shape[0])
    for s in range(samples.shape[0]):
        film_update(film, channel_values(curves, samples[s]), first_sample + s)
    return film


def bgra(film, which, matrix):
    """drt_read_sensor_bgra: which 0 = sum / filter, 1 = mean; row r of the 3 x n matrix: m[r][0] * v_0, then + m[r][k] * v_k in order;
    clamp to [0, 1], x 255, truncate, a NaN gives 0; stored B, G, R, 255"""
    px, av, _ = film
    matrix = np.asarray(matrix, dtype=np.float64)
    n = av.shape[1]
    assert matrix.shape == (3, n)
    out = np.empty((px.shape[0], 4), dtype=np.uint8)
    out[:, 3] = 255
    with np.errstate(all="ignore"):
        for r in range(3):
            f = None
            for k in range(n):
                v = px[:, k] / px[:, n] if which == 0 else av[:, k]
                t = matrix[r, k] * v
                f = t if f is None else f + t
            nan = np.isnan(f)
            f = np.where(f < 0.0, 0.0, f)
            f = np.where(f > 1.0, 1.0, f)
            out[:, 2 - r] = np.where(nan, 0.0, f * 255.0).astype(np.uint8)
    return out
