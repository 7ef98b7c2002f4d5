"""Bucket films (drt_bind_buckets): the rule, in plain numpy with + - * / and < only.

Bucket films. A context is bound to n buckets, 1 <= n <= 8. Sample number m (absolute) belongs to bucket b = m % n, as that bucket's
sample number j = m // n. Its contribution c[0..S) -- what the film update of src/daily_ray_trace.c:732 takes, vignette included -- goes
through the reference's film update (:732-743, as oracle/drt_oracle.c:1076-1086 restates it) into bucket b's film only: sum = sum + c,
the running mean and the variance accumulator with the divisor (double)(j + 1), the filter column += 1.0. The samples of one bucket
are applied in ascending m. With n = 1 the bucket film is the main film.

Resolve, for trim count t with 0 <= 2 t < n and n >= 2, per pixel and wavelength over the buckets' running means x_0 .. x_{n-1}:
  1. mu = x_0, then mu = mu + x_b for b = 1 .. n-1 in order, then mu = mu / (double)n;
  2. d_b = x_b - mu; q = d_0 * d_0, then q = q + d_b * d_b in order; error = q / (double)(n * (n - 1));
  3. y = x sorted by odd-even transposition: for round r = 0 .. n-1, for i = r % 2, r % 2 + 2, ... < n - 1: when y[i+1] < y[i] the two
     change places. A comparison with a NaN is false and exchanges nothing, and so is -0 < +0;
  4. e = y[t], then e = e + y[i] for i = t+1 .. n-1-t in order, then estimate = e / (double)(n - 2 t).
numpy's float64 `+ - * /` on arrays are IEEE operations one element at a time and contract nothing; the exchange copies values (np.where
on the comparison's result), so a NaN's payload and a zero's sign travel with it."""
import numpy as np

MAX_BUCKETS = 8


def empty_film(P, S):
    return np.zeros((P, S + 1)), np.zeros((P, S)), np.zeros((P, S))


def film_update(film, c, j):
    """in place: film = (pixels [P][S+1], means [P][S], variances [P][S]), c [P][S] the sample that is number j of this film"""
    px, av, va = film
    S = c.shape[1]
    with np.errstate(all="ignore"):
        px[:, :S] = px[:, :S] + c
        t0 = c - av
        t1 = t0
        t0 = t0 / float(j + 1)
        av[:] = av + t0
        t0 = c - av
        t0 = t1 * t0
        va[:] = va + t0
        px[:, S] = px[:, S] + 1.0


def bucket_films(n, samples, first_sample=0, films=None):
    """the n bucket films after samples first_sample, first_sample + 1, ...: samples [M][P][S] per-sample contributions. `films`: those of
    earlier calls, continued in place"""
    assert 1 <= n <= MAX_BUCKETS
    samples = np.asarray(samples, dtype=np.float64)
    if films is None:
        films = [empty_film(samples.shape[1], samples.shape[2]) for _ in range(n)]
    assert len(films) == n
    for s in range(samples.shape[0]):
        m = first_sample + s
        film_update(films[m % n], samples[s], m // n)
    return films


def sort_network(x):
    """step 3: x [n][...] -> y [n][...], a copy sorted by the odd-even transposition network along axis 0"""
    y = [np.array(v, dtype=np.float64, copy=True) for v in x]
    n = len(y)
    with np.errstate(all="ignore"):
        for r in range(n):
            for i in range(r % 2, n - 1, 2):
                swap = y[i + 1] < y[i]
                lo = np.where(swap, y[i + 1], y[i])
                hi = np.where(swap, y[i], y[i + 1])
                y[i], y[i + 1] = lo, hi
    return y


def resolve(means, t):
    """steps 1 to 4: means [n][...] -> (estimate [...], error [...])"""
    x = [np.asarray(v, dtype=np.float64) for v in means]
    n = len(x)
    assert n >= 2 and 0 <= 2 * t < n
    with np.errstate(all="ignore"):
        mu = x[0]
        for b in range(1, n):
            mu = mu + x[b]
        mu = mu / float(n)
        d = x[0] - mu
        q = d * d
        for b in range(1, n):
            d = x[b] - mu
            q = q + d * d
        err = q / float(n * (n - 1))
        y = sort_network(x)
        e = y[t]
        for i in range(t + 1, n - t):
            e = e + y[i]
        e = e / float(n - 2 * t)
    return e, err


def legal_trims(n):
    return [t for t in range(n) if 2 * t < n]


def median_trim(n):
    """the trim count of the median (n odd) or of the mean of the two middle values (n even)"""
    return (n - 1) // 2

