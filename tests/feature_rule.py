"""The first-hit feature buffers (include/drt_hip.h, drt_features), restated: per tile pixel the running mean
and the sum of squared deviations of eight numbers of its samples' first hits -- normal, depth, coverage, albedo -- and the surface
the first sample sees. Only + - * / sqrt enter, every sum is sequential, nothing is contracted. Not a test file: the feature tests
import it.

A sample's camera ray is the path's own: the oracle's RNG seeded with the path key of (x, y, sample), the draws camera_ray takes in
its order, then camera_ray's arithmetic operation by operation (here, vectorised over all the samples at once); the closest hit is
the oracle's find_ray_intersection. The running update is the film's (d = phi - m; m = m + d / k; M2 = M2 + d (phi - m)).

Like denoise_rule the rule counts the quotients it takes that are subnormal and not zero: the device's division may be one unit off
there, so a bitwise test asserts that its input has none."""
import ctypes as C

import numpy as np

import oracle_py as O
import pydrt

CHANNELS = 8  # DRT_FEATURE_CHANNELS: normal x y z, depth, coverage, albedo X Y Z
_TINY = np.finfo(np.float64).tiny
_f64p = C.POINTER(C.c_double)


def _subnormal(q):
    q = np.asarray(q)
    return int(np.count_nonzero((q != 0.0) & (np.abs(q) < _TINY)))


def colour_table(bundle):
    """[num_materials][3]: XYZ of a material's emission (emissive) or of (diffuse + glossy) + mirror, an SPD index of -1 reading as
    zeros; channel k with CMF row ck is (sum_i ck[i] r[i] rw[i]) * (interval / N), N the normalisation of the denoiser's guide step.
    Returns (table, subnormal quotients)."""
    sc = bundle.scene
    spds = bundle.spds()
    S = bundle.S
    rw, cy = spds[int(sc.cmf_rw)], spds[int(sc.cmf_y)]
    interval = np.float64(sc.wavelength_interval)
    N = np.float64(0.0)
    for i in range(S):
        N = N + cy[i] * rw[i]
    N = N * interval
    with np.errstate(all="ignore"):
        scale = interval / N
    zeros = np.zeros(S)

    def row(i):
        return spds[i] if i >= 0 else zeros

    table = np.zeros((int(sc.num_materials), 3))
    for m in range(int(sc.num_materials)):
        mat = sc.materials[m]
        if mat.is_emissive:
            r = row(int(mat.emission_spd))
        else:
            r = (row(int(mat.diffuse_spd)) + row(int(mat.glossy_spd))) + row(int(mat.mirror_spd))
        for k, c in enumerate((int(sc.cmf_x), int(sc.cmf_y), int(sc.cmf_z))):
            ck = spds[c]
            acc = np.float64(0.0)
            for i in range(S):
                acc = acc + ck[i] * r[i] * rw[i]
            table[m, k] = acc * scale
    return table, _subnormal(scale)


def tile_pixels(params):
    """(x [P], y [P]) image coordinates of the tile pixels, tile row by tile row"""
    stride = int(params.row_stride) or 1
    i = np.tile(np.arange(int(params.tile_w)), int(params.tile_h))
    j = np.repeat(np.arange(int(params.tile_h)), int(params.tile_w))
    return int(params.x0) + i, int(params.y0) + j * stride


def sample_draws(bundle, params, x, y, sample):
    """What camera_ray draws for the samples (x[n], y[n], sample[n]): the two film offsets (0.5 with FILM_SAMPLE_CENTER) and, behind a
    lens, the disc sample. DEVICE arithmetic (the disc sample takes the path's own sincos)."""
    L = O.oracle_lib()
    O.set_math_mode(O.MATH_DEVICE)
    n = len(x)
    scheme = int(params.pixel_scheme)
    lens = float(bundle.camera.aperture_radius) > 0.0
    px, py, disc = np.zeros(n), np.zeros(n), np.zeros((n, 3))
    if scheme == pydrt.FILM_SAMPLE_CENTER:
        px[:] = 0.5
        py[:] = 0.5
    out = (C.c_double * 3)()
    seed, w, h = int(params.seed), int(params.width), int(params.height)
    for k in range(n):
        if scheme != pydrt.FILM_SAMPLE_RANDOM and not lens:
            break
        L.drt_oracle_seed_path(L.drt_oracle_path_key(seed, w, h, int(x[k]), int(y[k]), int(sample[k])))
        if scheme == pydrt.FILM_SAMPLE_RANDOM:
            px[k] = L.drt_oracle_rng()
            py[k] = L.drt_oracle_rng()
        if lens:
            L.drt_oracle_uniform_sample_disc(out)
            disc[k] = out[0], out[1], out[2]
    return px, py, disc


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalise(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def camera_rays(bundle, x, y, px, py, disc):
    """camera_ray (csrc/drt_kernels.h; sample_scene's ray set-up, src/daily_ray_trace.c:550-607) on n samples at once: origin [n][3]
    and direction [n][3]. A camera without a field of view gives NaN, as it does there."""
    cam = bundle.camera
    forward, right, up = (np.array(list(v)) for v in (cam.forward, cam.right, cam.up))
    ap, bl = np.array(list(cam.aperture_position)), np.array(list(cam.film_bottom_left))
    with np.errstate(all="ignore"):
        film_x = (np.asarray(x, dtype=np.float64) + px) * np.float64(cam.pixel_width)
        film_y = (np.asarray(y, dtype=np.float64) + py) * np.float64(cam.pixel_height)
        bottom = up[None, :] * film_y[:, None]
        left = right[None, :] * film_x[:, None]
        pixel_point = (left + bottom) + bl[None, :]
        if float(cam.aperture_radius) > 0.0:
            focus_dir = _normalise(ap[None, :] - pixel_point)
            focus_dir = focus_dir * (np.float64(cam.focal_depth) / _dot(focus_dir, forward[None, :]))[:, None]
            focus_point = pixel_point + focus_dir
            cols = (C.c_double * 9)()
            O.oracle_lib().drt_oracle_rotation_between((C.c_double * 3)(0.0, 0.0, 1.0), (C.c_double * 3)(*forward), cols)
            m = np.array(list(cols)).reshape(3, 3)  # m[c][r]: column c, row r
            disc_point = disc * np.float64(cam.aperture_radius)
            # m_vmul: component r is the dot product of ROW r with the vector, summed left to right
            lens_point = np.stack([m[0, r] * disc_point[:, 0] + m[1, r] * disc_point[:, 1] + m[2, r] * disc_point[:, 2] for r in range(3)], axis=1)
            ro = ap[None, :] + lens_point
            rd = _normalise(focus_point - ro)
        else:
            ro = pixel_point
            rd = _normalise(ap[None, :] - ro)
    return ro, rd


def first_hit_vectors(bundle, ro, rd, table):
    """phi [n][8] and the closest-hit index [n] of n rays: find_ray_intersection as the oracle restates it (fudged origin, facing
    normal after the flip); a miss -- a NaN ray misses -- has phi0..4 = 0 and the escape material's colour."""
    L = O.oracle_lib()
    sc = bundle.scene
    cam = bundle.camera
    ap, fw = [np.float64(v) for v in cam.aperture_position], [np.float64(v) for v in cam.forward]
    n = ro.shape[0]
    phi = np.zeros((n, CHANNELS))
    ids = np.full(n, -1, dtype=np.int32)
    pt = O.Point()
    ro = np.ascontiguousarray(ro)
    rd = np.ascontiguousarray(rd)
    escape = table[int(sc.escape_material)]
    for k in range(n):
        idx = L.drt_oracle_find_ray_intersection(C.byref(sc), ro[k].ctypes.data_as(_f64p), rd[k].ctypes.data_as(_f64p), C.byref(pt))
        ids[k] = idx
        if idx < 0:
            phi[k, 5:8] = escape
            continue
        phi[k, 0], phi[k, 1], phi[k, 2] = pt.normal[0], pt.normal[1], pt.normal[2]
        dx, dy, dz = np.float64(pt.position[0]) - ap[0], np.float64(pt.position[1]) - ap[1], np.float64(pt.position[2]) - ap[2]
        phi[k, 3] = dx * fw[0] + dy * fw[1] + dz * fw[2]
        phi[k, 4] = 1.0
        phi[k, 5:8] = table[int(pt.surface_material)]
    return phi, ids


def running_moments(phi, counts):
    """The film's update (reference render_image, lines 736-743) over phi [P][max count][...]: pixel p takes its first counts[p]
    entries, in order. Returns (mean, M2, subnormal quotients)."""
    phi = np.asarray(phi, dtype=np.float64)
    counts = np.asarray(counts).reshape(-1)
    m = np.zeros((phi.shape[0],) + phi.shape[2:])
    M2 = np.zeros_like(m)
    sub = 0
    for k in range(int(counts.max()) if counts.size else 0):
        on = (k < counts).reshape((-1,) + (1,) * (m.ndim - 1))
        with np.errstate(all="ignore"):
            d = phi[:, k] - m
            q = d / np.float64(k + 1)
            sub += _subnormal(np.where(on, q, 0.0))
            m_new = m + q
            M2_new = M2 + d * (phi[:, k] - m_new)
        m = np.where(on, m_new, m)
        M2 = np.where(on, M2_new, M2)
    return m, M2, sub


def features(bundle, params, n_samples=None, first_sample=0, counts=None):
    """The whole rule over the tile of `params`: n_samples of every pixel, or counts[p] of pixel p (a film's filter column), from
    sample first_sample on. Returns (mean [P][8], m2 [P][8], ids [P] int32, empty pixels, subnormal quotients)."""
    x, y = tile_pixels(params)
    P = len(x)
    counts = np.full(P, int(n_samples), dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64).reshape(P)
    assert counts.min() >= 1
    cmax = int(counts.max())
    table, sub = colour_table(bundle)
    # every (pixel, k < count) pair, pixel-major
    pix = np.repeat(np.arange(P), counts)
    k = np.concatenate([np.arange(c) for c in counts])
    sx, sy, smp = x[pix], y[pix], int(first_sample) + k
    px, py, disc = sample_draws(bundle, params, sx, sy, smp)
    ro, rd = camera_rays(bundle, sx, sy, px, py, disc)
    phi_flat, ids_flat = first_hit_vectors(bundle, ro, rd, table)
    phi = np.zeros((P, cmax, CHANNELS))
    phi[pix, k] = phi_flat
    ids = ids_flat[k == 0].astype(np.int32)
    mean, m2, s2 = running_moments(phi, counts)
    empty = int(np.count_nonzero(mean[:, 4] == 0.0))
    return mean, m2, ids, empty, sub + s2


def feature_bgra(mean, which, lo, hi):
    """drt_read_feature_bgra's bytes [P][4]: which 0 normal (x, y, z to R, G, B), 1 depth, 2 coverage (grey); t = (v - lo) / (hi - lo)
    clamped to [0, 1], byte = (uint8)(t * 255.0 + 0.5); a NaN gives 0; alpha 255."""
    mean = np.asarray(mean, dtype=np.float64)
    v = mean[:, 0:3] if which == 0 else np.repeat(mean[:, 3 if which == 1 else 4][:, None], 3, axis=1)
    with np.errstate(all="ignore"):
        t = (v - np.float64(lo)) / (np.float64(hi) - np.float64(lo))
        t = np.where(t < 0.0, 0.0, t)
        t = np.where(t > 1.0, 1.0, t)
        b = np.where(np.isnan(t), 0.0, t * 255.0 + 0.5).astype(np.uint8)
    out = np.empty((mean.shape[0], 4), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = b[:, 2], b[:, 1], b[:, 0], 255
    return out
