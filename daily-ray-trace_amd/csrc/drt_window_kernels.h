/*
 * drt_window_kernels.h -- the live window's two helpers (drt_window_rule.h has the rule, DESIGN.md section 3 the proof).
 *
 * A windowed kernel pair traces and shades the window's pixels only, on a compact staging film [win_h][win_w] that the unchanged
 * dense kernels see as their tile. drt_window_copy_kernel moves the window's film rows between the tile's film and the staging
 * film (once each way per render call); drt_window_fill_kernel gives every tile pixel outside the window, per kernel pair, what n
 * samples worth +0 leave on the film.
 */
#ifndef DRT_WINDOW_KERNELS_H
#define DRT_WINDOW_KERNELS_H

#define WINDOW_BLOCK 256

struct WindowParams
{
    uint32_t tile_w;             /* row pitch of the tile's film, in pixels */
    uint32_t row0, rows;         /* the pair's tile rows [row0, row0 + rows) */
    uint32_t wx0, wx1, wy0, wy1; /* the window in tile columns [wx0, wx1) and tile rows [wy0, wy1) */
    uint32_t S, xyz, tail;       /* wavelengths; XYZ film (then only `pixels`, XYZ_FILM_WORDS words a pixel); the film has tail wavelengths */
    uint32_t first_sample, n_samples;
    uint32_t draws;              /* pixel draws per path: 2 under DRT_FILM_SAMPLE_RANDOM, else 0 */
};

/* One thread per word of the window's rows of one film buffer: `words` words per pixel. to_stage: film -> staging, else back. */
__global__ void __launch_bounds__(WINDOW_BLOCK) drt_window_copy_kernel(double *film, double *stage, WindowParams wp, uint32_t words, int to_stage)
{
    const uint64_t row_words = (uint64_t)(wp.wx1 - wp.wx0) * words;
    const uint64_t n = (uint64_t)(wp.wy1 - wp.wy0) * row_words;
    for (uint64_t i = (uint64_t)blockIdx.x * WINDOW_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * WINDOW_BLOCK)
    {
        const uint64_t r = i / row_words, c = i - r * row_words;
        double *f = film + ((uint64_t)(wp.wy0 + r) * wp.tile_w + wp.wx0) * words + c;
        if (to_stage) stage[i] = *f;
        else *f = stage[i];
    }
}

/* One thread per (pixel of the pair's rows, wavelength); a pixel inside the window is the dense kernels' business. A wavelength whose
 * three accumulators are all +0 (bit pattern zero) stays as it is -- the DARK rule of shade_pixels, which holds per wavelength --
 * otherwise it gets the film update of n samples of value +0 in order: the expressions of shade_pixels' film update, same denom. The
 * filter word gets += n. Nothing is done after a pair whose record pool ran out: that pair is rendered again, and filled again. One
 * thread adds the dead paths to the pair's statistics: a path, one closest-hit scan and its pixel draws each. */
__global__ void __launch_bounds__(WINDOW_BLOCK) drt_window_fill_kernel(double *pixels, double *avgs, double *vars, WindowParams wp, const uint32_t *overflow,
                                                                        unsigned long long *pair_counters)
{
    if (*overflow != 0u) return;
    const uint32_t lanes = wp.xyz ? 7u : wp.S + 1u; /* threads per pixel: the wavelengths and the filter word; XYZ: its seven accumulators */
    const uint64_t n = (uint64_t)wp.rows * wp.tile_w * lanes;
    const uint64_t i = (uint64_t)blockIdx.x * WINDOW_BLOCK + threadIdx.x;
    if (i == 0)
    {
        const uint64_t r_lo = wp.wy0 > wp.row0 ? wp.wy0 : wp.row0, r_hi = wp.wy1 < wp.row0 + wp.rows ? wp.wy1 : wp.row0 + wp.rows;
        const uint64_t live = r_hi > r_lo ? (r_hi - r_lo) * (wp.wx1 - wp.wx0) : 0u;
        const unsigned long long dead = ((uint64_t)wp.rows * wp.tile_w - live) * wp.n_samples;
        atomicAdd(pair_counters + 0, dead);
        atomicAdd(pair_counters + 1, dead);
        atomicAdd(pair_counters + 4, dead * wp.draws);
    }
    if (i >= n) return;
    const uint64_t q = i / lanes;
    const uint32_t lam = (uint32_t)(i - q * lanes);
    const uint32_t row = wp.row0 + (uint32_t)(q / wp.tile_w), col = (uint32_t)(q % wp.tile_w);
    if (row >= wp.wy0 && row < wp.wy1 && col >= wp.wx0 && col < wp.wx1) return;
    const uint64_t pix = (uint64_t)row * wp.tile_w + col;
    if (wp.xyz)
    {
        double *px = pixels + pix * XYZ_FILM_WORDS;
        if (lam == 3u) px[3] += (double)wp.n_samples * 1.0;
        else if (lam < 3u || wp.tail) px[lam] += 0.0; /* the pair's spectral sum is +0 at every wavelength, and so are its X, Y, Z (words 4..6: the tail pass's) */
        return;
    }
    double *px = pixels + pix * (uint64_t)(wp.S + 1u);
    if (lam == wp.S)
    {
        px[wp.S] += (double)wp.n_samples * 1.0; /* filter sum: += 1.0 per sample */
        return;
    }
    double *pa = avgs + pix * (uint64_t)wp.S, *pv = vars + pix * (uint64_t)wp.S;
    double f_sum = px[lam], f_avg = pa[lam], f_var = pv[lam];
    if (((uint64_t)__double_as_longlong(f_sum) | (uint64_t)__double_as_longlong(f_avg) | (uint64_t)__double_as_longlong(f_var)) == 0ull) return;
    const double contribution = 0.0;
    for (uint32_t s = 0; s < wp.n_samples; s += 1)
    {
        const double denom = (double)(wp.first_sample + s + 1u);
        f_sum = f_sum + contribution;
        double t0 = contribution - f_avg;
        double t1 = t0;
        t0 = t0 / denom;
        f_avg = f_avg + t0;
        t0 = contribution - f_avg;
        t0 = t1 * t0;
        f_var = f_var + t0;
    }
    px[lam] = f_sum;
    pa[lam] = f_avg;
    pv[lam] = f_var;
}

#endif
