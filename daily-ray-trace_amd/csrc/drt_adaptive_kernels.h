/*
 * drt_adaptive_kernels.h -- the convergence test of adaptive sampling (drt_render_adaptive) and the stable compaction of the
 * pixels that go on to the next round. DESIGN.md, "Adaptive sampling", states the rule; tests/adaptive_rule.py restates it.
 *
 * A round ends with three small kernels over the round's list of pixels (list_in; NULL in round 0: every tile pixel, in order):
 *   drt_converge_kernel   per list entry: Y and E from the pixel's film rows, the count, the keep bit (one ballot word per wave)
 *                         and the entries a block keeps
 *   drt_converge_scan     one block: exclusive offsets of the blocks' kept entries, and the total (the next round's active count)
 *   drt_converge_scatter  the kept entries to list_out at block offset + wave offset + prefix count: ascending tile order stays
 * All three do nothing when the round's record pool ran out (the host renders those samples again and re-enqueues them).
 *
 * A pixel's count is its filter sum (the film's column S: +1.0 per sample), read where it is needed: the test uses c = the pixel's own
 * count, and rerunning the kernels after a redone pair records the same counts again. drt_render_adaptive_continue starts from a film
 * it did not render: drt_adopt_counts_kernel checks every tile pixel's filter sum and takes it as the count, the three kernels above
 * test every pixel on the rows it holds, and drt_contract_kernel reduces the counts of the pixels that stay active to the three words
 * the allotment contract is decided on.
 */
#pragma once

#define CONVERGE_BLOCK 256
#define CONVERGE_WAVES (CONVERGE_BLOCK / 64)
#define CONVERGE_CHUNK 16                   /* wavelengths a wave stages per pass: 64 pixels x 16 doubles, 128 contiguous bytes per row */
#define CONVERGE_PAD (CONVERGE_CHUNK + 1)  /* LDS row stride in doubles: a lane reads its own row, odd stride spreads the banks */
#define CONVERGE_SCAN_BLOCK 1024
#define CONVERGE_MAX_S 256                  /* the white and y-bar rows in LDS (64 * SHADE_MAX_SETS wavelengths at most) */

struct ConvergeParams
{
    const uint32_t *list_in; /* [n_in] tile pixels of the round; NULL: entry e is tile pixel e */
    uint32_t n_in;
    uint32_t max_spp;        /* the cap (a listed pixel's count after this round is its filter sum) */
    uint32_t cmf_rw, cmf_y;  /* SPD rows of the white table and y-bar */
    double   interval, rel_error, floor;
    uint32_t *counts;        /* [tile pixels] samples per pixel */
    unsigned long long *keep_mask; /* [ceil(n_in / 64)] per wave: bit l, entry (wave * 64 + l) stays active */
    uint32_t *block_keep;    /* [grid] kept entries per block, then (drt_converge_scan) their exclusive offsets */
    uint32_t *active;        /* the next round's active count */
    uint32_t *list_out;      /* [n_in at most] */
    const uint32_t *overflow;
    const double *pixels;    /* the film's sums, [tile pixels][S + 1]: column S is the pixel's count */
    uint32_t *at_max;        /* += listed pixels whose count is max_spp or more (each is listed for the last time then) */
};

/* words of the report drt_adopt_counts_kernel and drt_contract_kernel leave (the host presets BAD and MIN to 0xFFFFFFFF, the rest to 0) */
#define ADOPT_BAD 0 /* the first tile pixel whose filter sum is not a whole number in [2, 2^32) */
#define ADOPT_MIN 1 /* over the active list: the smallest count, */
#define ADOPT_MAX 2 /* the largest, */
#define ADOPT_REM 3 /* and whether some max_spp - count is not a multiple of step */
#define ADOPT_WORDS 4

/* the lanes of one wave agree on their LDS slab: every lane's writes come before any lane's reads that follow (LDS operations of one
 * wave run in order; the fence keeps the compiler from moving them across) */
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(CONVERGE_BLOCK) void drt_converge_kernel(DevScene sc, ConvergeParams cp, const double *__restrict__ avgs,
                                                                      const double *__restrict__ vars)
{
    __shared__ double s_rows[CONVERGE_WAVES][64 * CONVERGE_PAD];
    __shared__ uint32_t s_pix[CONVERGE_WAVES][64];
    __shared__ uint32_t s_kept[CONVERGE_WAVES];
    __shared__ double s_rw[CONVERGE_MAX_S], s_cy[CONVERGE_MAX_S];
    if (*cp.overflow) return; /* block-uniform */
    const uint32_t S = sc.S;
    for (uint32_t i = threadIdx.x; i < S; i += CONVERGE_BLOCK)
    {
        s_rw[i] = sc.spds[(size_t)cp.cmf_rw * S + i];
        s_cy[i] = sc.spds[(size_t)cp.cmf_y * S + i];
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t e = (uint64_t)blockIdx.x * CONVERGE_BLOCK + threadIdx.x;
    const bool valid = e < cp.n_in;
    const uint32_t pixel = valid ? (cp.list_in ? cp.list_in[e] : (uint32_t)e) : 0u;
    s_pix[wave][lane] = pixel;
    const unsigned long long valid_mask = __ballot(valid);
    const double *rw = s_rw, *cy = s_cy;
    __syncthreads();
    /* the normalisation of drt_film_xyz_kernel, in its order */
    double N = 0.0;
    for (uint32_t i = 0; i < S; i += 1) N += (cy[i] * rw[i]);
    N *= cp.interval;
    const double c = valid ? cp.pixels[(size_t)pixel * (S + 1) + S] : 2.0; /* the pixel's count: what its rows were averaged over */
    const uint32_t n = (uint32_t)c;
    const double d = c * (c - 1.0);
    double Y = 0.0, E = 0.0;
    double *rows = s_rows[wave];
    /* Each wave works on its own slab from here on, so it waits for its own lanes only (wave_sync), never for the block's other waves;
     * and the avg and var pieces of a chunk are loaded in one go, so a wave has one round of loads in flight per chunk, not two. */
    for (uint32_t i0 = 0; i0 < S; i0 += CONVERGE_CHUNK)
    {
        const uint32_t w = (S - i0 < CONVERGE_CHUNK) ? S - i0 : CONVERGE_CHUNK;
        /* lanes 16r .. 16r+15 load a 16-double piece of one pixel's row, four rows per load instruction */
        double a_piece[CONVERGE_CHUNK], v_piece[CONVERGE_CHUNK];
#pragma unroll
        for (uint32_t r = 0; r < CONVERGE_CHUNK; r += 1)
        {
            const uint32_t k = r * 64u + lane, row = k / CONVERGE_CHUNK, col = k % CONVERGE_CHUNK;
            const bool ld = ((valid_mask >> row) & 1ull) && col < w;
            const size_t at = (size_t)s_pix[wave][row] * S + i0 + col;
            a_piece[r] = ld ? avgs[at] : 0.0;
            v_piece[r] = ld ? vars[at] : 0.0;
        }
#pragma unroll
        for (uint32_t r = 0; r < CONVERGE_CHUNK; r += 1)
        {
            const uint32_t k = r * 64u + lane;
            rows[(k / CONVERGE_CHUNK) * CONVERGE_PAD + k % CONVERGE_CHUNK] = a_piece[r];
        }
        wave_sync();
        /* the pixel's own sums, sequential over ascending wavelength */
        const double *mine = rows + lane * CONVERGE_PAD;
        if (valid)
            for (uint32_t t = 0; t < w; t += 1) Y += (cy[i0 + t] * mine[t] * rw[i0 + t]);
        wave_sync();
#pragma unroll
        for (uint32_t r = 0; r < CONVERGE_CHUNK; r += 1)
        {
            const uint32_t k = r * 64u + lane;
            rows[(k / CONVERGE_CHUNK) * CONVERGE_PAD + k % CONVERGE_CHUNK] = v_piece[r];
        }
        wave_sync();
        if (valid)
            for (uint32_t t = 0; t < w; t += 1) E += (cy[i0 + t] * __builtin_sqrt(mine[t] / d) * rw[i0 + t]);
        wave_sync();
    }
    Y = Y * (cp.interval / N);
    E = E * (cp.interval / N);
    const double aY = fabs(Y);
    const double m = aY >= cp.floor ? aY : cp.floor;
    const bool keep = valid && n < cp.max_spp && !(E <= cp.rel_error * m); /* a NaN stays */
    if (valid) cp.counts[pixel] = n;
    const unsigned long long mask = __ballot(keep);
    const unsigned long long full = __ballot(valid && n >= cp.max_spp);
    if (lane == 0)
    {
        if (full) atomicAdd(cp.at_max, (uint32_t)__popcll(full));
        if (e < cp.n_in) cp.keep_mask[e / 64u] = mask;
        s_kept[wave] = (uint32_t)__popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t t = 0;
        for (uint32_t k = 0; k < CONVERGE_WAVES; k += 1) t += s_kept[k];
        cp.block_keep[blockIdx.x] = t;
    }
}

/* one block: block_keep[0 .. n_blocks) -> exclusive offsets, in place; the total to *active */
__global__ __launch_bounds__(CONVERGE_SCAN_BLOCK) void drt_converge_scan(ConvergeParams cp, uint32_t n_blocks)
{
    __shared__ uint32_t s_sum[CONVERGE_SCAN_BLOCK];
    if (*cp.overflow) return;
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_blocks + CONVERGE_SCAN_BLOCK - 1) / CONVERGE_SCAN_BLOCK;
    const uint32_t b0 = t * per, b1 = (b0 + per < n_blocks) ? b0 + per : n_blocks;
    uint32_t mine = 0;
    for (uint32_t b = b0; b < b1; b += 1) mine += cp.block_keep[b];
    s_sum[t] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < CONVERGE_SCAN_BLOCK; off *= 2) /* inclusive scan of the threads' sums */
    {
        const uint32_t v = t >= off ? s_sum[t - off] : 0u;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    uint32_t run = s_sum[t] - mine;
    for (uint32_t b = b0; b < b1; b += 1)
    {
        const uint32_t k = cp.block_keep[b];
        cp.block_keep[b] = run;
        run += k;
    }
    if (t == CONVERGE_SCAN_BLOCK - 1) *cp.active = s_sum[t];
}

__global__ __launch_bounds__(CONVERGE_BLOCK) void drt_converge_scatter(ConvergeParams cp)
{
    if (*cp.overflow) return;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t e = (uint64_t)blockIdx.x * CONVERGE_BLOCK + threadIdx.x;
    const uint64_t w0 = (uint64_t)blockIdx.x * CONVERGE_WAVES; /* the block's first wave word */
    const uint64_t n_words = ((uint64_t)cp.n_in + 63u) / 64u;
    if (w0 + wave >= n_words) return;
    uint32_t at = cp.block_keep[blockIdx.x];
    for (uint32_t k = 0; k < wave; k += 1) at += (uint32_t)__popcll(cp.keep_mask[w0 + k]);
    const unsigned long long mask = cp.keep_mask[w0 + wave];
    if ((mask >> lane) & 1ull)
    {
        at += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        cp.list_out[at] = cp.list_in ? cp.list_in[e] : (uint32_t)e;
    }
}

/* Every tile pixel's count from its filter sum; report[ADOPT_BAD] = the first pixel whose sum is no count (a count is a whole number in
 * [2, 2^32): the variance needs two samples). One atomic per wave that holds such a pixel. */
__global__ __launch_bounds__(CONVERGE_BLOCK) void drt_adopt_counts_kernel(const double *__restrict__ pixels, uint32_t S, uint32_t n_pix,
                                                                          uint32_t *__restrict__ counts, uint32_t *report)
{
    const uint64_t p = (uint64_t)blockIdx.x * CONVERGE_BLOCK + threadIdx.x;
    const bool valid = p < n_pix;
    const double f = valid ? pixels[(size_t)p * (S + 1) + S] : 2.0;
    const bool ok = f >= 2.0 && f < 4294967296.0 && f == __builtin_floor(f); /* a NaN fails the first comparison */
    if (valid) counts[p] = ok ? (uint32_t)f : 0u;
    const unsigned long long bad = __ballot(valid && !ok);
    if (bad && (threadIdx.x & 63u) == 0) atomicMin(report + ADOPT_BAD, (uint32_t)(p + (uint32_t)__builtin_ctzll(bad)));
}

/* The allotment contract's three words over the active list the convergence kernels have just written: wave reductions, then one
 * atomic per word and wave. The list's length is read on the device (*n_active); the grid covers the longest list there can be. */
__global__ __launch_bounds__(CONVERGE_BLOCK) void drt_contract_kernel(const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_active,
                                                                      const uint32_t *__restrict__ counts, uint32_t max_spp, uint32_t step,
                                                                      uint32_t *report, const uint32_t *overflow)
{
    if (*overflow) return;
    const uint64_t e = (uint64_t)blockIdx.x * CONVERGE_BLOCK + threadIdx.x;
    const bool valid = e < *n_active;
    const uint32_t n = valid ? counts[list[e]] : 0u;
    uint32_t lo = valid ? n : 0xFFFFFFFFu, hi = valid ? n : 0u;
    for (int off = 32; off > 0; off >>= 1)
    {
        const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, off), h2 = (uint32_t)__shfl_xor((int)hi, off);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    const unsigned long long rem = __ballot(valid && (max_spp - n) % step != 0u); /* an active pixel has n < max_spp */
    const unsigned long long any = __ballot(valid);
    if ((threadIdx.x & 63u) == 0 && any)
    {
        atomicMin(report + ADOPT_MIN, lo);
        atomicMax(report + ADOPT_MAX, hi);
        if (rem) atomicOr(report + ADOPT_REM, 1u);
    }
}
