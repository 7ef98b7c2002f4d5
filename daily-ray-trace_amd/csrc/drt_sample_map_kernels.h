/*
 * drt_sample_map_kernels.h -- sample maps (drt_render_sample_map): every tile pixel rendered to a count the caller gives. DESIGN.md,
 * section 5k, states the rule; tests/sample_map_rule.py restates it.
 *
 * A pixel's count n_p is its filter sum (the film's column S). The map gives it a remainder R_p (absolute mode: target - n_p where
 * the target is larger; DRT_MAP_ADD: the target itself), and the call renders R_p in binary rounds: for every set bit b of
 * B = OR_p R_p, ascending, the next 2^b samples of the pixels whose R_p has bit b, each from the count it holds then.
 *   drt_map_adopt_kernel   once per call: counts and remainders of every tile pixel, and the call's report (MAP_* words below), reduced
 *                          in the wave, then in the block: at most one atomic per block and word
 *   drt_map_select_kernel  per round: counts refreshed from the filter sums, one ballot word per wave and the block's kept count
 *                          for drt_converge_scan and drt_converge_scatter (list_in == NULL), which write the round's list
 * One lane per tile pixel, blocks of CONVERGE_BLOCK threads (drt_adaptive_kernels.h comes first in the launcher).
 */
#pragma once

/* words of the report (the host presets BAD and OVER to 0xFFFFFFFF, the rest to 0) */
#define MAP_BAD 0      /* the first tile pixel whose filter sum is not a whole number in [0, 2^32) */
#define MAP_OVER 1     /* DRT_MAP_ADD: the first tile pixel whose count + target passes 2^32 - 1 */
#define MAP_BITS 2     /* B: the OR of the remainders */
#define MAP_MAX 3      /* the largest count + remainder */
#define MAP_RENDERED 4 /* pixels with a remainder */
#define MAP_ABOVE 5    /* absolute mode: pixels whose count is above their target */
#define MAP_PATHS 6    /* the sum of the remainders, 64 bits (words 6 and 7) */
#define MAP_WORDS 8

__global__ __launch_bounds__(CONVERGE_BLOCK) void drt_map_adopt_kernel(const double *__restrict__ pixels, uint32_t S, uint32_t n_pix,
                                                                       const uint32_t *__restrict__ targets, uint32_t add,
                                                                       uint32_t *__restrict__ counts, uint32_t *__restrict__ remainder,
                                                                       uint32_t *report)
{
    const uint64_t p = (uint64_t)blockIdx.x * CONVERGE_BLOCK + threadIdx.x;
    const bool valid = p < n_pix;
    const double f = valid ? pixels[(size_t)p * (S + 1) + S] : 0.0;
    const bool ok = f >= 0.0 && f < 4294967296.0 && f == __builtin_floor(f); /* a NaN fails the first comparison */
    const uint32_t n = ok ? (uint32_t)f : 0u;
    const uint32_t t = valid ? targets[p] : 0u;
    const bool over = valid && ok && add && t > 0xFFFFFFFFu - n;
    const bool above = valid && ok && !add && n > t;
    uint32_t R = 0u;
    if (valid && ok && !over) R = add ? t : (t > n ? t - n : 0u);
    if (valid)
    {
        counts[p] = n;
        remainder[p] = R;
    }
    const unsigned long long bad_mask = __ballot(valid && !ok);
    const unsigned long long over_mask = __ballot(over);
    const unsigned long long some_mask = __ballot(R != 0u);
    const unsigned long long above_mask = __ballot(above);
    /* the wave's OR, maximum and 64-bit sum (64 remainders of 32 bits: the sum is kept in two halves that each fit 32 bits) */
    uint32_t bits = R, hi = valid ? n + R : 0u, sum_lo = R & 0xFFFFu, sum_hi = R >> 16;
    for (int off = 32; off > 0; off >>= 1)
    {
        bits |= (uint32_t)__shfl_xor((int)bits, off);
        const uint32_t h2 = (uint32_t)__shfl_xor((int)hi, off);
        hi = h2 > hi ? h2 : hi;
        sum_lo += (uint32_t)__shfl_xor((int)sum_lo, off);
        sum_hi += (uint32_t)__shfl_xor((int)sum_hi, off);
    }
    /* the block's waves through LDS, then one atomic per block and word that has something to say (a million pixels' waves, each with
     * its own atomics on these eight words, took 0.77 ms; the blocks' take a quarter of them) */
    __shared__ uint32_t s_first[CONVERGE_WAVES][2], s_word[CONVERGE_WAVES][6];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0)
    {
        const uint32_t p0 = (uint32_t)p; /* the wave's first pixel: lane l is pixel p0 + l */
        s_first[wave][0] = bad_mask ? p0 + (uint32_t)__builtin_ctzll(bad_mask) : 0xFFFFFFFFu;
        s_first[wave][1] = over_mask ? p0 + (uint32_t)__builtin_ctzll(over_mask) : 0xFFFFFFFFu;
        s_word[wave][0] = bits;
        s_word[wave][1] = hi;
        s_word[wave][2] = (uint32_t)__popcll(some_mask);
        s_word[wave][3] = (uint32_t)__popcll(above_mask);
        s_word[wave][4] = sum_lo;
        s_word[wave][5] = sum_hi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t bad = 0xFFFFFFFFu, ovr = 0xFFFFFFFFu, all_bits = 0, top = 0, some = 0, abv = 0;
        unsigned long long paths = 0;
        for (uint32_t k = 0; k < CONVERGE_WAVES; k += 1)
        {
            bad = s_first[k][0] < bad ? s_first[k][0] : bad;
            ovr = s_first[k][1] < ovr ? s_first[k][1] : ovr;
            all_bits |= s_word[k][0];
            top = s_word[k][1] > top ? s_word[k][1] : top;
            some += s_word[k][2];
            abv += s_word[k][3];
            paths += ((unsigned long long)s_word[k][5] << 16) + (unsigned long long)s_word[k][4];
        }
        if (bad != 0xFFFFFFFFu) atomicMin(report + MAP_BAD, bad);
        if (ovr != 0xFFFFFFFFu) atomicMin(report + MAP_OVER, ovr);
        if (all_bits) atomicOr(report + MAP_BITS, all_bits);
        if (top) atomicMax(report + MAP_MAX, top);
        if (some)
        {
            atomicAdd(report + MAP_RENDERED, some);
            atomicAdd((unsigned long long *)(report + MAP_PATHS), paths);
        }
        if (abv) atomicAdd(report + MAP_ABOVE, abv);
    }
}

/* Round b's keep bits over every tile pixel: bit b of the pixel's remainder (b == 32: none, the pass after the last round, which
 * leaves the counts current and the list empty). Nothing but the remainders and the filter sums is read, so the kernel rerun
 * after a redone pair writes the same words. */
__global__ __launch_bounds__(CONVERGE_BLOCK) void drt_map_select_kernel(const double *__restrict__ pixels, uint32_t S, uint32_t n_pix,
                                                                        const uint32_t *__restrict__ remainder, uint32_t b,
                                                                        uint32_t *__restrict__ counts, unsigned long long *__restrict__ keep_mask,
                                                                        uint32_t *__restrict__ block_keep, const uint32_t *overflow)
{
    __shared__ uint32_t s_kept[CONVERGE_WAVES];
    if (*overflow) return; /* block-uniform: the previous round's pairs are rendered again first */
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t p = (uint64_t)blockIdx.x * CONVERGE_BLOCK + threadIdx.x;
    const bool valid = p < n_pix;
    if (valid) counts[p] = (uint32_t)pixels[(size_t)p * (S + 1) + S];
    const bool keep = valid && b < 32u && ((remainder[p] >> b) & 1u);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0)
    {
        if (valid) keep_mask[p / 64u] = mask;
        s_kept[wave] = (uint32_t)__popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t t = 0;
        for (uint32_t k = 0; k < CONVERGE_WAVES; k += 1) t += s_kept[k];
        block_keep[blockIdx.x] = t;
    }
}
