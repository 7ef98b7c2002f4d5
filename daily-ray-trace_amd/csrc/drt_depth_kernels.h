/*
 * drt_depth_kernels.h -- depth-cut films (drt_bind_depth_cuts): beside the film of a render at max_depth D,
 * the film of the same render at every bound cut depth d_0 < d_1 < ... <= D, from one trace.
 *
 * The path generator is keyed by (seed, pixel, sample) only, so a render at max_depth = d walks the first d loop iterations of the
 * render at max_depth = D: its film is cast_ray's `dst` after those iterations (src/daily_ray_trace.c:440-472), times the vignette
 * (:615), through the film update (:732-743). The vertex records the trace stage wrote hold all of that; drt_depth_cut_kernel replays
 * them a second time, beside the shade kernel, and stops where the shade kernel's registers never do.
 *
 * For a path with n shaded vertices, (dst_j, throughput_j) being the state after j of them, cut d is worth dst_min(n, d), plus
 * throughput_n * emission when the path ended on an emitter (header term == 1) and n < d: the break of :452-457 happens in loop
 * iteration n, which a render at max_depth = d <= n never reaches.
 *
 * One wave per (pixel, wavelength set), lane = wavelength 64 * set + lane. The pixel's samples in order; a path is replayed once, up
 * to min(n, d_last) vertices, and `dst` goes through cut c's film update when the vertex count reaches d_c (or, for the cuts beyond
 * n, when the path ends). The cuts' accumulators -- sum, mean, variance: six 32-bit registers per cut -- stay in registers over the
 * launch's samples: every cut film is read and written once per launch, as the main film is. NCUTS is a template argument, so the
 * accumulators are registers by name and `c` never indexes them at run time.
 *
 * The vertex is the shade kernel's general loop and nothing else: record fields lifted to scalars by v_readlane, bdsf_at_wavelength
 * over the record's own list, the light block `((sum + 0) * em) * c`. None of the main pass's shortcuts (the header's plastic mask
 * and light-0 bits, the fixed-list bodies, the staged tails) are read: they change no bit and are why the main pass is hard to change.
 */
#pragma once

#include "drt_kernels.h"

#define DEPTH_BLOCK 256
#define DEPTH_WAVES (DEPTH_BLOCK / 64)

struct DepthCutParams
{
    uint64_t n_pix;                  /* pixels of this launch: the films below start at its first pixel */
    uint32_t n_samples, first_sample, vertex_words, block_words;
    uint32_t n_lights, batch;        /* batch: sample slots per pixel in the header array */
    const uint32_t *overflow;        /* the trace launch ran out of record blocks: nothing here is touched */
    uint32_t n_sets, n_items;        /* wavelength sets per pixel (ceil(S / 64)); work items: n_pix * n_sets */
    uint32_t depth[DRT_MAX_DEPTH_CUTS];        /* ascending, each in 1 .. max_depth; the first NCUTS count */
    double  *pixels[DRT_MAX_DEPTH_CUTS];       /* per cut: [n_pix][S + 1] sum + filter */
    double  *avgs[DRT_MAX_DEPTH_CUTS];         /* [n_pix][S] */
    double  *vars[DRT_MAX_DEPTH_CUTS];         /* [n_pix][S] */
};

/* The kernel's argument list, in its order: the kernarg segment has this very layout (as ShadeConst). The 24 film pointers are read
 * from there where a work item starts and ends -- scalar loads -- instead of living in scalar registers, or parked in vector lanes,
 * across the sample loop. */
struct DepthConst
{
    DevScene       sc;
    DepthCutParams dp;
    const uint64_t *records, *headers;
    unsigned long long *work_counter;
};
static_assert(sizeof(DevScene) % 8 == 0 && sizeof(DepthCutParams) % 8 == 0, "DepthConst mirrors the kernarg segment only while every argument ends on an 8-byte boundary");
__device__ __forceinline__ const DepthConst &depth_const()
{
    uint32_t off = 0;
    asm volatile("" : "+s"(off));
    return *(const DepthConst *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + off);
}

/* the first 64 words (or all, when it has fewer) of vertex v's record, word `lane` in lane `lane` */
__device__ __forceinline__ uint64_t depth_vertex_words(const uint64_t *__restrict__ records, const DepthCutParams &dp, uint64_t h2, uint64_t h3, uint32_t v,
                                                       uint32_t lane)
{
    return lane < dp.vertex_words ? path_vertex(records, dp.block_words, dp.vertex_words, h2, h3, v)[lane] : 0;
}

template <int NCUTS, bool SPDS_IN_LDS>
__global__ __launch_bounds__(DEPTH_BLOCK) void drt_depth_cut_kernel(DevScene sc, DepthCutParams dp, const uint64_t *__restrict__ records,
                                                                    const uint64_t *__restrict__ headers, unsigned long long *__restrict__ work_counter)
{
    extern __shared__ double lds[];
    const uint32_t S = sc.S;
    if (*dp.overflow) return; /* the records of this launch are incomplete: the cut films stay as they are, as the main film does */
    if (SPDS_IN_LDS)
    {
        const uint32_t spd_words = sc.n_spd * S;
        for (uint32_t k = threadIdx.x; k < spd_words; k += DEPTH_BLOCK) lds[k] = sc.spds[k];
        __syncthreads();
    }
    const double *table = SPDS_IN_LDS ? (const double *)lds : sc.spds;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t vw = dp.vertex_words;
    const uint32_t d_last = dp.depth[NCUTS - 1];

    for (;;)
    {
        /* the next (pixel, wavelength set): waves are persistent and draw from a counter, because pixel cost varies */
        uint32_t item = 0;
        if (lane == 0) item = (uint32_t)atomicAdd(work_counter, 1ull);
        item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= dp.n_items) break;
        const uint64_t pix = item / dp.n_sets;
        const uint32_t lam = 64u * (item - (uint32_t)pix * dp.n_sets) + lane;
        const bool active = lam < S;
        const uint32_t lam_c = active ? lam : 0; /* lanes past the table read row element 0 and are never stored */

        double f_sum[NCUTS], f_avg[NCUTS], f_var[NCUTS];
        {
        const DepthCutParams &kc = depth_const().dp;
#pragma unroll
        for (int c = 0; c < NCUTS; c += 1)
        {
            f_sum[c] = active ? kc.pixels[c][pix * (uint64_t)(S + 1) + lam] : 0.0;
            f_avg[c] = active ? kc.avgs[c][pix * (uint64_t)S + lam] : 0.0;
            f_var[c] = active ? kc.vars[c][pix * (uint64_t)S + lam] : 0.0;
        }
        }

        for (uint32_t s0 = 0; s0 < dp.n_samples; s0 += 64u)
        {
            /* the headers of a window of samples in one coalesced load, lane s <- sample s (as the shade kernel) */
            const uint32_t n_win = (uint32_t)__builtin_amdgcn_readfirstlane((int)((dp.n_samples - s0 < 64u) ? dp.n_samples - s0 : 64u));
            uint64_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;
            if (lane < n_win)
            {
                const uint64_t *h = headers + (pix * dp.batch + s0 + lane) * REC_HEADER_WORDS;
                h0 = h[0];
                h1 = h[1];
                h2 = h[2];
                h3 = h[3];
            }
            for (uint32_t s = 0; s < n_win; s += 1)
            {
                const uint64_t hs = readlane64(h0, s);
                const double vignette = word_as_double(readlane64(h1, s));
                const uint32_t n_shaded = (uint32_t)(hs & 0xFFFFu);
                const uint32_t term = (uint32_t)(hs >> 16) & HDR_TERM_MASK;
                const uint32_t term_spd = (uint32_t)(hs >> 32) & 0xFFFFu;
                const uint64_t hs2 = readlane64(h2, s), hs3 = readlane64(h3, s);
                const uint32_t n_replay = n_shaded < d_last ? n_shaded : d_last;
                const double denom = (double)(dp.first_sample + s0 + s + 1);

                /* cut c's film update with this sample's value, :615 and :732-743 */
                auto film_update = [&](int c, double value) {
                    const double contribution = value * vignette;
                    f_sum[c] = f_sum[c] + contribution;
                    double t0 = contribution - f_avg[c];
                    double t1 = t0;
                    t0 = t0 / denom;
                    f_avg[c] = f_avg[c] + t0;
                    t0 = contribution - f_avg[c];
                    t0 = t1 * t0;
                    f_var[c] = f_var[c] + t0;
                };

                double throughput = 1.0, dst = 0.0; /* :440 */
                uint64_t next = n_replay != 0u ? depth_vertex_words(records, dp, hs2, hs3, 0u, lane) : 0;
                for (uint32_t v = 0; v < n_replay; v += 1)
                {
                    const uint64_t src = next;
                    if (v + 1u < n_replay) next = depth_vertex_words(records, dp, hs2, hs3, v + 1u, lane); /* in flight while this one is replayed */
                    const uint64_t list = readlane64(src, 0);
                    const uint64_t w1 = readlane64(src, 1);
                    const uint32_t num_bdsfs = (uint32_t)(w1 & 0xFFu);
                    const uint32_t sflags = (uint32_t)(w1 >> 8) & 0xFFu;
                    const uint64_t w2 = readlane64(src, 2);
                    const double on_dot = word_as_double(readlane64(src, 3));
                    const double dir_pdf = word_as_double(readlane64(src, 4));
                    const uint32_t i_diffuse = (uint32_t)(w1 >> 16) & 0xFFFFu, i_glossy = (uint32_t)(w1 >> 32) & 0xFFFFu;
                    const uint32_t i_mirror = (uint32_t)(w1 >> 48) & 0xFFFFu;
                    uint32_t i_ir, i_tr, i_te;
                    bool paired;
                    fresnel_rows(w2, i_ir, i_tr, i_te, paired);
                    const double diffuse = spd_at(table, S, i_diffuse, lam_c), glossy = spd_at(table, S, i_glossy, lam_c);
                    const double mirror = spd_at(table, S, i_mirror, lam_c), ir = spd_at(table, S, i_ir, lam_c);
                    const double tr = spd_at(table, S, i_tr, lam_c), te = spd_at(table, S, i_te, lam_c);
                    double contribution = 0.0;
                    for (uint32_t l = 0; l < dp.n_lights; l += 1) /* direct_light_contribution, :272-332 */
                    {
                        const uint32_t off = REC_VERTEX_WORDS + l * REC_LIGHT_WORDS;
                        uint64_t lw[REC_LIGHT_WORDS];
                        if (off + REC_LIGHT_WORDS <= 64u)
                        {
#pragma unroll
                            for (int k = 0; k < REC_LIGHT_WORDS; k += 1) lw[k] = readlane64(src, off + k);
                        }
                        else
                        {
                            /* light block beyond the 64 words fetched: uniform loads straight from the record */
                            const uint64_t *lp = path_vertex(records, dp.block_words, vw, hs2, hs3, v) + off;
#pragma unroll
                            for (int k = 0; k < REC_LIGHT_WORDS; k += 1) lw[k] = readlane64(lp[k], 0);
                        }
                        const uint32_t lflags = (uint32_t)(lw[0] >> 16) & 0xFFu;
                        if (!(lflags & FLAG_VISIBLE)) continue;
                        const uint32_t i_em = (uint32_t)(lw[0] & 0xFFFFu);
                        const double c = word_as_double(lw[1]);
                        double reflectance = bdsf_at_wavelength<false>(list, num_bdsfs, diffuse, glossy, mirror, ir, tr, te, on_dot, word_as_double(lw[2]),
                                                                       word_as_double(lw[3]), word_as_double(lw[4]), word_as_double(lw[5]), lflags, paired);
                        contribution = contribution + reflectance;                    /* :323 */
                        contribution = contribution * spd_at(table, S, i_em, lam_c); /* :324 */
                        contribution = contribution * c;                              /* :326-327 */
                    }
                    const double s_a_in = word_as_double(readlane64(src, 5)), s_spec = word_as_double(readlane64(src, 6));
                    const double s_mn = word_as_double(readlane64(src, 7)), s_ct = word_as_double(readlane64(src, 8));
                    dst = dst + throughput * contribution; /* :461-462 */
                    double reflectance = bdsf_at_wavelength<false>(list, num_bdsfs, diffuse, glossy, mirror, ir, tr, te, on_dot, s_a_in, s_spec, s_mn, s_ct,
                                                                   sflags, paired);
                    reflectance = reflectance * dir_pdf; /* :468 */
                    throughput = throughput * reflectance; /* :469 */
                    /* v + 1 vertices done: a render at that max_depth ends here, whatever this path went on to do */
#pragma unroll
                    for (int c = 0; c < NCUTS; c += 1)
                        if (dp.depth[c] == v + 1u) film_update(c, dst);
                }
                /* the cuts the path did not reach: it ended in loop iteration n_shaded, on an emitter or on nothing */
                if (n_shaded < d_last)
                {
                    double value = dst;
                    if (term == 1u) value = dst + throughput * spd_at(table, S, term_spd, lam_c); /* emissive black body hit, :452-457 */
#pragma unroll
                    for (int c = 0; c < NCUTS; c += 1)
                        if (dp.depth[c] > n_shaded) film_update(c, value);
                }
            }
        }
        const DepthCutParams &kc = depth_const().dp;
#pragma unroll
        for (int c = 0; c < NCUTS; c += 1)
        {
            if (active)
            {
                kc.pixels[c][pix * (uint64_t)(S + 1) + lam] = f_sum[c];
                kc.avgs[c][pix * (uint64_t)S + lam] = f_avg[c];
                kc.vars[c][pix * (uint64_t)S + lam] = f_var[c];
            }
            if (lam == 0u) kc.pixels[c][pix * (uint64_t)(S + 1) + S] += (double)dp.n_samples * 1.0; /* filter sum: += 1.0 per sample, :733 */
        }
    }
}
