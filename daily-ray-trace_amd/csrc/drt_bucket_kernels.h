/*
 * drt_bucket_kernels.h -- bucket films (drt_bind_buckets): beside the film of a render, n films of the same
 * render's samples dealt out in turn -- sample number m (absolute) goes to bucket m % n as that bucket's sample number m / n -- and a
 * robust resolve over the n running means.
 *
 * The rule (tests/bucket_rule.py restates it in numpy). For pixel p, sample m and its contribution c[0..S) -- what the film update of
 * src/daily_ray_trace.c:732 takes, vignette included -- c goes through the film update (:732-743) of bucket b = m % n only, with the
 * divisor (double)(m / n + 1); the filter column of that bucket gets += 1.0. With n = 1 that is the main film.
 *
 * The resolve, per (pixel, wavelength), over the buckets' running means x_0 .. x_{n-1} and a trim count t, 0 <= 2 t < n:
 *   1. mu = x_0, then mu = mu + x_b for b = 1 .. n - 1 in order, then mu = mu / (double)n;
 *   2. d_b = x_b - mu; q = d_0 * d_0, then q = q + d_b * d_b in order; error = q / (double)(n * (n - 1));
 *   3. y = x sorted by odd-even transposition: for round r = 0 .. n - 1, for i = r % 2, r % 2 + 2, ... < n - 1: when y[i+1] < y[i]
 *      the two change places (a comparison with a NaN is false, and so is -0 < +0: the network says where those end up);
 *   4. e = y[t], then e = e + y[i] for i = t + 1 .. n - 1 - t in order, then estimate = e / (double)(n - 2 t).
 * Nothing is contracted (-ffp-contract=off).
 *
 * drt_bucket_kernel's replay is drt_depth_cut_kernel's at full depth and nothing else: headers by windows of 64 samples, path_vertex,
 * fresnel_rows, spd_at and bdsf_at_wavelength<false> over the record's own list, the light block `((sum + 0) * em) * c`, light blocks
 * beyond word 64 by uniform loads, the emitter term when term == 1, times the vignette. None of the main pass's shortcuts are read.
 *
 * One wave per (pixel, wavelength set), lane = wavelength 64 * set + lane. The sink is NB accumulator triples -- sum, mean, variance:
 * six 32-bit registers per bucket -- that stay in registers over the launch's samples: every bucket film is read and written once per
 * launch. NB is a template argument, so the triples are registers by name and nothing indexes them at run time. The bucket of a
 * sample is the same in every lane: it and the sample's number inside the bucket are two running scalar counters, set from
 * first_sample where a work item starts (two divisions by the constant NB) and stepped per sample, and a scalar branch per bucket
 * takes the sample to its one film update and its one division.
 */
#pragma once

#include "drt_depth_kernels.h"

#define BUCKET_BLOCK 256
#define BUCKET_WAVES (BUCKET_BLOCK / 64)

struct BucketParams
{
    uint64_t n_pix;                  /* pixels of this launch: the films below start at its first pixel */
    uint32_t n_samples, first_sample, vertex_words, block_words;
    uint32_t n_lights, batch;        /* batch: sample slots per pixel in the header array */
    const uint32_t *overflow;        /* the trace launch ran out of record blocks: nothing here is touched */
    uint32_t n_sets, n_items;        /* wavelength sets per pixel (ceil(S / 64)); work items: n_pix * n_sets */
    uint32_t max_depth, pad_;        /* the render's max_depth */
    double  *pixels[DRT_MAX_BUCKETS];          /* per bucket: [n_pix][S + 1] sum + filter; the first NB count */
    double  *avgs[DRT_MAX_BUCKETS];            /* [n_pix][S] */
    double  *vars[DRT_MAX_BUCKETS];            /* [n_pix][S] */
};

/* The kernel's argument list, in its order (as DepthConst): the 24 film pointers are read from the kernarg segment where a work item
 * starts and ends -- scalar loads -- instead of living in scalar registers across the sample loop. */
struct BucketConst
{
    DevScene       sc;
    BucketParams   bp;
    const uint64_t *records, *headers;
    unsigned long long *work_counter;
};
static_assert(sizeof(DevScene) % 8 == 0 && sizeof(BucketParams) % 8 == 0, "BucketConst mirrors the kernarg segment only while every argument ends on an 8-byte boundary");
__device__ __forceinline__ const BucketConst &bucket_const()
{
    uint32_t off = 0;
    asm volatile("" : "+s"(off));
    return *(const BucketConst *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + off);
}

/* the first 64 words (or all, when it has fewer) of vertex v's record, word `lane` in lane `lane` (as depth_vertex_words) */
__device__ __forceinline__ uint64_t bucket_vertex_words(const uint64_t *__restrict__ records, const BucketParams &bp, uint64_t h2, uint64_t h3, uint32_t v,
                                                        uint32_t lane)
{
    return lane < bp.vertex_words ? path_vertex(records, bp.block_words, bp.vertex_words, h2, h3, v)[lane] : 0;
}

/* of the n samples whose buckets are b0, b0 + 1, ... (mod NB), how many fall into bucket c: those at offsets r, r + NB, ... */
template <int NB>
__device__ __forceinline__ uint32_t bucket_share(uint32_t b0, uint32_t n, uint32_t c)
{
    const uint32_t r = c >= b0 ? c - b0 : c + (uint32_t)NB - b0;
    return r < n ? (n - r + (uint32_t)NB - 1u) / (uint32_t)NB : 0u;
}

template <int NB, bool SPDS_IN_LDS>
__global__ __launch_bounds__(BUCKET_BLOCK) void drt_bucket_kernel(DevScene sc, BucketParams bp, const uint64_t *__restrict__ records,
                                                                  const uint64_t *__restrict__ headers, unsigned long long *__restrict__ work_counter)
{
    static_assert(NB >= 1 && NB <= DRT_MAX_BUCKETS, "one instantiation per bucket count");
    extern __shared__ double lds[];
    const uint32_t S = sc.S;
    if (*bp.overflow) return; /* the records of this launch are incomplete: the bucket films stay as they are, as the main film does */
    if (SPDS_IN_LDS)
    {
        const uint32_t spd_words = sc.n_spd * S;
        for (uint32_t k = threadIdx.x; k < spd_words; k += BUCKET_BLOCK) lds[k] = sc.spds[k];
        __syncthreads();
    }
    const double *table = SPDS_IN_LDS ? (const double *)lds : sc.spds;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t vw = bp.vertex_words;
    /* the first sample's bucket and its number inside the bucket: the same for every work item (NB is a constant: no division) */
    const uint32_t b_first = bp.first_sample % (uint32_t)NB, j_first = bp.first_sample / (uint32_t)NB;

    for (;;)
    {
        /* the next (pixel, wavelength set): waves are persistent and draw from a counter, because pixel cost varies */
        uint32_t item = 0;
        if (lane == 0) item = (uint32_t)atomicAdd(work_counter, 1ull);
        item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= bp.n_items) break;
        const uint64_t pix = item / bp.n_sets;
        const uint32_t lam = 64u * (item - (uint32_t)pix * bp.n_sets) + lane;
        const bool active = lam < S;
        const uint32_t lam_c = active ? lam : 0; /* lanes past the table read row element 0 and are never stored */

        double f_sum[NB], f_avg[NB], f_var[NB];
        {
        const BucketParams &kc = bucket_const().bp;
#pragma unroll
        for (int c = 0; c < NB; c += 1)
        {
            f_sum[c] = active ? kc.pixels[c][pix * (uint64_t)(S + 1) + lam] : 0.0;
            f_avg[c] = active ? kc.avgs[c][pix * (uint64_t)S + lam] : 0.0;
            f_var[c] = active ? kc.vars[c][pix * (uint64_t)S + lam] : 0.0;
        }
        }
        uint32_t b = b_first, j = j_first; /* the running counters: m % NB and m / NB of the sample at hand */

        for (uint32_t s0 = 0; s0 < bp.n_samples; s0 += 64u)
        {
            /* the headers of a window of samples in one coalesced load, lane s <- sample s (as the shade kernel) */
            const uint32_t n_win = (uint32_t)__builtin_amdgcn_readfirstlane((int)((bp.n_samples - s0 < 64u) ? bp.n_samples - s0 : 64u));
            uint64_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;
            if (lane < n_win)
            {
                const uint64_t *h = headers + (pix * bp.batch + s0 + lane) * REC_HEADER_WORDS;
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
                const uint32_t n_replay = n_shaded < bp.max_depth ? n_shaded : bp.max_depth;

                double throughput = 1.0, dst = 0.0; /* :440 */
                uint64_t next = n_replay != 0u ? bucket_vertex_words(records, bp, hs2, hs3, 0u, lane) : 0;
                for (uint32_t v = 0; v < n_replay; v += 1)
                {
                    const uint64_t src = next;
                    if (v + 1u < n_replay) next = bucket_vertex_words(records, bp, hs2, hs3, v + 1u, lane); /* in flight while this one is replayed */
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
                    for (uint32_t l = 0; l < bp.n_lights; l += 1) /* direct_light_contribution, :272-332 */
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
                            const uint64_t *lp = path_vertex(records, bp.block_words, vw, hs2, hs3, v) + off;
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
                }
                double value = dst;
                /* the path ended in loop iteration n_shaded, on an emitter or on nothing (emissive black body hit, :452-457) */
                if (n_shaded < bp.max_depth && term == 1u) value = dst + throughput * spd_at(table, S, term_spd, lam_c);
                const double c_lam = value * vignette; /* :615 */

                /* the film update of the sample's own bucket, :732-743, with its number inside the bucket; b is a scalar, and each
                 * branch below a scalar one around the one update (and its one division) this sample runs */
                const double denom = (double)(j + 1u);
#pragma unroll
                for (int c = 0; c < NB; c += 1)
                    if (b == (uint32_t)c)
                    {
                        f_sum[c] = f_sum[c] + c_lam;
                        double t0 = c_lam - f_avg[c];
                        double t1 = t0;
                        t0 = t0 / denom;
                        f_avg[c] = f_avg[c] + t0;
                        t0 = c_lam - f_avg[c];
                        t0 = t1 * t0;
                        f_var[c] = f_var[c] + t0;
                    }
                b += 1u;
                if (b == (uint32_t)NB)
                {
                    b = 0u;
                    j += 1u;
                }
            }
        }
        const BucketParams &kc = bucket_const().bp;
#pragma unroll
        for (int c = 0; c < NB; c += 1)
        {
            if (active)
            {
                kc.pixels[c][pix * (uint64_t)(S + 1) + lam] = f_sum[c];
                kc.avgs[c][pix * (uint64_t)S + lam] = f_avg[c];
                kc.vars[c][pix * (uint64_t)S + lam] = f_var[c];
            }
            /* filter sum: += 1.0 per sample of this launch that fell into bucket c, :733 -- a small integer, exact */
            if (lam == 0u) kc.pixels[c][pix * (uint64_t)(S + 1) + S] += (double)bucket_share<NB>(b_first, bp.n_samples, (uint32_t)c) * 1.0;
        }
    }
}

/* [n_pix][S] -> [n_pix][S + 1] with a last column of 1.0: the layout drt_film_xyz_kernel reads, which divides by that column */
__global__ void drt_bucket_pack_kernel(uint64_t n_values, uint32_t S, const double *__restrict__ estimate, double *__restrict__ packed)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_values) return;
    const uint64_t p = i / (S + 1u);
    const uint32_t k = (uint32_t)(i - p * (S + 1u));
    packed[i] = k < S ? estimate[p * S + k] : 1.0;
}

/* The resolve: one thread per (pixel, wavelength), the NB means in registers, steps 1 to 4 of the rule with the network unrolled. */
struct BucketMeans { const double *avgs[DRT_MAX_BUCKETS]; };

template <int NB>
__global__ __launch_bounds__(256) void drt_bucket_resolve_kernel(uint64_t n_values, BucketMeans means, uint32_t trim, double *__restrict__ estimate,
                                                                 double *__restrict__ error)
{
    static_assert(NB >= 2 && NB <= DRT_MAX_BUCKETS, "the resolve needs two buckets");
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_values) return;
    double x[NB], y[NB];
#pragma unroll
    for (int b = 0; b < NB; b += 1) x[b] = means.avgs[b][i];
    /* 1. the mean, in bucket order */
    double mu = x[0];
#pragma unroll
    for (int b = 1; b < NB; b += 1) mu = mu + x[b];
    mu = mu / (double)NB;
    /* 2. the squared standard error of that mean across the buckets */
    double q = 0.0;
#pragma unroll
    for (int b = 0; b < NB; b += 1)
    {
        const double d = x[b] - mu;
        const double dd = d * d;
        q = b == 0 ? dd : q + dd;
    }
    error[i] = q / (double)(NB * (NB - 1));
    /* 3. odd-even transposition: NB rounds */
#pragma unroll
    for (int b = 0; b < NB; b += 1) y[b] = x[b];
#pragma unroll
    for (int r = 0; r < NB; r += 1)
    {
#pragma unroll
        for (int k = r % 2; k < NB - 1; k += 2)
        {
            const bool swap = y[k + 1] < y[k];
            const double lo = swap ? y[k + 1] : y[k], hi = swap ? y[k] : y[k + 1];
            y[k] = lo;
            y[k + 1] = hi;
        }
    }
    /* 4. the mean of y[trim .. NB - 1 - trim], summed in sorted order (trim is the same in every thread) */
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < NB; k += 1)
    {
        if ((uint32_t)k == trim) e = y[k];
        else if ((uint32_t)k > trim && (uint32_t)k + trim <= (uint32_t)(NB - 1)) e = e + y[k];
    }
    estimate[i] = e / (double)((uint32_t)NB - 2u * trim);
}
