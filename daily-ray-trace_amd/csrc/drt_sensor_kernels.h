/*
 * drt_sensor_kernels.h -- sensor films (drt_bind_sensor): beside the spectral film, the film of up to
 * DRT_MAX_SENSOR_CHANNELS channels, each the sample's spectrum weighted by a caller-given curve and summed, per sample -- so that the
 * channel has a running mean and a variance of its own, which the spectral film's per-wavelength variances cannot give.
 *
 * The rule (tests/sensor_rule.py restates it in numpy). For pixel p, sample m, contribution c[0..S) -- what the film update of
 * src/daily_ray_trace.c:732 takes, vignette included -- and curve R[k][0..S):
 *   1. per wavelength set j: q[i] = R[k][64 j + i] * c[64 j + i] where 64 j + i < S, +0.0 elsewhere (i = 0..63);
 *   2. six times q = q[0::2] + q[1::2]; t_j = q[0];
 *   3. v_k = t_0, then v_k = v_k + t_j for j = 1, 2, ... in order;
 *   4. v_k through the film update (:732-743) with the divisor (double)(m + 1).
 * Step 2 here is the butterfly x = x + x[lane ^ 1], ^ 2, ^ 4, ^ 8, ^ 16 and then lane 0 + lane 32: in lane 0 those are the pairs of
 * the rule (`+` is commutative), and nothing is contracted (-ffp-contract=off).
 *
 * The replay is drt_depth_cut_kernel's at full depth and nothing else: headers by windows of 64 samples, path_vertex, fresnel_rows,
 * spd_at and bdsf_at_wavelength<false> over the record's own list, the light block `((sum + 0) * em) * c`, light blocks beyond word
 * 64 by uniform loads, the emitter term when term == 1, times the vignette. None of the main pass's shortcuts are read.
 *
 * One wave per pixel, lane = wavelength 64 * set + lane; the wave walks its pixel's sets itself, one replay per (sample, set), so the
 * sum of step 3 stays inside the wave. The curves are in LDS behind the SPD table. After the reductions lane k (k < n) holds v_k and
 * channel k's sum, mean and variance: the film update of all channels is one instruction sequence with one division per sample, and
 * the sensor film is read and written once per launch.
 */
#pragma once

#include "drt_depth_kernels.h"

#define SENSOR_BLOCK 256
#define SENSOR_WAVES (SENSOR_BLOCK / 64)

struct SensorParams
{
    uint64_t n_pix;                  /* pixels of this launch: the films below start at its first pixel; one work item each */
    uint32_t n_samples, first_sample, vertex_words, block_words;
    uint32_t n_lights, batch;        /* batch: sample slots per pixel in the header array */
    const uint32_t *overflow;        /* the trace launch ran out of record blocks: nothing here is touched */
    uint32_t n_sets, max_depth;      /* wavelength sets per pixel (ceil(S / 64)); the render's max_depth */
    uint32_t n_channels, n_items;    /* work items: one per pixel, n_pix in the 32 bits of the work counter's draw */
    const double *curves;            /* [n_channels][S] */
    double  *pixels;                 /* [n_pix][n_channels + 1] sum + filter */
    double  *avgs;                   /* [n_pix][n_channels] */
    double  *vars;                   /* [n_pix][n_channels] */
};

/* the first 64 words (or all, when it has fewer) of vertex v's record, word `lane` in lane `lane` (as depth_vertex_words) */
__device__ __forceinline__ uint64_t sensor_vertex_words(const uint64_t *__restrict__ records, const SensorParams &np, uint64_t h2, uint64_t h3, uint32_t v,
                                                        uint32_t lane)
{
    return lane < np.vertex_words ? path_vertex(records, np.block_words, np.vertex_words, h2, h3, v)[lane] : 0;
}

/* x[lane] + x[lane ^ mask], mask < 32, through ds_swizzle's bit mode: no address register */
template <int MASK>
__device__ __forceinline__ double sensor_add_xor(double x)
{
    const uint64_t w = (uint64_t)__double_as_longlong(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)w, (MASK << 10) | 0x1F);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)(w >> 32), (MASK << 10) | 0x1F);
    return x + __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

/* step 2 of the rule over the wave's 64 values; every lane returns what the rule's q[0] is */
__device__ __forceinline__ double sensor_tree_sum(double q)
{
    q = sensor_add_xor<1>(q);
    q = sensor_add_xor<2>(q);
    q = sensor_add_xor<4>(q);
    q = sensor_add_xor<8>(q);
    q = sensor_add_xor<16>(q);
    const uint64_t w = (uint64_t)__double_as_longlong(q);
    return word_as_double(readlane64(w, 0)) + word_as_double(readlane64(w, 32));
}

template <bool SPDS_IN_LDS>
__global__ __launch_bounds__(SENSOR_BLOCK) void drt_sensor_kernel(DevScene sc, SensorParams np, const uint64_t *__restrict__ records,
                                                                  const uint64_t *__restrict__ headers, unsigned long long *__restrict__ work_counter)
{
    extern __shared__ double lds[];
    const uint32_t S = sc.S;
    if (*np.overflow) return; /* the records of this launch are incomplete: the sensor film stays as it is, as the main film does */
    const uint32_t spd_words = SPDS_IN_LDS ? sc.n_spd * S : 0u;
    const uint32_t curve_words = np.n_channels * S;
    if (SPDS_IN_LDS)
        for (uint32_t k = threadIdx.x; k < spd_words; k += SENSOR_BLOCK) lds[k] = sc.spds[k];
    for (uint32_t k = threadIdx.x; k < curve_words; k += SENSOR_BLOCK) lds[spd_words + k] = np.curves[k];
    __syncthreads();
    const double *table = SPDS_IN_LDS ? (const double *)lds : sc.spds;
    const double *curves = lds + spd_words;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t vw = np.vertex_words;
    const uint32_t n = np.n_channels;

    for (;;)
    {
        /* the next pixel: waves are persistent and draw from a counter, because pixel cost varies */
        uint32_t item = 0;
        if (lane == 0) item = (uint32_t)atomicAdd(work_counter, 1ull);
        item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= np.n_items) break;
        const uint64_t pix = item;
        const bool channel = lane < n; /* lane k holds channel k */

        double f_sum = channel ? np.pixels[pix * (uint64_t)(n + 1) + lane] : 0.0;
        double f_avg = channel ? np.avgs[pix * (uint64_t)n + lane] : 0.0;
        double f_var = channel ? np.vars[pix * (uint64_t)n + lane] : 0.0;

        for (uint32_t s0 = 0; s0 < np.n_samples; s0 += 64u)
        {
            /* the headers of a window of samples in one coalesced load, lane s <- sample s (as the shade kernel) */
            const uint32_t n_win = (uint32_t)__builtin_amdgcn_readfirstlane((int)((np.n_samples - s0 < 64u) ? np.n_samples - s0 : 64u));
            uint64_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;
            if (lane < n_win)
            {
                const uint64_t *h = headers + (pix * np.batch + s0 + lane) * REC_HEADER_WORDS;
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
                const uint32_t n_replay = n_shaded < np.max_depth ? n_shaded : np.max_depth;
                const double denom = (double)(np.first_sample + s0 + s + 1);

                double v_k = 0.0; /* lane k: channel k's value of this sample */
                for (uint32_t set = 0; set < np.n_sets; set += 1)
                {
                    const uint32_t lam = 64u * set + lane;
                    const bool active = lam < S;
                    const uint32_t lam_c = active ? lam : 0; /* lanes past the table read row element 0 and weigh nothing */

                    double throughput = 1.0, dst = 0.0; /* :440 */
                    uint64_t next = n_replay != 0u ? sensor_vertex_words(records, np, hs2, hs3, 0u, lane) : 0;
                    for (uint32_t v = 0; v < n_replay; v += 1)
                    {
                        const uint64_t src = next;
                        if (v + 1u < n_replay) next = sensor_vertex_words(records, np, hs2, hs3, v + 1u, lane); /* in flight while this one is replayed */
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
                        for (uint32_t l = 0; l < np.n_lights; l += 1) /* direct_light_contribution, :272-332 */
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
                                const uint64_t *lp = path_vertex(records, np.block_words, vw, hs2, hs3, v) + off;
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
                    if (n_shaded < np.max_depth && term == 1u) value = dst + throughput * spd_at(table, S, term_spd, lam_c);
                    const double c_lam = value * vignette; /* :615 */

                    /* steps 1 to 3 of the rule, channel by channel; lane k keeps channel k's */
                    for (uint32_t k = 0; k < n; k += 1)
                    {
                        const double q = active ? curves[k * S + lam_c] * c_lam : 0.0;
                        const double t = sensor_tree_sum(q);
                        if (lane == k) v_k = set == 0u ? t : v_k + t;
                    }
                }
                /* step 4: the film update with this sample's channel values, :732-743 */
                f_sum = f_sum + v_k;
                double t0 = v_k - f_avg;
                double t1 = t0;
                t0 = t0 / denom;
                f_avg = f_avg + t0;
                t0 = v_k - f_avg;
                t0 = t1 * t0;
                f_var = f_var + t0;
            }
        }
        if (channel)
        {
            np.pixels[pix * (uint64_t)(n + 1) + lane] = f_sum;
            np.avgs[pix * (uint64_t)n + lane] = f_avg;
            np.vars[pix * (uint64_t)n + lane] = f_var;
        }
        /* filter sum: += 1.0 per sample, :733 -- by lane n, the column's own. (Not lane 0: under the condition of the work draw above
         * the compiler joins this block to the draw and sends the other lanes round the loop without it, which never ends.) */
        if (lane == n) np.pixels[pix * (uint64_t)(n + 1) + n] += (double)np.n_samples * 1.0;
    }
}

/*
 * Sensor film -> BMP pixel bytes: the channels (which 0: sum / filter, 1: running mean) through the caller's 3 x n matrix to R, G, B
 * -- row r: m[r][0] * v_0, then + m[r][k] * v_k for k = 1, 2, ... in order -- and from there as drt_film_bgra_kernel behind its own
 * matrix: clamp to [0, 1], x 255, truncate, a NaN to 0; stored B, G, R, 255.
 */
struct SensorMatrix { double m[3][DRT_MAX_SENSOR_CHANNELS]; };

__global__ void drt_sensor_bgra_kernel(uint64_t n_pix, uint32_t n, const double *__restrict__ film, int which, SensorMatrix mat, uint8_t *__restrict__ bgra)
{
    uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    const double *px = film + p * (uint64_t)(which == 0 ? n + 1 : n);
    uint8_t out[3];
    for (int r = 0; r < 3; r += 1)
    {
        double f = 0.0;
        for (uint32_t k = 0; k < n; k += 1)
        {
            const double v = which == 0 ? px[k] / px[n] : px[k];
            const double t = mat.m[r][k] * v;
            f = k == 0 ? t : f + t;
        }
        f = (f < 0.0) ? 0.0 : f;
        f = (f > 1.0) ? 1.0 : f;
        out[r] = (f == f) ? (uint8_t)(f * 255.0) : (uint8_t)0;
    }
    uchar4 o;
    o.x = out[2];
    o.y = out[1];
    o.z = out[0];
    o.w = 255;
    ((uchar4 *)bgra)[p] = o;
}
