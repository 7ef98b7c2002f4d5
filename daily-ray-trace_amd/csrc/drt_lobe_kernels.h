/*
 * drt_lobe_kernels.h -- lobe films (drt_bind_lobes): beside the film of a render, n films that split it by what
 * the first surface did with the light -- by the entry of vertex 0's own BDSF list whose addend carries the light, direct and
 * indirect apart -- and by emission seen by the camera ray itself.
 *
 * The rule (`+ - *` and the film update's `/`, nothing contracted; include/drt_hip.h states it in full). For one sample, with f_i the
 * i-th entry of vertex 0's list and a_i(args) the dispatcher's bdsf_result after entry i (the function's value, or the value carried
 * over from the entry before when its direction test fails -- Q1 -- or 0.0 when nothing came before):
 *   R^c_K(args) = 0.0, then R = a_i + R over the positions i with K[f_i] == c, in list order (K: the map's direct or indirect row);
 *   C^c = 0.0, then per visible light l in order: C = C + R^c_direct(light l); C = C * em_l; C = C * c_l -- for every film;
 *   vertex 0:      dst^c = 0.0 + 1.0 * C^c;  T^c = 1.0 * (R^c_indirect(sample) * dir_pdf);
 *   vertex v >= 1: C_v and R_v are the bucket kernel's, shared by the films; dst^c = dst^c + T^c * C_v;  T^c = T^c * (R_v * dir_pdf_v);
 *   the end, with n_shaded < max_depth && term == 1: n_shaded >= 1: value^c = dst^c + T^c * spd(term_spd) for every film;
 *                                                    n_shaded == 0: value = 0.0 + 1.0 * spd(term_spd) for film `emission`, 0.0 for the others;
 *   value^c * vignette goes through the film update (:732-743) of film c with the sample's own number + 1 as the divisor; every film
 *   takes every sample, zeros included, and its filter column += 1.0.
 * A map that sends all 15 entries to film 0 makes film 0 the main film, bit for bit: R^0 is then the dispatcher's own sum.
 *
 * drt_lobe_kernel's replay is drt_bucket_kernel's with another sink: one wave per (pixel, wavelength set), lane = wavelength, persistent
 * waves that draw work items from a counter, headers by windows of 64 samples, path_vertex, fresnel_rows, spd_at, light blocks beyond
 * word 64 by uniform loads, an immediate return when the trace launch ran out of records. Vertices behind the first go through
 * bdsf_at_wavelength<false> as they do there. Vertex 0 needs the addends one by one: lobe_addends below is the dispatcher's loop with
 * the sum routed -- the same *_sel helpers, the same pins, the same carry-over.
 *
 * The film of a list position is the same in every lane (the list comes from the record by v_readlane, the map from the kernel's
 * arguments), so routing is scalar branches over c = 0 .. NF - 1, unrolled: the NF accumulator triples and the NF (dst, T) pairs are
 * registers by name and nothing indexes them at run time. During vertex 0, dst^c holds C^c and T^c holds R^c_indirect. Each sample runs
 * NF film updates, so NF divisions by one divisor, in the plain form: a shared reciprocal after v_div_shared was bit-exact and measured
 * slower, as was one walker for every vertex in bdsf_at_wavelength's place (DESIGN.md 5n has both figures).
 */
#pragma once

#include "drt_depth_kernels.h"

#define LOBE_BLOCK 256
#define LOBE_WAVES (LOBE_BLOCK / 64)

struct LobeParams
{
    uint64_t n_pix;                  /* pixels of this launch: the films below start at its first pixel */
    uint32_t n_samples, first_sample, vertex_words, block_words;
    uint32_t n_lights, batch;        /* batch: sample slots per pixel in the header array */
    const uint32_t *overflow;        /* the trace launch ran out of record blocks: nothing here is touched */
    uint32_t n_sets, n_items;        /* wavelength sets per pixel (ceil(S / 64)); work items: n_pix * n_sets */
    uint32_t max_depth, emission;    /* the render's max_depth; the map's emission film */
    uint64_t direct, indirect;       /* the map's two rows: byte f is the film of function f (DRT_LOBE_NONE: none) */
    double  *pixels[DRT_MAX_LOBE_FILMS];       /* per film: [n_pix][S + 1] sum + filter; the first NF count */
    double  *avgs[DRT_MAX_LOBE_FILMS];         /* [n_pix][S] */
    double  *vars[DRT_MAX_LOBE_FILMS];         /* [n_pix][S] */
};

/* The kernel's argument list, in its order (as BucketConst): the 24 film pointers are read from the kernarg segment where a work item
 * starts and ends -- scalar loads -- instead of living in scalar registers across the sample loop. */
struct LobeConst
{
    DevScene       sc;
    LobeParams     lp;
    const uint64_t *records, *headers;
    unsigned long long *work_counter;
};
static_assert(sizeof(DevScene) % 8 == 0 && sizeof(LobeParams) % 8 == 0, "LobeConst mirrors the kernarg segment only while every argument ends on an 8-byte boundary");
__device__ __forceinline__ const LobeConst &lobe_const()
{
    uint32_t off = 0;
    asm volatile("" : "+s"(off));
    return *(const LobeConst *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + off);
}

/* the first 64 words (or all, when it has fewer) of vertex v's record, word `lane` in lane `lane` (as depth_vertex_words) */
__device__ __forceinline__ uint64_t lobe_vertex_words(const uint64_t *__restrict__ records, const LobeParams &lp, uint64_t h2, uint64_t h3, uint32_t v,
                                                      uint32_t lane)
{
    return lane < lp.vertex_words ? path_vertex(records, lp.block_words, lp.vertex_words, h2, h3, v)[lane] : 0;
}

/* The addend walker: bdsf_at_wavelength<false>'s loop (drt_kernels.h) with `reflectance = bdsf_result + reflectance` routed -- entry i's
 * addend goes to R[c] for the one c that is the film of its function in `row`, or nowhere. `row` and `list` are wave-uniform. With
 * every byte of `row` equal to c, R[c] is bdsf_at_wavelength's return value, bit for bit (tests/test_gpu_lobes.py holds it there). */
template <int NF>
__device__ __forceinline__ void lobe_addends(double (&R)[NF], uint64_t row, uint64_t list, uint32_t num_bdsfs, double diffuse_pi, double glossy, double mirror,
                                             double ir, double tr, double te, double on_dot, double a_in, double spec, double mn_dot, double ct_coef,
                                             uint32_t flags, bool paired)
{
    double bdsf_result = 0.0;
/* as in bdsf_at_wavelength: the empty asm ties each Fresnel term to its `case` */
#define DRT_PIN_HERE(x) asm volatile("" : "+v"(x))
    for (uint32_t i = 0; i < num_bdsfs; i += 1)
    {
        const uint32_t f = (uint32_t)(list >> (4 * i)) & 15u;
        switch (f)
        {
            case DRT_BDSF_bp_diffuse_bdsf: /* src/bdsf.c:105-109 */
                bdsf_result = diffuse_pi * a_in;
                break;
            case DRT_BDSF_bp_glossy_bdsf: /* :111-119 */
                bdsf_result = (glossy * spec) * a_in;
                break;
            case DRT_BDSF_mirror_bdsf: /* :121-132 */
                bdsf_result = (flags & FLAG_EQR) ? mirror : 0.0;
                break;
            case DRT_BDSF_fs_conductor_bdsf: /* :134-146 */
                if (flags & FLAG_EQR)
                {
                    DRT_PIN_HERE(ir);
                    double c2 = on_dot * on_dot;
                    bdsf_result = conductor_reflectance_sel(paired, ir, tr, te, on_dot, c2, 1.0 - c2);
                }
                break;
            case DRT_BDSF_fs_dielectric_reflectance_bdsf: /* :148-159 */
                if (flags & FLAG_EQR)
                {
                    DRT_PIN_HERE(ir);
                    bdsf_result = dielectric_reflectance_sel(paired, ir, tr, te, on_dot, 1.0 - on_dot * on_dot);
                }
                break;
            case DRT_BDSF_fs_dielectric_transmittance_bdsf: /* :161-172, :69-76 */
                if (flags & FLAG_EQT)
                {
                    DRT_PIN_HERE(ir);
                    bdsf_result = 1.0 - dielectric_reflectance_sel(paired, ir, tr, te, on_dot, 1.0 - on_dot * on_dot);
                }
                break;
            case DRT_BDSF_ct_conductor_bdsf: /* :174-186 */
            {
                DRT_PIN_HERE(ir);
                double c2 = mn_dot * mn_dot;
                bdsf_result = conductor_reflectance_sel(paired, ir, tr, te, mn_dot, c2, 1.0 - c2) * ct_coef;
                break;
            }
            default: break;
        }
        /* the film of this position: a scalar, and each branch below a scalar one around the one sum this addend joins */
        /* (a nibble that names no function cannot occur: build_device_scene refuses such a list when the context is created, and material
         * updates keep the lists. The guard only keeps the shift in range; bdsf_at_wavelength's `default:` would sum the carried value.) */
        const uint32_t film = f < (uint32_t)DRT_NUM_BDSFS ? (uint32_t)(row >> (8u * f)) & 0xFFu : (uint32_t)DRT_LOBE_NONE;
#pragma unroll
        for (int c = 0; c < NF; c += 1)
            if (film == (uint32_t)c) R[c] = bdsf_result + R[c];
    }
#undef DRT_PIN_HERE
}

template <int NF, bool SPDS_IN_LDS>
__global__ __launch_bounds__(LOBE_BLOCK) void drt_lobe_kernel(DevScene sc, LobeParams lp, const uint64_t *__restrict__ records,
                                                              const uint64_t *__restrict__ headers, unsigned long long *__restrict__ work_counter)
{
    static_assert(NF >= 1 && NF <= DRT_MAX_LOBE_FILMS, "one instantiation per film count");
    extern __shared__ double lds[];
    const uint32_t S = sc.S;
    if (*lp.overflow) return; /* the records of this launch are incomplete: the lobe films stay as they are, as the main film does */
    if (SPDS_IN_LDS)
    {
        const uint32_t spd_words = sc.n_spd * S;
        for (uint32_t k = threadIdx.x; k < spd_words; k += LOBE_BLOCK) lds[k] = sc.spds[k];
        __syncthreads();
    }
    const double *table = SPDS_IN_LDS ? (const double *)lds : sc.spds;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t vw = lp.vertex_words;

    for (;;)
    {
        /* the next (pixel, wavelength set): waves are persistent and draw from a counter, because pixel cost varies */
        uint32_t item = 0;
        if (lane == 0) item = (uint32_t)atomicAdd(work_counter, 1ull);
        item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= lp.n_items) break;
        const uint64_t pix = item / lp.n_sets;
        const uint32_t lam = 64u * (item - (uint32_t)pix * lp.n_sets) + lane;
        const bool active = lam < S;
        const uint32_t lam_c = active ? lam : 0; /* lanes past the table read row element 0 and are never stored */

        double f_sum[NF], f_avg[NF], f_var[NF];
        {
        const LobeParams &kc = lobe_const().lp;
#pragma unroll
        for (int c = 0; c < NF; c += 1)
        {
            f_sum[c] = active ? kc.pixels[c][pix * (uint64_t)(S + 1) + lam] : 0.0;
            f_avg[c] = active ? kc.avgs[c][pix * (uint64_t)S + lam] : 0.0;
            f_var[c] = active ? kc.vars[c][pix * (uint64_t)S + lam] : 0.0;
        }
        }

        for (uint32_t s0 = 0; s0 < lp.n_samples; s0 += 64u)
        {
            /* the headers of a window of samples in one coalesced load, lane s <- sample s (as the shade kernel) */
            const uint32_t n_win = (uint32_t)__builtin_amdgcn_readfirstlane((int)((lp.n_samples - s0 < 64u) ? lp.n_samples - s0 : 64u));
            uint64_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;
            if (lane < n_win)
            {
                const uint64_t *h = headers + (pix * lp.batch + s0 + lane) * REC_HEADER_WORDS;
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
                const uint32_t n_replay = n_shaded < lp.max_depth ? n_shaded : lp.max_depth;

                double T[NF], dst[NF]; /* per film: the throughput and the radiance so far (:440); in vertex 0, R^c_indirect and C^c */
#pragma unroll
                for (int c = 0; c < NF; c += 1) T[c] = dst[c] = 0.0;
                uint64_t next = n_replay != 0u ? lobe_vertex_words(records, lp, hs2, hs3, 0u, lane) : 0;
                for (uint32_t v = 0; v < n_replay; v += 1)
                {
                    const uint64_t src = next;
                    if (v + 1u < n_replay) next = lobe_vertex_words(records, lp, hs2, hs3, v + 1u, lane); /* in flight while this one is replayed */
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
                    double contribution = 0.0; /* vertices behind the first: C_v, shared by the films */
                    for (uint32_t l = 0; l < lp.n_lights; l += 1) /* direct_light_contribution, :272-332 */
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
                            const uint64_t *lptr = path_vertex(records, lp.block_words, vw, hs2, hs3, v) + off;
#pragma unroll
                            for (int k = 0; k < REC_LIGHT_WORDS; k += 1) lw[k] = readlane64(lptr[k], 0);
                        }
                        const uint32_t lflags = (uint32_t)(lw[0] >> 16) & 0xFFu;
                        if (!(lflags & FLAG_VISIBLE)) continue;
                        const uint32_t i_em = (uint32_t)(lw[0] & 0xFFFFu);
                        const double em = spd_at(table, S, i_em, lam_c);
                        const double c_l = word_as_double(lw[1]);
                        if (v == 0u)
                        {
                            /* the light fold per film, :323-327, each with the sum of its own addends; dst^c is C^c here */
                            double R[NF];
#pragma unroll
                            for (int c = 0; c < NF; c += 1) R[c] = 0.0;
                            lobe_addends<NF>(R, lp.direct, list, num_bdsfs, diffuse, glossy, mirror, ir, tr, te, on_dot, word_as_double(lw[2]),
                                             word_as_double(lw[3]), word_as_double(lw[4]), word_as_double(lw[5]), lflags, paired);
#pragma unroll
                            for (int c = 0; c < NF; c += 1)
                            {
                                dst[c] = dst[c] + R[c];
                                dst[c] = dst[c] * em;
                                dst[c] = dst[c] * c_l;
                            }
                        }
                        else
                        {
                            double reflectance = bdsf_at_wavelength<false>(list, num_bdsfs, diffuse, glossy, mirror, ir, tr, te, on_dot, word_as_double(lw[2]),
                                                                           word_as_double(lw[3]), word_as_double(lw[4]), word_as_double(lw[5]), lflags, paired);
                            contribution = contribution + reflectance; /* :323 */
                            contribution = contribution * em;          /* :324 */
                            contribution = contribution * c_l;         /* :326-327 */
                        }
                    }
                    const double s_a_in = word_as_double(readlane64(src, 5)), s_spec = word_as_double(readlane64(src, 6));
                    const double s_mn = word_as_double(readlane64(src, 7)), s_ct = word_as_double(readlane64(src, 8));
                    if (v == 0u)
                    {
                        /* T^c is 0.0 here: it takes the sum of film c's addends for the sampled direction, then :468-469 with throughput 1.0 */
                        lobe_addends<NF>(T, lp.indirect, list, num_bdsfs, diffuse, glossy, mirror, ir, tr, te, on_dot, s_a_in, s_spec, s_mn, s_ct, sflags,
                                         paired);
#pragma unroll
                        for (int c = 0; c < NF; c += 1)
                        {
                            dst[c] = 0.0 + 1.0 * dst[c]; /* :461-462 */
                            T[c] = 1.0 * (T[c] * dir_pdf);
                        }
                    }
                    else
                    {
                        double reflectance = bdsf_at_wavelength<false>(list, num_bdsfs, diffuse, glossy, mirror, ir, tr, te, on_dot, s_a_in, s_spec, s_mn, s_ct,
                                                                       sflags, paired);
                        reflectance = reflectance * dir_pdf; /* :468 */
#pragma unroll
                        for (int c = 0; c < NF; c += 1)
                        {
                            dst[c] = dst[c] + T[c] * contribution; /* :461-462 */
                            T[c] = T[c] * reflectance;             /* :469 */
                        }
                    }
                }
                /* the path ended in loop iteration n_shaded, on an emitter or on nothing (emissive black body hit, :452-457) */
                const bool emitter = n_shaded < lp.max_depth && term == 1u;
                const double e_spd = emitter ? spd_at(table, S, term_spd, lam_c) : 0.0;
                /* the film update of every film, :732-743, with the sample's own number: one divisor, NF divisions */
                const double denom = (double)(lp.first_sample + s0 + s + 1u);
#pragma unroll
                for (int c = 0; c < NF; c += 1)
                {
                    double value = dst[c];
                    if (emitter)
                    {
                        if (n_shaded != 0u) value = dst[c] + T[c] * e_spd;
                        else if (lp.emission == (uint32_t)c) value = 0.0 + 1.0 * e_spd; /* the camera ray's own emitter: no vertex, one film */
                    }
                    const double c_lam = value * vignette; /* :615 */
                    f_sum[c] = f_sum[c] + c_lam;
                    double t0 = c_lam - f_avg[c];
                    double t1 = t0;
                    t0 = t0 / denom;
                    f_avg[c] = f_avg[c] + t0;
                    t0 = c_lam - f_avg[c];
                    t0 = t1 * t0;
                    f_var[c] = f_var[c] + t0;
                }
            }
        }
        const LobeParams &kc = lobe_const().lp;
#pragma unroll
        for (int c = 0; c < NF; c += 1)
        {
            if (active)
            {
                kc.pixels[c][pix * (uint64_t)(S + 1) + lam] = f_sum[c];
                kc.avgs[c][pix * (uint64_t)S + lam] = f_avg[c];
                kc.vars[c][pix * (uint64_t)S + lam] = f_var[c];
            }
            /* filter sum: += 1.0 per sample of this launch, :733 -- a small integer, exact */
            if (lam == 0u) kc.pixels[c][pix * (uint64_t)(S + 1) + S] += (double)lp.n_samples * 1.0;
        }
    }
}
