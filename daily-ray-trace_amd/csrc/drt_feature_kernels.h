/*
 * drt_feature_kernels.h -- the first-hit feature buffers (drt_render_features): per tile pixel the running mean and the sum of squared
 * deviations of DRT_FEATURE_CHANNELS numbers of its samples' first hits -- normal, depth, coverage, albedo -- and the surface its
 * first sample sees. DESIGN.md, section 5c, states the rule; tests/feature_rule.py restates it, and these kernels are held to that
 * bit for bit: only + - * / sqrt, every sum sequential in the rule's order, no contraction.
 *
 * One lane per tile pixel, its samples in ascending order: the pixel passes of drt_first_hit.h, which own the loop, the camera ray
 * (the path's own: path_key, camera_ray, the same draws in the same order) and the closest hit (the trace stage's own scans).
 * FeatureAcc is what a lane keeps of them.
 *
 *   drt_feature_kernel         scenes in LDS
 *   drt_feature_bvh_kernel     scenes behind the hierarchy
 *   drt_feature_counts_kernel  n_samples = 0: every pixel's count from the film's filter column, and the first pixel that holds none.
 *   drt_feature_bgra_kernel    mean normal / depth / coverage as .bmp pixel bytes.
 */
#pragma once

#include "drt_first_hit.h"

#define FEATURE_BLOCK 256
#define FEATURE_INFO_WORDS 2 /* d_ft_info, 8-byte words: pixels whose coverage is 0, rays */

/* a lane's running moments, and the surface its first sample sees */
struct FeatureAcc
{
    const FeatureParams &fp;
    const DevCamera &cam;
    double m[DRT_FEATURE_CHANNELS], M2[DRT_FEATURE_CHANNELS];
    int first_id;

    __device__ __forceinline__ FeatureAcc(const FeatureParams &fp_, const DevCamera &cam_) : fp(fp_), cam(cam_) {}

    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int c = 0; c < DRT_FEATURE_CHANNELS; c += 1) m[c] = M2[c] = 0.0;
        first_id = -1;
    }

    /* the feature vector of a first hit, and the film's update with it (reference render_image, lines 736-743); k samples came before */
    __device__ __forceinline__ void add(const HitPoint &ip, uint32_t k)
    {
        if (k == 0) first_id = ip.index;
        const bool hit = ip.index >= 0;
        double phi[DRT_FEATURE_CHANNELS];
        const V3 d = v_sub(ip.position, cam.aperture_position);
        phi[0] = hit ? ip.normal.x : 0.0;
        phi[1] = hit ? ip.normal.y : 0.0;
        phi[2] = hit ? ip.normal.z : 0.0;
        phi[3] = hit ? d.x * cam.forward.x + d.y * cam.forward.y + d.z * cam.forward.z : 0.0;
        phi[4] = hit ? 1.0 : 0.0;
        const double *c = fp.colour + (size_t)ip.surface_mat * 3u; /* a miss: the escape material */
        phi[5] = c[0];
        phi[6] = c[1];
        phi[7] = c[2];
        const double n = (double)(k + 1u);
#pragma unroll
        for (int j = 0; j < DRT_FEATURE_CHANNELS; j += 1)
        {
            const double dd = phi[j] - m[j];
            m[j] = m[j] + dd / n;
            M2[j] = M2[j] + dd * (phi[j] - m[j]);
        }
    }

    /* the lane's results, and the launch's two sums: one atomic per word and wave */
    __device__ __forceinline__ void store(uint64_t p, bool valid, uint32_t count)
    {
        if (valid)
        {
            double *mean = fp.mean + (size_t)p * DRT_FEATURE_CHANNELS, *m2 = fp.m2 + (size_t)p * DRT_FEATURE_CHANNELS;
#pragma unroll
            for (int j = 0; j < DRT_FEATURE_CHANNELS; j += 1)
            {
                mean[j] = m[j];
                m2[j] = M2[j];
            }
            fp.ids[p] = first_id;
        }
        const unsigned long long empty = __ballot(valid && m[4] == 0.0);
        uint64_t rays = valid ? count : 0u;
        for (int off = 32; off > 0; off >>= 1) rays += __shfl_down(rays, off);
        if ((threadIdx.x & 63u) == 0)
        {
            if (empty) atomicAdd(fp.info, (unsigned long long)__popcll(empty));
            if (rays) atomicAdd(fp.info + 1, (unsigned long long)rays);
        }
    }
};

__global__ __launch_bounds__(FEATURE_BLOCK) void drt_feature_kernel(DevScene sc, DevCamera cam, FeatureParams fp)
{
    extern __shared__ double ft_lds[];
    FeatureAcc a(fp, cam);
    a.clear();
    const PixelLane px = first_hit_pixels_lds<FEATURE_BLOCK>(sc, cam, fp, ft_lds, [&](const HitPoint &ip, uint32_t k) { a.add(ip, k); });
    a.store(px.p, px.valid, px.count);
}

__global__ __launch_bounds__(FEATURE_BLOCK) void drt_feature_bvh_kernel(DevScene sc, DevCamera cam, FeatureParams fp)
{
    FeatureAcc a(fp, cam);
    a.clear();
    FIRST_HIT_PIXELS_BVH(FEATURE_BLOCK, sc, cam, fp, px, a)
    a.store(px.p, px.valid, px.count);
}

/* report[0]: the first tile pixel whose filter sum is no count (a whole number in [1, 2^32)), report[1]: the largest count.
 * One atomic per word and wave. */
__global__ __launch_bounds__(FEATURE_BLOCK) void drt_feature_counts_kernel(const double *__restrict__ pixels, uint32_t S, uint32_t n_pix,
                                                                           uint32_t *__restrict__ counts, uint32_t *report)
{
    const uint64_t p = (uint64_t)blockIdx.x * FEATURE_BLOCK + threadIdx.x;
    const bool valid = p < n_pix;
    const double f = valid ? pixels[(size_t)p * (S + 1) + S] : 1.0;
    const bool ok = f >= 1.0 && f < 4294967296.0 && f == __builtin_floor(f); /* a NaN fails the first comparison */
    uint32_t c = (valid && ok) ? (uint32_t)f : 0u;
    if (valid) counts[p] = c;
    const unsigned long long bad = __ballot(valid && !ok);
    for (int off = 32; off > 0; off >>= 1)
    {
        const uint32_t c2 = (uint32_t)__shfl_xor((int)c, off);
        c = c2 > c ? c2 : c;
    }
    if ((threadIdx.x & 63u) == 0)
    {
        if (bad) atomicMin(report, (uint32_t)(p + (uint32_t)__builtin_ctzll(bad)));
        atomicMax(report + 1, c);
    }
}

/* which: 0 the mean normal (x, y, z to R, G, B), 1 depth, 2 coverage (grey). t = (v - lo) / (hi - lo) clamped to [0, 1],
 * byte = (uint8_t)(t * 255.0 + 0.5); a NaN gives 0; alpha 255 */
__device__ __forceinline__ uint8_t feature_byte(double v, double lo, double hi)
{
    double t = (v - lo) / (hi - lo);
    t = t < 0.0 ? 0.0 : t;
    t = t > 1.0 ? 1.0 : t;
    return t == t ? (uint8_t)(t * 255.0 + 0.5) : (uint8_t)0;
}
__global__ __launch_bounds__(FEATURE_BLOCK) void drt_feature_bgra_kernel(const double *__restrict__ mean, uint64_t n_pix, int which, double lo, double hi,
                                                                         uint8_t *__restrict__ bgra)
{
    const uint64_t p = (uint64_t)blockIdx.x * FEATURE_BLOCK + threadIdx.x;
    if (p >= n_pix) return;
    const double *m = mean + (size_t)p * DRT_FEATURE_CHANNELS;
    uint8_t r, g, b;
    if (which == 0)
    {
        r = feature_byte(m[0], lo, hi);
        g = feature_byte(m[1], lo, hi);
        b = feature_byte(m[2], lo, hi);
    }
    else r = g = b = feature_byte(m[which == 1 ? 3 : 4], lo, hi);
    bgra[p * 4 + 0] = b;
    bgra[p * 4 + 1] = g;
    bgra[p * 4 + 2] = r;
    bgra[p * 4 + 3] = 255;
}
