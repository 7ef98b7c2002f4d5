/*
 * drt_feature_kernels.h -- the first-hit feature buffers (drt_render_features): per tile pixel the running mean and the sum of squared
 * deviations of DRT_FEATURE_CHANNELS numbers of its samples' first hits -- normal, depth, coverage, albedo -- and the surface its
 * first sample sees. DESIGN.md, section 5c, states the rule; tests/feature_rule.py restates it, and these kernels are held to that
 * bit for bit: only + - * / sqrt, every sum sequential in the rule's order, no contraction.
 *
 * One lane per tile pixel; the lane loops over its own samples in ascending order, because the running update is sequential per
 * pixel. A sample's camera ray is the path's own (path_key, camera_ray: the same draws in the same order), its closest hit the trace
 * stage's own: find_ray_intersection<true> over surface rows staged in LDS as drt_trace_kernel stages them, or, for a scene behind
 * the hierarchy, one bvh_walk per lane and hit_point_from_scan, as drt_bounce_kernel takes a continuation ray.
 *
 *   drt_feature_kernel         scenes in LDS. Lanes of a wave may hold different counts: a lane that is done waits for the others.
 *   drt_feature_bvh_kernel     scenes behind the hierarchy. bvh_walk is a whole-wave function: a lane that is done walks with JOB_NONE.
 *   drt_feature_counts_kernel  n_samples = 0: every pixel's count from the film's filter column, and the first pixel that holds none.
 *   drt_feature_bgra_kernel    mean normal / depth / coverage as .bmp pixel bytes.
 */
#pragma once

#include "drt_bvh_kernels.h"

#define FEATURE_BLOCK 256
#define FEATURE_INFO_WORDS 2 /* d_ft_info, 8-byte words: pixels whose coverage is 0, rays */

struct FeatureParams
{
    uint32_t width, height, x0, y0, tile_w, tile_h, row_stride;
    uint32_t n_samples, first_sample, pixel_scheme;
    uint64_t seed, n_pix;
    const uint32_t *counts; /* [n_pix] samples per pixel; NULL: n_samples of every pixel */
    const double   *colour; /* [n_mat][3]: a material's XYZ (the launcher's feature_colour_table) */
    double   *mean, *m2;    /* [n_pix][DRT_FEATURE_CHANNELS] */
    int32_t  *ids;          /* [n_pix] closest-hit index of the first sample */
    unsigned long long *info; /* FEATURE_INFO_WORDS */
};

struct FeatureAcc
{
    double m[DRT_FEATURE_CHANNELS], M2[DRT_FEATURE_CHANNELS];
};

/* tile pixel p's image coordinates, and the camera ray of its sample: the `started` block of drt_trace_kernel */
__device__ __forceinline__ void feature_ray(const FeatureParams &fp, const DevCamera &cam, uint32_t x, uint32_t y, uint32_t sample, V3 &ro, V3 &rd)
{
    TraceParams tp{}; /* what path_key reads of it */
    tp.seed = fp.seed;
    tp.width = fp.width;
    tp.height = fp.height;
    PathStart ps{};
    ps.x = x;
    ps.y = y;
    ps.sample = sample;
    uint64_t rs = drt_splitmix64(path_key(tp, ps));
    uint32_t draws = 0;
    camera_ray(cam, fp.pixel_scheme, x, y, rs, draws, ro, rd);
}

/* the feature vector of a first hit, and the film's update with it (reference render_image, lines 736-743); k = samples so far, this one included */
__device__ __forceinline__ void feature_update(FeatureAcc &a, const HitPoint &ip, const DevCamera &cam, const double *__restrict__ colour, uint32_t k)
{
    const bool hit = ip.index >= 0;
    double phi[DRT_FEATURE_CHANNELS];
    const V3 d = v_sub(ip.position, cam.aperture_position);
    phi[0] = hit ? ip.normal.x : 0.0;
    phi[1] = hit ? ip.normal.y : 0.0;
    phi[2] = hit ? ip.normal.z : 0.0;
    phi[3] = hit ? d.x * cam.forward.x + d.y * cam.forward.y + d.z * cam.forward.z : 0.0;
    phi[4] = hit ? 1.0 : 0.0;
    const double *c = colour + (size_t)ip.surface_mat * 3u; /* a miss: the escape material */
    phi[5] = c[0];
    phi[6] = c[1];
    phi[7] = c[2];
    const double n = (double)k;
#pragma unroll
    for (int j = 0; j < DRT_FEATURE_CHANNELS; j += 1)
    {
        const double dd = phi[j] - a.m[j];
        a.m[j] = a.m[j] + dd / n;
        a.M2[j] = a.M2[j] + dd * (phi[j] - a.m[j]);
    }
}

/* the lane's results, and the launch's two sums: one atomic per word and wave */
__device__ __forceinline__ void feature_store(const FeatureParams &fp, uint64_t p, bool valid, const FeatureAcc &a, int first_id, uint32_t count)
{
    if (valid)
    {
        double *mean = fp.mean + (size_t)p * DRT_FEATURE_CHANNELS, *m2 = fp.m2 + (size_t)p * DRT_FEATURE_CHANNELS;
#pragma unroll
        for (int j = 0; j < DRT_FEATURE_CHANNELS; j += 1)
        {
            mean[j] = a.m[j];
            m2[j] = a.M2[j];
        }
        fp.ids[p] = first_id;
    }
    const unsigned long long empty = __ballot(valid && a.m[4] == 0.0);
    uint64_t rays = valid ? count : 0u;
    for (int off = 32; off > 0; off >>= 1) rays += __shfl_down(rays, off);
    if ((threadIdx.x & 63u) == 0)
    {
        if (empty) atomicAdd(fp.info, (unsigned long long)__popcll(empty));
        if (rays) atomicAdd(fp.info + 1, (unsigned long long)rays);
    }
}

/* LDS carve-up (8-byte aligned): the scans' surface rows, the SoA surface table, then the types and materials (feature_lds_bytes in
 * the launcher). Lights and materials are not read: a first hit needs neither. */
__global__ __launch_bounds__(FEATURE_BLOCK) void drt_feature_kernel(DevScene sc, DevCamera cam, FeatureParams fp)
{
    extern __shared__ double ft_lds[];
    SceneView sv;
    sv.n_surf = sc.n_surf;
    sv.n_lights = sc.n_lights;
    {
        double *l_rows = ft_lds;
        double *l_surf = l_rows + (size_t)SR_STRIDE * sc.n_surf;
        uint32_t *l_u32 = (uint32_t *)(l_surf + (size_t)SF_COUNT * sc.n_surf);
        for (uint32_t k = threadIdx.x; k < SR_STRIDE * sc.n_surf; k += FEATURE_BLOCK)
        {
            const uint32_t i = k / SR_STRIDE, f = k % SR_STRIDE;
            l_rows[k] = f < SF_COUNT ? sc.surf[f * sc.n_surf + i] : f == SR_TYPE ? __longlong_as_double((long long)sc.surf_type[i]) : 0.0;
        }
        for (uint32_t k = threadIdx.x; k < SF_COUNT * sc.n_surf; k += FEATURE_BLOCK) l_surf[k] = sc.surf[k];
        for (uint32_t k = threadIdx.x; k < sc.n_surf; k += FEATURE_BLOCK)
        {
            l_u32[k] = sc.surf_type[k];
            l_u32[sc.n_surf + k] = sc.surf_mat[k];
        }
        __syncthreads();
        sv.rows = l_rows;
        sv.surf = l_surf;
        sv.surf_type = l_u32;
        sv.surf_mat = l_u32 + sc.n_surf;
        sv.lights = sc.lights;
        sv.light_type = sc.light_type;
        sv.light_mat = sc.light_mat;
        sv.mats = sc.mats;
        sv.bvh_nodes = nullptr; /* a scene that fits LDS is scanned whole */
        sv.bvh_leaf = nullptr;
    }
    const uint64_t p = (uint64_t)blockIdx.x * FEATURE_BLOCK + threadIdx.x;
    const bool valid = p < fp.n_pix;
    const uint32_t count = valid ? (fp.counts ? fp.counts[p] : fp.n_samples) : 0u;
    uint32_t i, j;
    tile_pixel_ij(valid ? p : 0, fp.tile_w, i, j);
    const uint32_t x = fp.x0 + i, y = fp.y0 + j * fp.row_stride;
    FeatureAcc a;
#pragma unroll
    for (int c = 0; c < DRT_FEATURE_CHANNELS; c += 1) a.m[c] = a.M2[c] = 0.0;
    int first_id = -1;
    for (uint32_t k = 0; k < count; k += 1)
    {
        V3 ro, rd;
        feature_ray(fp, cam, x, y, fp.first_sample + k, ro, rd);
        HitPoint ip;
        ip.position = ip.normal = v3(0, 0, 0);
        find_ray_intersection<true>(sv, sc, ip, ro, rd);
        if (k == 0) first_id = ip.index;
        feature_update(a, ip, cam, fp.colour, k + 1u);
    }
    feature_store(fp, p, valid, a, first_id, count);
}

__global__ __launch_bounds__(FEATURE_BLOCK) void drt_feature_bvh_kernel(DevScene sc, DevCamera cam, FeatureParams fp)
{
    __shared__ int s_stack[FEATURE_BLOCK / 64][BVH_LDS_STACK * 64];
    __shared__ int s_leaf_queue[FEATURE_BLOCK / 64][BVH_QUEUE_WORDS];
    SceneView sv;
    sv.n_surf = sc.n_surf; sv.n_lights = sc.n_lights;
    sv.surf = sc.surf; sv.lights = sc.lights; sv.surf_type = sc.surf_type; sv.surf_mat = sc.surf_mat;
    sv.light_type = sc.light_type; sv.light_mat = sc.light_mat; sv.mats = sc.mats;
    sv.bvh_nodes = sc.bvh_nodes; sv.bvh_leaf = sc.bvh_leaf;
    const uint32_t lane = threadIdx.x & 63u;
    int *stack = s_stack[threadIdx.x >> 6];
    int *leaf_queue = s_leaf_queue[threadIdx.x >> 6];
    const uint64_t p = (uint64_t)blockIdx.x * FEATURE_BLOCK + threadIdx.x;
    const bool valid = p < fp.n_pix;
    const uint32_t count = valid ? (fp.counts ? fp.counts[p] : fp.n_samples) : 0u;
    uint32_t i, j;
    tile_pixel_ij(valid ? p : 0, fp.tile_w, i, j);
    const uint32_t x = fp.x0 + i, y = fp.y0 + j * fp.row_stride;
    FeatureAcc a;
#pragma unroll
    for (int c = 0; c < DRT_FEATURE_CHANNELS; c += 1) a.m[c] = a.M2[c] = 0.0;
    int first_id = -1;
    /* the whole wave goes round until its last lane is done */
    for (uint32_t k = 0; __any(k < count); k += 1)
    {
        const bool mine = k < count;
        V3 ro = v3(0, 0, 0), rd = v3(0, 0, 1);
        if (mine) feature_ray(fp, cam, x, y, fp.first_sample + k, ro, rd);
        const V3 jo = v_sum(ro, v_mul(rd, DRT_VIS_FUDGE)); /* src/daily_ray_trace.c:339 */
        double limit = DRT_INF;
        int index = -1;
        bool occluded = false;
        bvh_walk(sv, stack, leaf_queue, lane, mine ? JOB_CLOSEST : JOB_NONE, jo, rd, limit, index, occluded);
        if (mine)
        {
            HitPoint ip;
            ip.position = ip.normal = v3(0, 0, 0);
            hit_point_from_scan(sv, sc, ip, jo, rd, limit, index);
            if (k == 0) first_id = ip.index;
            feature_update(a, ip, cam, fp.colour, k + 1u);
        }
    }
    feature_store(fp, p, valid, a, first_id, count);
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
