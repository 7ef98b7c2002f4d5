/*
 * drt_ray_kernels.h -- ray queries (drt_cast_rays, drt_test_visibility, drt_cast_pixels): the path's two scene-level functions,
 * find_ray_intersection and points_mutually_visible, on rays the caller supplies. DESIGN.md, section 5e, states the semantics; the
 * oracle's drt_oracle_find_ray_intersection and drt_oracle_points_mutually_visible are the rule, and these kernels are held to
 * them bit for bit. They call the render path's device functions and copy none; they read the scene tables and the camera only.
 *
 * One ray per lane, RAY_BLOCK lanes per workgroup, a workgroup loops over ray blocks (grid-stride): the LDS kernels pay their
 * staging once per workgroup. Both scans hold whole-wave operations (wave-uniform surface loops, __any in the shadow scan), so every
 * lane of a wave runs them: a lane past n takes the last ray of the list -- a ray of its own block, since a block that starts past
 * n is not entered -- and stores nothing. In the hierarchy kernels such a lane walks with JOB_NONE. The scene views, the wave's
 * traversal storage and the first-hit step are drt_first_hit.h's, which states the whole-wave contract.
 *
 *   drt_ray_closest_kernel<PIXELS>      scenes in LDS: first_hit_lds
 *   drt_ray_visible_kernel              scenes in LDS: points_mutually_visible<true>
 *   drt_ray_closest_bvh_kernel<PIXELS>  scenes behind the hierarchy: first_hit_bvh; a caller's direction that is not of unit length
 *                                       (RAY_UNIT_TOLERANCE): the LDS kernel's loop over the tables in HBM
 *   drt_ray_visible_bvh_kernel          scenes behind the hierarchy: bvh_walk JOB_SHADOW
 * PIXELS: the lane builds the path's own camera ray of (x, y, sample) with feature_ray in place of loading a ray (drt_cast_pixels).
 */
#pragma once

#include "drt_first_hit.h"

#define RAY_BLOCK 256

static_assert(sizeof(drt_ray_hit) == 104, "drt_ray_hit is 13 8-byte words");

struct RayParams
{
    uint64_t n;
    const double *a, *b;      /* [n][3] each: origins and directions, or p0 and p1 */
    drt_ray_hit *hits;        /* [n] */
    uint8_t     *visible;     /* [n] */
    /* PIXELS */
    const uint32_t *xy, *samples; /* [n][2], [n] */
    double *out_a, *out_b;        /* [n][3] each, or null: the rays cast */
    uint32_t width, height, pixel_scheme;
    uint64_t seed;
};

__device__ __forceinline__ V3 ray_load3(const double *p, uint64_t i) { return v3(p[i * 3 + 0], p[i * 3 + 1], p[i * 3 + 2]); }
__device__ __forceinline__ void ray_store3(double *p, uint64_t i, V3 v)
{
    p[i * 3 + 0] = v.x;
    p[i * 3 + 1] = v.y;
    p[i * 3 + 2] = v.z;
}

/* query j's ray: loaded, or the camera ray of its pixel and sample */
template <bool PIXELS>
__device__ __forceinline__ void ray_fetch(const RayParams &rp, const DevCamera &cam, uint64_t j, bool valid, V3 &ro, V3 &rd)
{
    if (PIXELS)
    {
        FeatureParams fp{}; /* what feature_ray reads of it */
        fp.seed = rp.seed;
        fp.width = rp.width;
        fp.height = rp.height;
        fp.pixel_scheme = rp.pixel_scheme;
        const uint32_t x = rp.xy[j * 2 + 0], y = rp.xy[j * 2 + 1];
        feature_ray(fp, cam, x, y, rp.samples[j], ro, rd);
        /* device mode: the host cannot look at xy, so a pixel outside the image is answered here -- by a NaN ray, which misses */
        if (x >= rp.width || y >= rp.height)
        {
            ro = v3(0, 0, 0);
            rd = v3(__builtin_nan(""), __builtin_nan(""), __builtin_nan(""));
        }
        if (valid && rp.out_a) ray_store3(rp.out_a, j, ro);
        if (valid && rp.out_b) ray_store3(rp.out_b, j, rd);
    }
    else
    {
        ro = ray_load3(rp.a, j);
        rd = ray_load3(rp.b, j);
    }
}

/* A lane's 104 bytes as thirteen 8-byte words; a wave's 64 structs are one contiguous run of 6656 bytes. A miss: index -1, the escape
 * material, every other word +0. */
__device__ __forceinline__ void ray_store_hit(drt_ray_hit *hits, uint64_t i, const HitPoint &ip, double distance)
{
    const bool hit = ip.index >= 0;
    unsigned long long *w = (unsigned long long *)(hits + i);
    double *d = (double *)w;
    d[0] = hit ? ip.position.x : 0.0;
    d[1] = hit ? ip.position.y : 0.0;
    d[2] = hit ? ip.position.z : 0.0;
    d[3] = hit ? ip.normal.x : 0.0;
    d[4] = hit ? ip.normal.y : 0.0;
    d[5] = hit ? ip.normal.z : 0.0;
    d[6] = hit ? ip.out.x : 0.0;
    d[7] = hit ? ip.out.y : 0.0;
    d[8] = hit ? ip.out.z : 0.0;
    d[9] = hit ? ip.on_dot : 0.0;
    d[10] = hit ? distance : 0.0;
    const uint32_t inc = hit ? ip.incident_mat : 0u, tra = hit ? ip.transmit_mat : 0u;
    w[11] = (unsigned long long)(uint32_t)ip.index | ((unsigned long long)ip.surface_mat << 32);
    w[12] = (unsigned long long)inc | ((unsigned long long)tra << 32);
}

/* A wave's 64 answers are 64 contiguous bytes: where the wave is whole and its run 8-byte aligned, lanes 0..7 store one 8-byte word
 * each, made from the wave's ballot; otherwise (the list's last wave, a caller's odd pointer) every valid lane stores its byte. */
__device__ __forceinline__ void ray_store_visible(uint8_t *visible, uint64_t i, bool valid, bool vis)
{
    const unsigned long long mask = __ballot(valid && vis), all = __ballot(valid);
    const uint32_t lane = threadIdx.x & 63u;
    uint8_t *run = visible + (i - lane);
    if (all == ~0ull && ((uintptr_t)run & 7u) == 0u)
    {
        if (lane < 8u)
        {
            const unsigned long long bits = (mask >> (lane * 8u)) & 0xFFull;
            unsigned long long word = 0; /* bit k of `bits` to byte k: 0 or 1 */
#pragma unroll
            for (int k = 0; k < 8; k += 1) word |= ((bits >> k) & 1ull) << (8 * k);
            ((unsigned long long *)run)[lane] = word;
        }
    }
    else if (valid) visible[i] = vis ? 1 : 0;
}

template <bool PIXELS>
__global__ __launch_bounds__(RAY_BLOCK) void drt_ray_closest_kernel(DevScene sc, DevCamera cam, RayParams rp)
{
    extern __shared__ double ray_lds[];
    SceneView sv;
    stage_surfaces<RAY_BLOCK>(sc, ray_lds, sv);
    for (uint64_t base = (uint64_t)blockIdx.x * RAY_BLOCK; base < rp.n; base += (uint64_t)gridDim.x * RAY_BLOCK)
    {
        const uint64_t i = base + threadIdx.x;
        const bool valid = i < rp.n;
        const uint64_t j = valid ? i : rp.n - 1;
        V3 ro, rd;
        ray_fetch<PIXELS>(rp, cam, j, valid, ro, rd);
        const HitPoint ip = first_hit_lds(sv, sc, ro, rd);
        /* min_dist: the hit surface's intersector again, on the operands the scan gave it (src/daily_ray_trace.c:339-364) */
        double distance = 0.0;
        if (ip.index >= 0) distance = surface_distance(sv, (uint32_t)ip.index, sv.surf_type[ip.index], v_sum(ro, v_mul(rd, DRT_VIS_FUDGE)), rd);
        if (valid) ray_store_hit(rp.hits, i, ip, distance);
    }
}

__global__ __launch_bounds__(RAY_BLOCK) void drt_ray_visible_kernel(DevScene sc, RayParams rp)
{
    extern __shared__ double ray_lds[];
    SceneView sv;
    stage_surfaces<RAY_BLOCK>(sc, ray_lds, sv);
    for (uint64_t base = (uint64_t)blockIdx.x * RAY_BLOCK; base < rp.n; base += (uint64_t)gridDim.x * RAY_BLOCK)
    {
        const uint64_t i = base + threadIdx.x;
        const bool valid = i < rp.n;
        const uint64_t j = valid ? i : rp.n - 1;
        const bool vis = points_mutually_visible<true>(sv, ray_load3(rp.a, j), ray_load3(rp.b, j));
        ray_store_visible(rp.visible, i, valid, vis);
    }
}

/* A caller's ray whose direction is finite and farther than RAY_UNIT_TOLERANCE (2^-42, drt_kernels.h: ray_off_unit) from unit length
 * does not take the hierarchy walk: it is answered by the reference's own loop over all surfaces, exact, and as slow as a scene of
 * that size without a hierarchy. NaN and infinite directions walk, and miss. */
template <bool PIXELS>
__global__ __launch_bounds__(RAY_BLOCK) void drt_ray_closest_bvh_kernel(DevScene sc, DevCamera cam, RayParams rp)
{
    const SceneView sv = scene_view_global(sc);
    const WaveStore store = wave_store<RAY_BLOCK>();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * RAY_BLOCK; base < rp.n; base += (uint64_t)gridDim.x * RAY_BLOCK)
    {
        const uint64_t i = base + threadIdx.x;
        const bool valid = i < rp.n;
        V3 ro = v3(0, 0, 0), rd = v3(0, 0, 1);
        if (valid) ray_fetch<PIXELS>(rp, cam, i, true, ro, rd);
        const bool scan = !PIXELS && valid && ray_off_unit(rd); /* (a camera ray is normalised) */
        first_hit_bvh(sv, sc, store, lane, valid && !scan, ro, rd, [&](const HitPoint &ip, double min_dist) { ray_store_hit(rp.hits, i, ip, min_dist); });
        if (scan)
        {
            /* as drt_ray_closest_kernel, on the tables where they lie; the loop holds no whole-wave operation, so it may run divergent */
            HitPoint ip = no_hit_point();
            find_ray_intersection<false>(sv, sc, ip, ro, rd);
            double distance = 0.0;
            if (ip.index >= 0) distance = surface_distance(sv, (uint32_t)ip.index, sv.surf_type[ip.index], v_sum(ro, v_mul(rd, DRT_VIS_FUDGE)), rd);
            ray_store_hit(rp.hits, i, ip, distance);
        }
    }
}

/* the shadow job: the one walk outside first_hit_bvh, under the same contract (drt_first_hit.h) */
__global__ __launch_bounds__(RAY_BLOCK) void drt_ray_visible_bvh_kernel(DevScene sc, RayParams rp)
{
    const SceneView sv = scene_view_global(sc);
    const WaveStore store = wave_store<RAY_BLOCK>();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * RAY_BLOCK; base < rp.n; base += (uint64_t)gridDim.x * RAY_BLOCK)
    {
        const uint64_t i = base + threadIdx.x;
        const bool valid = i < rp.n;
        V3 jo = v3(0, 0, 0), jd = v3(0, 0, 1);
        double limit = DRT_INF;
        if (valid)
        {
            /* points_mutually_visible, src/daily_ray_trace.c:238-270, as drt_bounce_kernel sets its shadow job up */
            const V3 p0 = ray_load3(rp.a, i), p1 = ray_load3(rp.b, i);
            jd = v_normalise(v_sub(p1, p0));
            jo = v_sum(p0, v_mul(jd, DRT_VIS_FUDGE));
            limit = v_length(v_sub(p1, jo)) - DRT_VIS_FUDGE;
        }
        int index = -1;
        bool occluded = false;
        bvh_walk(sv, store.stack, store.leaf_queue, lane, valid ? JOB_SHADOW : JOB_NONE, jo, jd, limit, index, occluded);
        ray_store_visible(rp.visible, i, valid, !occluded);
    }
}
