/*
 * drt_first_hit.h -- "what does this ray hit first?" outside the render path: what the feature buffers (drt_feature_kernels.h), the ID
 * mattes (drt_matte_kernels.h) and the ray queries (drt_ray_kernels.h) share. The scene as the scans read it (staged in LDS, or the
 * tables behind the hierarchy), a wave's traversal storage, the first-hit step in both forms, and the loop of the passes that give
 * every tile pixel a lane and hand its samples' first hits to the pass's accumulator. They call the render path's device functions --
 * path_key, camera_ray, find_ray_intersection<true>, bvh_walk, hit_point_from_scan -- and copy none.
 *
 * THE WAVE-UNIFORM CONTRACT. bvh_walk is a whole-wave function (ballots and __any in its loops): every lane of a wave enters it
 * together or the wave hangs. So first_hit_bvh is called by every lane of the wave, in wave-uniform control flow. A lane that has no
 * ray says so with mine = false and walks as JOB_NONE; what is done with a hit is handed in and runs on the lanes that have one. A
 * loop round it runs until the wave's last lane is done (__any), never until the lane's own count. The LDS form has no such rule
 * for its callers' loops, but its scans hold wave-uniform surface loops too: a lane without work of its own is given a ray of its
 * block (drt_ray_kernels.h) or waits after the loop (first_hit_pixels_lds).
 */
#pragma once

#include "drt_bvh_kernels.h"

/* a pixel pass: the tile, the samples, and where the feature pass puts its results (drt_matte_kernels.h wraps it with its own) */
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

/* the camera ray of a pixel's sample: the `started` block of drt_trace_kernel */
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

/* the scene behind the hierarchy: the tables where they lie */
__device__ __forceinline__ SceneView scene_view_global(const DevScene &sc)
{
    SceneView sv;
    sv.n_surf = sc.n_surf; sv.n_lights = sc.n_lights;
    sv.surf = sc.surf; sv.lights = sc.lights; sv.surf_type = sc.surf_type; sv.surf_mat = sc.surf_mat;
    sv.light_type = sc.light_type; sv.light_mat = sc.light_mat; sv.mats = sc.mats;
    sv.bvh_nodes = sc.bvh_nodes; sv.bvh_leaf = sc.bvh_leaf;
    return sv;
}

/* A scene that fits LDS, staged by a workgroup of BLOCK lanes (8-byte aligned): the scans' surface rows, the SoA surface table, then
 * the types and materials, 256 bytes per surface -- feature_lds_bytes in the launcher is this carve-up's size rule. Lights and
 * materials are not read: a first hit needs neither. Ends with the workgroup's barrier. */
template <int BLOCK>
__device__ __forceinline__ void stage_surfaces(const DevScene &sc, double *lds, SceneView &sv)
{
    double *l_rows = lds;
    double *l_surf = l_rows + (size_t)SR_STRIDE * sc.n_surf;
    uint32_t *l_u32 = (uint32_t *)(l_surf + (size_t)SF_COUNT * sc.n_surf);
    for (uint32_t k = threadIdx.x; k < SR_STRIDE * sc.n_surf; k += BLOCK)
    {
        const uint32_t i = k / SR_STRIDE, f = k % SR_STRIDE;
        l_rows[k] = f < SF_COUNT ? sc.surf[f * sc.n_surf + i] : f == SR_TYPE ? __longlong_as_double((long long)sc.surf_type[i]) : 0.0;
    }
    for (uint32_t k = threadIdx.x; k < SF_COUNT * sc.n_surf; k += BLOCK) l_surf[k] = sc.surf[k];
    for (uint32_t k = threadIdx.x; k < sc.n_surf; k += BLOCK)
    {
        l_u32[k] = sc.surf_type[k];
        l_u32[sc.n_surf + k] = sc.surf_mat[k];
    }
    __syncthreads();
    sv.n_surf = sc.n_surf;
    sv.n_lights = sc.n_lights;
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

/* what bvh_walk keeps per wave: the lanes' stacks and leaf queues, in LDS as in drt_bounce_kernel (36 KB for a workgroup of 256) */
struct WaveStore
{
    int *stack, *leaf_queue;
};
template <int BLOCK>
__device__ __forceinline__ WaveStore wave_store()
{
    __shared__ int s_stack[BLOCK / 64][BVH_LDS_STACK * 64];
    __shared__ int s_leaf_queue[BLOCK / 64][BVH_QUEUE_WORDS];
    WaveStore w;
    w.stack = s_stack[threadIdx.x >> 6];
    w.leaf_queue = s_leaf_queue[threadIdx.x >> 6];
    return w;
}

__device__ __forceinline__ HitPoint no_hit_point()
{
    HitPoint ip;
    ip.position = ip.normal = ip.out = v3(0, 0, 0);
    ip.on_dot = 0.0;
    ip.surface_mat = ip.incident_mat = ip.transmit_mat = 0u;
    ip.index = -1;
    return ip;
}

/* the closest hit of (ro, rd) in a staged scene */
__device__ __forceinline__ HitPoint first_hit_lds(const SceneView &sv, const DevScene &sc, V3 ro, V3 rd)
{
    HitPoint ip = no_hit_point();
    find_ray_intersection<true>(sv, sc, ip, ro, rd);
    return ip;
}

/* The same behind the hierarchy, as drt_bounce_kernel takes a continuation ray. Under the contract above: every lane of the wave
 * calls it; where `mine`, then(ip, min_dist) is given the ray's hit point and its distance from the moved origin. (Handed on inside the
 * branch and not returned: a returned hit point is made for every lane and merged after the branch, which cost the callers
 * registers and time.) */
template <class Then>
__device__ __forceinline__ void first_hit_bvh(const SceneView &sv, const DevScene &sc, const WaveStore &store, uint32_t lane, bool mine, V3 ro, V3 rd,
                                              Then then)
{
    const V3 jo = v_sum(ro, v_mul(rd, DRT_VIS_FUDGE)); /* src/daily_ray_trace.c:339 */
    double limit = DRT_INF;
    int index = -1;
    bool occluded = false;
    bvh_walk(sv, store.stack, store.leaf_queue, lane, mine ? JOB_CLOSEST : JOB_NONE, jo, rd, limit, index, occluded);
    if (mine)
    {
        HitPoint ip = no_hit_point();
        hit_point_from_scan(sv, sc, ip, jo, rd, limit, index);
        then(ip, limit);
    }
}

/* one lane per tile pixel: the lane's pixel, whether the tile has it, its samples and its image coordinates */
struct PixelLane
{
    uint64_t p;
    bool     valid;
    uint32_t count, x, y;
};
template <int BLOCK>
__device__ __forceinline__ PixelLane pixel_lane(const FeatureParams &fp)
{
    PixelLane px;
    px.p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    px.valid = px.p < fp.n_pix;
    px.count = px.valid ? (fp.counts ? fp.counts[px.p] : fp.n_samples) : 0u;
    uint32_t i, j;
    tile_pixel_ij(px.valid ? px.p : 0, fp.tile_w, i, j);
    px.x = fp.x0 + i;
    px.y = fp.y0 + j * fp.row_stride;
    return px;
}

/* The pixel passes. The lane loops over its own samples in ascending order, because what a pass keeps per pixel is sequential:
 * add(ip, k) is called with the first hit of sample first_sample + k for k = 0 .. count - 1, and the lane's PixelLane comes back for
 * the caller's store, which every lane of the workgroup runs (it holds the wave's sums). Lanes of a wave may hold different counts
 * (adaptive films), and a tile's last wave has lanes without a pixel (count 0).
 * Scenes in LDS: a lane that is done waits for the others after the loop. */
template <int BLOCK, class Add>
__device__ __forceinline__ PixelLane first_hit_pixels_lds(const DevScene &sc, const DevCamera &cam, const FeatureParams &fp, double *lds, Add add)
{
    SceneView sv;
    stage_surfaces<BLOCK>(sc, lds, sv);
    const PixelLane px = pixel_lane<BLOCK>(fp);
    for (uint32_t k = 0; k < px.count; k += 1)
    {
        V3 ro, rd;
        feature_ray(fp, cam, px.x, px.y, fp.first_sample + k, ro, rd);
        add(first_hit_lds(sv, sc, ro, rd), k);
    }
    return px;
}

/* Scenes behind the hierarchy: the whole wave goes round until its last lane is done, and a lane that is done walks along
 * (mine = false). Declares `const PixelLane px` and calls a.add(ip, k) as first_hit_pixels_lds calls add. A macro for the kernel's own
 * body, and on purpose: as a function round this loop -- the accumulator or a callable handed in, by value or by reference, the
 * store inside or outside -- it compiles to the same registers but to another schedule of the accumulator's code after the walk,
 * which was measured at 1.6 % of drt_matte_bvh_kernel's time and up to 2.3 % of drt_feature_bvh_kernel's; expanded in the kernel it
 * runs at the time of the loop written out there (profiles/NOTES.md). */
#define FIRST_HIT_PIXELS_BVH(BLOCK, sc, cam, fp, px, a)                                                                        \
    const SceneView fh_sv = scene_view_global(sc);                                                                             \
    const WaveStore fh_store = wave_store<BLOCK>();                                                                            \
    const uint32_t fh_lane = threadIdx.x & 63u;                                                                                \
    const PixelLane px = pixel_lane<BLOCK>(fp);                                                                                \
    for (uint32_t fh_k = 0; __any(fh_k < px.count); fh_k += 1)                                                                 \
    {                                                                                                                          \
        const bool fh_mine = fh_k < px.count;                                                                                  \
        V3 fh_ro = v3(0, 0, 0), fh_rd = v3(0, 0, 1);                                                                           \
        if (fh_mine) feature_ray(fp, cam, px.x, px.y, (fp).first_sample + fh_k, fh_ro, fh_rd);                                 \
        first_hit_bvh(fh_sv, sc, fh_store, fh_lane, fh_mine, fh_ro, fh_rd, [&](const HitPoint &ip, double) { (a).add(ip, fh_k); }); \
    }
