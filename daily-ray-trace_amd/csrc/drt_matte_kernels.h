/*
 * drt_matte_kernels.h -- the ID mattes (drt_render_mattes): per tile pixel and layer (the surface a sample's first hit lands on, and that
 * surface's material) DRT_MATTE_SLOTS ranked (id, count) pairs, the samples that hit an id no slot had room for, and the samples that
 * hit nothing. DESIGN.md, section 5d, states the rule; tests/matte_rule.py restates it. Integer counting only: the kernels equal the
 * rule with ==.
 *
 * The two render kernels are the pixel passes of drt_first_hit.h, as drt_feature_kernel and drt_feature_bvh_kernel are: one lane per
 * tile pixel, its samples in ascending order. What a lane carries differs (MatteAcc): twelve (id, count) slots in registers, updated
 * by an unrolled compare / select chain (no runtime index, so nothing goes to scratch), ranked once at the end by a fixed network.
 *
 *   drt_matte_kernel         scenes in LDS
 *   drt_matte_bvh_kernel     scenes behind the hierarchy
 *   drt_matte_select_kernel  drt_read_matte: the share of a pixel's samples whose id is in a list
 *   drt_matte_bgra_kernel    drt_read_matte_bgra: the slots' palette colours weighted by their shares, as .bmp pixel bytes
 */
#pragma once

#include "drt_feature_kernels.h"

#define MATTE_INFO_WORDS 4 /* d_mt_info, 8-byte words: pixels that hit nothing, pixels with other > 0 per layer, rays */

struct MatteParams
{
    FeatureParams fp;       /* what feature_ray reads, n_pix and counts; mean, m2, ids, colour and info are not used */
    int32_t  *ids;          /* [n_pix][DRT_MATTE_LAYERS][DRT_MATTE_SLOTS] */
    uint32_t *counts;       /* likewise */
    uint32_t *tail;         /* [n_pix][4]: c_p, misses, other of the surface layer, other of the material layer */
    unsigned long long *info; /* MATTE_INFO_WORDS */
};

/* an empty slot is (-1, 0); the slots fill from the lowest, so the empty ones are the highest */
struct MatteLayer
{
    int32_t  id[DRT_MATTE_SLOTS];
    uint32_t n[DRT_MATTE_SLOTS];
    uint32_t other;
};

/* A hit's id goes to the slot that holds it, else to the lowest empty one, else to `other`. Going up the slots, the first that holds
 * the id or is empty is the one: an empty slot has only empty slots above it, so the id is in none of those. Selects only, and `hit`
 * is an operand instead of a branch round the call: a branch here has the compiler merge the two sides' updates of `other` and
 * `misses` into one store through a chosen address, which puts those three words into scratch. */
__device__ __forceinline__ void matte_layer_add(MatteLayer &l, bool hit, int32_t id)
{
    bool placed = !hit;
#pragma unroll
    for (int k = 0; k < DRT_MATTE_SLOTS; k += 1)
    {
        const bool take = !placed && (l.id[k] == id || l.id[k] < 0);
        l.id[k] = take ? id : l.id[k];
        l.n[k] += take ? 1u : 0u;
        placed = placed || take;
    }
    l.other += placed ? 0u : 1u;
}

/* slots i < j in rank order: count descending, then id ascending (an empty slot, count 0, after every used one) */
__device__ __forceinline__ void matte_exchange(MatteLayer &l, int i, int j)
{
    const bool swap = l.n[j] > l.n[i] || (l.n[j] == l.n[i] && l.id[j] < l.id[i]);
    const int32_t id_i = l.id[i], id_j = l.id[j];
    const uint32_t n_i = l.n[i], n_j = l.n[j];
    l.id[i] = swap ? id_j : id_i;
    l.id[j] = swap ? id_i : id_j;
    l.n[i] = swap ? n_j : n_i;
    l.n[j] = swap ? n_i : n_j;
}

/* the twelve-exchange sorting network for six inputs */
__device__ __forceinline__ void matte_rank(MatteLayer &l)
{
    static_assert(DRT_MATTE_SLOTS == 6, "matte_rank is the network for six slots");
    matte_exchange(l, 0, 5); matte_exchange(l, 1, 3); matte_exchange(l, 2, 4);
    matte_exchange(l, 1, 2); matte_exchange(l, 3, 4);
    matte_exchange(l, 0, 3); matte_exchange(l, 2, 5);
    matte_exchange(l, 0, 1); matte_exchange(l, 2, 3); matte_exchange(l, 4, 5);
    matte_exchange(l, 1, 2); matte_exchange(l, 3, 4);
}

/* a lane's two layers and its misses */
struct MatteAcc
{
    const MatteParams &mp;
    MatteLayer l[DRT_MATTE_LAYERS];
    uint32_t misses;

    __device__ __forceinline__ explicit MatteAcc(const MatteParams &mp_) : mp(mp_) {}

    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int y = 0; y < DRT_MATTE_LAYERS; y += 1)
        {
#pragma unroll
            for (int k = 0; k < DRT_MATTE_SLOTS; k += 1)
            {
                l[y].id[k] = DRT_MATTE_ID_MISS;
                l[y].n[k] = 0u;
            }
            l[y].other = 0u;
        }
        misses = 0u;
    }

    /* one sample: its closest-hit index and that surface's material, or a miss */
    __device__ __forceinline__ void add(const HitPoint &ip, uint32_t)
    {
        const bool hit = ip.index >= 0;
        matte_layer_add(l[DRT_MATTE_SURFACE], hit, ip.index);
        matte_layer_add(l[DRT_MATTE_MATERIAL], hit, (int32_t)ip.surface_mat);
        misses += hit ? 0u : 1u;
    }

    /* ranks the lane's slots and stores them, and the launch's four sums: one atomic per word and wave */
    __device__ __forceinline__ void store(uint64_t p, bool valid, uint32_t count)
    {
        matte_rank(l[0]);
        matte_rank(l[1]);
        if (valid)
        {
            int32_t *ids = mp.ids + (size_t)p * (DRT_MATTE_LAYERS * DRT_MATTE_SLOTS);
            uint32_t *counts = mp.counts + (size_t)p * (DRT_MATTE_LAYERS * DRT_MATTE_SLOTS);
#pragma unroll
            for (int y = 0; y < DRT_MATTE_LAYERS; y += 1)
            {
#pragma unroll
                for (int k = 0; k < DRT_MATTE_SLOTS; k += 1)
                {
                    ids[y * DRT_MATTE_SLOTS + k] = l[y].id[k];
                    counts[y * DRT_MATTE_SLOTS + k] = l[y].n[k];
                }
            }
            uint32_t *tail = mp.tail + (size_t)p * 4u;
            tail[0] = count;
            tail[1] = misses;
            tail[2] = l[0].other;
            tail[3] = l[1].other;
        }
        const unsigned long long empty = __ballot(valid && misses == count);
        const unsigned long long over0 = __ballot(valid && l[0].other > 0u);
        const unsigned long long over1 = __ballot(valid && l[1].other > 0u);
        uint64_t rays = valid ? count : 0u;
        for (int off = 32; off > 0; off >>= 1) rays += __shfl_down(rays, off);
        if ((threadIdx.x & 63u) == 0)
        {
            if (empty) atomicAdd(mp.info, (unsigned long long)__popcll(empty));
            if (over0) atomicAdd(mp.info + 1, (unsigned long long)__popcll(over0));
            if (over1) atomicAdd(mp.info + 2, (unsigned long long)__popcll(over1));
            if (rays) atomicAdd(mp.info + 3, (unsigned long long)rays);
        }
    }
};

/* the dynamic LDS is first_hit_pixels_lds's (feature_lds_bytes in the launcher) */
__global__ __launch_bounds__(FEATURE_BLOCK) void drt_matte_kernel(DevScene sc, DevCamera cam, MatteParams mp)
{
    extern __shared__ double mt_lds[];
    MatteAcc a(mp);
    a.clear();
    const PixelLane px = first_hit_pixels_lds<FEATURE_BLOCK>(sc, cam, mp.fp, mt_lds, [&](const HitPoint &ip, uint32_t k) { a.add(ip, k); });
    a.store(px.p, px.valid, px.count);
}

__global__ __launch_bounds__(FEATURE_BLOCK) void drt_matte_bvh_kernel(DevScene sc, DevCamera cam, MatteParams mp)
{
    MatteAcc a(mp);
    a.clear();
    FIRST_HIT_PIXELS_BVH(FEATURE_BLOCK, sc, cam, mp.fp, px, a)
    a.store(px.p, px.valid, px.count);
}

/* coverage[p] = (the counts of the layer's slots whose id is in id_list, summed in integers, plus misses if the list holds
 * DRT_MATTE_ID_MISS) / c_p: one division. One lane per pixel; every lane reads the same list entry at the same time. */
__global__ __launch_bounds__(FEATURE_BLOCK) void drt_matte_select_kernel(const int32_t *__restrict__ ids, const uint32_t *__restrict__ counts,
                                                                        const uint32_t *__restrict__ tail, uint64_t n_pix, int layer,
                                                                        const int32_t *__restrict__ id_list, uint32_t n_ids,
                                                                        double *__restrict__ coverage)
{
    const uint64_t p = (uint64_t)blockIdx.x * FEATURE_BLOCK + threadIdx.x;
    if (p >= n_pix) return;
    const size_t at = ((size_t)p * DRT_MATTE_LAYERS + (size_t)layer) * DRT_MATTE_SLOTS;
    int32_t id[DRT_MATTE_SLOTS];
    bool in[DRT_MATTE_SLOTS];
#pragma unroll
    for (int k = 0; k < DRT_MATTE_SLOTS; k += 1)
    {
        id[k] = ids[at + k];
        in[k] = false;
    }
    bool miss = false;
    for (uint32_t e = 0; e < n_ids; e += 1)
    {
        const int32_t want = id_list[e];
        miss = miss || want == DRT_MATTE_ID_MISS;
#pragma unroll
        for (int k = 0; k < DRT_MATTE_SLOTS; k += 1) in[k] = in[k] || (want >= 0 && id[k] == want);
    }
    uint64_t sum = miss ? tail[p * 4u + 1u] : 0u;
#pragma unroll
    for (int k = 0; k < DRT_MATTE_SLOTS; k += 1) sum += in[k] ? counts[at + k] : 0u;
    coverage[p] = (double)sum / (double)tail[p * 4u];
}

/* the palette: h = (uint32_t)(id + 1) * 0x9E3779B1u; h ^= h >> 16; channel c (0 R, 1 G, 2 B) is 64 + ((h >> 8 c) & 127) */
__device__ __forceinline__ double matte_palette(int32_t id, int c)
{
    uint32_t h = (uint32_t)(id + 1) * 0x9E3779B1u;
    h ^= h >> 16;
    return (double)(64u + ((h >> (8 * c)) & 127u));
}
/* per channel v = sum over the ranked slots, from +0, of (count / c_p) * palette; byte = (uint8_t)(v + 0.5), at most 191; alpha 255 */
__global__ __launch_bounds__(FEATURE_BLOCK) void drt_matte_bgra_kernel(const int32_t *__restrict__ ids, const uint32_t *__restrict__ counts,
                                                                      const uint32_t *__restrict__ tail, uint64_t n_pix, int layer,
                                                                      uint8_t *__restrict__ bgra)
{
    const uint64_t p = (uint64_t)blockIdx.x * FEATURE_BLOCK + threadIdx.x;
    if (p >= n_pix) return;
    const size_t at = ((size_t)p * DRT_MATTE_LAYERS + (size_t)layer) * DRT_MATTE_SLOTS;
    const double c_p = (double)tail[p * 4u];
    double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < DRT_MATTE_SLOTS; k += 1)
    {
        const double share = (double)counts[at + k] / c_p;
        const int32_t id = ids[at + k];
#pragma unroll
        for (int c = 0; c < 3; c += 1) v[c] = v[c] + share * matte_palette(id, c);
    }
    bgra[p * 4 + 0] = (uint8_t)(v[2] + 0.5);
    bgra[p * 4 + 1] = (uint8_t)(v[1] + 0.5);
    bgra[p * 4 + 2] = (uint8_t)(v[0] + 0.5);
    bgra[p * 4 + 3] = 255;
}
