/*
 * drt_build_kernels.h -- the hierarchy of a live context built anew on the device (include/drt_hip.h: drt_rebuild_hierarchy;
 * DESIGN.md 5h). A pass of its own beside the render path, as drt_update_kernels.h is: it reads the boxes the derive kernel wrote,
 * writes the tree's links and leaf order into the allocations the context has, and hands over to drt_bvh_leaf_kernel for the leaves'
 * numbers and boxes. The tree is the one drt_build_rule.h states, so a test can hold it to a restatement byte for byte.
 *
 *   drt_build_init_kernel       the status words: centre bounds at their identities, one item (the root) on level 0
 *   drt_build_bounds_kernel     one lane per tree surface: the smallest and largest box centre per axis over the bounded surfaces
 *   drt_build_keys_kernel       one lane per tree surface: its 63-bit key and its position as the sort's payload
 *   drt_build_count_kernel      } one pass of a stable least-significant-digit radix sort, 8 bits at a time: digit counts per
 *   drt_build_scan_kernel       } workgroup, the exclusive scan of the [digit][workgroup] table, the scatter of every tile in
 *   drt_build_scatter_kernel    } element order
 *   drt_build_topology_kernel   one launch per tree level, top down: an item is an inner node and its range of the sorted keys
 *   drt_build_refit_kernel      one launch per tree level, deepest first: drt_bvh_refit_kernel's union, its range of the level table
 *                               read from device memory (the host does not know a level's size when it enqueues the launch)
 *
 * Kernel boundaries are the only hand-off between workgroups: no counter, flag or waiting lane crosses one. What a launch reads of
 * another workgroup's writing was written by an earlier launch; the atomics only count and reduce, nobody reads them back in the
 * same launch. Plain C++ throughout: every store is a vector store or a vector atomic.
 */
#pragma once

#include "drt_build_rule.h"
#include "drt_update_kernels.h"

#define BUILD_BLOCK 256
#define SORT_ITEMS 4                               /* elements per lane and pass */
#define SORT_TILE (BUILD_BLOCK * SORT_ITEMS)       /* elements per workgroup */
#define SORT_DIGITS 256
#define SORT_PASSES 8                              /* 8 x 8 bits cover the 63-bit key; an even count leaves the result where it started */

/* status words of a build, all written by drt_build_init_kernel: +0..2 the smallest centre per axis, +3..5 the largest, as
 * order-preserving bit patterns; then, as 32-bit words behind them, the number of items (inner nodes) on every level */
#define BUILD_BOUND_WORDS 6
#define BUILD_LEVELS BUILD_RULE_STACK
#define BUILD_STATUS_BYTES (BUILD_BOUND_WORDS * 8 + (BUILD_LEVELS + 1) * 4)

struct BuildTables
{
    const double   *boxes;      /* [n_surf][6]: drt_surface_derive_kernel's */
    const uint32_t *tree_surf;  /* [m]: the surface of tree position k (spheres and planes in surface order) */
    unsigned long long *bounds; /* BUILD_BOUND_WORDS */
    uint32_t       *level_count; /* [BUILD_LEVELS + 1] */
    uint32_t        m;
};

/* a double as a pattern that orders, unsigned, like the number (no NaN comes here) */
__device__ __forceinline__ unsigned long long build_ordered(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double build_unordered(unsigned long long p)
{
    return __longlong_as_double((long long)((p >> 63) ? (p & 0x7FFFFFFFFFFFFFFFull) : ~p));
}

__global__ void __launch_bounds__(64) drt_build_init_kernel(BuildTables t, uint4 *items)
{
    const uint32_t i = threadIdx.x;
    if (i < 3u) t.bounds[i] = ~0ull;
    else if (i < BUILD_BOUND_WORDS) t.bounds[i] = 0ull;
    if (i <= BUILD_LEVELS) t.level_count[i] = i == 0u ? 1u : 0u;
    if (i == 0u) items[0] = make_uint4(0u, 0u, t.m, 0u); /* the root over every position */
}

/* is the box bounded, and its centre: 0.5 * (lo + hi) per axis, as BvhBuilder::build */
__device__ __forceinline__ bool build_centre(const BuildTables &t, uint32_t k, double c[3])
{
    const double *box = t.boxes + (size_t)t.tree_surf[k] * 6;
    bool bounded = true;
    for (int a = 0; a < 3; a += 1)
    {
        const double lo = box[a], hi = box[3 + a];
        bounded = bounded && build_bounded(lo) && build_bounded(hi);
        c[a] = 0.5 * (lo + hi);
    }
    return bounded;
}

__global__ void __launch_bounds__(BUILD_BLOCK) drt_build_bounds_kernel(BuildTables t)
{
    const uint32_t k = blockIdx.x * BUILD_BLOCK + threadIdx.x;
    double c[3] = {0.0, 0.0, 0.0};
    const bool mine = k < t.m && build_centre(t, k, c);
    /* the wave's minimum and maximum of the lanes that have one, then one atomic per wave and word (the derive kernel's extent) */
    unsigned long long lo[3], hi[3];
    for (int a = 0; a < 3; a += 1)
    {
        lo[a] = mine ? build_ordered(c[a]) : ~0ull;
        hi[a] = mine ? build_ordered(c[a]) : 0ull;
        for (int off = 32; off > 0; off >>= 1)
        {
            const unsigned long long l = __shfl_xor(lo[a], off, 64), h = __shfl_xor(hi[a], off, 64);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    }
    if ((threadIdx.x & 63u) == 0u && hi[0] != 0ull) /* (a bounded centre's pattern is never 0) */
        for (int a = 0; a < 3; a += 1)
        {
            atomicMin(t.bounds + a, lo[a]);
            atomicMax(t.bounds + 3 + a, hi[a]);
        }
}

__global__ void __launch_bounds__(BUILD_BLOCK) drt_build_keys_kernel(BuildTables t, uint64_t *keys, uint32_t *pos)
{
    const uint32_t k = blockIdx.x * BUILD_BLOCK + threadIdx.x;
    if (k >= t.m) return;
    double c[3];
    uint64_t key = BUILD_KEY_UNBOUNDED;
    if (build_centre(t, k, c))
    {
        uint32_t q[3];
        for (int a = 0; a < 3; a += 1) q[a] = build_quantise(c[a], build_unordered(t.bounds[a]), build_unordered(t.bounds[3 + a]));
        key = build_key(q[0], q[1], q[2]);
    }
    keys[k] = key;
    pos[k] = k;
}

/* ---- the sort: element p of tile w is w * SORT_TILE + p, p = round * BUILD_BLOCK + lane: element order is (round, lane) order ---- */

__global__ void __launch_bounds__(BUILD_BLOCK) drt_build_count_kernel(const uint64_t *keys, uint32_t m, uint32_t shift, uint32_t *table, uint32_t n_tiles)
{
    __shared__ uint32_t s_count[SORT_DIGITS];
    s_count[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * SORT_TILE;
    for (int r = 0; r < SORT_ITEMS; r += 1)
    {
        const uint32_t i = base + r * BUILD_BLOCK + threadIdx.x;
        if (i < m) atomicAdd(&s_count[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * n_tiles + blockIdx.x] = s_count[threadIdx.x];
}

/* one workgroup, one lane per digit: the table, digit-major, becomes its own exclusive scan */
__global__ void __launch_bounds__(SORT_DIGITS) drt_build_scan_kernel(uint32_t *table, uint32_t n_tiles)
{
    __shared__ uint32_t s_total[SORT_DIGITS];
    uint32_t *row = table + (size_t)threadIdx.x * n_tiles;
    uint32_t sum = 0u;
    for (uint32_t w = 0; w < n_tiles; w += 1) sum += row[w];
    s_total[threadIdx.x] = sum;
    __syncthreads();
    uint32_t before = 0u; /* everything with a smaller digit */
    for (uint32_t d = 0; d < threadIdx.x; d += 1) before += s_total[d];
    for (uint32_t w = 0; w < n_tiles; w += 1)
    {
        const uint32_t c = row[w];
        row[w] = before;
        before += c;
    }
}

__global__ void __launch_bounds__(BUILD_BLOCK) drt_build_scatter_kernel(const uint64_t *keys, const uint32_t *pos, uint64_t *keys_out, uint32_t *pos_out, uint32_t m,
                                                                        uint32_t shift, const uint32_t *table, uint32_t n_tiles)
{
    __shared__ uint32_t s_next[SORT_DIGITS];                 /* where the tile's next element with this digit goes */
    __shared__ uint32_t s_wave[BUILD_BLOCK / 64][SORT_DIGITS]; /* this round: elements with this digit in each wave */
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    s_next[threadIdx.x] = table[(size_t)threadIdx.x * n_tiles + blockIdx.x];
    const uint32_t base = blockIdx.x * SORT_TILE;
    for (int r = 0; r < SORT_ITEMS; r += 1)
    {
        for (int w = 0; w < BUILD_BLOCK / 64; w += 1) s_wave[w][threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t i = base + r * BUILD_BLOCK + threadIdx.x;
        const bool valid = i < m;
        uint64_t key = 0;
        uint32_t payload = 0, digit = 0;
        if (valid)
        {
            key = keys[i];
            payload = pos[i];
            digit = (uint32_t)(key >> shift) & 255u;
        }
        /* the lanes of this wave with the same digit, bit by bit */
        unsigned long long peers = __ballot(valid);
        for (int bit = 0; bit < 8; bit += 1)
        {
            const unsigned long long set = __ballot(valid && ((digit >> bit) & 1u));
            peers &= ((digit >> bit) & 1u) ? set : ~set;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) s_wave[wave][digit] = (uint32_t)__popcll(peers); /* one lane per digit and wave */
        __syncthreads();
        if (valid)
        {
            uint32_t at = s_next[digit] + rank;
            for (uint32_t w = 0; w < wave; w += 1) at += s_wave[w][digit];
            keys_out[at] = key;
            pos_out[at] = payload;
        }
        __syncthreads();
        uint32_t all = 0u;
        for (int w = 0; w < BUILD_BLOCK / 64; w += 1) all += s_wave[w][threadIdx.x];
        s_next[threadIdx.x] += all;
        __syncthreads();
    }
}

/* ---- the topology ---- */

struct TopologyTables
{
    const uint64_t *keys;         /* [m] sorted */
    const uint32_t *pos;          /* [m]: the tree position in every leaf slot */
    const uint32_t *tree_surf;    /* [m] */
    const uint32_t *surf_type;    /* DevScene.surf_type */
    BvhNode        *nodes;        /* DevScene.bvh_nodes: child and count are written, the boxes are the leaf and refit kernels' */
    BvhLeafPrim    *leaf;         /* DevScene.bvh_leaf: index and type, and a plane's constants */
    uint32_t       *leaf_parent;  /* [m]: node * 2 + child slot */
    uint32_t       *order;        /* [m]: the surface in every leaf slot, for the host's copy */
    uint2          *levels;       /* [m - 2]: (inner node, parent * 2 + child slot), the deepest level first */
    uint32_t       *level_count;  /* [BUILD_LEVELS + 1] */
    uint32_t        m;
};

/* where level `level` (>= 1) begins in the level table: the table holds the m - 2 inner nodes below the root, the deepest level
 * first, so level 1 ends the table and every level ends where the one above it begins */
__device__ __forceinline__ uint32_t build_level_end(const uint32_t *level_count, uint32_t m, uint32_t level)
{
    uint32_t above = 0u;
    for (uint32_t l = 1; l < level; l += 1) above += level_count[l];
    return (m - 2u) - above;
}

/* the items of level `depth` are complete (an earlier launch wrote them); their inner children are appended to level depth + 1,
 * in any order: nodes and leaves do not depend on it */
__global__ void __launch_bounds__(BUILD_BLOCK) drt_build_topology_kernel(TopologyTables t, const uint4 *items, uint4 *next, uint32_t depth)
{
    const uint32_t n_items = t.level_count[depth];
    const uint32_t next_end = build_level_end(t.level_count, t.m, depth + 1u);
    for (uint32_t k = blockIdx.x * BUILD_BLOCK + threadIdx.x; k < n_items; k += gridDim.x * BUILD_BLOCK)
    {
        const uint4 it = items[k];
        const uint32_t node = it.x, b = it.y, e = it.z;
        const uint32_t mid = build_split(t.keys, b, e, depth);
        for (int c = 0; c < 2; c += 1)
        {
            const uint32_t cb = c ? mid : b, ce = c ? e : mid;
            if (ce - cb == 1u)
            {
                const uint32_t surface = t.tree_surf[t.pos[cb]];
                t.nodes[node].child[c] = build_leaf_ref(cb);
                t.nodes[node].count[c] = 1;
                BvhLeafPrim *lp = t.leaf + cb;
                lp->index = surface;
                lp->type = t.surf_type[surface];
                lp->c32[0] = lp->c32[1] = lp->c32[2] = 0.0f; /* a plane's: drt_bvh_leaf_kernel writes a sphere's */
                lp->reach32 = INFINITY;
                t.leaf_parent[cb] = node * 2u + (uint32_t)c;
                t.order[cb] = surface;
                continue;
            }
            const uint32_t me = build_child_node(node, b, mid, c);
            t.nodes[node].child[c] = (int32_t)me;
            t.nodes[node].count[c] = 0;
            const uint32_t slot = atomicAdd(t.level_count + depth + 1u, 1u);
            next[slot] = make_uint4(me, cb, ce, 0u);
            t.levels[next_end - 1u - slot] = make_uint2(me, node * 2u + (uint32_t)c);
        }
    }
}

/* drt_bvh_refit_kernel for a level whose place in the table only the device knows */
__global__ void __launch_bounds__(BUILD_BLOCK) drt_build_refit_kernel(BvhNode *nodes, const uint2 *levels, const uint32_t *level_count, uint32_t m, uint32_t level)
{
    const uint32_t n_entries = level_count[level];
    const uint2 *entries = levels + (build_level_end(level_count, m, level) - n_entries);
    for (uint32_t k = blockIdx.x * BUILD_BLOCK + threadIdx.x; k < n_entries; k += gridDim.x * BUILD_BLOCK)
    {
        const uint2 e = entries[k];
        const BvhNode *me = nodes + e.x;
        BvhNode *parent = nodes + (e.y >> 1);
        const uint32_t c = e.y & 1u;
        for (int a = 0; a < 3; a += 1)
        {
            parent->lo[c][a] = fminf(me->lo[0][a], me->lo[1][a]);
            parent->hi[c][a] = fmaxf(me->hi[0][a], me->hi[1][a]);
        }
    }
}
