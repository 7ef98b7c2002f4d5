/*
 * drt_build_rule.h -- the rule a device-built hierarchy follows (include/drt_hip.h: drt_rebuild_hierarchy): a surface's
 * sort key, where a range of the sorted keys is split, and how the nodes are numbered. The tree is a function of the surfaces' boxes
 * alone, so tests/hierarchy_rule.py restates it in numpy and holds the device to it byte for byte.
 *
 * No HIP include: drt_build_kernels.h compiles this text for the device, tests/host/hierarchy_rule_main.cpp for the host.
 */
#pragma once

#include <stdint.h>

#ifndef DRT_RULE_FN
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRT_RULE_FN __host__ __device__ inline
#else
#define DRT_RULE_FN inline
#endif
#endif

#define BUILD_KEY_BITS 21                          /* per axis */
#define BUILD_KEY_UNBOUNDED 0x7FFFFFFFFFFFFFFFull  /* a surface with an unbounded box: behind every bounded one */
#define BUILD_RULE_STACK 32                        /* BVH_STACK (drt_kernels.h): the levels a traversal stack holds */

/* a box value the builder takes for bounded (BvhBuilder::build, drt_launcher.hip); false for a NaN */
DRT_RULE_FN bool build_bounded(double x) { return (x < 0.0 ? -x : x) < 1e299; }

/* A leaf sphere's reach for the f32 filter (drt_kernels.h, sphere_certainly_missed): |radius| + 64 u E = 2^-18 E, E the extent the
 * hierarchy holds for, to f32 and then up by two f32 steps. The one statement of the pad: build_device_scene, drt_bvh_leaf_kernel and
 * drt_selftest_unit's function 14 call it. */
DRT_RULE_FN float build_f32_up(float x) /* nextafterf(x, +inf), without an include: +inf and NaN stay, +-0 give the least subnormal */
{
    if (!(x <= 3.402823466e+38f)) return x;
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    u = x == 0.0f ? 1u : x > 0.0f ? u + 1u : u - 1u;
    __builtin_memcpy(&x, &u, 4);
    return x;
}
DRT_RULE_FN float bvh_sphere_reach32(double radius, double extent)
{
    const float reach = (float)((radius < 0.0 ? -radius : radius) + extent * 3.814697265625e-06 /* 2^-18 */);
    return build_f32_up(build_f32_up(reach));
}

/* the centre of a bounded surface's box along one axis, on the 2^21 grid between the smallest and the largest centre: - / * only */
DRT_RULE_FN uint32_t build_quantise(double c, double clo, double chi)
{
    const double ext = chi - clo;
    if (!(ext > 0.0)) return 0u;
    const uint32_t q = (uint32_t)((c - clo) / ext * 2097152.0);
    return q < 2097151u ? q : 2097151u;
}

/* bit b of v to bit 3 b */
DRT_RULE_FN uint64_t build_spread3(uint32_t v)
{
    uint64_t x = (uint64_t)v & 0x1FFFFFull;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

/* 63 bits: bit 3 b + 2 is x's bit b, 3 b + 1 y's, 3 b z's */
DRT_RULE_FN uint64_t build_key(uint32_t qx, uint32_t qy, uint32_t qz) { return (build_spread3(qx) << 2) | (build_spread3(qy) << 1) | build_spread3(qz); }

/* Where the range [b, e) of the sorted keys (e - b >= 2) is split, for the inner node `depth` levels below the root: at the first key
 * that has the highest bit in which the range's first and last key differ, while a median-split subtree below the node's children
 * would still fit the traversal stack (BvhBuilder::split's budget, word for word); at the middle otherwise, and where all keys are
 * equal. A tree deeper than the stack cannot come out. */
DRT_RULE_FN uint32_t build_split(const uint64_t *key, uint32_t b, uint32_t e, uint32_t depth)
{
    uint32_t log2m = 0;
    while (((uint32_t)1 << log2m) < e - b) log2m += 1;
    const uint64_t first = key[b], diff = first ^ key[e - 1];
    if (!(depth + 2 + log2m < BUILD_RULE_STACK) || diff == 0ull) return b + (e - b) / 2;
    int top = 63;
    while (!((diff >> top) & 1ull)) top -= 1;
    /* keys ascend and agree above `top`: those without the bit come first. The first with it, by bisection: key[lo] has it not, key[hi] has */
    uint32_t lo = b, hi = e - 1;
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((key[mid] >> top) & 1ull) hi = mid;
        else lo = mid;
    }
    return hi;
}

/* Numbering: pre-order, the root 0. Node `node` over [b, e) split at mid: a child over one surface is the leaf of that slot, an inner
 * child over [cb, ce) is node + 1 on the left and node + (mid - b) on the right (a subtree over n surfaces has n - 1 nodes). */
DRT_RULE_FN int32_t build_leaf_ref(uint32_t slot) { return -2 - (int32_t)(slot * 8u); }
DRT_RULE_FN uint32_t build_child_node(uint32_t node, uint32_t b, uint32_t mid, int c) { return c == 0 ? node + 1u : node + (mid - b); }

/* the whole topology on one thread (the host program, and the statement of what the level-by-level kernel must equal):
 * child[2 i + c] and count[2 i + c] of the max(m - 1, 1) nodes; returns the levels of the tree as BvhBuilder counts them */
DRT_RULE_FN uint32_t build_topology_serial(const uint64_t *key, uint32_t m, int32_t *child, int32_t *count)
{
    child[0] = child[1] = -1;
    count[0] = count[1] = -1;
    if (m == 0u) return 0u;
    if (m == 1u)
    {
        child[0] = build_leaf_ref(0u);
        count[0] = 1;
        return 1u;
    }
    /* an explicit stack: one entry per level at most besides the node in hand */
    uint32_t st_node[BUILD_RULE_STACK + 1], st_b[BUILD_RULE_STACK + 1], st_e[BUILD_RULE_STACK + 1], st_d[BUILD_RULE_STACK + 1];
    uint32_t sp = 0, levels = 0;
    st_node[0] = 0u; st_b[0] = 0u; st_e[0] = m; st_d[0] = 0u;
    sp = 1;
    while (sp > 0)
    {
        sp -= 1;
        const uint32_t node = st_node[sp], b = st_b[sp], e = st_e[sp], d = st_d[sp];
        const uint32_t mid = build_split(key, b, e, d);
        if (d + 1u > levels) levels = d + 1u;
        for (int c = 1; c >= 0; c -= 1)
        {
            const uint32_t cb = c ? mid : b, ce = c ? e : mid;
            if (ce - cb == 1u)
            {
                child[2u * node + c] = build_leaf_ref(cb);
                count[2u * node + c] = 1;
                continue;
            }
            child[2u * node + c] = (int32_t)build_child_node(node, b, mid, c);
            count[2u * node + c] = 0;
            st_node[sp] = build_child_node(node, b, mid, c); st_b[sp] = cb; st_e[sp] = ce; st_d[sp] = d + 1u;
            sp += 1;
        }
    }
    return levels;
}
