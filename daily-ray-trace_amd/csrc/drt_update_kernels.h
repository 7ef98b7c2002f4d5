/*
 * drt_update_kernels.h -- scene updates of a live context (include/drt_hip.h: drt_update_surfaces, drt_set_camera).
 *
 * A pass of its own beside the render path: it rewrites, in place and on the context's stream, the four device tables everything
 * that depends on geometry is read from -- DevScene.surf, DevScene.lights, DevScene.bvh_leaf and the boxes in DevScene.bvh_nodes --
 * from the caller's raw drt_surface records. No render, feature, matte or ray kernel knows of it.
 *
 *   drt_surface_derive_kernel   one lane per surface: the SF_* columns, the LF_* column of an emissive surface, the surface's box
 *                               and its share of the extent, as build_device_scene and prim_bounds (drt_launcher.hip) compute them:
 *                               the same operations in the same order, + - * / sqrt fabs only, no contraction, so
 *                               the columns equal the host's bit for bit
 *   drt_bvh_leaf_kernel         one lane per leaf slot, after the extent is final: the BvhLeafPrim and the leaf's padded f32 box
 *                               in its parent's child slot
 *   drt_bvh_refit_kernel        one launch per tree level, deepest first: the union of a node's two child boxes into its parent
 *
 * Kernel boundaries are the only hand-off between the three: no counter, flag or waiting lane crosses workgroups.
 */
#pragma once

#include "drt_kernels.h"

#define UPDATE_BLOCK 256
#define UPDATE_EXTENT_LIMIT 134217728.0 /* 2^27: what the hierarchy's f32 box test holds (drt_kernels.h, bvh_inv32) */

/* a drt_surface as 14 doubles: word 0 holds type and material (not read: they cannot change), then position, radius, normal, u, v */
#define RAW_WORDS 14
#define RAW_POS 1
#define RAW_RADIUS 4
#define RAW_NORMAL 5
#define RAW_U 8
#define RAW_V 11

/* status words of an update, zeroed before the derive kernel: +0 the bit pattern of the largest |coordinate| of the surfaces' boxes
 * (a non-negative double: its bit pattern orders like the number), +1 nonzero when that reached UPDATE_EXTENT_LIMIT */
#define UPD_STATUS_WORDS 2

struct UpdateTables
{
    const double   *raw;        /* [n_surf][RAW_WORDS] */
    double         *surf;       /* DevScene.surf */
    double         *lights;     /* DevScene.lights */
    const int32_t  *light_slot; /* [n_surf]: the surface's column of `lights`, -1 when it is no light */
    double         *boxes;      /* [n_surf][6] lo, hi: hierarchy contexts only (else NULL) */
    unsigned long long *status; /* UPD_STATUS_WORDS */
};

/* std::min / std::max as prim_bounds uses them: the FIRST argument stays when the comparison is false (a NaN included) */
__device__ __forceinline__ double upd_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double upd_max(double a, double b) { return a < b ? b : a; }

/* prim_bounds (drt_launcher.hip), operation for operation */
__device__ __forceinline__ void upd_prim_bounds(uint32_t type, const double *r, double lo[3], double hi[3])
{
    if (type == DRT_GEO_SPHERE)
    {
        for (int k = 0; k < 3; k += 1)
        {
            lo[k] = r[RAW_POS + k] - __builtin_fabs(r[RAW_RADIUS]);
            hi[k] = r[RAW_POS + k] + __builtin_fabs(r[RAW_RADIUS]);
        }
    }
    else
    {
        const double *u = r + RAW_U, *v = r + RAW_V, *n = r + RAW_NORMAL;
        const double ul = __builtin_sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), vl = __builtin_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const double un[3] = {u[0] / ul, u[1] / ul, u[2] / ul}, vn[3] = {v[0] / vl, v[1] / vl, v[2] / vl};
        const double c0[3] = {vn[1] * n[2] - vn[2] * n[1], vn[2] * n[0] - vn[0] * n[2], vn[0] * n[1] - vn[1] * n[0]};
        const double c1[3] = {n[1] * un[2] - n[2] * un[1], n[2] * un[0] - n[0] * un[2], n[0] * un[1] - n[1] * un[0]};
        const double det = un[0] * c0[0] + un[1] * c0[1] + un[2] * c0[2];
        const bool ok = isfinite(det) && __builtin_fabs(det) > 1e-6 && isfinite(ul) && isfinite(vl);
        for (int k = 0; k < 3; k += 1)
        {
            lo[k] = HUGE_VAL;
            hi[k] = -HUGE_VAL;
        }
        if (ok)
            for (int corner = 0; corner < 4; corner += 1)
            {
                const double a = (corner & 1) ? ul : 0.0, b = (corner & 2) ? vl : 0.0;
                for (int k = 0; k < 3; k += 1)
                {
                    const double j = (a * c0[k] + b * c1[k]) / det;
                    lo[k] = upd_min(lo[k], r[RAW_POS + k] + j);
                    hi[k] = upd_max(hi[k], r[RAW_POS + k] + j);
                }
            }
        else
            for (int k = 0; k < 3; k += 1)
            {
                lo[k] = -1e300;
                hi[k] = 1e300;
            }
    }
    for (int k = 0; k < 3; k += 1)
    {
        const double pad = 1e-5 + 1e-9 * upd_max(__builtin_fabs(lo[k]), __builtin_fabs(hi[k]));
        lo[k] -= pad;
        hi[k] += pad;
    }
}

__global__ void __launch_bounds__(UPDATE_BLOCK) drt_surface_derive_kernel(DevScene sc, UpdateTables t)
{
    const uint32_t i = blockIdx.x * UPDATE_BLOCK + threadIdx.x;
    const uint32_t n = sc.n_surf;
    double reach = 0.0; /* this surface's share of the extent */
    if (i < n)
    {
        double r[RAW_WORDS];
        for (int k = 1; k < RAW_WORDS; k += 1) r[k] = t.raw[(size_t)i * RAW_WORDS + k];
        const uint32_t type = sc.surf_type[i];
        double *surf = t.surf;
        surf[(size_t)SF_PX * n + i] = r[RAW_POS];
        surf[(size_t)SF_PY * n + i] = r[RAW_POS + 1];
        surf[(size_t)SF_PZ * n + i] = r[RAW_POS + 2];
        surf[(size_t)SF_RADIUS * n + i] = r[RAW_RADIUS];
        const double *u = r + RAW_U, *v = r + RAW_V;
        if (type == DRT_GEO_PLANE)
        {
            const double ul = __builtin_sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), vl = __builtin_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            for (int k = 0; k < 3; k += 1)
            {
                surf[(size_t)(SF_NX + k) * n + i] = r[RAW_NORMAL + k];
                surf[(size_t)(SF_UNX + k) * n + i] = u[k] / ul;
                surf[(size_t)(SF_VNX + k) * n + i] = v[k] / vl;
            }
            surf[(size_t)SF_ULEN * n + i] = ul;
            surf[(size_t)SF_VLEN * n + i] = vl;
        }
        const int32_t l = t.light_slot[i];
        if (l >= 0)
        {
            const uint32_t nl = sc.n_lights;
            double *lights = t.lights;
            for (int k = 0; k < 3; k += 1)
            {
                lights[(size_t)(LF_PX + k) * nl + l] = r[RAW_POS + k];
                lights[(size_t)(LF_UX + k) * nl + l] = u[k];
                lights[(size_t)(LF_VX + k) * nl + l] = v[k];
            }
            lights[(size_t)LF_RADIUS * nl + l] = r[RAW_RADIUS];
            double pdf = 1.0;
            if (type == DRT_GEO_SPHERE) pdf = ((4.0 * DRT_PI) * r[RAW_RADIUS]) * r[RAW_RADIUS];
            else if (type == DRT_GEO_PLANE)
            {
                const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
                pdf = __builtin_sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            }
            lights[(size_t)LF_PDF * nl + l] = pdf;
        }
        if (t.boxes && (type == DRT_GEO_SPHERE || type == DRT_GEO_PLANE)) /* points are never intersected: no box, no share */
        {
            double lo[3], hi[3];
            upd_prim_bounds(type, r, lo, hi);
            for (int k = 0; k < 3; k += 1)
            {
                t.boxes[(size_t)i * 6 + k] = lo[k];
                t.boxes[(size_t)i * 6 + 3 + k] = hi[k];
                if (__builtin_fabs(lo[k]) < 1e299) reach = upd_max(reach, __builtin_fabs(lo[k]));
                if (__builtin_fabs(hi[k]) < 1e299) reach = upd_max(reach, __builtin_fabs(hi[k]));
            }
        }
    }
    if (!t.boxes) return; /* (uniform: a kernel argument) */
    /* the wave's maximum, then one atomic per wave on the bit pattern: shares are finite and >= +0, so the patterns order like them */
    for (int off = 32; off > 0; off >>= 1) reach = upd_max(reach, __shfl_xor(reach, off, 64));
    if ((threadIdx.x & 63u) == 0u && reach > 0.0)
    {
        atomicMax(t.status + 0, (unsigned long long)__double_as_longlong(reach));
        if (!(reach < UPDATE_EXTENT_LIMIT)) atomicOr(t.status + 1, 1ull);
    }
}

struct LeafTables
{
    const double   *raw;          /* [n_surf][RAW_WORDS] */
    const double   *boxes;        /* [n_surf][6] */
    const uint32_t *leaf_parent;  /* [n_leaf]: node * 2 + child slot the leaf hangs in */
    BvhLeafPrim    *leaf;         /* DevScene.bvh_leaf: index and type stay as the host wrote them */
    BvhNode        *nodes;        /* DevScene.bvh_nodes */
    const unsigned long long *status;
};

/* a double to f32, rounded towards -inf / +inf: the stored box must contain the f64 box */
__device__ __forceinline__ float upd_f32_down(double x)
{
    float f = __double2float_rd(x);
    if ((double)f > x) f = nextafterf(f, -INFINITY);
    return f;
}
__device__ __forceinline__ float upd_f32_up(double x)
{
    float f = __double2float_ru(x);
    if ((double)f < x) f = nextafterf(f, INFINITY);
    return f;
}

__global__ void __launch_bounds__(UPDATE_BLOCK) drt_bvh_leaf_kernel(LeafTables t, uint32_t n_leaf, double camera_reach)
{
    const uint32_t k = blockIdx.x * UPDATE_BLOCK + threadIdx.x;
    if (k >= n_leaf) return;
    /* the extent the hierarchy holds for: the camera's reach and the surfaces' boxes (BvhBuilder::build) */
    const double extent = upd_max(camera_reach, __longlong_as_double((long long)t.status[0]));
    BvhLeafPrim *lp = t.leaf + k;
    const uint32_t i = lp->index;
    const double *r = t.raw + (size_t)i * RAW_WORDS;
    for (int f = 0; f < 4; f += 1) lp->f[f] = r[RAW_POS + f]; /* position, radius */
    if (lp->type == DRT_GEO_SPHERE)
    {
        for (int f = 0; f < 3; f += 1) lp->c32[f] = (float)r[RAW_POS + f];
        lp->reach32 = bvh_sphere_reach32(r[RAW_RADIUS], extent);
    }
    /* the leaf's box, padded by 2^-19 extent for the f32 test (BvhBuilder::set_child) */
    const double pad32 = extent * 0x1p-19;
    const uint32_t pc = t.leaf_parent[k];
    BvhNode *node = t.nodes + (pc >> 1);
    const uint32_t c = pc & 1u;
    for (int a = 0; a < 3; a += 1)
    {
        node->lo[c][a] = upd_f32_down(t.boxes[(size_t)i * 6 + a] - pad32);
        node->hi[c][a] = upd_f32_up(t.boxes[(size_t)i * 6 + 3 + a] + pad32);
    }
}

/* entries of ONE level: inner node `x` hangs in child slot (y & 1) of node (y >> 1), which is one level up. The node's own two child
 * boxes are final: leaves were written by drt_bvh_leaf_kernel, inner children by the launch of the level below. A union of f32 boxes
 * is exact; a NaN bound (a surface no ray can hit) is passed over, as std::min / std::max pass over it in BvhBuilder::bounds. */
__global__ void __launch_bounds__(UPDATE_BLOCK) drt_bvh_refit_kernel(BvhNode *nodes, const uint2 *entries, uint32_t n_entries)
{
    const uint32_t k = blockIdx.x * UPDATE_BLOCK + threadIdx.x;
    if (k >= n_entries) return;
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
