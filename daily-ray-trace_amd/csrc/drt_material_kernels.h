/*
 * drt_material_kernels.h -- material updates of a live context (include/drt_hip.h: drt_update_spectra, drt_update_materials;
 * DESIGN.md 5i).
 *
 * A pass of its own beside the render path: it rewrites, in place and on the context's stream, the three device tables everything
 * spectral is read from -- DevScene.spds with its derived rows, DevMaterial.refract_i0 / refract_i1 in DevScene.mats, and the trace
 * kernel's tail columns -- from the caller's raw SPD rows. No render, feature, matte, ray, adaptive or denoise kernel knows of it.
 *
 *   drt_spectra_derive_kernel   one lane per (row, wavelength) of the device table. A caller's row inside the updated range is copied
 *                               from `src` into the context's raw copy and into the table; a derived row is computed as
 *                               build_device_scene (drt_launcher.hip) computes it: the same operations in the same order, * / - only,
 *                               no contraction, so the table equals a fresh context's bit for bit. A derived row's
 *                               operands inside the updated range are read from `src`, the others from the raw copy: no lane reads
 *                               what another lane of the launch writes.
 *   drt_spectra_finish_kernel   after the table is final: the two samples around 630 nm of every material with a refract row, and
 *                               (trace_tail contexts) the tail columns
 *
 * The kernel boundary is the only hand-off between the two: no counter, flag or waiting lane crosses workgroups.
 */
#pragma once

#include "drt_kernels.h"

#define MATERIAL_BLOCK 256

/* what a row of the device table is made from (SpdRowDesc.kind); a source row of -1 is a spectrum that is not given: zeros */
#define SPD_ROW_SCENE 0u       /* the caller's row a */
#define SPD_ROW_DIFFUSE_PI 1u  /* a * (1 / PI) */
#define SPD_ROW_REL_SQ 2u      /* rel * rel, rel = a / b */
#define SPD_ROW_CONDUCTOR_A 3u /* rr_sq - re_sq, rr = a / c, re = b / c */
#define SPD_ROW_CONDUCTOR_B 4u /* 4.0 * rr_sq * re_sq */
#define SPD_ROW_ZERO 5u        /* the all-zero row: stays */

struct SpdRowDesc
{
    uint32_t kind;
    int32_t  a, b, c; /* scene rows (drt_scene.spds numbering) */
};

struct SpectraTables
{
    const double     *src;   /* [count][S]: the new values of scene rows [first_row, first_row + count) */
    double           *raw;   /* [n_scene][S]: the caller's rows as the context holds them */
    double           *table; /* DevScene.spds */
    const SpdRowDesc *desc;  /* [n_spd] */
    uint32_t first_row, count, n_spd, S;
};

/* scene row r at wavelength k as it will be after this update (never from a word this launch writes) */
__device__ __forceinline__ double spectra_at(const SpectraTables &t, int32_t r, uint32_t k)
{
    if (r < 0) return 0.0;
    const uint32_t ur = (uint32_t)r;
    if (ur >= t.first_row && ur - t.first_row < t.count) return t.src[(size_t)(ur - t.first_row) * t.S + k];
    return t.raw[(size_t)ur * t.S + k];
}

__global__ void __launch_bounds__(MATERIAL_BLOCK) drt_spectra_derive_kernel(SpectraTables t)
{
    const uint64_t i = (uint64_t)blockIdx.x * MATERIAL_BLOCK + threadIdx.x;
    if (i >= (uint64_t)t.n_spd * t.S) return;
    const uint32_t row = (uint32_t)(i / t.S), k = (uint32_t)(i % t.S);
    const SpdRowDesc d = t.desc[row];
    if (d.kind == SPD_ROW_SCENE)
    {
        const uint32_t r = (uint32_t)d.a;
        if (r >= t.first_row && r - t.first_row < t.count)
        {
            const double v = t.src[(size_t)(r - t.first_row) * t.S + k];
            t.raw[(size_t)r * t.S + k] = v;
            t.table[i] = v;
        }
    }
    else if (d.kind == SPD_ROW_DIFFUSE_PI)
    {
        const double inv_pi = 1.0 / DRT_PI;
        t.table[i] = spectra_at(t, d.a, k) * inv_pi;
    }
    else if (d.kind == SPD_ROW_REL_SQ)
    {
        const double rel = spectra_at(t, d.a, k) / spectra_at(t, d.b, k);
        t.table[i] = rel * rel;
    }
    else if (d.kind == SPD_ROW_CONDUCTOR_A || d.kind == SPD_ROW_CONDUCTOR_B)
    {
        const double ir = spectra_at(t, d.c, k), rr = spectra_at(t, d.a, k) / ir, re = spectra_at(t, d.b, k) / ir;
        const double rr_sq = rr * rr, re_sq = re * re;
        t.table[i] = d.kind == SPD_ROW_CONDUCTOR_A ? rr_sq - re_sq : 4.0 * rr_sq * re_sq;
    }
}

struct SpectraFinish
{
    const double  *table;       /* DevScene.spds, final */
    DevMaterial   *mats;        /* DevScene.mats */
    const int32_t *mat_refract; /* [n_mat]: the material's refract row in the table, -1 when it has none */
    double        *tail;        /* [n_spd][tail_count] or NULL */
    uint32_t n_mat, n_spd, S, trans_i0, tail_first, tail_count;
};

__global__ void __launch_bounds__(MATERIAL_BLOCK) drt_spectra_finish_kernel(SpectraFinish f)
{
    const uint64_t i = (uint64_t)blockIdx.x * MATERIAL_BLOCK + threadIdx.x;
    if (i < f.n_mat)
    {
        const int32_t r = f.mat_refract[i];
        if (r >= 0)
        {
            f.mats[i].refract_i0 = f.table[(size_t)r * f.S + f.trans_i0];
            f.mats[i].refract_i1 = f.table[(size_t)r * f.S + f.trans_i0 + 1];
        }
        return;
    }
    const uint64_t j = i - f.n_mat;
    if (!f.tail || j >= (uint64_t)f.n_spd * f.tail_count) return;
    const uint32_t r = (uint32_t)(j / f.tail_count), c = (uint32_t)(j % f.tail_count);
    f.tail[j] = f.table[(size_t)r * f.S + f.tail_first + c];
}
