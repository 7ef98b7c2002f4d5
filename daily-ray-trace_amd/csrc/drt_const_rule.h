/*
 * drt_const_rule.h -- quotients whose divisor is a constant, formed without a division in the path loop.
 *
 * Plain C++, no HIP: the kernels (drt_device.h, drt_kernels.h) and the launcher include it, and a host program runs the very same
 * text (tests/host/const_rule_main.cpp). Like everything else it is compiled without floating-point contraction: every fma below
 * is written out, every other operation is rounded on its own.
 *
 * 1. The draw's quotient, n / (2^31 - 1) for the 31-bit integer n a draw takes from the generator's state (drt_rng).
 * 2. The glass constants of a material: its refractive index at the scene's trans_wl and the quotients ir / tr of the pair of media
 *    (base material, this material), which every glass vertex of a frame would otherwise divide out again.
 */
#ifndef DRT_CONST_RULE_H
#define DRT_CONST_RULE_H

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRT_CONST_FN __host__ __device__ __forceinline__
#else
#define DRT_CONST_FN static inline
#endif

/* ---- n / (2^31 - 1) ----------------------------------------------------------------------------------------------------------
 * With M = 2^31 - 1 and R = RN(1 / M) = 2^-31 + 2^-62 (1 / M = 2^-31 + 2^-62 + 2^-93 + ..., the next term lies below R's last bit):
 *     y = n 2^-31            exact: a power of two
 *     q = fma(y, R, y)       y (1 + R), rounded once
 * n / M = y / (1 - 2^-31) = y (1 + 2^-31 + 2^-62 + 2^-93 + ...), so before its one rounding q is the quotient short of y 2^-93 and a
 * little: a relative error near 2^-93. The quotient itself cannot lie that close to where rounding to 53 bits turns over: 2^31 = 1
 * (mod M), so the binary digits of n / M are n's 31 digits repeated for ever, and the digits behind the 53rd are neither forty zeros
 * nor forty ones unless n = 0 (q = +0, like 0 / M) or n = M (q = RN(1 - 2^-93) = 1, like M / M). So q = RN(n / M) for EVERY n in
 * [0, 2^31) -- and since an argument is no test, all of them are run against `/` (tests/test_const_rule_cpu.py).
 * (The textbook form -- y = RN(n R), r = fma(-y, M, n), q = fma(r, R, y) -- gives the same bits in three operations and two
 * constants that are not inline operands; this one needs two operations and one.) */
#define DRT_DRAW_DIVISOR 2147483647.0
#define DRT_DRAW_RECIPROCAL 0x1.00000002p-31
static_assert(DRT_DRAW_RECIPROCAL == 1.0 / DRT_DRAW_DIVISOR, "R is the double nearest 1 / (2^31 - 1)");

DRT_CONST_FN double drt_draw_quotient(uint32_t n)
{
    const double y = (double)n * 0x1p-31;
    return __builtin_fma(y, DRT_DRAW_RECIPROCAL, y);
}

/* ---- glass constants ---------------------------------------------------------------------------------------------------------
 * What vertex_dirs and the reflect-or-transmit sampler (drt_kernels.h) compute per vertex from values that are the scene's:
 *   - a material's refractive index at trans_wl: value_at_wl's lerp between the two samples i0, i1 of its refraction spectrum that
 *     bracket trans_wl (drt_lerp, drt_device.h; src/utils.c:1-4 as src/spectrum.c:150-162 calls it), and
 *   - rel = ir / tr (vec3_transmit, src/geometry.c:96; fs_dielectric_reflectance, src/bdsf.c:52) at i0, at i1 and at trans_wl, for the
 *     two orientations the pair rows distinguish: `out`, incident = the base material and transmit = this one, and `in`, the reverse.
 * The very operations in the very order of those expressions, each rounded on its own: the same bits. Nothing is special-cased: equal
 * indices give 1, a zero index gives inf or NaN, a missing spectrum (i0 = i1 = 0) gives 0 / 0 = NaN, w0 == w1 gives (y1 - y0) / 0 --
 * whatever the expressions give per vertex. */
struct DrtGlassConst
{
    double at_wl;      /* the material's index at trans_wl */
    double rel_out[3]; /* base / this at i0, i1, trans_wl */
    double rel_in[3];  /* this / base at i0, i1, trans_wl */
};

DRT_CONST_FN double drt_glass_index(double wl, double w0, double w1, double i0, double i1)
{
    return i0 + ((wl - w0) * ((i1 - i0) / (w1 - w0)));
}

DRT_CONST_FN DrtGlassConst drt_glass_constants(double wl, double w0, double w1, double base_i0, double base_i1, double i0, double i1)
{
    DrtGlassConst g;
    const double base_wl = drt_glass_index(wl, w0, w1, base_i0, base_i1);
    g.at_wl = drt_glass_index(wl, w0, w1, i0, i1);
    g.rel_out[0] = base_i0 / i0;
    g.rel_out[1] = base_i1 / i1;
    g.rel_out[2] = base_wl / g.at_wl;
    g.rel_in[0] = i0 / base_i0;
    g.rel_in[1] = i1 / base_i1;
    g.rel_in[2] = g.at_wl / base_wl;
    return g;
}

#endif
