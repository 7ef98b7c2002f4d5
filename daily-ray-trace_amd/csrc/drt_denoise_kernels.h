/*
 * drt_denoise_kernels.h -- the variance-guided denoiser of the spectral film (drt_denoise_film, drt_denoise_buffers). DESIGN.md,
 * section 5b, states the rule; tests/denoise_rule.py restates it in numpy, and these kernels are held to that bit for bit: only
 * + - * / sqrt, every sum sequential in the rule's order, no contraction.
 *
 * Three kernels over a tile_w x tile_h film:
 *   drt_denoise_guide_kernel   per pixel: XYZ of the mean (G), the squared XYZ of the standard error (V), c (c - 1) and the usable
 *                              flag, 64 bytes. 64 pixels per wave, film rows staged through LDS as in drt_converge_kernel.
 *   drt_denoise_weight_kernel  a 16 x 16 pixel tile per workgroup, its guide halo of (16 + 2 (R + F))^2 entries in LDS, one pixel
 *                              per lane: the (2R + 1)^2 weights of the pixel's window and their sum W.
 *   drt_denoise_apply_kernel   lane = wavelength, in sets of 64: an 8 x 8 pixel block per workgroup, 16 pixels per wave one after
 *                              the other. A pixel's weights are wave-uniform (scalar loads); a neighbour's rows are S contiguous
 *                              doubles, and the block's windows overlap, so they come from L2.
 */
#pragma once

#define DENOISE_BLOCK 256
#define DENOISE_WAVES (DENOISE_BLOCK / 64)
#define DENOISE_MAX_S CONVERGE_MAX_S
#define DENOISE_TILE 16        /* the weight kernel's tile side: 256 pixels, one per lane */
#define DENOISE_APPLY_SIDE 8   /* the apply kernel's pixel block side */
#define DENOISE_MAX_RADIUS 10
#define DENOISE_MAX_PATCH 3
#define DENOISE_GUIDE_WORDS 8  /* G[3], V[3], c (c - 1), usable (1.0 / 0.0) */
#define DENOISE_LDS_FIELDS 7   /* what the weight kernel keeps of them: G[3], V[3], usable */

struct DenoiseParams
{
    uint32_t S, tile_w, tile_h, radius, patch, n_window; /* n_window = (2 radius + 1)^2 */
    double   interval, k2, alpha;
    const double *rw, *cx, *cy, *cz; /* the SPD rows cmf_rw, cmf_x, cmf_y, cmf_z */
    const double *pixels, *avgs, *vars; /* the film: [P][S + 1], [P][S], [P][S] */
    double   *guide;    /* [P][DENOISE_GUIDE_WORDS] */
    double   *weights;  /* [P][n_window], window order */
    double   *wsum;     /* [P] */
    double   *mean, *var; /* the result, [P][S] each */
    uint32_t *unusable; /* += pixels that are not usable */
};

__global__ __launch_bounds__(DENOISE_BLOCK) void drt_denoise_guide_kernel(DenoiseParams dp)
{
    __shared__ double s_rows[DENOISE_WAVES][64 * CONVERGE_PAD];
    __shared__ double s_rw[DENOISE_MAX_S], s_c[3][DENOISE_MAX_S];
    const uint32_t S = dp.S;
    const uint64_t n_pix = (uint64_t)dp.tile_w * dp.tile_h;
    for (uint32_t i = threadIdx.x; i < S; i += DENOISE_BLOCK)
    {
        s_rw[i] = dp.rw[i];
        s_c[0][i] = dp.cx[i];
        s_c[1][i] = dp.cy[i];
        s_c[2][i] = dp.cz[i];
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t p = (uint64_t)blockIdx.x * DENOISE_BLOCK + threadIdx.x;
    const uint64_t p0 = (uint64_t)blockIdx.x * DENOISE_BLOCK + wave * 64u; /* the wave's first pixel */
    const bool valid = p < n_pix;
    const unsigned long long valid_mask = __ballot(valid);
    __syncthreads();
    /* the normalisation of drt_film_xyz_kernel, in its order */
    double N = 0.0;
    for (uint32_t i = 0; i < S; i += 1) N += (s_c[1][i] * s_rw[i]);
    N *= dp.interval;
    const double c = valid ? dp.pixels[(size_t)p * (S + 1) + S] : 2.0;
    const double d = c * (c - 1.0);
    double G[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
    double *rows = s_rows[wave];
    for (uint32_t i0 = 0; i0 < S; i0 += CONVERGE_CHUNK)
    {
        const uint32_t w = (S - i0 < CONVERGE_CHUNK) ? S - i0 : CONVERGE_CHUNK;
        /* lanes 16r .. 16r+15 load a 16-double piece of one pixel's row, four rows per load instruction */
        double a_piece[CONVERGE_CHUNK], v_piece[CONVERGE_CHUNK];
#pragma unroll
        for (uint32_t r = 0; r < CONVERGE_CHUNK; r += 1)
        {
            const uint32_t k = r * 64u + lane, row = k / CONVERGE_CHUNK, col = k % CONVERGE_CHUNK;
            const bool ld = ((valid_mask >> row) & 1ull) && col < w;
            const size_t at = (size_t)(p0 + row) * S + i0 + col;
            a_piece[r] = ld ? dp.avgs[at] : 0.0;
            v_piece[r] = ld ? dp.vars[at] : 0.0;
        }
#pragma unroll
        for (uint32_t r = 0; r < CONVERGE_CHUNK; r += 1)
        {
            const uint32_t k = r * 64u + lane;
            rows[(k / CONVERGE_CHUNK) * CONVERGE_PAD + k % CONVERGE_CHUNK] = a_piece[r];
        }
        wave_sync();
        /* the pixel's own sums, sequential over ascending wavelength */
        const double *mine = rows + lane * CONVERGE_PAD;
        if (valid)
            for (uint32_t t = 0; t < w; t += 1)
            {
                const double a = mine[t], white = s_rw[i0 + t];
                G[0] += (s_c[0][i0 + t] * a * white);
                G[1] += (s_c[1][i0 + t] * a * white);
                G[2] += (s_c[2][i0 + t] * a * white);
            }
        wave_sync();
#pragma unroll
        for (uint32_t r = 0; r < CONVERGE_CHUNK; r += 1)
        {
            const uint32_t k = r * 64u + lane;
            rows[(k / CONVERGE_CHUNK) * CONVERGE_PAD + k % CONVERGE_CHUNK] = v_piece[r];
        }
        wave_sync();
        if (valid)
            for (uint32_t t = 0; t < w; t += 1)
            {
                const double r = __builtin_sqrt(mine[t] / d), white = s_rw[i0 + t];
                s[0] += (s_c[0][i0 + t] * r * white);
                s[1] += (s_c[1][i0 + t] * r * white);
                s[2] += (s_c[2][i0 + t] * r * white);
            }
        wave_sync();
    }
    const double scale = dp.interval / N;
    bool ok = c >= 2.0 && c < 4294967296.0 && c == __builtin_floor(c); /* a NaN fails the first comparison */
    double V[3];
    for (int k = 0; k < 3; k += 1)
    {
        G[k] = G[k] * scale;
        s[k] = s[k] * scale;
        V[k] = s[k] * s[k];
        ok = ok && __builtin_isfinite(G[k]) && __builtin_isfinite(V[k]);
    }
    if (valid)
    {
        double *g = dp.guide + (size_t)p * DENOISE_GUIDE_WORDS;
        for (int k = 0; k < 3; k += 1)
        {
            g[k] = G[k];
            g[3 + k] = V[k];
        }
        g[6] = d;
        g[7] = ok ? 1.0 : 0.0;
    }
    const unsigned long long bad = __ballot(valid && !ok);
    if (bad && lane == 0) atomicAdd(dp.unusable, (uint32_t)__popcll(bad));
}

/* e(a, b) of two usable halo entries (rule, step 2): the three channels' distances, summed left to right */
__device__ __forceinline__ double denoise_pair(const double *__restrict__ h, uint32_t n, uint32_t a, uint32_t b, double k2, double alpha)
{
    double e = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < 3; k += 1)
    {
        const double Ga = h[k * n + a], Gb = h[k * n + b], Va = h[(3 + k) * n + a], Vb = h[(3 + k) * n + b];
        const double diff = Ga - Gb;
        const double num = (diff * diff) - (alpha * (Va + (Vb < Va ? Vb : Va)));
        const double den = k2 * (Va + Vb);
        const double delta = den > 0.0 ? num / den : (num <= 0.0 ? 0.0 : __builtin_inf());
        e = k == 0 ? delta : e + delta;
    }
    return e;
}

__device__ __forceinline__ double denoise_falloff(double x) /* (x < 1) ? (1 - max(x, 0))^2 : 0; a NaN gives 0 */
{
    const double t = 1.0 - (x > 0.0 ? x : 0.0);
    return x < 1.0 ? t * t : 0.0;
}

/* blockDim = (16, 16); dynamic LDS: DENOISE_LDS_FIELDS * side^2 doubles, side = 16 + 2 (radius + patch); field-major, so that the
 * lanes of a row read neighbouring words */
__global__ __launch_bounds__(DENOISE_BLOCK) void drt_denoise_weight_kernel(DenoiseParams dp)
{
    extern __shared__ double dn_halo[];
    const int R = (int)dp.radius, F = (int)dp.patch, B = R + F;
    const int side = DENOISE_TILE + 2 * B;
    const uint32_t n = (uint32_t)(side * side);
    const int W = (int)dp.tile_w, H = (int)dp.tile_h;
    const int x0 = (int)blockIdx.x * DENOISE_TILE - B, y0 = (int)blockIdx.y * DENOISE_TILE - B;
    const uint32_t tid = threadIdx.y * DENOISE_TILE + threadIdx.x;
    for (uint32_t at = tid; at < n; at += DENOISE_BLOCK)
    {
        const int x = x0 + (int)(at % (uint32_t)side), y = y0 + (int)(at / (uint32_t)side);
        const bool in = x >= 0 && x < W && y >= 0 && y < H;
        const double *g = dp.guide + ((size_t)(in ? y : 0) * W + (in ? x : 0)) * DENOISE_GUIDE_WORDS;
#pragma unroll
        for (uint32_t k = 0; k < 6; k += 1) dn_halo[k * n + at] = in ? g[k] : 0.0;
        dn_halo[6 * n + at] = in ? g[7] : 0.0; /* outside the tile: as an unusable pixel, it never counts */
    }
    __syncthreads();
    const int px = (int)(blockIdx.x * DENOISE_TILE + threadIdx.x), py = (int)(blockIdx.y * DENOISE_TILE + threadIdx.y);
    if (px >= W || py >= H) return;
    const double *flag = dn_halo + 6 * n;
    const int pc = ((int)threadIdx.y + B) * side + (int)threadIdx.x + B;
    const bool p_ok = flag[pc] != 0.0;
    const size_t p = (size_t)py * W + px;
    double *wrow = dp.weights + p * dp.n_window;
    double Wsum = 0.0;
    uint32_t qi = 0;
    for (int dy = -R; dy <= R; dy += 1)
        for (int dx = -R; dx <= R; dx += 1, qi += 1)
        {
            const int qc = pc + dy * side + dx;
            double w = 0.0;
            if (p_ok && flag[qc] != 0.0)
            {
                double total = 0.0, cnt = 0.0;
                for (int oy = -F; oy <= F; oy += 1)
                    for (int ox = -F; ox <= F; ox += 1)
                    {
                        const int o = oy * side + ox;
                        if (flag[pc + o] != 0.0 && flag[qc + o] != 0.0)
                        {
                            total = total + denoise_pair(dn_halo, n, (uint32_t)(pc + o), (uint32_t)(qc + o), dp.k2, dp.alpha);
                            cnt += 1.0;
                        }
                    }
                const double D = total / (3.0 * cnt);
                const double Dc = denoise_pair(dn_halo, n, (uint32_t)pc, (uint32_t)qc, dp.k2, dp.alpha) / 3.0;
                const double fD = denoise_falloff(D), fc = denoise_falloff(Dc);
                w = fc < fD ? fc : fD;
            }
            wrow[qi] = w;
            Wsum = Wsum + w;
        }
    dp.wsum[p] = Wsum;
}

/* grid = (ceil(tile_w / 8), ceil(tile_h / 8)): wave k of a block takes rows 2k, 2k + 1 of its 8 x 8 pixels, one pixel at a time */
__global__ __launch_bounds__(DENOISE_BLOCK) void drt_denoise_apply_kernel(DenoiseParams dp)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint32_t S = dp.S;
    const int W = (int)dp.tile_w, H = (int)dp.tile_h, R = (int)dp.radius;
    for (uint32_t j = 0; j < 2 * DENOISE_APPLY_SIDE; j += 1)
    {
        const int x = (int)(blockIdx.x * DENOISE_APPLY_SIDE + (j & (DENOISE_APPLY_SIDE - 1)));
        const int y = (int)(blockIdx.y * DENOISE_APPLY_SIDE + 2 * wave + j / DENOISE_APPLY_SIDE);
        if (x >= W || y >= H) continue; /* wave-uniform */
        const size_t p = (size_t)y * W + x;
        const double *g = dp.guide + p * DENOISE_GUIDE_WORDS;
        const double cc = g[6];
        const bool usable = g[7] != 0.0;
        const double *wrow = dp.weights + p * dp.n_window;
        const double Wsum = dp.wsum[p];
        for (uint32_t i = lane; i < S; i += 64u)
        {
            if (!usable) /* passes through: the mean as it is, the variance of the mean whatever IEEE gives */
            {
                dp.mean[p * S + i] = dp.avgs[p * S + i];
                dp.var[p * S + i] = dp.vars[p * S + i] / cc;
                continue;
            }
            double am = 0.0, av = 0.0;
            uint32_t qi = 0;
            for (int dy = -R; dy <= R; dy += 1)
                for (int dx = -R; dx <= R; dx += 1, qi += 1)
                {
                    const double w = wrow[qi];
                    const int qx = x + dx, qy = y + dy;
                    /* a term of weight 0 adds a zero to a sum that is never -0: leaving it out changes no bit (only pixels inside
                     * the tile have a weight other than 0) */
                    if (w == 0.0 || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qy * W + qx;
                    const double ccq = dp.guide[q * DENOISE_GUIDE_WORDS + 6];
                    am = am + (w * dp.avgs[q * S + i]);
                    av = av + ((w * w) * (dp.vars[q * S + i] / ccq));
                }
            dp.mean[p * S + i] = am / Wsum;
            dp.var[p * S + i] = av / (Wsum * Wsum);
        }
    }
}
