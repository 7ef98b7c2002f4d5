/*
 * drt_pair_rule.h -- the plan of a kernel pair: what a caller asks for (PairSpan), the tile its trace launch sees (TraceTile), where its
 * pixels lie in the film and in the live window's staging film (PairGeometry), and the shapes of its two work queues.
 *
 * Plain C++, no HIP: the launcher (drt_launcher.hip: enqueue_pair, enqueue_trace, window_copy, create_impl and the callers that split
 * a call into pairs) launches from what these rules return, and a host program can run the very same text (tests/host). Constants the
 * kernels share (TRACE_BLOCK, SHADE_WAVES, SHADE_PIXEL_CHUNK) come in as arguments. Films are bit-identical whatever the shaping
 * rules return; only the benchmark sees them change, which is why they are held to their figures here, number for number.
 */
#ifndef DRT_PAIR_RULE_H
#define DRT_PAIR_RULE_H

#include <algorithm>
#include <cstdint>

#include "drt_hip.h"

/* ---- what a caller asks for ---- */

/* Samples [first_sample, first_sample + n_samples) of tile rows [row0, row0 + rows), or of the pixels of a list. */
struct PairSpan
{
    uint32_t first_sample, n_samples;
    uint32_t hits_sample_offset; /* the hit log is indexed by sample offset within the caller's drt_render call */
    uint32_t row0, rows;         /* rows == 0: the whole tile */
    uint32_t stride;             /* sample slots per pixel in the header array; 0: the context's batch_spp (a launch over fewer rows may take more samples) */
    const uint32_t *list;        /* the pixels of an adaptive or sample-map round, anywhere in the whole tile; null: rows */
    uint64_t list_len;

    static PairSpan whole_tile(uint32_t first_sample, uint32_t n, uint32_t hits_sample_offset)
    {
        return {first_sample, n, hits_sample_offset, 0u, 0u, 0u, nullptr, 0u};
    }
    static PairSpan row_block(uint32_t first_sample, uint32_t n, uint32_t row0, uint32_t rows) { return {first_sample, n, 0u, row0, rows, n, nullptr, 0u}; }
    static PairSpan list_range(uint32_t first_sample, uint32_t n, const uint32_t *list, uint64_t len) { return {first_sample, n, 0u, 0u, 0u, n, list, len}; }
    /* samples [done, done + n) of this span, in the context's own header slots: what a redo launches */
    PairSpan narrowed(uint32_t done, uint32_t n) const
    {
        PairSpan s = *this;
        s.first_sample += done; s.n_samples = n; s.hits_sample_offset += done; s.stride = 0u;
        return s;
    }
};

/* the live window in tile columns and tile rows; open: between window_open and window_close */
struct PairWindow
{
    bool     open;
    uint32_t wx0, wx1, wy0, wy1;
};

/* ---- where a pair's pixels lie ---- */

/* The window's part of tile rows [row0, row0 + rows) (rows == 0: of the whole tile): rows [lo, hi), and their first pixel in the staging
 * film. The one place that maps tile rows to rows of the staging film: window_copy moves these rows, a windowed pair renders them. */
struct WindowRows
{
    uint32_t lo, hi;
    uint64_t stage0;
    bool     nothing; /* no live pixel in these rows */
};
static inline WindowRows window_rows(uint32_t row0, uint32_t rows, uint32_t tile_h, const PairWindow &w)
{
    if (rows == 0) { row0 = 0; rows = tile_h; }
    const uint32_t lo = std::max(row0, w.wy0), hi = std::min(row0 + rows, w.wy1);
    WindowRows r = {lo, std::max(lo, hi), 0u, hi <= lo || w.wx1 <= w.wx0};
    if (!r.nothing) r.stage0 = (uint64_t)(lo - w.wy0) * (w.wx1 - w.wx0);
    return r;
}

struct PairGeometry
{
    bool     windowed;       /* the kernels' tile is the live window's part of the pair's rows, their film the staging film */
    bool     nothing;        /* ... and nothing is live in these rows: no kernels, the fill pass only */
    uint32_t t_row0, t_rows; /* the pair's tile rows */
    uint32_t l_row0, l_rows, col0, l_cols; /* the rows and columns the kernels are launched over */
    uint64_t n_pix;          /* pixels of the launch */
    uint64_t pix0;           /* its first pixel in the tile's film (a list: 0, its pixels are numbered in the whole tile) */
    uint64_t stage0;         /* ... and in the staging film (windowed) */
    uint64_t counted_paths;  /* what the pair's timing is divided by: a windowed pair renders all its rows' pixels */
};
/* a pixel list ignores an open window: its pairs write the film itself */
static inline PairGeometry pair_geometry(const PairSpan &s, uint32_t tile_w, uint32_t tile_h, const PairWindow &w)
{
    PairGeometry g{};
    g.windowed = w.open && !s.list;
    g.t_row0 = s.rows ? s.row0 : 0u;
    g.t_rows = s.rows ? s.rows : tile_h;
    g.l_row0 = g.t_row0; g.l_rows = g.t_rows; g.col0 = 0u; g.l_cols = tile_w;
    if (g.windowed)
    {
        const WindowRows r = window_rows(g.t_row0, g.t_rows, tile_h, w);
        g.l_row0 = r.lo;
        g.l_rows = r.hi - r.lo;
        g.col0 = w.wx0;
        g.l_cols = w.wx1 - w.wx0;
        g.nothing = r.nothing;
        g.stage0 = r.stage0;
    }
    g.n_pix = s.list ? s.list_len : (uint64_t)g.l_rows * g.l_cols;
    g.pix0 = (s.rows && !s.list) ? (uint64_t)s.row0 * tile_w : 0u;
    g.counted_paths = (g.windowed ? (uint64_t)g.t_rows * tile_w : g.n_pix) * s.n_samples;
    return g;
}

/* ---- the tile a trace launch sees ---- */

struct TraceTile
{
    uint32_t x0, y0, tile_w, tile_h, row_stride; /* in image pixels: the kernels see a tile that starts at the launch's first row and column */
    uint64_t n_pix;       /* headers, records and the staging buffers are indexed from the launch's first pixel */
    uint32_t batch;       /* sample slots per pixel in the header array */
    uint32_t record_hits;
    uint64_t t_offset;    /* a bound ray table: a launch over rows [row0, ...) numbers its pixels from there; a list's pixels are numbered in the whole tile */
};
/* rows of the span, columns [col0, col0 + cols) of those rows (cols == 0: all of them); n_pix: the context's pixel count */
static inline TraceTile trace_tile(const drt_params &p, uint64_t n_pix, uint32_t batch_spp, const PairSpan &s, uint32_t col0 = 0, uint32_t cols = 0)
{
    const bool whole = s.rows == 0;
    const uint32_t row0 = whole ? 0u : s.row0, rows = whole ? p.tile_h : s.rows;
    if (cols == 0) { col0 = 0; cols = p.tile_w; }
    TraceTile t{};
    t.x0 = p.x0 + col0; t.y0 = p.y0 + row0 * p.row_stride;
    t.tile_w = cols; t.tile_h = rows; t.row_stride = p.row_stride;
    t.n_pix = s.list ? s.list_len : (whole && cols == p.tile_w) ? n_pix : (uint64_t)rows * cols;
    t.batch = s.stride ? s.stride : batch_spp;
    t.record_hits = (p.flags & DRT_FLAG_RECORD_HITS) ? 1u : 0u;
    t.t_offset = (s.list || whole) ? 0u : (uint64_t)row0 * p.tile_w;
    return t;
}
/* the tile of a pair's trace launch: a windowed pair's is the live window's part of its rows (g.nothing: there is no launch) */
static inline TraceTile pair_trace_tile(const drt_params &p, uint64_t n_pix, uint32_t batch_spp, const PairSpan &s, const PairGeometry &g)
{
    if (!g.windowed) return trace_tile(p, n_pix, batch_spp, s);
    PairSpan l = s;
    l.row0 = g.l_row0; l.rows = g.l_rows;
    return trace_tile(p, n_pix, batch_spp, l, g.col0, g.l_cols);
}

/* The sample of the tile the record pool is measured on when a context is created: every k-th row, one sample per pixel, one header
 * slot, no hit log. Where dense pairs will go out windowed (w.open, and the window holds a pixel), the rows and columns of the window. */
static inline uint32_t pool_sample_step(uint64_t live_px) { return (uint32_t)std::max<uint64_t>(1, live_px / (128u << 10)); } /* about 128 k paths */
static inline TraceTile pool_sample_tile(const drt_params &p, const PairWindow &w, uint32_t k)
{
    TraceTile t{};
    t.x0 = p.x0; t.y0 = p.y0; t.tile_w = p.tile_w; t.tile_h = p.tile_h;
    if (w.open && (uint64_t)(w.wx1 - w.wx0) * (w.wy1 - w.wy0) > 0)
    {
        t.x0 += w.wx0;
        t.tile_w = w.wx1 - w.wx0;
        t.y0 += w.wy0 * p.row_stride;
        t.tile_h = w.wy1 - w.wy0;
    }
    t.tile_h = (t.tile_h + k - 1) / k;
    t.row_stride = p.row_stride * k;
    t.n_pix = (uint64_t)t.tile_w * t.tile_h;
    t.batch = 1u;
    return t;
}

/* ---- the trace work queue ---- */

static inline uint32_t trace_grid(uint64_t n_paths, uint32_t trace_block, uint32_t grid_cap)
{
    return (uint32_t)std::min<uint64_t>((n_paths + trace_block - 1) / trace_block, (uint64_t)grid_cap);
}
/* work-queue granularity: about 16 draws per wave, so that the last draws finish together; 64..1024 path ids. Behind the hierarchy
 * (bvh) queued paths all cost alike: small draws (config 5: 827 ms at 64-256, 855 at 1024) */
static inline uint32_t trace_chunk(uint64_t n_paths, uint32_t grid, uint32_t trace_block, bool bvh, uint32_t override)
{
    const uint64_t waves = (uint64_t)grid * (trace_block / 64);
    const uint64_t c = waves ? n_paths / (waves * 16) / 64 * 64 : 0;
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(c, 64), bvh ? 256 : 1024);
    return override ? override : chunk;
}

/* ---- the shade work queue ---- */

/* the tuning knobs, read when the context is created */
struct ShadeOverrides
{
    int64_t  chunk = -1;      /* DRT_SHADE_CHUNK: pixels per group, clamped to [1, the default]; -1: unset */
    uint32_t subs = ~0u;      /* DRT_SHADE_SUBS: main-pass pieces per group; ~0u: unset */
    uint32_t tail_period = 0; /* DRT_TAIL_PERIOD; 0: unset */
};
struct ShadeQueue
{
    uint32_t chunk;             /* pixels per group */
    uint32_t sub_pixels, items_per_group, n_items, tail_period_mains;
    uint32_t grid;
    bool     too_large;         /* more items than the 32-bit work queue counts: nothing else is set */
};
/* tail_staged: the tail pass has nothing to replay (every path's tail was carried by the trace kernel) */
static inline ShadeQueue shade_queue(uint64_t n_pix, uint32_t n_samples, uint32_t tail_count, uint32_t tail_staged, uint32_t shade_grid_cap,
                                     uint32_t shade_waves, uint32_t pixel_chunk, const ShadeOverrides &o)
{
    ShadeQueue q{};
    const uint32_t chunk0 = tail_count ? 64u / tail_count : pixel_chunk;
    const uint64_t waves = (uint64_t)shade_grid_cap * shade_waves;
    q.chunk = chunk0;
    if (tail_count && !tail_staged)
    {
        /* A group's tail-pass item is the longest item of the queue: the replay of every path of its pixels that the trace kernel did
         * not carry, 1-4 ms where glass fills them -- the floor under a small launch. Its lane groups take PATHS, not pixels, so a group
         * of fewer pixels is replayed by the same 64 / R lane groups in that much less time, and only the short film phase runs with
         * lanes to spare. Worth it where a wave gets fewer than two such items (64 rows x 1024 px x 256 spp: shade 6.8 -> 6.1 ms with
         * half the pixels per group, 8 rows: 3.9 -> 1.6 with a quarter); the whole frame loses (80.2 -> 82.7: more, emptier film phases). */
        const uint64_t tail_items = (n_pix + q.chunk - 1) / q.chunk;
        if (2 * tail_items < waves) q.chunk = std::max(1u, q.chunk / 4);
        else if (tail_items < 2 * waves) q.chunk = std::max(1u, q.chunk / 2);
    }
    if (o.chunk >= 0) q.chunk = std::max(1u, std::min(chunk0, (uint32_t)o.chunk)); /* tuning knob */
    const uint64_t groups = (n_pix + q.chunk - 1) / q.chunk;
    const bool inline_tail = tail_count != 0;
    /* work items: a group's main pass in pieces of sub_pixels pixels (+ its tail pass as an item of its own) when the
     * groups alone are too few to keep the last round of the persistent waves short */
    uint32_t subs = o.subs;
    if (subs == ~0u)
    {
        /* pixels per main-pass item: small enough for >= 64 items per wave (short last round), large enough for
         * >= 256 paths per item (the queue is one atomic counter) */
        const uint64_t p_balance = n_pix / (waves * 64);
        const uint64_t p_atomic = (256 + n_samples - 1) / n_samples;
        const uint32_t P = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(std::max(p_balance, p_atomic), 1), q.chunk);
        subs = (q.chunk + P - 1) / P;
        if (subs == 1 && !inline_tail) subs = 0;
    }
    subs = std::min(subs, q.chunk);
    if (subs == 0 || (subs == 1 && !inline_tail) || groups * (uint64_t)(q.chunk + 1) >= 0xFFFFFFFFull)
    {
        q.sub_pixels = q.chunk;
        q.items_per_group = 1;
    }
    else
    {
        q.sub_pixels = (q.chunk + subs - 1) / subs;
        q.items_per_group = (q.chunk + q.sub_pixels - 1) / q.sub_pixels + (inline_tail ? 1 : 0);
    }
    if (groups * q.items_per_group >= 0xFFFFFFFFull)
    {
        q.too_large = true;
        return q;
    }
    q.n_items = (uint32_t)(groups * q.items_per_group);
    if (inline_tail && q.items_per_group > 1)
    {
        const uint32_t mains = q.items_per_group - 1;
        /* tail items (the longest ones, about a millisecond each) evenly through the queue when every wave gets many of them; when a
         * wave gets only a few (a rank's share of a frame, a row block of the one-shot call), they go out in the first third of the
         * queue and the launch ends on main-pass pieces only (64 rows x 1024 px x 256 spp: shade 7.0 -> 6.2 ms with the tails in the
         * first 1/6 to 1/2 of the queue, 7.8 when spread over all of it; the whole frame does not care: 79.9-80.1 ms at any setting) */
        q.tail_period_mains = (groups >= 8 * waves) ? mains : std::max<uint32_t>(1, mains / 3);
        if (o.tail_period) q.tail_period_mains = std::min(mains, o.tail_period);
    }
    q.grid = (uint32_t)std::min<uint64_t>(((uint64_t)q.n_items + shade_waves - 1) / shade_waves, (uint64_t)shade_grid_cap);
    return q;
}

/* ---- a call's samples in pairs ---- */

/* num_samples in as few pairs as take at most `fit` each, of equal size: 256 samples where 125 fit go out as 86 + 85 + 85, not
 * 125 + 125 + 6 (a launch of 6 samples fills the chip for a moment only); 100 where 64 fit are 50 + 50. Pair i takes size(i). */
struct EqualSplit
{
    uint32_t n_pairs, base, extra; /* the first `extra` pairs take base + 1 */
    uint32_t size(uint32_t i) const { return base + (i < extra ? 1u : 0u); }
};
static inline EqualSplit equal_split(uint32_t num_samples, uint32_t fit)
{
    const uint32_t n_pairs = (uint32_t)(((uint64_t)num_samples + fit - 1) / fit);
    if (n_pairs == 0) return {0u, 0u, 0u};
    return {n_pairs, num_samples / n_pairs, num_samples % n_pairs};
}

/* More samples than one pair takes over the whole tile, on a tile so large that a pair takes few samples of each pixel: row blocks,
 * so that the film is passed over fewer times (config 5, 4096^2 at 16 samples a pair: 208 bytes of film per path; in blocks
 * 1141 -> 1196 Mpaths/s). Where a pair takes 32 samples or more the film is a small part of the traffic and the smaller launches
 * cost more than they save (1024^2, 64 a pair: 1493 -> 1452). Returns the number of blocks; 1: no row blocks. */
static inline uint32_t row_block_count(uint32_t num_samples, uint32_t batch_spp, uint32_t tile_h)
{
    if (!(num_samples > batch_spp && batch_spp < 32 && tile_h >= 64)) return 1u;
    const uint64_t want = ((uint64_t)num_samples * 8 + (uint64_t)batch_spp * 5 - 1) / ((uint64_t)batch_spp * 5); /* blocks for one pair each */
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(want, 16), tile_h / 16));
}
/* rows per block of a tile in n_blocks row blocks */
static inline uint32_t row_block_rows(uint32_t tile_h, uint32_t n_blocks) { return (tile_h + n_blocks - 1) / n_blocks; }
/* Samples per pair of a block of `per` rows: a pair then covers fewer pixels and more samples of each (the record pool holds the same
 * number of paths). Five eighths of what the pool's size would allow, because it is sized from the tile's AVERAGE path and the rows of
 * an image that hold its objects run above that (a block that runs out anyway is rendered again); at most 4096 samples of a pixel. */
static inline uint32_t row_block_fit(uint32_t num_samples, uint64_t n_pix, uint32_t batch_spp, uint32_t per, uint32_t tile_w)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(num_samples, 4096), n_pix * (uint64_t)batch_spp * 5 / 8 / ((uint64_t)per * tile_w)));
}

/* the kernel pairs of a round that renders k samples of each of n_in listed pixels: m samples and P pixels per pair. A pair takes up
 * to five eighths of the paths the record pool is sized for and at most 4096 samples of a pixel; pairs of equal size */
struct RoundPairs { uint32_t m; uint64_t P; };
static inline RoundPairs round_pairs(uint64_t n_pix, uint32_t batch_spp, uint32_t k, uint64_t n_in)
{
    const uint64_t budget = std::max<uint64_t>(1, n_pix * (uint64_t)batch_spp * 5 / 8);
    const uint32_t m_fit = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(k, budget), 4096);
    const uint32_t n_sp = (k + m_fit - 1) / m_fit, m = (k + n_sp - 1) / n_sp;   /* samples per pair */
    const uint64_t p_fit = std::max<uint64_t>(1, budget / m);
    const uint64_t n_pp = (n_in + p_fit - 1) / p_fit, P = (n_in + n_pp - 1) / n_pp; /* pixels per pair */
    return {m, P};
}

#endif
