/* Host program of tests/test_pair_rule_cpu.py: the plan of a kernel pair (drt_pair_rule.h) as the launcher makes it, printed field by
 * field.
 *
 * stdin, one case per line; stdout, one line per case, the case's word first:
 *   span whole F N HSO | span block F N ROW0 ROWS | span list F N LEN        the named constructors
 *   narrow <span> DONE N                                                      PairSpan::narrowed
 *        -> first_sample n_samples hits_sample_offset row0 rows stride has_list list_len
 *   pair X0 Y0 TILE_W TILE_H ROW_STRIDE FLAGS BATCH_SPP <span> <window>       pair_geometry, window_rows of the span's rows, pair_trace_tile
 *        -> windowed nothing t_row0 t_rows l_row0 l_rows col0 l_cols n_pix pix0 stage0 counted_paths | lo hi stage0 nothing |
 *           x0 y0 tile_w tile_h row_stride n_pix batch record_hits t_offset   (the tile: nine times -1 when there is no launch)
 *   sample X0 Y0 TILE_W TILE_H ROW_STRIDE <window> K                          pool_sample_tile -> the tile's nine fields
 *   step LIVE_PX                                                              pool_sample_step
 *   tgrid N_PATHS BLOCK CAP                                                   trace_grid
 *   trace N_PATHS GRID BLOCK BVH OVERRIDE                                     trace_chunk
 *   shade N_PIX N TAIL_COUNT TAIL_STAGED CAP WAVES PIXEL_CHUNK O_CHUNK O_SUBS O_TAIL_PERIOD   (O_CHUNK -1, O_SUBS 4294967295, O_TAIL_PERIOD 0: unset)
 *        -> chunk sub_pixels items_per_group n_items tail_period_mains grid too_large
 *   split NUM FIT                                                             equal_split -> n_pairs, then every pair's size
 *   blocks NUM BATCH_SPP TILE_H | brows TILE_H N_BLOCKS | fit NUM N_PIX BATCH_SPP PER TILE_W
 *   round N_PIX BATCH_SPP K N_IN                                              round_pairs -> m P
 * <span>: F N HSO ROW0 ROWS STRIDE HAS_LIST LIST_LEN; <window>: OPEN WX0 WX1 WY0 WY1.
 * A line it cannot read ends it with a message and status 1. */
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "drt_pair_rule.h"

static const uint32_t g_list[1] = {0u}; /* what a list span points at: the rules never read it */

static const char *g_at; /* the rest of the line */

static bool word(char *out, size_t cap)
{
    int used = 0;
    char buf[64];
    if (sscanf(g_at, "%63s%n", buf, &used) != 1) return false;
    g_at += used;
    snprintf(out, cap, "%s", buf);
    return true;
}
static bool num(long long &v)
{
    int used = 0;
    if (sscanf(g_at, "%lld%n", &v, &used) != 1) return false;
    g_at += used;
    return true;
}
template <typename T> static bool get(T &v)
{
    long long x = 0;
    if (!num(x)) return false;
    v = (T)x;
    return true;
}
static bool get_span(PairSpan &s)
{
    uint32_t has_list = 0;
    if (!(get(s.first_sample) && get(s.n_samples) && get(s.hits_sample_offset) && get(s.row0) && get(s.rows) && get(s.stride) && get(has_list) && get(s.list_len)))
        return false;
    s.list = has_list ? g_list : nullptr;
    return true;
}
static bool get_window(PairWindow &w)
{
    uint32_t open = 0;
    if (!(get(open) && get(w.wx0) && get(w.wx1) && get(w.wy0) && get(w.wy1))) return false;
    w.open = open != 0;
    return true;
}
static void put_span(const char *what, const PairSpan &s)
{
    printf("%s %u %u %u %u %u %u %d %" PRIu64 "\n", what, s.first_sample, s.n_samples, s.hits_sample_offset, s.row0, s.rows, s.stride, s.list ? 1 : 0, s.list_len);
}
static void put_tile(const TraceTile &t)
{
    printf("%u %u %u %u %u %" PRIu64 " %u %u %" PRIu64, t.x0, t.y0, t.tile_w, t.tile_h, t.row_stride, t.n_pix, t.batch, t.record_hits, t.t_offset);
}

static bool one_case(const char *what)
{
    if (!strcmp(what, "span"))
    {
        char kind[64];
        uint32_t f = 0, n = 0, a = 0, b = 0;
        uint64_t len = 0;
        if (!word(kind, sizeof(kind)) || !get(f) || !get(n)) return false;
        if (!strcmp(kind, "whole")) { if (!get(a)) return false; put_span(what, PairSpan::whole_tile(f, n, a)); }
        else if (!strcmp(kind, "block")) { if (!get(a) || !get(b)) return false; put_span(what, PairSpan::row_block(f, n, a, b)); }
        else if (!strcmp(kind, "list")) { if (!get(len)) return false; put_span(what, PairSpan::list_range(f, n, g_list, len)); }
        else return false;
        return true;
    }
    if (!strcmp(what, "narrow"))
    {
        PairSpan s{};
        uint32_t done = 0, n = 0;
        if (!get_span(s) || !get(done) || !get(n)) return false;
        put_span(what, s.narrowed(done, n));
        return true;
    }
    if (!strcmp(what, "pair"))
    {
        drt_params p{};
        uint32_t batch_spp = 0;
        PairSpan s{};
        PairWindow w{};
        if (!(get(p.x0) && get(p.y0) && get(p.tile_w) && get(p.tile_h) && get(p.row_stride) && get(p.flags) && get(batch_spp) && get_span(s) && get_window(w))) return false;
        const PairGeometry g = pair_geometry(s, p.tile_w, p.tile_h, w);
        const WindowRows r = window_rows(s.row0, s.rows, p.tile_h, w);
        printf("%s %d %d %u %u %u %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " | %u %u %" PRIu64 " %d | ", what, g.windowed ? 1 : 0, g.nothing ? 1 : 0, g.t_row0,
               g.t_rows, g.l_row0, g.l_rows, g.col0, g.l_cols, g.n_pix, g.pix0, g.stage0, g.counted_paths, r.lo, r.hi, r.stage0, r.nothing ? 1 : 0);
        if (g.nothing) printf("-1 -1 -1 -1 -1 -1 -1 -1 -1");
        else put_tile(pair_trace_tile(p, (uint64_t)p.tile_w * p.tile_h, batch_spp, s, g));
        printf("\n");
        return true;
    }
    if (!strcmp(what, "sample"))
    {
        drt_params p{};
        PairWindow w{};
        uint32_t k = 0;
        if (!(get(p.x0) && get(p.y0) && get(p.tile_w) && get(p.tile_h) && get(p.row_stride) && get_window(w) && get(k)) || k == 0) return false;
        printf("%s ", what);
        put_tile(pool_sample_tile(p, w, k));
        printf("\n");
        return true;
    }
    if (!strcmp(what, "step"))
    {
        uint64_t live = 0;
        if (!get(live)) return false;
        printf("%s %u\n", what, pool_sample_step(live));
        return true;
    }
    if (!strcmp(what, "tgrid"))
    {
        uint64_t n_paths = 0;
        uint32_t block = 0, cap = 0;
        if (!(get(n_paths) && get(block) && get(cap)) || block == 0) return false;
        printf("%s %u\n", what, trace_grid(n_paths, block, cap));
        return true;
    }
    if (!strcmp(what, "trace"))
    {
        uint64_t n_paths = 0;
        uint32_t grid = 0, block = 0, bvh = 0, over = 0;
        if (!(get(n_paths) && get(grid) && get(block) && get(bvh) && get(over))) return false;
        printf("%s %u\n", what, trace_chunk(n_paths, grid, block, bvh != 0, over));
        return true;
    }
    if (!strcmp(what, "shade"))
    {
        uint64_t n_pix = 0;
        uint32_t n = 0, tail_count = 0, staged = 0, cap = 0, waves = 0, pixel_chunk = 0;
        ShadeOverrides o;
        if (!(get(n_pix) && get(n) && get(tail_count) && get(staged) && get(cap) && get(waves) && get(pixel_chunk) && get(o.chunk) && get(o.subs) && get(o.tail_period)))
            return false;
        if (n == 0 || cap == 0 || waves == 0 || pixel_chunk == 0 || tail_count > 64) return false;
        const ShadeQueue q = shade_queue(n_pix, n, tail_count, staged, cap, waves, pixel_chunk, o);
        printf("%s %u %u %u %u %u %u %d\n", what, q.chunk, q.sub_pixels, q.items_per_group, q.n_items, q.tail_period_mains, q.grid, q.too_large ? 1 : 0);
        return true;
    }
    if (!strcmp(what, "split"))
    {
        uint32_t num_samples = 0, fit = 0;
        if (!(get(num_samples) && get(fit)) || fit == 0) return false;
        const EqualSplit e = equal_split(num_samples, fit);
        printf("%s %u", what, e.n_pairs);
        for (uint32_t i = 0; i < e.n_pairs; i += 1) printf(" %u", e.size(i));
        printf("\n");
        return true;
    }
    if (!strcmp(what, "blocks"))
    {
        uint32_t num_samples = 0, batch_spp = 0, tile_h = 0;
        if (!(get(num_samples) && get(batch_spp) && get(tile_h)) || batch_spp == 0) return false;
        printf("%s %u\n", what, row_block_count(num_samples, batch_spp, tile_h));
        return true;
    }
    if (!strcmp(what, "brows"))
    {
        uint32_t tile_h = 0, n_blocks = 0;
        if (!(get(tile_h) && get(n_blocks)) || n_blocks == 0) return false;
        printf("%s %u\n", what, row_block_rows(tile_h, n_blocks));
        return true;
    }
    if (!strcmp(what, "fit"))
    {
        uint32_t num_samples = 0, batch_spp = 0, per = 0, tile_w = 0;
        uint64_t n_pix = 0;
        if (!(get(num_samples) && get(n_pix) && get(batch_spp) && get(per) && get(tile_w)) || per == 0 || tile_w == 0) return false;
        printf("%s %u\n", what, row_block_fit(num_samples, n_pix, batch_spp, per, tile_w));
        return true;
    }
    if (!strcmp(what, "round"))
    {
        uint64_t n_pix = 0, n_in = 0;
        uint32_t batch_spp = 0, k = 0;
        if (!(get(n_pix) && get(batch_spp) && get(k) && get(n_in)) || k == 0 || n_in == 0) return false;
        const RoundPairs rp = round_pairs(n_pix, batch_spp, k, n_in);
        printf("%s %u %" PRIu64 "\n", what, rp.m, rp.P);
        return true;
    }
    return false;
}

int main()
{
    char line[512], what[64];
    unsigned long long n = 0;
    while (fgets(line, sizeof(line), stdin))
    {
        n += 1;
        g_at = line;
        if (!word(what, sizeof(what))) continue; /* an empty line */
        if (!one_case(what))
        {
            fprintf(stderr, "pair rule: cannot read line %llu: %s", n, line);
            return 1;
        }
    }
    return 0;
}
