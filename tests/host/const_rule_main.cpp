/* Host program of tests/test_const_rule_cpu.py: csrc/drt_const_rule.h run on the host, the very text the kernels compile.
 *
 *   const_rule_main sweep
 *       drt_draw_quotient(n) against (double)n / 2147483647.0 for all 2^31 values a draw can take, bit for bit, on a few threads.
 *       stdout: `sweep <values checked> <mismatches>`, and for the first mismatches `differs <n> <got bits> <want bits>`.
 *   const_rule_main draw N...
 *       stdout: one line `draw <n> <bits of drt_draw_quotient(n)>` per argument: what the test compares with its own division.
 *   const_rule_main glass
 *       stdin: rows of seven doubles as 16 hex digits each: trans_wl w0 w1 base_i0 base_i1 i0 i1.
 *       stdout: per row `glass` and the bits of drt_glass_constants' seven values: at_wl, rel_out[0..2], rel_in[0..2].
 *
 * Built without floating-point contraction, like the library. The sweep's loop is cloned for CPUs with a fused multiply-add: the
 * builtin is then one instruction, otherwise the C library's (correctly rounded, slow) fma. */
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "drt_const_rule.h"

static uint64_t bits_of(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}

struct SweepPart
{
    uint64_t first, end;   /* n in [first, end) */
    uint64_t mismatches;
    uint64_t first_bad[4]; /* the first few n that differ */
};

#if defined(__x86_64__) && defined(__GNUC__) && !defined(__clang__)
__attribute__((target_clones("fma", "default")))
#endif
static void sweep_part(SweepPart *p)
{
    uint64_t bad = 0;
    for (uint64_t n = p->first; n < p->end; n += 1)
    {
        const double got = drt_draw_quotient((uint32_t)n);
        const double want = (double)(uint32_t)n / 2147483647.0; /* drt_rng's division */
        if (bits_of(got) != bits_of(want))
        {
            if (bad < 4) p->first_bad[bad] = n;
            bad += 1;
        }
    }
    p->mismatches = bad;
}

static int sweep()
{
    const uint64_t total = 1ull << 31;
    unsigned n_threads = std::thread::hardware_concurrency();
    n_threads = n_threads < 1 ? 1 : n_threads > 16 ? 16 : n_threads;
    std::vector<SweepPart> parts(n_threads);
    std::vector<std::thread> threads;
    for (unsigned t = 0; t < n_threads; t += 1)
    {
        parts[t] = SweepPart{total * t / n_threads, total * (t + 1) / n_threads, 0, {0, 0, 0, 0}};
        threads.emplace_back(sweep_part, &parts[t]);
    }
    for (auto &t : threads) t.join();
    uint64_t checked = 0, bad = 0;
    for (const SweepPart &p : parts)
    {
        checked += p.end - p.first;
        for (uint64_t k = 0; k < p.mismatches && k < 4; k += 1)
        {
            const uint32_t n = (uint32_t)p.first_bad[k];
            printf("differs %" PRIu32 " %016" PRIx64 " %016" PRIx64 "\n", n, bits_of(drt_draw_quotient(n)), bits_of((double)n / 2147483647.0));
        }
        bad += p.mismatches;
    }
    printf("sweep %" PRIu64 " %" PRIu64 "\n", checked, bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    if (argc >= 3 && !strcmp(argv[1], "draw"))
    {
        for (int k = 2; k < argc; k += 1)
        {
            char *end = nullptr;
            const unsigned long long n = strtoull(argv[k], &end, 10);
            if (*end || n >= (1ull << 31))
            {
                fprintf(stderr, "const rule: `%s` is not a draw's integer\n", argv[k]);
                return 2;
            }
            printf("draw %llu %016" PRIx64 "\n", n, bits_of(drt_draw_quotient((uint32_t)n)));
        }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "glass"))
    {
        uint64_t w[7];
        for (;;)
        {
            int got = 0;
            while (got < 7 && scanf("%" SCNx64, &w[got]) == 1) got += 1;
            if (got == 0) return 0;
            if (got != 7)
            {
                fprintf(stderr, "const rule: a row of %d words, not 7\n", got);
                return 2;
            }
            double v[7];
            memcpy(v, w, sizeof(v));
            const DrtGlassConst g = drt_glass_constants(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
            printf("glass %016" PRIx64, bits_of(g.at_wl));
            for (int k = 0; k < 3; k += 1) printf(" %016" PRIx64, bits_of(g.rel_out[k]));
            for (int k = 0; k < 3; k += 1) printf(" %016" PRIx64, bits_of(g.rel_in[k]));
            printf("\n");
        }
    }
    fprintf(stderr, "usage: const_rule_main sweep | draw N... | glass\n");
    return 2;
}
