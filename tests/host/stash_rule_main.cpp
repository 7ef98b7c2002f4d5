/* Host program of tests/test_stash_rule_cpu.py: one wave of the trace kernel's stash form, driven by drt_stash_rule.h as the kernel
 * drives it, with a stash that holds path ids instead of rays.
 *
 * stdin:  CHUNK N_PATHS K, then K numbers of idle lanes (1..64), one per loop iteration.
 * stdout: per iteration one line `step <want> <id of rank 0> ... <id of rank want-1>` (-1: the lane stays idle), one line
 *         `fill <first id> <n> <chunk_end>` per fill and `draw <base>` per draw from the work counter.
 * It stops with a message and status 1 when an entry is read that no fill made, that was handed out before, or that lies at or
 * beyond chunk_end; the sanitizers it is built with catch an index outside the stash. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "drt_stash_rule.h"

static int fail(const char *what, long long a, long long b)
{
    fprintf(stderr, "stash rule: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

int main()
{
    unsigned long long chunk = 0, n_paths = 0, steps = 0;
    if (scanf("%llu %llu %llu", &chunk, &n_paths, &steps) != 3 || chunk == 0 || chunk % 64 != 0) return fail("bad header", 0, 0);
    std::vector<long long> stash(DRT_STASH_ENTRIES, -1); /* the id an entry holds, -1: none (never made, or taken) */
    StashState st = {0u, 0u};
    uint64_t chunk_next = 0, chunk_end = 0, counter = 0;
    bool exhausted = false;
    for (unsigned long long k = 0; k < steps; k += 1)
    {
        unsigned want = 0;
        if (scanf("%u", &want) != 1 || want < 1 || want > 64) return fail("bad idle count", (long long)k, want);
        std::vector<long long> got(want, -1);
        if (!exhausted)
        {
            for (uint32_t rank = 0; rank < want; rank += 1)
            {
                const int32_t e = stash_first_entry(st, want, rank);
                if (e < 0) continue;
                if (stash.at((size_t)e) < 0) return fail("step 1 reads an entry that holds nothing", e, rank);
                got[rank] = stash[(size_t)e];
                stash[(size_t)e] = -1;
            }
            const uint32_t take1 = stash_after_first(st, want);
            if (take1 < want)
            {
                if (st.count != 0) return fail("a fill with entries left", st.count, want);
                if (chunk_next == chunk_end)
                {
                    const uint64_t base = counter;
                    counter += chunk;
                    printf("draw %llu\n", (unsigned long long)base);
                    if (base >= n_paths)
                    {
                        exhausted = true;
                        chunk_next = chunk_end = 0;
                    }
                    else
                    {
                        chunk_next = base;
                        chunk_end = base + chunk < n_paths ? base + chunk : n_paths;
                    }
                }
                if (!exhausted)
                {
                    const uint32_t n = stash_fill_size(chunk_next, chunk_end);
                    if (n < 1 || n > DRT_STASH_ENTRIES) return fail("fill size", n, 0);
                    printf("fill %llu %u %llu\n", (unsigned long long)chunk_next, n, (unsigned long long)chunk_end);
                    for (uint32_t e = 0; e < DRT_STASH_ENTRIES; e += 1)
                    {
                        if (stash[e] >= 0) return fail("a fill overwrites an entry nobody took", e, stash[e]);
                        if (e < n)
                        {
                            if (chunk_next + e >= chunk_end) return fail("an entry beyond chunk_end", e, (long long)chunk_end);
                            stash[e] = (long long)(chunk_next + e);
                        }
                    }
                    for (uint32_t rank = 0; rank < want; rank += 1)
                    {
                        const int32_t e = stash_second_entry(n, want, take1, rank);
                        if (e < 0) continue;
                        if (got[rank] >= 0) return fail("a lane served twice", rank, e);
                        if (stash.at((size_t)e) < 0) return fail("step 2 reads an entry that holds nothing", e, rank);
                        got[rank] = stash[(size_t)e];
                        stash[(size_t)e] = -1;
                    }
                    stash_after_fill(st, chunk_next, n, want, take1);
                    if (chunk_next > chunk_end || st.head + st.count > DRT_STASH_ENTRIES) return fail("state after a fill", st.head, st.count);
                }
            }
        }
        printf("step %u", want);
        for (uint32_t rank = 0; rank < want; rank += 1) printf(" %lld", got[rank]);
        printf("\n");
    }
    /* what is left: the entries the state says are there hold ids, every other entry holds none */
    for (uint32_t e = 0; e < DRT_STASH_ENTRIES; e += 1)
    {
        const bool held = e >= st.head && e < st.head + st.count;
        if (held != (stash[e] >= 0)) return fail("the state and the stash disagree at entry", e, stash[e]);
    }
    printf("left %u %llu\n", st.count, (unsigned long long)(chunk_end - chunk_next));
    return 0;
}
