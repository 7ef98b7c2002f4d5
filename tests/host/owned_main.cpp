/*
 * owned_main.cpp -- csrc/drt_owned.h's Owned<T, Mem> on the host, with a malloc-backed policy that counts every call. Built with
 * -fsanitize=address,undefined by tests/test_owned_cpu.py: the counts below catch a free too many or too few, the sanitizers a
 * double free, a use after free and a leak. Exits non-zero on the first mismatch.
 */
#include "drt_owned.h"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

struct CountingMem
{
    static std::atomic<uint64_t> &live() { static std::atomic<uint64_t> n{0}; return n; }
    static inline uint64_t allocs = 0, frees = 0;
    static inline size_t   last_bytes = 0;
    static inline void    *last_freed = nullptr;
    static inline bool     fail_next = false;
    static int alloc(void **p, size_t bytes)
    {
        if (fail_next) { fail_next = false; return 2; }
        *p = malloc(bytes);
        if (!*p) return 1;
        allocs += 1; last_bytes = bytes; live() += 1;
        return 0;
    }
    static void free(void *p) { ::free(p); frees += 1; last_freed = p; live() -= 1; }
};
using Buf = Owned<double, CountingMem>;

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do                                                                               \
    {                                                                                \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); g_failed += 1; } \
    } while (0)
#define COUNTS(a, f) CHECK(CountingMem::allocs == (a) && CountingMem::frees == (f) && CountingMem::live() == (uint64_t)((a) - (f)))

static double sum(const double *p, size_t n) { double s = 0.0; for (size_t k = 0; k < n; k += 1) s += p[k]; return s; }

int main()
{
    {
        Buf b;
        CHECK(!b && b.count() == 0);
        b.reset(); /* empty: a no-op */
        COUNTS(0u, 0u);
        CHECK(b.need(4) == 0 && b && b.count() == 4 && CountingMem::last_bytes == 4 * sizeof(double));
        double *first = b;
        for (int k = 0; k < 4; k += 1) b[k] = k + 1.0;
        CHECK(b.need(100) == 0 && (double *)b == first && b.count() == 4); /* holds something: nothing happens */
        COUNTS(1u, 0u);
        const Buf &cb = b;
        CHECK(sum(cb, 4) == 10.0 && sum(b + 2, 2) == 7.0); /* const form -> const T *; pointer arithmetic */

        CHECK(b.remake(8) == 0 && b.count() == 8 && CountingMem::last_freed == first);
        COUNTS(2u, 1u);

        Buf z;
        CHECK(z.need(0) == 0 && z && z.count() == 1 && CountingMem::last_bytes == sizeof(double)); /* max(n, 1) */
        COUNTS(3u, 1u);
        z.reset();
        CHECK(!z && z.count() == 0);
        z.reset();
        COUNTS(3u, 2u);

        CountingMem::fail_next = true;
        CHECK(z.need(4) == 2 && !z && z.count() == 0); /* a failed allocation: the error, and still empty */
        COUNTS(3u, 2u);

        double *held = b;
        Buf c(std::move(b)); /* move construction: the source is empty, nothing is freed */
        CHECK(!b && b.count() == 0 && (double *)c == held && c.count() == 8);
        COUNTS(3u, 2u);

        Buf d;
        CHECK(d.need(2) == 0);
        double *old = d;
        d = std::move(c); /* move assignment: the destination's old block is freed once, the source is empty */
        CHECK(!c && (double *)d == held && d.count() == 8 && CountingMem::last_freed == old);
        COUNTS(4u, 3u);
        Buf &self = d;
        d = std::move(self); /* onto itself: nothing */
        CHECK((double *)d == held);
        COUNTS(4u, 3u);

        double *raw = d.release(); /* hands over without freeing */
        CHECK(raw == held && !d && d.count() == 0);
        COUNTS(4u, 3u);
        CountingMem::free(raw);
        COUNTS(4u, 4u);
    } /* b, c, d, z are empty here: their destructors free nothing */
    COUNTS(4u, 4u);
    {
        std::vector<Buf> v; /* grown one by one: every reallocation moves the owners */
        for (size_t k = 0; k < 37; k += 1)
        {
            v.emplace_back();
            CHECK(v.back().need(k + 1) == 0);
            v.back()[k] = (double)k;
        }
        COUNTS(4u + 37u, 4u);
        for (size_t k = 0; k < 37; k += 1) CHECK(v[k].count() == k + 1 && v[k][k] == (double)k);
        v.erase(v.begin() + 5); /* move assignment down the tail: one block goes */
        COUNTS(4u + 37u, 5u);
    } /* the vector's destructor frees each block once */
    COUNTS(4u + 37u, 4u + 37u);
    CHECK(CountingMem::live() == 0);
    if (g_failed) return 1;
    puts("owned ok");
    return 0;
}
