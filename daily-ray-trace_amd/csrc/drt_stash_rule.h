/*
 * drt_stash_rule.h -- the ray stash's hand-out rule: which entry an idle lane of the trace kernel takes, when the wave fills the stash,
 * how many entries a fill holds, and what head and count become.
 *
 * Plain C++, no HIP: drt_trace_kernel (drt_kernels.h) includes it, and a host program can run the very same text (tests/host).
 *
 * A wave draws chunks of consecutive path ids [chunk_next, chunk_end) from the work counter. Its stash holds the starts (camera ray,
 * generator state, vignette, header position) of up to 64 ids it has already taken from the chunk, made by all 64 lanes at once;
 * entries [head, head + count) have not been handed out yet. When `want` lanes are idle, the idle lane of rank r (its place among
 * the idle lanes, ascending) takes the r-th id the wave has not started yet:
 *   1. ranks [0, take1), take1 = min(want, count), take entries head + r: what is left of the stash goes first;
 *   2. if want > take1 the stash is empty. If the chunk is used up too, the wave draws a new one (and if there is none, stops: the
 *      other lanes stay idle). It then fills entries [0, n), n = min(64, chunk_end - chunk_next), with ids chunk_next + e, and
 *      ranks [take1, take1 + take2), take2 = min(want - take1, n), take entries r - take1.
 * Chunks are multiples of 64 ids except a launch's last, so only a launch's last fill is short, and a fill never reaches past
 * chunk_end: every id a stash holds is started by this wave. A lane of rank >= take1 + take2 stays idle until the next iteration,
 * as it does in the direct form when a launch's last chunk is smaller than the number of idle lanes.
 */
#ifndef DRT_STASH_RULE_H
#define DRT_STASH_RULE_H

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRT_STASH_FN __host__ __device__ __forceinline__
#else
#define DRT_STASH_FN static inline
#endif

#define DRT_STASH_ENTRIES 64u /* one per lane of the wave that fills it */

/* wave-uniform, in scalar registers across the path loop */
struct StashState
{
    uint32_t head;  /* the first entry not handed out yet */
    uint32_t count; /* entries [head, head + count) hold starts nobody has taken */
};

/* entries handed out of `have` to `want` idle lanes */
DRT_STASH_FN uint32_t stash_take(uint32_t want, uint32_t have) { return want < have ? want : have; }

/* entries of the next fill: the chunk's next ids, 64 at the most */
DRT_STASH_FN uint32_t stash_fill_size(uint64_t chunk_next, uint64_t chunk_end)
{
    const uint64_t rest = chunk_end - chunk_next;
    return rest < (uint64_t)DRT_STASH_ENTRIES ? (uint32_t)rest : DRT_STASH_ENTRIES;
}

/* step 1: the entry the idle lane of rank `rank` takes from the stash as it stands, or -1. Call stash_after_first once per wave afterwards. */
DRT_STASH_FN int32_t stash_first_entry(const StashState &st, uint32_t want, uint32_t rank)
{
    return rank < stash_take(want, st.count) ? (int32_t)(st.head + rank) : -1;
}
/* ... and how many lanes step 1 served; the state moves past them. want > the returned number: the stash is empty, step 2 follows */
DRT_STASH_FN uint32_t stash_after_first(StashState &st, uint32_t want)
{
    const uint32_t take1 = stash_take(want, st.count);
    st.head += take1;
    st.count -= take1;
    return take1;
}
/* step 2, after a fill of n entries (ids chunk_next + 0 .. n - 1): the entry of the idle lane of rank `rank` that step 1 (take1 lanes)
 * did not serve, or -1. Call stash_after_fill once per wave afterwards. */
DRT_STASH_FN int32_t stash_second_entry(uint32_t n, uint32_t want, uint32_t take1, uint32_t rank)
{
    return (rank >= take1 && rank - take1 < stash_take(want - take1, n)) ? (int32_t)(rank - take1) : -1;
}
DRT_STASH_FN void stash_after_fill(StashState &st, uint64_t &chunk_next, uint32_t n, uint32_t want, uint32_t take1)
{
    const uint32_t take2 = stash_take(want - take1, n);
    st.head = take2;
    st.count = n - take2;
    chunk_next += n; /* the stash's ids are taken from the chunk when they are made */
}

#endif
