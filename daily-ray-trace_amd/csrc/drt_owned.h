/*
 * drt_owned.h -- the launcher's owners: move-only holders of one device or pinned allocation, one HIP event, one HIP stream.
 * A member of one of these types is released when the struct that holds it is destroyed; a local, when its scope ends.
 *
 * Owned<T, Mem> knows nothing of HIP: Mem is a policy with two static functions, alloc(void **, size_t bytes), whose result
 * converts to false on success (hipError_t does), and free(void *). The launcher defines DeviceMem and PinnedMem; the host
 * test gives a malloc-backed one. Event and Stream need the HIP runtime and exist only where hipcc compiles this header.
 * Each policy, Event and Stream count their live objects in one process-wide atomic (drt_selftest_live_resources).
 */
#ifndef DRT_OWNED_H
#define DRT_OWNED_H

#include <atomic>
#include <cstddef>
#include <cstdint>

template <typename T, typename Mem>
class Owned
{
    T     *p_ = nullptr;
    size_t n_ = 0;

public:
    using Err = decltype(Mem::alloc((void **)nullptr, (size_t)0));

    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o)
        {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~Owned() { reset(); }

    operator T *() { return p_; }
    operator const T *() const { return p_; }
    T *get() { return p_; } /* where a conversion will not do: a cast to another pointer type, a deduced argument */
    const T *get() const { return p_; }
    size_t count() const { return n_; }

    /* empty: allocate max(n, 1) elements; holding something already: nothing (the `if (!p) hipMalloc` of the *_prepare functions) */
    Err need(size_t n)
    {
        if (p_) return Err{};
        if (n < 1) n = 1;
        void *p = nullptr;
        const Err e = Mem::alloc(&p, n * sizeof(T));
        if (!e) { p_ = (T *)p; n_ = n; }
        return e;
    }
    Err remake(size_t n) { reset(); return need(n); }
    void reset()
    {
        if (p_) Mem::free(p_);
        p_ = nullptr; n_ = 0;
    }
    /* hands the allocation to another owner of the same policy */
    T *release() { T *p = p_; p_ = nullptr; n_ = 0; return p; }
};

#ifdef __HIPCC__
class Event
{
    hipEvent_t e_ = nullptr;

public:
    static std::atomic<uint64_t> &live() { static std::atomic<uint64_t> n{0}; return n; }

    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
        return *this;
    }
    ~Event() { reset(); }

    operator hipEvent_t() const { return e_; }
    /* created at the first call, with that call's flags */
    hipError_t need(unsigned flags = hipEventDefault)
    {
        if (e_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e == hipSuccess) live() += 1; else e_ = nullptr;
        return e;
    }
    void reset()
    {
        if (e_) { (void)hipEventDestroy(e_); live() -= 1; }
        e_ = nullptr;
    }
};

class Stream
{
    hipStream_t s_ = nullptr;

public:
    static std::atomic<uint64_t> &live() { static std::atomic<uint64_t> n{0}; return n; }

    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream()
    {
        if (s_) { (void)hipStreamDestroy(s_); live() -= 1; }
    }

    operator hipStream_t() const { return s_; }
    hipError_t create(unsigned flags)
    {
        const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
        if (e == hipSuccess) live() += 1; else s_ = nullptr;
        return e;
    }
};
#endif

#endif
