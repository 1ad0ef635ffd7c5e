// The read-out slab of a device product, and the one place its life cycle is written:
//
//   configure   alloc(n_words, stream): the slab of 64-bit words on the device, zeroed, its pinned
//               mirror and (once per engine) the event
//   accumulate  the product's kernel adds to the slab in stream order; the caller counts n_acc
//   request     copy_out(stream, n_zero_words), whatever else the product orders behind the copy,
//               then mark(stream): the hot loop is never stalled
//   fetch       wait(), then the product unpacks host() -- pend_n accumulations
//   set         upload(words) behind a synchronised stream (resume), n_acc from the caller
//
// One request is in flight at most: `pending` from mark() to wait().  The product keeps its own
// argument checks and messages; a seventh product starts with a Readout member in its struct of
// mcmc_hip_ctx (ctx.h).  Private to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct Readout {
    unsigned long long* slab = nullptr;   // device [n_words]; non-null: configured
    unsigned long long* pin = nullptr;    // pinned host [n_words]
    size_t n_words = 0;
    int64_t n_acc = 0;                    // accumulations since the last closing request / set
    int64_t pend_n = 0;                   // ... of the pending read-out
    hipEvent_t ev = nullptr;
    bool pending = false;

    template <class T = unsigned long long> T* dev() const
    {
        static_assert(sizeof(T) == sizeof(unsigned long long), "a slab holds 64-bit words");
        return reinterpret_cast<T*>(slab);
    }
    template <class T = unsigned long long> const T* host() const
    {
        static_assert(sizeof(T) == sizeof(unsigned long long), "a slab holds 64-bit words");
        return reinterpret_cast<const T*>(pin);
    }
    size_t bytes() const { return sizeof(unsigned long long) * n_words; }

    // frees the slab and its mirror, forgets the counters and a pending request; the event stays
    void release()
    {
        if (slab) (void)hipFree(slab);
        if (pin) (void)hipHostFree(pin);
        slab = pin = nullptr;
        n_words = 0;
        n_acc = pend_n = 0;
        pending = false;
    }
    void destroy()
    {
        release();
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
    bool on() const { return slab != nullptr; }

    // a slab of n words (the caller has synchronised the stream), zeroed IN STREAM ORDER: the
    // engine's stream does not wait for the null stream, so a plain hipMemset could still be under
    // way when the first accumulation or read-out runs.  Released on any failure
    hipError_t alloc(size_t n, hipStream_t st)
    {
        release();
        hipError_t e = hipMalloc((void**)&slab, sizeof(unsigned long long) * n);
        if (e == hipSuccess) e = hipHostMalloc((void**)&pin, sizeof(unsigned long long) * n, hipHostMallocDefault);
        if (e == hipSuccess && !ev) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipMemsetAsync(slab, 0, sizeof(unsigned long long) * n, st);
        if (e == hipSuccess) n_words = n;
        else release();
        return e;
    }
    // queues the copy of the whole slab to its mirror and, behind it, the zeroing of the leading
    // n_zero_words: the interval closes.  n_zero_words == 0 is a peek: the interval stays open
    hipError_t copy_out(hipStream_t st, size_t n_zero_words)
    {
        hipError_t e = hipMemcpyAsync(pin, slab, bytes(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && n_zero_words)
            e = hipMemsetAsync(slab, 0, sizeof(unsigned long long) * n_zero_words, st);
        if (e != hipSuccess) return e;
        pend_n = n_acc;
        if (n_zero_words) n_acc = 0;
        return hipSuccess;
    }
    hipError_t mark(hipStream_t st)
    {
        const hipError_t e = hipEventRecord(ev, st);
        if (e == hipSuccess) pending = true;
        return e;
    }
    hipError_t wait()
    {
        const hipError_t e = hipEventSynchronize(ev);
        if (e == hipSuccess) pending = false;
        return e;
    }
    // n words from the host to the slab at word `at` (the caller has synchronised the stream)
    hipError_t upload(const void* words, size_t at, size_t n)
    {
        return n ? hipMemcpy(slab + at, words, sizeof(unsigned long long) * n, hipMemcpyHostToDevice) : hipSuccess;
    }
    hipError_t upload(const void* words) { return upload(words, 0, n_words); }
};
