// kv_mem.h -- the owners of device memory every source shares: a scoped buffer, the grow-only arena and the per-stream
// registry the arenas are kept in.  Included by kv_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>

// kv_host.hip (kv_internal.h says what they do)
hipError_t kv_hip_malloc(void **p, size_t bytes);
hipStream_t kv_stream_key(hipStream_t st);
void kv_thread_device();

// device buffer of one call: freed on scope exit
struct KvDevBuf {
    void *p = nullptr;
    ~KvDevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return kv_hip_malloc(&p, n ? n : 4); }
    template <typename T> T *as() { return (T *)p; }
};

// grow-only device scratch, kept between calls (hipMalloc / hipFree of gigabytes cost a hundred milliseconds); whoever keeps
// one releases it: there is no destructor, the registries below live until the process ends
struct KvArena {
    void *p = nullptr;
    size_t bytes = 0;
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    // an eighth of headroom: the geometry of the next batch (bucket sizes follow the previous batch's statistics) may
    // ask for a little more
    hipError_t need(size_t n)
    {
        if (n <= bytes) return hipSuccess;
        kv_thread_device();
        release();
        if (hipMalloc(&p, n + n / 8) == hipSuccess) { bytes = n + n / 8; return hipSuccess; }
        (void)hipGetLastError();
        p = nullptr;
        return need_exact(n);
    }
    // the same without headroom, for buffers whose size follows the caller's input and not a guess
    hipError_t need_exact(size_t n)
    {
        if (n <= bytes) return hipSuccess;
        release();
        const hipError_t e = kv_hip_malloc(&p, n);      // (gives the table cache and idle first-toucher arrays back before it fails)
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
};

// Consecutive pieces of an arena, or of one call's buffer, each rounded up to a multiple of 256 bytes.  The pieces' sizes are
// listed once: the arena is grown (the buffer allocated) to their sum and at<T>(i) is where piece i begins, so the two cannot
// disagree.  A piece of 0 bytes begins where the next one does.
template <size_t N>
struct KvCarve {
    size_t off[N + 1];
    unsigned char *base = nullptr;
    KvCarve(const size_t (&bytes)[N])
    {
        off[0] = 0;
        for (size_t i = 0; i < N; ++i) off[i + 1] = off[i] + (bytes[i] + 255) / 256 * 256;
    }
    size_t total() const { return off[N]; }
    hipError_t from(KvArena &a) { const hipError_t e = a.need(total()); base = (unsigned char *)a.p; return e; }
    hipError_t from(KvDevBuf &b) { const hipError_t e = b.alloc(total()); base = (unsigned char *)b.p; return e; }     // freed with b
    template <typename T> T *at(size_t i) const { return (T *)(base + off[i]); }
};

// One T per stream, so host threads working on different streams do not share buffers; keyed by kv_stream_key (a stream made by
// kv_stream_create finds the buffers of the stream that had its slot before).  References stay valid: entries are never erased.
// The mutex guards the map alone; a T that two threads may reach at once brings its own lock.
template <typename T>
struct KvPerStream {
    std::mutex mu;
    std::map<hipStream_t, T> by_key;
    T &get(hipStream_t st)
    {
        const hipStream_t key = kv_stream_key(st);
        std::lock_guard<std::mutex> lk(mu);
        return by_key[key];
    }
    template <typename F>
    void for_each(F f)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &kv : by_key) f(kv.second);
    }
};
