// A device buffer that frees itself.  No HIP types: the translation unit that includes this header defines the two functions declared
// below (wfs_engine.hip: hipMalloc / hipFree; tests/host/devbuf_main.cpp: a counting malloc / free), as wfs_boundary.h takes its
// stream query from the caller.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>

static int wfs_dev_alloc(void **p, size_t bytes);        // 0, or the allocator's error code (*p is not used then)
static void wfs_dev_free(void *p);

// Blocks and bytes that live DevBufs of this process hold (wfs_device_allocations): after the last handle is destroyed both are 0,
// which can be asserted exactly where the card's free-memory figure moves under other processes.
inline std::atomic<int64_t> wfs_dev_live_buffers{0}, wfs_dev_live_bytes{0};

struct DevBuf {
    void *p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    template <class T> T *as() const { return (T *)p; }
    void reset()
    {
        if (p) {
            wfs_dev_free(p);
            wfs_dev_live_buffers.fetch_sub(1, std::memory_order_relaxed);
            wfs_dev_live_bytes.fetch_sub((int64_t)cap, std::memory_order_relaxed);
        }
        p = nullptr; cap = 0;
    }
    // Room for bytes (0 counts as 16).  A buffer that has to grow is freed and allocated anew with an eighth and 256 bytes to spare;
    // its contents are not kept.  Returns wfs_dev_alloc's code; the buffer is empty after a failure.
    int ensure(size_t bytes)
    {
        if (bytes == 0) bytes = 16;
        if (cap >= bytes) return 0;
        reset();
        const size_t want = bytes + bytes / 8 + 256;
        void *q = nullptr;
        if (int e = wfs_dev_alloc(&q, want)) return e;
        p = q; cap = want;
        wfs_dev_live_buffers.fetch_add(1, std::memory_order_relaxed);
        wfs_dev_live_bytes.fetch_add((int64_t)want, std::memory_order_relaxed);
        return 0;
    }
};
