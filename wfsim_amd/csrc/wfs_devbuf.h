// A device buffer that frees itself (DevBuf: bytes) and the typed array on top of it (DevArr<T>: elements).  No HIP types: the
// translation unit that includes this header defines the two functions declared below (wfs_engine.hip: hipMalloc / hipFree;
// tests/host/devbuf_main.cpp: a counting malloc / free), as wfs_boundary.h takes its stream query from the caller.
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
    bool grows(size_t bytes) const { return cap < (bytes ? bytes : 16); }        // would ensure(bytes) allocate?
    // Room for bytes (0 counts as 16).  A buffer that has to grow is freed and allocated anew with an eighth and 256 bytes to spare;
    // its contents are not kept.  Returns wfs_dev_alloc's code; the buffer is empty after a failure.
    int ensure(size_t bytes)
    {
        if (!grows(bytes)) return 0;
        if (bytes == 0) bytes = 16;
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

// A device array of T: the element type stands in the declaration, the pointer is typed and every size is a count of elements.
// It owns a DevBuf and is none: a helper that takes a DevBuf and a size in bytes does not take a DevArr.  buf() is the block's
// identity and capacity for whoever compares buffers of different T.
template <class T> struct DevArr {
    T *p() const { return (T *)b.p; }
    const DevBuf &buf() const { return b; }
    void reset() { b.reset(); }
    bool grows(size_t count) const { return b.grows(count * sizeof(T)); }
    int ensure(size_t count) { return b.ensure(count * sizeof(T)); }        // room for count elements: DevBuf::ensure's rule and result
private:
    DevBuf b;
};
