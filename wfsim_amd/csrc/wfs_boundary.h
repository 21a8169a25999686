// Host side of a step boundary: wait for the sequence word that k_publish stores behind the scalar block (wfs_engine.hip read_scal).
// No HIP types: the stream is seen through a callable, so a host program can drive the loop with a thread in the device's place
// (tests/host/boundary_wait_main.cpp).
#pragma once
#include <chrono>
#include <cstdint>
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#endif

enum WfsQuery { WFS_QUERY_DONE = 0, WFS_QUERY_NOT_READY = 1, WFS_QUERY_ERROR = 2 };        // what the query callable says of the stream
enum WfsWait { WFS_WAIT_OK = 0, WFS_WAIT_FALLBACK = 1, WFS_WAIT_ERROR = 2 };

inline void wfs_cpu_pause()
{
#if defined(__x86_64__) || defined(__i386__)
    _mm_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#endif
}

inline uint64_t wfs_load_acquire(const uint64_t *word) { return __atomic_load_n(word, __ATOMIC_ACQUIRE); }

// Spins on *word until it holds seq (WFS_WAIT_OK: everything stored before the word's release store is visible).  The loop cannot
// hang on a word that never comes: every poll_us of waiting it asks query() for the state of the stream.
//   WFS_QUERY_NOT_READY  keep spinning
//   WFS_QUERY_DONE       the stream has run dry: one more load, then WFS_WAIT_FALLBACK (the caller fetches the block another way)
//   anything else        WFS_WAIT_ERROR (the callable keeps the error itself)
template <class Query>
inline WfsWait wfs_wait_seq(const uint64_t *word, uint64_t seq, Query &&query, int poll_us = 50)
{
    using clock = std::chrono::steady_clock;
    const auto poll = std::chrono::microseconds(poll_us);
    auto last = clock::now();
    for (unsigned spins = 1;; spins++) {
        if (wfs_load_acquire(word) == seq) return WFS_WAIT_OK;
        wfs_cpu_pause();
        if ((spins & 31u) != 0) continue;
        if (clock::now() - last < poll) continue;
        const int q = query();
        if (q == WFS_QUERY_DONE) return wfs_load_acquire(word) == seq ? WFS_WAIT_OK : WFS_WAIT_FALLBACK;
        if (q != WFS_QUERY_NOT_READY) return WFS_WAIT_ERROR;
        last = clock::now();
    }
}
