// Drives wfs_wait_seq (wfsim_amd/csrc/wfs_boundary.h) on the host: a std::thread plays the device, a counter plays hipStreamQuery.
// usage: boundary_wait_main <arrives|never|error>; prints one line "<case> <result> queries=<n> ms=<t>" and exits 0 when the
// result is the one the case must give (tests/test_boundary_wait_cpu.py).
#include "wfs_boundary.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

struct alignas(64) Block { uint64_t scal[64]; uint64_t seq; };

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s arrives|never|error\n", argv[0]); return 2; }
    const char *mode = argv[1];
    static Block b;
    memset(&b, 0, sizeof b);
    const uint64_t seq = 7;
    int queries = 0;
    const auto t0 = std::chrono::steady_clock::now();
    WfsWait w; bool ok = false;
    if (!strcmp(mode, "arrives")) {
        // the word arrives after the host has been told not-ready twice; the block stored before it must be visible
        std::atomic<int> polled{0};
        std::thread dev([&] {
            while (polled.load(std::memory_order_acquire) < 2) std::this_thread::yield();
            for (int i = 0; i < 64; i++) b.scal[i] = 1000 + i;
            __atomic_store_n(&b.seq, seq, __ATOMIC_RELEASE);
        });
        w = wfs_wait_seq(&b.seq, seq, [&] { queries++; polled.fetch_add(1, std::memory_order_release); return (int)WFS_QUERY_NOT_READY; });
        ok = w == WFS_WAIT_OK && queries >= 2;
        for (int i = 0; i < 64; i++) ok = ok && b.scal[i] == (uint64_t)(1000 + i);
        dev.join();
    } else if (!strcmp(mode, "never")) {
        // the stream has run dry and the word never changes (an older sequence number stays in it): fall back at the first query
        b.seq = seq - 1;
        w = wfs_wait_seq(&b.seq, seq, [&] { queries++; return (int)WFS_QUERY_DONE; });
        ok = w == WFS_WAIT_FALLBACK && queries == 1;
    } else if (!strcmp(mode, "error")) {
        // not-ready twice, then an error
        w = wfs_wait_seq(&b.seq, seq, [&] { return ++queries < 3 ? (int)WFS_QUERY_NOT_READY : 700; });
        ok = w == WFS_WAIT_ERROR && queries == 3;
    } else { fprintf(stderr, "unknown case %s\n", mode); return 2; }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("%s %s queries=%d ms=%.3f\n", mode, w == WFS_WAIT_OK ? "ok" : (w == WFS_WAIT_FALLBACK ? "fallback" : "error"), queries, ms);
    return ok ? 0 : 1;
}
