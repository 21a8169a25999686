// Drives PackFence (wfsim_amd/csrc/wfs_pack_fence.h) on the host as wfs_engine.hip does: a counting "device" plays the pack stream,
// the ready events and the waits.  Prints one line "<case> ok|FAILED ..." per case and exits 0 when every case holds
// (tests/test_pack_fence_cpu.py).
#include "wfs_pack_fence.h"
#include "wfs_devbuf.h"

#include <cstdio>
#include <cstdlib>

static int wfs_dev_alloc(void **p, size_t bytes) { *p = malloc(bytes); return *p ? 0 : 2; }
static void wfs_dev_free(void *p) { free(p); }

// The engine's side of the contract, with counters where it has HIP calls.  A pack "runs" from deferred until something waits for the
// event of its arena; a write, a free or a read of what it uses before that is a hazard.
struct Engine {
    PackFence pack;
    int rec_cur = 0;
    bool running = false;        // packers in flight that nothing has waited for (neither stream nor host)
    int recorded[2] = {0, 0};    // ready events recorded per arena
    int stream_waits = 0, host_waits = 0, hazards = 0;
    DevBuf tbuf, other;

    void host_wait() { if (pack.must_wait()) { host_waits++; running = false; pack.host_waited(); } }       // pack_wait
    void fence() { if (pack.take_fence()) { stream_waits++; running = false; } }                              // pack_fence
    void write_pack_buffer() { if (running) hazards++; }
    void grow(DevBuf &b, size_t bytes, bool pack_uses)                                                        // ensure
    {
        if (b.cap < (bytes ? bytes : 16) && pack.must_wait() && pack_uses) host_wait();
        if (b.cap < (bytes ? bytes : 16) && pack_uses && running) hazards++;       // the old block is freed under the packers
        if (b.ensure(bytes)) hazards++;
    }
    void run(bool tiles, bool defer, size_t tbuf_bytes)
    {
        // front end: electrons, block photons -- nothing here waits
        grow(other, 64, false);
        if (tiles) { fence(); grow(tbuf, tbuf_bytes, true); write_pack_buffer(); }
        fence();                                    // run_pulses, whether or not the tile path ran
        write_pack_buffer();
        rec_cur ^= 1;
        if (defer) { running = true; recorded[rec_cur]++; pack.deferred(rec_cur); }
    }
    void read_records() { host_wait(); if (running) hazards++; }
};

static int failures = 0;
static void report(const char *name, bool ok, const Engine &e)
{
    printf("%s %s stream_waits=%d host_waits=%d hazards=%d pending=%d fence_due=%d\n", name, ok ? "ok" : "FAILED", e.stream_waits, e.host_waits, e.hazards,
           (int)e.pack.pending, (int)e.pack.fence_due);
    if (!ok) failures++;
}

int main()
{
    {   // nothing deferred: nothing to wait for, however often it is asked
        Engine e;
        bool ok = !e.pack.must_wait() && !e.pack.take_fence() && !e.pack.take_fence();
        e.run(true, false, 100); e.read_records();
        ok = ok && e.stream_waits == 0 && e.host_waits == 0 && e.hazards == 0;
        report("idle", ok, e);
    }
    {   // pending -> fenced once per run -> waited by a reader
        Engine e;
        e.run(true, true, 100);
        bool ok = e.pack.pending && e.pack.fence_due && e.pack.arena == 1 && e.running;
        e.run(true, true, 100);                     // asks at the tile kernels and again at the pulses: one stream wait
        ok = ok && e.stream_waits == 1 && e.host_waits == 0 && e.pack.arena == 0 && e.pack.pending && e.pack.fence_due;
        e.run(false, true, 100);                    // without the tile path: the wait at the pulses
        ok = ok && e.stream_waits == 2 && e.host_waits == 0 && e.pack.arena == 1;
        e.read_records();
        ok = ok && e.host_waits == 1 && !e.pack.pending && !e.pack.fence_due && !e.running;
        e.read_records();                           // a second reader finds nothing to wait for
        ok = ok && e.host_waits == 1;
        e.run(true, true, 100);                     // and the next run has no fence to place
        ok = ok && e.stream_waits == 2 && e.hazards == 0;
        report("pending_fenced_read", ok, e);
    }
    {   // a reader on a stream of its own leaves the state alone: the next run still fences
        Engine e;
        e.run(true, true, 100);
        const bool waits = e.pack.must_wait();      // (the copy stream waits for ready[arena])
        e.run(true, true, 100);
        report("stream_reader_keeps_fence", waits && e.stream_waits == 1 && e.host_waits == 0 && e.hazards == 0, e);
    }
    {   // a grow of a buffer the packers use, while they are pending: the host waits before the old block is freed, and the fence is spent
        Engine e;
        e.run(true, true, 100);
        e.run(true, true, 100000);
        bool ok = e.hazards == 0 && e.host_waits == 1 && e.stream_waits == 1;      // (fence first, then the grow's host wait)
        e.grow(e.other, 1 << 20, false);            // another buffer grows without a wait
        ok = ok && e.host_waits == 1;
        Engine f;                                   // a grow in front of the fence (a load): the host wait stands in for the stream wait
        f.run(true, true, 100);
        f.grow(f.tbuf, 100000, true);
        ok = ok && f.host_waits == 1 && !f.pack.fence_due && f.hazards == 0;
        f.run(true, true, 100000);
        ok = ok && f.stream_waits == 0 && f.hazards == 0;
        report("grow_while_pending", ok, e);
    }
    {   // a serial run after a deferred one, with the mode change waiting in between (wfs_set_profiling)
        Engine e;
        e.run(true, true, 100);
        e.host_wait();
        e.run(true, false, 100);
        e.read_records();
        report("mode_change", e.host_waits == 1 && e.stream_waits == 0 && e.hazards == 0 && !e.pack.pending, e);
    }
    return failures ? 1 : 0;
}
