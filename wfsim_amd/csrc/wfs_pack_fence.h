// The packers of a batch (k_pack_desc, k_pack_res, k_pack) run on a stream of their own, under the front end of the next wfs_run.
// This is what the handle knows about packers that may still be running, and the only code that changes it.  It belongs to the
// handle's lifetime: run_begins() resets RunResult while a pack may be in flight.  No HIP types: the engine does the waits the
// answers ask for (wfs_engine.hip: pack_fence, pack_wait), tests/host/pack_fence_main.cpp plays them with the host compiler.
//
// The packers of successive batches are serialised on the one pack stream, so the ready event of the newest pack covers every older
// one: one pending pack, and the arena it writes, is all there is to remember.
#pragma once

struct PackFence {
    bool pending = false;        // packers were handed to the pack stream and the host has not waited for them since
    bool fence_due = false;      // ... and the main stream has not been made to wait for them either
    int arena = 0;               // the record arena they write: its ready event is the one to wait on

    // run_records handed the packers of `arena` to the pack stream and recorded the arena's ready event behind them
    void deferred(int a) { pending = true; fence_due = true; arena = a; }
    // A run reaches its first write to a buffer the packers read.  True: put one stream wait for ready[arena] on the main stream.
    // True once per deferred pack, however many places of a run ask.
    bool take_fence() { const bool due = fence_due; fence_due = false; return due; }
    // A reader of the records, a grow of a buffer the packers read, a setter of a table they read, a change of mode: true -> wait on
    // the host for ready[arena], then call host_waited().  (A reader that waits on a stream instead leaves the state as it is.)
    bool must_wait() const { return pending; }
    void host_waited() { pending = false; fence_due = false; }
};
