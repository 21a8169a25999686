// What a handle knows about the loaded batch and about the last run of it, and the only code that moves either from one state to
// the next.  A handle's state has three lifetimes: the handle's own (config, tables, maps, noise), the loaded batch's (BatchState)
// and the last run's (RunResult).  The two structs are reset by assignment of a value-initialised one, so a member added to either
// is reset with the rest.  No HIP types: tests/host/batch_state_main.cpp compiles this header with the host compiler.
#pragma once
#include <cstdint>
#include <vector>

typedef long long i64;        // (as wfs_device.h has them)
typedef int i32;

enum class BatchKind { None, Instructions, Photons, Optical };        // which wfs_load_* call committed the batch
// How far the last wfs_run of the batch came, in this order.  Generated: the photons are made (a run that stops there: wfs_set_debug
// bit 2).  Complete: the run came to its end and the device view still has the row layout it ran with, so everything can be copied
// out.  Finished: it came to its end, but the layout has changed since: records, counts and truth read as before, while the rows and
// intervals, which are decoded with the view's layout, are refused until the next run.
enum class RunStage { Nothing, Generated, Finished, Complete };

// Everything a wfs_load_* call and the per-instruction setters describe.  Reset when a load begins.
struct BatchState {
    BatchKind kind = BatchKind::None;
    i64 n_ins = 0, n_psets = 0, n_sets = 0, n_clusters = 0, n_emitters = 0, n_tiles = 0;
    i64 n_photons = 0;                // photons a photon or optical load brings (a generator batch makes its own: RunResult::n_gen_photons)
    bool ap_sets = false;                 // sets [n_psets, n_sets) are PMT afterpulse sets: an instruction or optical batch with afterpulses configured
    bool any_ptrs = false, run_sets_given = false, sets_aligned = true, any_s2 = false;
    // per-instruction options (wfs_set_instruction_*, wfs_eval_pattern_rows)
    bool ins_models = false, ins_gg_set = false, ins_aft_set = false;
    bool dev_rows_pending = false;        // rows of the device pattern map that wfs_eval_pattern_rows has yet to write
    i64 n_diff_rows = 0; double diff_r2 = 0;
    // host mirrors
    std::vector<i64> h_rs_off; std::vector<i32> h_rs_list;        // run set -> instructions
    std::vector<i64> h_set_off;       // photon batch: per set photon offsets (channel sorted input order)
    std::vector<i32> dev_row_ins;     // instructions whose channel row comes from the device pattern map, in row order
    std::vector<int8_t> h_ins_type; std::vector<uint8_t> ins_diff;        // instruction types; pattern averaged over the electrons (transverse diffusion)
    i64 n_host_rows = 0;              // channel rows the caller supplied; the device-evaluated ones follow
};

// What wfs_run found.  Reset when a run begins.
struct RunResult {
    RunStage stage = RunStage::Nothing;
    // generation (generator batches)
    bool fuse_on = false, fuse_full = false;
    i64 n_gen_photons = 0, p_fused = 0;
    i64 n_fused_tiles = 0 /* made by k_s2_tile */, n_gen_tiles = 0 /* tile-generated, pulse by the ordinary kernels */, n_bright_tiles = 0 /* made by k_s2_bright */;
    i64 n_ap_photons = 0;             // PMT afterpulse photons, behind the primary ones (0 without afterpulse sets)
    bool gen_order_ready = false;         // host tables of the generation order (gen_order_tables)
    std::vector<i64> go_off, go_block0; std::vector<i32> go_fused, go_tile_count;
    // geometry
    bool res_on = false;
    i64 n_groups = 0, n_front_rows = 0, n_res_rows = 0, n_short_rows = 0, n_active_rows = 0, n_res_tiles = 0, max_res_len = 0;
    i64 n_active_tiles = 0, n_tiny_tiles = 0, n_sparse_tiles = 0, n_dense_tiles = 0, n_wave_tiles = 0;
    i64 max_nb = 0, max_tile = 0, max_nb_dense = 0, max_tile_dense = 0;
    i64 s_raw = 0, s_raw_direct = 0, s_fin = 0, s_res = 0, s_sum = 0, sum_base = 0, n_sum_chunks = 0, n_itv_slots = 0;
    // records and debug copies
    i64 n_records = 0, cur_total = 0, row_dbg_total = 0;
};

// The transitions: nothing else writes BatchState::kind or RunResult::stage.
struct BatchRun {
    BatchState &batch; RunResult &run;
    // a wfs_load_* call passed its argument checks: no batch until it commits, so every error return in between leaves none
    void load_begins() const { batch = BatchState{}; run = RunResult{}; }
    void load_commits(BatchKind kind) const { batch.kind = kind; }
    // a per-instruction option or a delay table changed: what was generated no longer describes the batch
    void option_changed() const { run.stage = RunStage::Nothing; }
    void run_begins() const { run = RunResult{}; }
    void generation_done() const { run.stage = RunStage::Generated; }
    void run_complete() const { run.stage = RunStage::Complete; }
    // the device view no longer has the row layout of the last run: its rows and intervals cannot be decoded, so their copy-outs refuse
    void view_changed() const { if (run.stage == RunStage::Complete) run.stage = RunStage::Finished; }
};
