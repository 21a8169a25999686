// Drives the batch and run state of a handle (wfsim_amd/csrc/wfs_batch.h) on the host: the transitions are the only writers of the
// batch's kind and the run's stage, and a reset is an assignment of a value-initialised struct.
// Prints one line "<case> ok|FAILED" per case and exits 0 when every case holds (tests/test_batch_state_cpu.py).
#include "wfs_batch.h"

#include <cstdio>
#include <tuple>

// Every member of the two structs, once.  The structured bindings below name as many members as the structs have, so a member added
// to wfs_batch.h stops this file from compiling until it is listed here -- and then every "back at its initial value" check covers it.
static auto members(const BatchState &b)
{
    const auto &[kind, n_ins, n_psets, n_sets, n_clusters, n_emitters, n_tiles, n_photons, ap_sets, any_ptrs, run_sets_given, sets_aligned,
                 any_s2, ins_models, ins_gg_set, ins_aft_set, dev_rows_pending, n_diff_rows, diff_r2, h_rs_off, h_rs_list, h_set_off,
                 dev_row_ins, h_ins_type, ins_diff, n_host_rows] = b;
    return std::tie(kind, n_ins, n_psets, n_sets, n_clusters, n_emitters, n_tiles, n_photons, ap_sets, any_ptrs, run_sets_given, sets_aligned,
                    any_s2, ins_models, ins_gg_set, ins_aft_set, dev_rows_pending, n_diff_rows, diff_r2, h_rs_off, h_rs_list, h_set_off,
                    dev_row_ins, h_ins_type, ins_diff, n_host_rows);
}

static auto members(const RunResult &r)
{
    const auto &[stage, fuse_on, fuse_full, n_gen_photons, p_fused, n_fused_tiles, n_gen_tiles, n_bright_tiles, n_ap_photons, gen_order_ready,
                 go_off, go_block0, go_fused, go_tile_count, res_on, n_groups, n_front_rows, n_res_rows, n_short_rows, n_active_rows,
                 n_res_tiles, max_res_len, n_active_tiles, n_tiny_tiles, n_sparse_tiles, n_dense_tiles, n_wave_tiles, max_nb, max_tile,
                 max_nb_dense, max_tile_dense, s_raw, s_raw_direct, s_fin, s_res, s_sum, sum_base, n_sum_chunks, n_itv_slots, n_records,
                 cur_total, row_dbg_total] = r;
    return std::tie(stage, fuse_on, fuse_full, n_gen_photons, p_fused, n_fused_tiles, n_gen_tiles, n_bright_tiles, n_ap_photons, gen_order_ready,
                    go_off, go_block0, go_fused, go_tile_count, res_on, n_groups, n_front_rows, n_res_rows, n_short_rows, n_active_rows,
                    n_res_tiles, max_res_len, n_active_tiles, n_tiny_tiles, n_sparse_tiles, n_dense_tiles, n_wave_tiles, max_nb, max_tile,
                    max_nb_dense, max_tile_dense, s_raw, s_raw_direct, s_fin, s_res, s_sum, sum_base, n_sum_chunks, n_itv_slots, n_records,
                    cur_total, row_dbg_total);
}

template <class T> static bool same(const T &a, const T &b) { return members(a) == members(b); }
template <class T> static bool initial(const T &a) { return same(a, T{}); }

// a batch with every option set, every count non-zero and every host mirror non-empty
static void fill(BatchState &b, bool ap)
{
    b.n_ins = 7; b.n_psets = 7; b.n_sets = ap ? 14 : 7; b.n_clusters = 3; b.n_emitters = 900; b.n_tiles = b.n_sets * 494; b.n_photons = 12345;
    b.ap_sets = ap; b.any_ptrs = true; b.run_sets_given = true; b.sets_aligned = false; b.any_s2 = true;
    b.ins_models = true; b.ins_gg_set = true; b.ins_aft_set = true; b.dev_rows_pending = true; b.n_diff_rows = 2; b.diff_r2 = 66.4 * 66.4;
    b.h_rs_off = {0, 3, 7}; b.h_rs_list = {0, 1, 2, 3, 4, 5, 6}; b.h_set_off = {0, 10, 20}; b.dev_row_ins = {1, 4};
    b.h_ins_type = {1, 2, 2, 1, 2, 4, 6}; b.ins_diff = {0, 1, 0, 0, 1, 0, 0}; b.n_host_rows = 5;
}

// what a complete run leaves: every counter non-zero, the order tables built
static void fill(RunResult &r)
{
    r.fuse_on = r.fuse_full = r.gen_order_ready = r.res_on = true;
    r.go_off = {0, 5}; r.go_block0 = {0}; r.go_fused = {1}; r.go_tile_count = {2, 3};
    long long v = 1;
    for (long long *p : {&r.n_gen_photons, &r.p_fused, &r.n_fused_tiles, &r.n_gen_tiles, &r.n_bright_tiles, &r.n_ap_photons, &r.n_groups, &r.n_front_rows,
                         &r.n_res_rows, &r.n_short_rows, &r.n_active_rows, &r.n_res_tiles, &r.max_res_len, &r.n_active_tiles, &r.n_tiny_tiles,
                         &r.n_sparse_tiles, &r.n_dense_tiles, &r.n_wave_tiles, &r.max_nb, &r.max_tile, &r.max_nb_dense, &r.max_tile_dense, &r.s_raw,
                         &r.s_raw_direct, &r.s_fin, &r.s_res, &r.s_sum, &r.sum_base, &r.n_sum_chunks, &r.n_itv_slots, &r.n_records, &r.cur_total,
                         &r.row_dbg_total}) *p = v++;
}

static int failures = 0;
static void report(const char *name, bool ok)
{
    printf("%s %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) failures++;
}

// a load of the kind, every option set, run to its end
static void load_and_run(const BatchRun &s, BatchKind kind, bool ap)
{
    s.load_begins(); fill(s.batch, ap); s.load_commits(kind);
    s.run_begins(); fill(s.run); s.generation_done(); s.run_complete();
}

int main()
{
    const BatchKind kinds[3] = {BatchKind::Instructions, BatchKind::Photons, BatchKind::Optical};
    {
        BatchState b; RunResult r;
        report("fresh", b.kind == BatchKind::None && r.stage == RunStage::Nothing && initial(b) && initial(r));
        // (the fill helpers leave nothing at its initial value but the kind and the stage: what the reset cases below rely on)
        BatchState f; RunResult g;
        fill(f, true); fill(g);
        bool every = true;
        {
            const auto &[kind, n_ins, n_psets, n_sets, n_clusters, n_emitters, n_tiles, n_photons, ap_sets, any_ptrs, run_sets_given, sets_aligned,
                         any_s2, ins_models, ins_gg_set, ins_aft_set, dev_rows_pending, n_diff_rows, diff_r2, h_rs_off, h_rs_list, h_set_off,
                         dev_row_ins, h_ins_type, ins_diff, n_host_rows] = f;
            (void)kind;
            every = every && n_ins && n_psets && n_sets && n_clusters && n_emitters && n_tiles && n_photons && ap_sets && any_ptrs && run_sets_given
                    && !sets_aligned && any_s2 && ins_models && ins_gg_set && ins_aft_set && dev_rows_pending && n_diff_rows && diff_r2 != 0
                    && !h_rs_off.empty() && !h_rs_list.empty() && !h_set_off.empty() && !dev_row_ins.empty() && !h_ins_type.empty() && !ins_diff.empty()
                    && n_host_rows;
        }
        {
            const auto &[stage, fuse_on, fuse_full, n_gen_photons, p_fused, n_fused_tiles, n_gen_tiles, n_bright_tiles, n_ap_photons, gen_order_ready,
                         go_off, go_block0, go_fused, go_tile_count, res_on, n_groups, n_front_rows, n_res_rows, n_short_rows, n_active_rows,
                         n_res_tiles, max_res_len, n_active_tiles, n_tiny_tiles, n_sparse_tiles, n_dense_tiles, n_wave_tiles, max_nb, max_tile,
                         max_nb_dense, max_tile_dense, s_raw, s_raw_direct, s_fin, s_res, s_sum, sum_base, n_sum_chunks, n_itv_slots, n_records,
                         cur_total, row_dbg_total] = g;
            (void)stage;
            every = every && fuse_on && fuse_full && n_gen_photons && p_fused && n_fused_tiles && n_gen_tiles && n_bright_tiles && n_ap_photons
                    && gen_order_ready && !go_off.empty() && !go_block0.empty() && !go_fused.empty() && !go_tile_count.empty() && res_on && n_groups
                    && n_front_rows && n_res_rows && n_short_rows && n_active_rows && n_res_tiles && max_res_len && n_active_tiles && n_tiny_tiles
                    && n_sparse_tiles && n_dense_tiles && n_wave_tiles && max_nb && max_tile && max_nb_dense && max_tile_dense && s_raw && s_raw_direct
                    && s_fin && s_res && s_sum && sum_base && n_sum_chunks && n_itv_slots && n_records && cur_total && row_dbg_total;
        }
        report("fill_sets_every_member", every);
    }
    {   // begin, commit: the kind is None until the commit
        bool ok = true;
        for (BatchKind k : kinds) {
            BatchState b; RunResult r; const BatchRun s{b, r};
            s.load_begins();
            ok = ok && b.kind == BatchKind::None;
            b.n_ins = 3;
            ok = ok && b.kind == BatchKind::None;
            s.load_commits(k);
            ok = ok && b.kind == k && b.n_ins == 3 && r.stage == RunStage::Nothing;
        }
        report("begin_commit_each_kind", ok);
    }
    {   // a load that begins and never commits leaves no batch, whatever was there
        bool ok = true;
        for (BatchKind k : kinds) {
            BatchState b; RunResult r; const BatchRun s{b, r};
            load_and_run(s, k, true);
            ok = ok && b.kind == k && r.stage == RunStage::Complete;
            s.load_begins();
            b.n_ins = 9; b.n_tiles = 9 * 494;         // (the loader got as far as its sizes and then returned an error)
            ok = ok && b.kind == BatchKind::None && r.stage == RunStage::Nothing && initial(r);
        }
        report("begin_without_commit_leaves_none", ok);
    }
    {   // a new load clears every option, count and mirror of the batch before it, and the run's results
        bool ok = true;
        for (BatchKind k0 : kinds) for (BatchKind k1 : kinds) {
            BatchState b; RunResult r; const BatchRun s{b, r};
            load_and_run(s, k0, true);
            ok = ok && !initial(b) && !initial(r);
            s.load_begins();
            ok = ok && initial(b) && initial(r);
            s.load_commits(k1);
            BatchState want; want.kind = k1;
            ok = ok && same(b, want) && initial(r);
        }
        report("new_load_clears_previous_batch", ok);
    }
    {   // afterpulse sets do not outlive the batch that had them
        BatchState b; RunResult r; const BatchRun s{b, r};
        load_and_run(s, BatchKind::Instructions, true);
        bool ok = b.ap_sets;
        s.load_begins(); b.n_sets = 4; b.n_photons = 100; s.load_commits(BatchKind::Photons);
        ok = ok && !b.ap_sets && b.n_psets == 0 && b.kind == BatchKind::Photons;
        report("ap_sets_false_after_photon_load", ok);
    }
    {   // a per-instruction option changed after the generation (or after the whole run): the stage is Nothing, the batch stays
        bool ok = true;
        for (int complete = 0; complete < 2; complete++) {
            BatchState b; RunResult r; const BatchRun s{b, r};
            s.load_begins(); fill(b, false); s.load_commits(BatchKind::Instructions);
            s.run_begins(); s.generation_done();
            if (complete) s.run_complete();
            const BatchState before = b;
            s.option_changed();
            ok = ok && r.stage == RunStage::Nothing && same(b, before) && b.kind == BatchKind::Instructions;
        }
        report("option_changed_after_generation", ok);
    }
    {   // a run begins: the results of the run before are gone, the batch stays; twice in a row
        BatchState b; RunResult r; const BatchRun s{b, r};
        load_and_run(s, BatchKind::Optical, true);
        const BatchState before = b;
        bool ok = true;
        for (int pass = 0; pass < 2; pass++) {
            s.run_begins();
            ok = ok && initial(r) && same(b, before);
            fill(r); s.generation_done();
            ok = ok && r.stage == RunStage::Generated;
            s.run_complete();
            ok = ok && r.stage == RunStage::Complete && r.n_records != 0 && same(b, before);
        }
        report("run_begins_resets_results", ok);
    }
    {   // the device view changed: Complete falls back, nothing else moves; from below Complete nothing moves at all
        BatchState b; RunResult r; const BatchRun s{b, r};
        load_and_run(s, BatchKind::Instructions, false);
        const BatchState before = b;
        RunResult want = r;
        s.view_changed();
        want.stage = RunStage::Finished;
        bool ok = r.stage != RunStage::Complete && r.stage > RunStage::Generated && same(r, want) && same(b, before) && b.kind == BatchKind::Instructions;
        s.view_changed();
        ok = ok && same(r, want);
        s.run_begins(); s.generation_done();
        s.view_changed();
        ok = ok && r.stage == RunStage::Generated && same(b, before);
        s.option_changed();
        s.view_changed();
        ok = ok && r.stage == RunStage::Nothing && same(b, before);
        s.run_begins(); s.generation_done(); s.run_complete();
        ok = ok && r.stage == RunStage::Complete;
        report("view_changed_falls_back_from_complete", ok);
    }
    return failures ? 1 : 0;
}
