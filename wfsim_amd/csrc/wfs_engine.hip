// wfs_engine.hip -- host side of libwfsim_amd.so: the C ABI of include/wfsim_amd.h, device memory arenas,
// stage orchestration on one HIP stream (the record packers of a batch on a second one, under the next run: wfs_pack_fence.h).
// gfx950 (MI355X) only.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "wfs_kernels.h"
#include "wfs_tilegen.h"
#include "wfs_boundary.h"
#include "wfs_devbuf.h"
#include "wfs_family.h"
#include "wfs_batch.h"
#include "wfs_pack_fence.h"
#include "../../include/wfsim_amd.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

namespace {

struct Pmf { std::vector<double> p; long vmin = 0; };      // probability mass function of an integer delay term

struct ApElem { int n_bins_delay = 0, n_bins_amp = 0, amp_2d = 0, is_uniform = 0; double delay_bin = 0, amp_bin = 0; DevArr<double> delay_cdf, amp_cdf, prob; DevArr<u32> thr; DevArr<ApGuide> delay_guide, amp_guide;
                std::vector<double> prob_h; double thr_mod = -1.0;      // host copy of the probability column; modifier the thresholds were built for
                int delay_sorted = 0, amp_sorted = 0; };

struct KernelTime { std::string name; hipEvent_t a, b; };
inline void clear_times(std::vector<KernelTime> &times)
{
    for (auto &t : times) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
    times.clear();
}

// bits of wfs_set_debug (wfs_handle::debug_bits); include/wfsim_amd.h documents them by number
enum : int {
    DBG_CURRENTS = 1,            // keep the f64 tile currents and the finished rows
    DBG_FORCE_DENSE = 2,         // every tile to the dense pulse kernel
    DBG_GEN_ONLY = 4,            // wfs_run stops after the photon generation
    DBG_CHECK_LAUNCHES = 8,      // check every kernel launch on the spot
    DBG_KEEP_PHOTONS = 16        // store the photons of tile-generated instructions
};

// elements per item of the arrays that hold several, as the kernels index them (wfs_kernels.h, wfs_tilegen.h)
constexpr size_t TRUTH_PER_SET = 16;       // truth[set][16]: the sums of a pulse set, the moments of its photon times behind them (k_truth_reduce)
constexpr size_t TRUTH_PER_TILE = 8;       // tile_truth[tile][8]: the partial sums of one tile
constexpr size_t STAT_PER_INS = 4;         // el_stat[ins][4]: n, sum t, sum t^2 of its electrons
constexpr size_t MINMAX = 2;               // (min, max) pairs of tminmax[set] and el_minmax[ins]; (first, last) emitter of blk_e[block]

}  // namespace

// the allocator of wfs_devbuf.h
static int wfs_dev_alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
static void wfs_dev_free(void *p) { (void)hipFree(p); }

// What orders the records of a row list by (time, channel) (order_records): keys and record indices in and out of the sort, each record's sorted slot
struct RecOrder { DevArr<u64> key, key2; DevArr<u32> val, val2, dest; };
struct wfs_handle {
    // ---------------- the handle: written by wfs_create and the wfs_set_* calls, kept until wfs_destroy; no load and no run resets it
    // device and streams
    int device = 0, n_cus = 256;
    hipStream_t stream = nullptr; bool own_stream = false;
    WfsScal *h_scal = nullptr;        // host copy of scal in page-locked memory: read_scal's copy needs no staging buffer (five of them per batch)
    // step boundaries that publish (read_scal): h_scal is mapped and coherent, k_publish copies the block into it and stores the
    // sequence number of the boundary into the word on the cache line behind it; the host spins on that word (wfs_boundary.h)
    bool publish = false;             // false: the copy + synchronise path (the mapped allocation failed, or WFS_HOST_SYNC=copy)
    uint64_t *h_seq = nullptr; u64 *d_hseq = nullptr, seq = 0; WfsScal *d_hscal = nullptr;
    i64 zero64 = 0;                   // host source of the one value an empty scan uploads (scan_into)
    std::string err, launch_err; // wfs_last_error; first failed launch of the current call (wfs_set_debug bit 3: every launch is checked)
    int n_fail = 0;             // calls of fail(): a FillGroup that dies with segments checks that an error return is why
    int fail(int code, const std::string &msg) { err = msg; n_fail++; return code; }

    // config and device view: dev is what the kernels see, rebuilt from cfg and the switches below by refresh_dev
    wfs_config cfg; WfsDev dev;
    bool generic_geom = false;            // sample_duration / template length other than 10 ns / 22 samples: k_pulse_generic for every tile
    i32 res_env = -1;                // WFS_ROW_RESIDENT=0/1 overrides the config switch (A/B runs)
    i32 res_max_len = 1024;          // segment of a resident row (k_row_pulse: 4 bytes of LDS per sample and wave; longer rows take several); WFS_RES_MAX_LEN overrides
    int tap_sparse_max = 48;     // tap_block: occupied cells up to which a wave of the dense pulse kernels walks them (WFS_TAP_SPARSE_MAX)
    i32 bright_lds = 0, bright_max_bins = 0;      // LDS a bright tile may take for H table + ballots (device grant, BRIGHT_LDS_MAX); start bins (WFS_BRIGHT_MAX_BINS)
    bool bright_on = true, sum_on = false, sort_records = false;      // wfs_set_bright_tiles, wfs_set_sum_signal (one more row slot per window), wfs_set_record_order
    int carry_has = 0; i64 carry_runmax = 0, n_noise_override = 0;    // wfs_set_window_carry; wfs_set_noise_offsets
    bool full_on = false;            // wfs_set_full_readout: every row slot of a digitise window has a row of the window's range
    i64 full_max_samples = (i64)1 << 36;      // most finished samples of rows without a pulse in one batch (128 GiB of them); WFS_FULL_READOUT_MAX_SAMPLES overrides

    // tables, maps and noise
    bool tables_set = false;
    std::vector<double> h_templates, h_gains, h_lum_x, h_lum_t;      // host copies: [dt][tlen]; per channel; the luminescence table (enters the S2 delay table)
    ApElem ap[WFS_MAX_AP];
    // model variants of the photon delays
    std::vector<DevArr<uint2>> x_alias; std::vector<AliasTab> h_tabs; i32 n_user_tabs = 0;
    std::vector<Pmf> base_pmf;           // transit time only, S1 terms, S2 terms, S2 terms without the 'simple' luminescence
    i32 prop_nz = 0, prop_nu = 0; double prop_u0 = 0, prop_du = 1;      // wfs_set_s1_propagation
    i32 gg_n = 0, gg_L = 0;              // 'garfield_gas_gap' luminescence (wfs_set_gas_gap_model)
    // pattern maps evaluated on the device
    struct PatternMap { bool set = false; i32 dims = 0, n[3] = {1, 1, 1}, w[3] = {0, 0, 0}, n_map_ch = 0; double lo[3] = {0, 0, 0}, hgrid[3] = {1, 1, 1}; DevArr<float> values;
                        i64 n_points = 0; DevArr<double> points;
                        DevArr<i32> cell_start, cell_pts; i32 cnx = 0, cny = 0; double cell_lo[2] = {0, 0}, cell_h = 1; } pmap[2];       // 2-D point lists: cell index (transverse diffusion)
    // scalar maps (kind 0: weighted nearest neighbours on a regular grid, 1: on a point list, 2: RectBivariateSpline)
    struct ScalarMap { int kind = 0; int nv = 1; PatternMap g; DevArr<double> values; i32 nx = 0, ny = 0, kx = 0, ky = 0; DevArr<double> tx, ty, c; };      // kind 0 / 1: nearest neighbours on a grid / a point list, 2: spline, 3: multilinear grid
    std::vector<std::unique_ptr<ScalarMap>> smaps;
    // the noise model, its colour and its slow levels (wfs_noise.h): written by the transitions alone, which name the device buffers
    // (nm_cells, nc_buf: NoiseColourLayout, ns_buf: NoiseSlowLayout) that go with what they reset
    NoiseModelState noise;
    NoiseTransitions noise_state() { return NoiseTransitions{noise}; }
    void noise_moves(unsigned dropped)
    {
        if (dropped & NOISE_BUF_CELLS) nm_cells.reset();
        if (dropped & NOISE_BUF_COLOUR) nc_buf.reset();
        if (dropped & NOISE_BUF_SLOW) ns_buf.reset();
    }
    i32 table_channels = 0;           // columns of the noise table (dev.noise_channels counts the model's channels while a model is set)
    // PMT dark counts (wfs_dark.h): the thresholds as dk_thr holds them; written by wfs_set_dark_counts alone
    DarkState dark;

    // packed records: two arenas used in turn, so that the device -> host copy of one batch (copy stream, pinned host memory)
    // runs under the kernels of the next batch
    DevBuf records_ab[2]; int rec_cur = 0; hipStream_t copy_stream = nullptr; hipEvent_t rec_copied[2] = {nullptr, nullptr}; bool rec_pending[2] = {false, false};
    DevBuf &records_buf() { return records_ab[rec_cur]; }
    // the packers of a batch on a stream of their own, under the front end of the next run (wfs_pack_fence.h): pack_go[a] is recorded on
    // the main stream once everything the packers of arena a read is written, rec_ready[a] on the pack stream behind them
    hipStream_t pack_stream = nullptr; hipEvent_t pack_go[2] = {nullptr, nullptr}, rec_ready[2] = {nullptr, nullptr}; PackFence pack;
    bool pack_sync = false;           // WFS_PACK_SYNC=1: the packers stay on the main stream in front of the last boundary (A/B runs, tests)

    // profiling and debug
    int debug_bits = 0, profiling = 0;      // wfs_set_debug (DBG_*), wfs_set_profiling
    std::vector<KernelTime> times;

    // ---------------- the loaded batch: reset when a wfs_load_* call begins, filled by that call and the per-instruction setters
    BatchState batch;
    // ---------------- the last run: reset when wfs_run begins (and with the batch)
    RunResult run;
    // kernel arguments of the last generation (HIP types, hence not in RunResult): written by every generation, read from stage Generated on
    GenArgs gen_args{}; FuseArgs fuse_args{}; BrightArgs bright_args{};      // (gen_args: kept for wfs_gather_photon_times)
    BatchRun state() { return BatchRun{batch, run}; }        // the transitions of wfs_batch.h: the only writers of batch.kind and run.stage

    // ---------------- device buffers: capacity, not state.  They grow on demand, free themselves, and no reset touches them
    // (the element type stands in the declaration and every size is a count: wfs_devbuf.h; bytes: the record arenas above and sort_tmp)
    DevArr<u32> set_gid, opt_item; DevArr<i32> opt_t, opt_first, opt_last, opt_ch; DevArr<i64> opt_time;
    DevArr<double> t_templates, t_spe, t_gains, t_thr_truth, t_lumx, t_lumt, t_noise_f; DevArr<i64> t_thr_zle; DevArr<int16_t> t_noise;
    DevArr<int8_t> ins_type; DevArr<i64> ins_time, em_off, set_ins_off; DevArr<i32> ins_amp, ins_cdfrow, ins_set, set_ins_list; DevArr<u32> ins_gid, ins_embase;
    DevArr<double> ins_p, ins_dm, ins_ds, ins_sc, cdf_table, em_zg; DevArr<uint2> chan_alias;
    DevArr<i32> set_cluster, set_mode, cl_group; DevArr<i64> set_t0, cl_tmin, cl_end; DevArr<u32> cl_gid;
    DevArr<i64> em_time, em_ph_off, el_minmax, blk_e, ins_ph0; DevArr<i32> em_nph, em_ins, blk_ins, eblk_ins; DevArr<double> el_stat; DevArr<u32> blk_base;
    DevArr<unsigned short> blk_cnt; DevArr<BlockDesc> blk_desc;
    DevArr<i32> tile_count, tile_cursor, tile_tmin, tile_tmax, active_tiles, sparse_tiles, dense_tiles, wave_tiles; DevArr<i64> tile_off;
    DevArr<PhotonRec> ph; DevArr<double> ph_gain; DevArr<u32> ph_idx, ap_key, ins_sbase; DevArr<OrderRange> order_list, order_list2; DevArr<i32> tile_tail, tile_tailbase, ins_fullsort;
    DevArr<i64> grp_lo, grp_hi, grp_left, grp_right, grp_ixrand; DevArr<u32> grp_gid;
    DevArr<i64> row_lo, row_hi, acc_off, itv_off; DevArr<i32> acc_len, itv_cap, active_rows, raw;
    DevArr<i64> itv_left, itv_right, rec_off; DevArr<i32> itv_n, row_nrec;
    DevArr<double> truth, tile_truth, currents; DevArr<i64> tminmax, gather_idx, gather_out, cur_off, row_dbg_off; DevArr<TileDesc> tile_desc; DevArr<i32> row_dbg; DevArr<TileTimeReq> gather_req;      // (wfs_gather_photon_times: the requests of tile-generated instructions; gather_idx holds those of the block generator)
    DevArr<unsigned long long> stamps; DevArr<RowDesc> row_desc; RecOrder rec; DevBuf sort_tmp;      // (sort_tmp: rocPRIM's scratch, of every rocPRIM call of the file: two_step)
    DevArr<i64> scan_tmp, noise_override; DevArr<WfsScal> scal; DevArr<NoiseCell> nm_cells; DevArr<i32> nc_buf, ns_buf; DevArr<u32> dk_thr; DevArr<PackDesc> pack_desc;
    DevArr<i32> row_bad, fin_len, res_cnt, res_long; DevArr<i64> fin_off, res_toff; DevArr<TileDesc> res_desc; DevArr<int16_t> fin; DevArr<ResRow> res_rows;      // resident rows (k_row_pulse)
    DevArr<uint2> tt_alias[6]; DevArr<i32> ap_ins, ap_ch, ap_t; DevArr<double> ap_gain; DevArr<ApCand> ap_cand; DevArr<ApArgs> ap_args_dev; DevArr<ApSeg> ap_seg;
    DevArr<AliasTab> d_tabs; DevArr<double> prop_top, prop_bot, ins_pzf, gg_inv, ins_ggw; DevArr<i32> ins_tab, ins_tabb, ins_pzi, ins_gg; DevArr<i64> ins_ggsum;
    DevArr<double> pois_cdf; DevArr<i32> pois_kmin;         // Poisson tables of the secondary gain per instruction (k_poisson_tables)
    DevArr<double> smap_pos, smap_out, smap_nb_w, ins_aft; DevArr<i64> smap_nb_idx;
    // transverse diffusion with field maps: instructions whose pattern is averaged over their electrons (k_diffuse_patterns)
    DevArr<double> ins_sigr, ins_siga, diff_pre; DevArr<i32> diff_row_ins; DevArr<i64> diff_row_id;
    DevArr<i32> map_row_ins[2]; DevArr<i64> map_row_id[2], map_nb_idx[2]; DevArr<float> map_x, map_y, map_z; DevArr<double> map_nb_w[2];
    // tile-local generation (wfs_tilegen.h): S2 instructions whose photons are made inside the pulse workgroup
    DevArr<i64> huge_start, huge_cbeg; DevArr<u32> huge_keys, huge_keys2, huge_vals, huge_vals2; DevArr<PhotonRec> huge_rec; DevArr<double> huge_gain;      // ordering of tiles beyond TILE_ORDER_MAX photons
    DevArr<double> row_pmax; DevArr<i32> ins_fused, ins_nsurv, ins_bcap, ins_bcap_all, et32, tbuf, row_cnt, row_tile, tile_done; DevArr<i64> ins_boff; DevArr<FTile> ftiles; DevArr<int8_t> tile_kind;
    // the bottom-array sum row (k_sum_signal): range, length, chunks, offsets per window; its samples sit behind the accumulators in raw, from run.sum_base
    DevArr<i64> sum_lo, sum_hi, sum_off, sum_chunk_off; DevArr<i32> sum_len, sum_nchunk;
    // full readout (k_row_empty): finished samples reserved per row slot for a row without a pulse, their offsets, the list of those rows
    DevArr<i32> fr_len, empty_rows; DevArr<i64> fr_off;
    // lone-hit rows (wfs_lone_hits, wfs_lone.h): a pass has buffers of its own for everything it writes -- counters, seed keys, rows,
    // intervals, finished samples, records -- so that the batch it follows, whose packers may still run, keeps every byte
    struct Lone {
        DevArr<WfsScal> scal; DevArr<u64> keys, keys2; RecOrder rec;
        DevArr<i64> win_l, win_r, row_of, itv_off, fin_off, itv_left, itv_right, rec_off, out_left, out_right, out_ixr;
        DevArr<i32> win_g, flag, cap, flen, itv_n, row_nrec, out_channel, out_nph, out_nnz;
        DevArr<int16_t> fin; DevArr<RowDesc> desc; DevArr<PackDesc> pdesc; DevBuf records_ab[1];      // (one record arena: a pass returns when its records exist)
        i64 n_rows = 0, n_records = 0;      // of the last pass
        bool noise_hits = false;            // wfs_set_lone_noise_hits: samples of the noise model that cross are seeds too
        DevBuf &records_buf() { return records_ab[0]; }
    } lone;
    // the overlay pass (wfs_overlay_records, wfs_overlay.h): buffers of its own for everything it writes, allocated by its first call
    struct Overlay {
        DevArr<OverlayScal> scal; DevArr<u32> src_a, src_b, val, val2, plen, plen2, oval, oval2, out;
        DevArr<u64> key, key2, pkey, pkey2, ekey, run_max, m_first, m_last, okey, okey2;
        DevArr<i32> base, flag, pulse_of, head, merged_of; DevArr<i64> m_nrec, rec_end;
        i64 n_records = 0;                  // of the last pass
    } overlay;

    // what is not a device buffer; the buffers, and the members that hold some, free themselves after this body
    ~wfs_handle()
    {
        clear_times(times);
        if (own_stream) hipStreamDestroy(stream);
        if (copy_stream) { hipStreamSynchronize(copy_stream); hipStreamDestroy(copy_stream); }
        for (hipEvent_t e : rec_copied) if (e) hipEventDestroy(e);
        if (pack_stream) { hipStreamSynchronize(pack_stream); hipStreamDestroy(pack_stream); }
        for (hipEvent_t e : pack_go) if (e) hipEventDestroy(e);
        for (hipEvent_t e : rec_ready) if (e) hipEventDestroy(e);
        if (h_scal) hipHostFree(h_scal);
    }
};

namespace {

#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    return h->fail(WFS_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } } while (0)

// Screening threshold of the afterpulse generator for one (element, channel, single / double PE parent): the uniform of the
// acceptance test is rU0 = 1 - u53(x, y) (afterpulse.py:196), accepted when rU0 / modifier [/ 2] <= prob.  With a = x >> 5 (the top
// 27 bits of u53) rU0 > 1 - (a + 1) 2^-27, so a < floor((1 - prob * modifier * k * (1 + 1e-9)) 2^27) - 2 cannot be accepted whatever
// the low bits and the two roundings of the divisions are.  Everything else is a candidate and gets the reference's comparison.
static u32 ap_threshold(double prob, double modifier, bool dpe)
{
    if (modifier == 0.0) return 134217728u;                        // rU0 / 0 = inf <= prob never holds (afterpulse.py:198): no photon is a candidate
    if (!(modifier > 0.0) || !(prob == prob)) return 0u;           // (negative / NaN: nothing screened, the exact comparison decides)
    const double pm = prob * modifier * (dpe ? 2.0 : 1.0) * (1.0 + 1e-9);
    if (!(pm < 1.0)) return 0u;
    const double a = std::floor((1.0 - pm) * 134217728.0) - 2.0;
    return a <= 0.0 ? 0u : (a >= 134217728.0 ? 134217728u : (u32)a);
}

// The host waits for packers that may still be running on the pack stream: readers of the records, setters of the tables the packers
// read, changes of mode.  Returns at once when none are pending.
int pack_wait(wfs_handle *h)
{
    if (!h->pack.must_wait()) return WFS_OK;
    HIPCHK(hipEventSynchronize(h->rec_ready[h->pack.arena]));
    h->pack.host_waited();
    return WFS_OK;
}
// The fence of a run: the main stream waits for the previous batch's packers.  Called in front of the first write of a run to a
// buffer they read (the tile buffers, else the accumulators); one stream wait per pending pack, none otherwise.
int pack_fence(wfs_handle *h)
{
    if (h->pack.take_fence()) HIPCHK(hipStreamWaitEvent(h->stream, h->rec_ready[h->pack.arena], 0));
    return WFS_OK;
}
// the buffers the packers read or write (the noise tables behind WfsDev apart: their setters wait on the host)
bool pack_uses(const wfs_handle *h, const DevBuf &b)
{
    for (const DevBuf *q : {&h->pack_desc.buf(), &h->row_desc.buf(), &h->rec_off.buf(), &h->itv_n.buf(), &h->itv_left.buf(), &h->itv_right.buf(), &h->rec.dest.buf(),
                            &h->tbuf.buf(), &h->raw.buf(), &h->fin.buf(), &h->records_ab[0], &h->records_ab[1]})
        if (q == &b) return true;
    return false;
}
template <class T> bool pack_uses(const wfs_handle *h, const DevArr<T> &a) { return pack_uses(h, a.buf()); }

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// Room for n in the buffer's own unit: elements of a DevArr<T>, bytes of a DevBuf (the record arenas, sort_tmp).
// (a grow frees the old block: one of a buffer that pending packers use waits for them on the host first)
template <class B> int ensure(wfs_handle *h, B &b, size_t n)
{
    if (b.grows(n) && h->pack.must_wait() && pack_uses(h, b)) TRY(pack_wait(h));
    if (int e = b.ensure(n)) return h->fail(WFS_E_HIP, std::string("hipMalloc: ") + hipGetErrorString((hipError_t)e));
    return WFS_OK;
}

// The buffers of a run that full readout multiplies -- every row slot of every window has a row: interval slots, the wider accumulators,
// finished samples, records.  One that cannot be had ends the run in WFS_E_NOMEM with a message that names the mode.
template <class B> int ensure_rows(wfs_handle *h, B &b, size_t n, const char *what)
{
    const int rc = ensure(h, b, n);
    if (rc == WFS_OK || !h->dev.full_readout) return rc;
    return h->fail(WFS_E_NOMEM, std::string("full readout: no device memory for ") + what + " (" + h->err + "): every row slot of every window has a row, load fewer windows per batch");
}

// Copies between typed pointers are sized by the element: the bytes of n elements.  The two sides name one type, or two integer types
// of one size and signedness (the ABI's int64_t is long, i64 is long long).
template <class D, class S> constexpr size_t copy_bytes(size_t n)
{
    static_assert(std::is_same<D, S>::value || (std::is_integral<D>::value && std::is_integral<S>::value && sizeof(D) == sizeof(S) && std::is_signed<D>::value == std::is_signed<S>::value),
                  "source and destination of a copy hold the same elements");
    return n * sizeof(S);
}
// n elements on the handle's stream; n elements of device memory to the host, a blocking copy
template <class D, class S> int copy_async(wfs_handle *h, D *dst, const S *src, size_t n, hipMemcpyKind kind) { HIPCHK(hipMemcpyAsync(dst, src, copy_bytes<D, S>(n), kind, h->stream)); return WFS_OK; }
template <class D, class S> int copy_out(wfs_handle *h, D *dst, const S *src, size_t n) { HIPCHK(hipMemcpy(dst, src, copy_bytes<D, S>(n), hipMemcpyDeviceToHost)); return WFS_OK; }

template <class T, class S> int upload(wfs_handle *h, DevArr<T> &a, const S *src, size_t count)
{
    TRY(ensure(h, a, count));
    return count ? copy_async(h, a.p(), src, count, hipMemcpyHostToDevice) : WFS_OK;
}

// n elements of a device array on the host, a blocking copy.  A HIP error is recorded on the handle (fail) and thrown: the firewall of
// the C ABI (wfs_caught) hands its code back like the return of a HIPCHK.
struct WfsHipError { int code; };
template <class T> std::vector<T> download(wfs_handle *h, const DevArr<T> &a, size_t n)
{
    std::vector<T> v(n);
    if (n) if (int rc = copy_out(h, v.data(), a.p(), n)) throw WfsHipError{rc};
    return v;
}

// The listed tiles in work-list order with their sample windows, and the offsets of their currents (the total behind the last): what a
// run with DBG_CURRENTS uploads as cur_off and what wfs_copy_pulses hands out.
struct ListedTiles { std::vector<i32> tile; std::vector<TileWindow> win; std::vector<i64> off; };
ListedTiles listed_tiles(wfs_handle *h)
{
    const WfsDev &d = h->dev;
    ListedTiles r;
    r.tile = download(h, h->active_tiles, (size_t)h->run.n_active_tiles);
    const std::vector<i32> tmn = download(h, h->tile_tmin, (size_t)h->batch.n_tiles), tmx = download(h, h->tile_tmax, (size_t)h->batch.n_tiles);
    const std::vector<i64> t0 = download(h, h->set_t0, (size_t)h->batch.n_sets);
    r.win.resize(r.tile.size()); r.off.assign(r.tile.size() + 1, 0);
    for (size_t k = 0; k < r.tile.size(); k++) {
        const i32 tile = r.tile[k];
        r.win[k] = tile_window(d, t0[tile / d.n_tpc], tmn[tile], tmx[tile]);
        r.off[k + 1] = r.off[k] + r.win[k].L;
    }
    return r;
}
// full readout: the rows without a pulse of the last run (behind the resident rows of the row list) and their finished samples (behind
// s_fin).  They live in the scalar block alone: k_row_len and the scan of fr_len write them before the geometry's read-back, nothing
// clears them before the next run or load does, and a run with the switch off leaves both 0
i64 n_empty_rows(const wfs_handle *h) { return h->h_scal->n_empty_rows; }
i64 s_empty(const wfs_handle *h) { return h->h_scal->n_empty_samples; }
// The rows with data in row-list order: slot, first and last pulse sample (absolute) of each, and the offsets of their debug copies
// (the total behind the last): row_dbg_off of a run with DBG_CURRENTS and data_off of wfs_copy_rows.
struct ListedRows { std::vector<RowSlot> slot; std::vector<i64> lo, hi, off; };
ListedRows listed_rows(wfs_handle *h)
{
    const WfsDev &d = h->dev;
    const size_t CG = (size_t)h->batch.n_clusters + 1;
    const std::vector<i32> ar = download(h, h->active_rows, (size_t)(h->run.n_active_rows - n_empty_rows(h)));      // (full readout: the rows with pulses)
    const std::vector<i64> lo = download(h, h->row_lo, CG * d.n_tpc), hi = download(h, h->row_hi, CG * d.n_tpc);
    std::vector<i64> slo, shi;
    if (d.sum_channel >= 0) { slo = download(h, h->sum_lo, CG); shi = download(h, h->sum_hi, CG); }
    ListedRows r;
    r.slot.resize(ar.size()); r.lo.resize(ar.size()); r.hi.resize(ar.size()); r.off.assign(ar.size() + 1, 0);
    for (size_t k = 0; k < ar.size(); k++) {
        const RowSlot s = r.slot[k] = row_slot(d, ar[k]);
        r.lo[k] = s.sum ? slo[s.g] : lo[s.g * d.n_tpc + s.acc_ch]; r.hi[k] = s.sum ? shi[s.g] : hi[s.g * d.n_tpc + s.acc_ch];
        r.off[k + 1] = r.off[k] + row_span(r.lo[k], r.hi[k], d.tw).len;
    }
    return r;
}
// n, mean + origin, min, max, sigma of n values with sum s1 and sum of squares s2 about `origin`; NaN for all but n when there are none
void stat5(double *o, double n, double s1, double s2, double origin, i64 lo, i64 hi)
{
    const double mean = n > 0 ? s1 / n : 0, var = n > 0 ? s2 / n - mean * mean : 0;
    o[0] = n; o[1] = n > 0 ? origin + mean : NAN;
    o[2] = n > 0 ? (double)lo : NAN; o[3] = n > 0 ? (double)hi : NAN;
    o[4] = n > 0 ? sqrt(var > 0 ? var : 0) : NAN;
}

// Brackets one kernel launch, or several under one name: HIP events when profiling is on; with wfs_set_debug bit 3 what was launched is
// checked on the spot (hipGetLastError + a stream synchronisation), so that a failed launch or a faulting kernel is reported under its
// own name instead of ~25 launches later at the end of wfs_run.  timed = false: the check alone, no entry in wfs_kernel_times; no name: neither.
struct Timer {
    wfs_handle *h; bool on; const char *name;
    Timer(wfs_handle *h_, const char *name_, bool timed = true) : h(h_), on(timed && name_ && h_->profiling != 0), name(name_)
    {
        if (!on) return;
        KernelTime kt; kt.name = name;
        hipEventCreate(&kt.a); hipEventCreate(&kt.b);
        hipEventRecord(kt.a, h->stream);
        h->times.push_back(kt);
    }
    ~Timer()
    {
        if (on) hipEventRecord(h->times.back().b, h->stream);
        if (name && (h->debug_bits & DBG_CHECK_LAUNCHES)) {
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess && h->launch_err.empty()) { try { h->launch_err = std::string(name) + ": " + hipGetErrorString(e); } catch (...) {} }
        }
    }
};
#define CHECK_LAUNCHES() do { if (!h->launch_err.empty()) { const std::string m_ = h->launch_err; h->launch_err.clear(); return h->fail(WFS_E_HIP, m_); } } while (0)

// grid size for n items; never 0 (a launch with an empty grid is an error, every kernel bounds-checks its index)
inline unsigned nblocks(i64 n, int tpb) { return n > 0 ? (unsigned)((n + tpb - 1) / tpb) : 1u; }

// The shape of a launch.  The recurring ones have names: a thread, a wave or a workgroup per item.
struct Shape {
    dim3 grid, block; size_t lds = 0;
    bool elsewhere = false; hipStream_t other = nullptr;      // on(): not the handle's stream
    Shape(dim3 grid_, dim3 block_, size_t lds_ = 0) : grid(grid_), block(block_), lds(lds_) {}
    Shape on(hipStream_t s) const { Shape r = *this; r.elsewhere = true; r.other = s; return r; }
};
inline Shape per_thread(i64 n, int tpb = 256) { return Shape(dim3(nblocks(n, tpb)), dim3((unsigned)tpb)); }
inline Shape per_wave(i64 n, size_t lds = 0) { return Shape(dim3(nblocks(n, 4)), dim3(256), lds); }                  // four waves of 64 to a workgroup
inline Shape per_group(i64 n, int tpb = 256, size_t lds = 0) { return Shape(dim3((unsigned)n), dim3((unsigned)tpb), lds); }      // (the callers have n > 0)

// The one way a kernel is launched: under a Timer of its own name, on the handle's stream unless the shape names another (the packers;
// their entry is recorded on the main stream all the same).  A null kernel -- a family member picked with an index outside its axis --
// is refused and nothing is launched.
template <class... P, class... A> int launch_as(wfs_handle *h, bool timed, Kernel<void (*)(P...)> k, const Shape &s, A &&...args)
{
    if (!k.fn) return h->fail(WFS_E_STATE, std::string("internal: kernel family ") + k.name + " has no such member");
    Timer t(h, k.name, timed);
    hipLaunchKernelGGL(k.fn, s.grid, s.block, s.lds, s.elsewhere ? s.other : h->stream, std::forward<A>(args)...);
    return WFS_OK;
}
template <class K, class... A> int launch(wfs_handle *h, K k, const Shape &s, A &&...args) { return launch_as(h, true, k, s, std::forward<A>(args)...); }
// Not timed: no entry in wfs_kernel_times, the check of bit 3 under the kernel's own name all the same.  For the launches inside a Timer
// scope that brackets several under one name, and for those outside the profiled step.
template <class K, class... A> int launch_untimed(wfs_handle *h, K k, const Shape &s, A &&...args) { return launch_as(h, false, k, s, std::forward<A>(args)...); }
// a kernel that is no template, under its own name
#define PLAIN(k) kernel(&k, #k)

// ---- The kernel families of this file: every template kernel's instantiations, each axis with what picks it at run time.
// fma: every pulse kernel exists in two forms, FMA = true (wfs_config.fma, one rounding per template * gain term) and FMA = false (numpy's
//      two roundings, currents bit-exact with the reference); cfg.fma picks one at launch time.
// ap:  batch.ap_sets -- PMT afterpulses are on and the batch has sets that take them (run_generation's ap_on).
// ext: batch.ins_models -- some instruction carries a delay model of its own (wfs_set_delay_models).
// nk:  noise_kind_of(dev) when the configuration enables noise, else NOISE_NONE (RowsRun::noise_kind).  The row kernels take the kind as
//      a template parameter (no branch between their loads): NoiseKind of wfs_noise.h, 0 none, 1 int16 table, 2 float table, 3 the
//      noise model, 4 the noise model with a colour, 5 the same with slow levels.
// dk:  dev.dk_thr -- PMT dark counts are set (wfs_set_dark_counts); with the feature off the row kernels are the kernels they were.
// The cap is the LDS_CAP_ constant of wfs_layout.h, checked there against the largest total of the kernel's layout; wfs_create raises
// the limit of every member that has one.
constexpr int LDS_CAP_GRANT = -1;       // k_s2_bright: what the device grants one workgroup, worked out by wfs_create
const auto K_S2_TILE = family<2, 2>("k_s2_tile", LDS_CAP_TILE, [](auto ap, auto fma) { return &k_s2_tile<ap() != 0, fma() != 0>; });
const auto K_S2_TILE_GEN = family<2>("k_s2_tile_gen", 0, [](auto ap) { return &k_s2_tile_gen<ap() != 0>; });
const auto K_S2_BRIGHT = family<2, 2>("k_s2_bright", LDS_CAP_GRANT, [](auto ap, auto fma) { return &k_s2_bright<ap() != 0, fma() != 0>; });
const auto K_PHOTON_FILL = family<2, 2>("k_photon_fill", LDS_CAP_FILL, [](auto ap, auto ext) { return &k_photon_fill<ap() != 0, ext() != 0>; });
// k_pulse: wide -- 256 threads, not 128: the `small` rule of run_pulses (tiles of few samples); res -- the `resident` rule there
// (the templates of the tile's dt sit in LDS)
const auto K_PULSE = family<2, 2, 2>("k_pulse_dense", LDS_CAP_PULSE, [](auto wide, auto res, auto fma) { return &k_pulse<wide() ? 256 : 128, res() != 0, fma() != 0>; });
const auto K_PULSE_GENERIC = family<2>("k_pulse_generic", LDS_CAP_GENERIC, [](auto fma) { return &k_pulse_generic<256, fma() != 0>; });
const auto K_PULSE_SPARSE = family<2>("k_pulse_sparse", LDS_CAP_SPARSE, [](auto fma) { return &k_pulse_sparse<SPARSE_TPB, fma() != 0>; });
const auto K_PULSE_TINY = family<2>("k_pulse_tiny", 0, [](auto fma) { return &k_pulse_tiny<fma() != 0>; });
const auto K_PULSE_WAVE = family<2>("k_pulse_wave", 0, [](auto fma) { return &k_pulse_wave<fma() != 0>; });
// k_row_pulse: seg -- the long rows of a run, which take several segments of res_max_len samples (run_rows' second part); they alone
// ask for more LDS than the default limit
const auto K_ROW_PULSE = family<NOISE_KINDS, 2, 2, 2>("k_row_pulse", [](int, int, int seg, int) { return seg ? LDS_CAP_ROW : 0; },
                                                      [](auto nk, auto fma, auto seg, auto dk) { return &k_row_pulse<nk(), fma() != 0, seg() != 0, dk() != 0>; });
const auto K_ROW_EMPTY = family<NOISE_KINDS, 2>("k_row_empty", 0, [](auto nk, auto dk) { return &k_row_empty<nk(), dk() != 0>; });
const auto K_ZLE = family<NOISE_KINDS, 2>("k_zle", 0, [](auto nk, auto dk) { return &k_zle<nk(), dk() != 0>; });
const auto K_PACK = family<NOISE_KINDS, 2>("k_pack", 0, [](auto nk, auto dk) { return &k_pack<nk(), dk() != 0>; });
// place: the second of the two passes (count, then place) of the afterpulse segments and of the optical load
const auto K_AP_SEG = family<2>("k_ap_seg", 0, [](auto place) { return &k_ap_seg<place() != 0>; });
const auto K_OPTICAL_BUCKET = family<2>("k_optical_bucket", 0, [](auto place) { return &k_optical_bucket<place() != 0>; });
// slow: noise_kind_of(dev) == NOISE_SLOW, the probe of a colour with slow levels
const auto K_NOISE_COLOUR_SAMPLES = family<2>("k_noise_colour_samples", 0, [](auto slow) { return &k_noise_colour_samples<slow() != 0>; });
// (no template, but a cap)
const auto K_TILE_ORDER_BIG = family<1>("k_tile_order_big", LDS_CAP_ORDER, [](auto) { return &k_tile_order_big; });

// The fills of one stage, collected and written by one dispatch of k_fill_group instead of one runtime fill or fill kernel each.
// A stage adds its segments where it used to fill them and calls flush() before it launches the first kernel that reads or writes
// one of them; nothing else is launched in between, so only fills change places with fills.  One Timer entry per dispatch, named
// for the stage.  A segment above FILL_RUNTIME_BYTES stays with the runtime's fill: its time is bandwidth, not dispatch, and the
// group's grid is sized for the small segments beside it (the accumulators of a mixed batch are 10.9 GB).
struct FillGroup {
    static constexpr size_t FILL_RUNTIME_BYTES = (size_t)64 << 20;
    wfs_handle *h; const char *name; FillSegs a{}; int n = 0; size_t longest = 0;
    FillGroup(wfs_handle *h_, const char *name_) : h(h_), name(name_), n_fail0(h_->n_fail) {}
    // a group may die with segments only on an error return (HIPCHK / TRY between add and flush); anywhere else a flush() is missing
    ~FillGroup() { if (n > 0 && h->n_fail == n_fail0) fprintf(stderr, "wfsim_amd: internal error: fill group %s dropped %d fills\n", name, n); }
    int n_fail0 = 0;
    int add(void *p, size_t bytes, u32 p0, u32 p1, u32 p2, u32 p3)
    {
        if (bytes == 0) return WFS_OK;
        if (bytes > FILL_RUNTIME_BYTES && p0 == p1 && p0 == p2 && p0 == p3 && (bytes & 3) == 0) { HIPCHK(hipMemsetD32Async((hipDeviceptr_t)p, (int)p0, bytes / 4, h->stream)); return WFS_OK; }
        if (n == FILL_GROUP_MAX) TRY(flush());
        a.s[n].p = (unsigned char *)p; a.s[n].bytes = bytes; a.s[n].pat[0] = p0; a.s[n].pat[1] = p1; a.s[n].pat[2] = p2; a.s[n].pat[3] = p3;
        n++; longest = std::max(longest, bytes);
        return WFS_OK;
    }
    // count elements from p on (p may point into an array: tile_count + TP): every byte 0 or 0xff, or the value v
    template <class T> int zero(T *p, i64 count) { return add(p, (size_t)count * sizeof(T), 0, 0, 0, 0); }
    template <class T> int ones(T *p, i64 count) { return add(p, (size_t)count * sizeof(T), ~0u, ~0u, ~0u, ~0u); }
    int fill(i32 *p, i64 count, i32 v) { return add(p, (size_t)count * sizeof(i32), (u32)v, (u32)v, (u32)v, (u32)v); }
    int fill(i64 *p, i64 count, i64 v) { return pairs(p, count, v, v); }
    // count i64 that alternate between even and odd
    int pairs(i64 *p, i64 count, i64 even, i64 odd) { return add(p, (size_t)count * sizeof(i64), (u32)(u64)even, (u32)((u64)even >> 32), (u32)(u64)odd, (u32)((u64)odd >> 32)); }
    int flush()
    {
        if (n == 0) return WFS_OK;
        // 64 bytes per thread of the longest segment, at most 1024 workgroups per segment (the rest is the grid stride)
        const unsigned gx = (unsigned)std::min<size_t>((longest + 256 * 64 - 1) / (256 * 64), 1024);
        TRY(launch(h, kernel(&k_fill_group, name), Shape(dim3(gx, (unsigned)n), dim3(256)), a));
        n = 0; longest = 0;
        return WFS_OK;
    }
};

// exclusive scan i32[n] -> i64[n+1] into a caller-provided range, every output shifted by offset; total as for scan
// (block: the scalar block that takes the total -- the run's, or the one a pass of wfs_lone_hits counts in)
int scan_into(wfs_handle *h, const i32 *in, i64 n, i64 *outp, i64 WfsScal::*total_member, i64 offset, WfsScal *block = nullptr)
{
    i64 nb = (n + SCAN_TILE - 1) / SCAN_TILE; if (nb < 1) nb = 1;
    TRY(ensure(h, h->scan_tmp, (size_t)nb));
    i64 *total = &((block ? block : h->scal.p())->*total_member);       // (a device address: computed, never dereferenced here)
    if (n == 0) { h->zero64 = offset; TRY(copy_async(h, outp, &h->zero64, 1, hipMemcpyHostToDevice)); HIPCHK(hipMemsetAsync(total, 0, sizeof *total, h->stream)); return WFS_OK; }
    TRY(launch(h, PLAIN(k_scan_reduce), per_group(nb, SCAN_TPB), in, n, h->scan_tmp.p()));
    TRY(launch(h, PLAIN(k_scan_spine), Shape(dim3(1), dim3(1024)), h->scan_tmp.p(), nb, total));
    TRY(launch(h, PLAIN(k_scan_down), per_group(nb, SCAN_TPB), in, n, h->scan_tmp.p(), outp, offset));
    return WFS_OK;
}

// exclusive scan i32[n] -> i64[n+1]; total written to the member `total` of the device scalar block
int scan(wfs_handle *h, const i32 *in, i64 n, DevArr<i64> &out, i64 WfsScal::*total_member, WfsScal *block = nullptr)
{
    TRY(ensure(h, out, (size_t)(n + 1)));
    return scan_into(h, in, n, out.p(), total_member, 0, block);
}

// The one way rocPRIM is called.  Its device functions take a scratch block and its size and, given a null block, only say how much
// they need: call(tmp, bytes) is made once for the size and, with sort_tmp grown to it, once for the work (under a Timer where timed_as
// names one).  One block serves every user: all are enqueued on the handle's stream, and a grow frees through hipFree, which waits.
template <class Call> int two_step(wfs_handle *h, const char *what, Call call, const char *timed_as = nullptr)
{
    size_t bytes = 0; hipError_t e = call(nullptr, bytes);
    if (e == hipSuccess) TRY(ensure(h, h->sort_tmp, bytes));
    if (e == hipSuccess) { Timer t(h, timed_as); e = call(h->sort_tmp.p, bytes); }
    return e == hipSuccess ? WFS_OK : h->fail(WFS_E_HIP, std::string("rocPRIM, ") + what + ": " + hipGetErrorString(e));
}
// the two operations with several users: n (key, value) pairs sorted by the key bits below end_bit; an inclusive scan of n elements
template <class K, class V> int sort_pairs(wfs_handle *h, const char *what, K *k_in, K *k_out, V *v_in, V *v_out, i64 n, unsigned end_bit, const char *timed_as = nullptr)
{ return two_step(h, what, [&](void *tmp, size_t &bytes) { return rocprim::radix_sort_pairs(tmp, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0u, end_bit, h->stream); }, timed_as); }
template <class T, class Op> int scan_inclusive(wfs_handle *h, const char *what, const T *in, T *out, i64 n, Op op)
{ return two_step(h, what, [&](void *tmp, size_t &bytes) { return rocprim::inclusive_scan(tmp, bytes, in, out, (size_t)n, op, h->stream); }); }
template <class... A> int ensure_each(wfs_handle *h, size_t n, A &...arrays) { int rc = WFS_OK; ((rc = rc ? rc : ensure(h, arrays, n)), ...); return rc; }      // room for n elements in each array

// The records of a row list into (time, channel) order as strax.sort_by_time leaves them: a key per record (k_rec_keys), one radix sort
// over the key bits in use, the sorted slot of every record (k_invert_perm), which the packers write to.  za describes the n_rows rows and
// takes keys, values and slots; key_origin, key_end: of the rows' counter block.  too_many: the caller's words for more records than
// the sort counts; timed_as: the sort's entry in wfs_kernel_times, if any.
int order_records(wfs_handle *h, RecOrder &o, ZleArgs &za, i64 n_rows, i64 n_rec, i64 key_origin, i64 key_end, const char *too_many, const char *timed_as = nullptr)
{
    if (n_rec > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, too_many);
    TRY(ensure_each(h, (size_t)n_rec, o.key, o.key2, o.val, o.val2, o.dest));
    za.rec_key = o.key.p(); za.rec_val = o.val.p();
    TRY(launch(h, PLAIN(k_rec_keys), per_wave(n_rows), h->dev, za));
    TRY(sort_pairs(h, "record sort", o.key.p(), o.key2.p(), o.val.p(), o.val2.p(), n_rec, rec_key_end_bit((u64)std::max<i64>(key_end - key_origin, 1)), timed_as));
    TRY(launch(h, PLAIN(k_invert_perm), per_thread(n_rec), o.val2.p(), o.dest.p(), n_rec));
    za.rec_dest = o.dest.p(); return WFS_OK;
}
// The packers of rows that exist as finished samples, on the stream `on`: k_pack_desc over the n_rows rows of za, k_pack_res over the
// n_fin of them from row first_fin on, whose samples lie in fin.
int pack_finished_rows(wfs_handle *h, const ZleArgs &za, i64 n_rows, const int16_t *fin, i64 first_fin, i64 n_fin, hipStream_t on)
{
    TRY(launch(h, PLAIN(k_pack_desc), per_thread(n_rows).on(on), za));
    if (n_fin == 0) return WFS_OK;
    PackResArgs pr{za.pdesc + first_fin, fin, za.itv_left, za.itv_right, za.records, za.rec_dest, za.rec_capacity, n_fin, za.spr, (i32)h->dev.dt};
    return launch(h, PLAIN(k_pack_res), per_wave(n_fin).on(on), pr);
}
// A pass's counter block on the host as of this point of the stream, and the host waits; the same for the last element of an inclusive
// scan, its total, alone or beside the block under the one wait.  pass_done: the end of a pass, a failed launch is reported.
template <class D, class S> int read_block(wfs_handle *h, D &host, const S *dev) { TRY(copy_async(h, &host, dev, 1, hipMemcpyDeviceToHost)); HIPCHK(hipStreamSynchronize(h->stream)); return WFS_OK; }
template <class D, class S, class T> int read_block(wfs_handle *h, D &host, const S *dev, T &total, const T *last) { TRY(copy_async(h, &host, dev, 1, hipMemcpyDeviceToHost)); return read_block(h, total, last); }
int pass_done(wfs_handle *h) { HIPCHK(hipStreamSynchronize(h->stream)); HIPCHK(hipGetLastError()); CHECK_LAUNCHES(); return WFS_OK; }

// A step boundary: on return *h->h_scal is the device scalar block as of this point of the stream.  By default k_publish writes
// it into the mapped host copy and the host spins on the sequence word (no copy command, no wake-up through the runtime's signal);
// a stream given by wfs_set_stream, the launch-checking debug mode, WFS_HOST_SYNC=copy and a handle without mapped memory copy and
// synchronise.  So does a boundary whose stream ran dry without the word arriving (the launch of k_publish failed).
int read_scal(wfs_handle *h)
{
    bool published = false;
    if (h->publish && h->own_stream && !(h->debug_bits & DBG_CHECK_LAUNCHES)) {
        const u64 seq = ++h->seq;
        // (the profiled step counts the boundaries that publish: one "k_publish" entry each, none for one that copies)
        TRY(launch(h, PLAIN(k_publish), Shape(dim3(1), dim3(64)), h->scal.p(), h->d_hscal, h->d_hseq, seq));
        hipError_t qe = hipSuccess;
        const WfsWait w = wfs_wait_seq(h->h_seq, seq, [&]() {
            qe = hipStreamQuery(h->stream);
            return qe == hipSuccess ? WFS_QUERY_DONE : (qe == hipErrorNotReady ? WFS_QUERY_NOT_READY : WFS_QUERY_ERROR);
        });
        if (w == WFS_WAIT_ERROR) return h->fail(WFS_E_HIP, std::string("hipStreamQuery(h->stream): ") + hipGetErrorString(qe));
        published = w == WFS_WAIT_OK;
    }
    if (!published) {
        TRY(copy_async(h, h->h_scal, h->scal.p(), 1, hipMemcpyDeviceToHost));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (!h->launch_err.empty()) { const std::string m = h->launch_err; h->launch_err.clear(); return h->fail(WFS_E_HIP, m); }     // (wfs_set_debug bit 3)
    return WFS_OK;
}

// The kind of noise (the nk axis of the row kernels' families) that the device view holds, whether or not the configuration enables noise (wfs_run asks d.enable_noise first):
static NoiseKind noise_kind_of(const WfsDev &d)
{
    if (d.nm_cells) return d.ns_shift ? NOISE_SLOW : (d.nc_taps ? NOISE_COLOUR : NOISE_MODEL);
    return d.noise_f ? NOISE_TABLE_F64 : (d.noise ? NOISE_TABLE_I16 : NOISE_NONE);
}

// What the probe entry points of the noise model share once they know their stream: the checks of (t0, n, out), a scratch buffer of n
// elements, the launch into it (probe(T *device_buffer), which hands back launch's code) and the copy back.  fn: the entry point, for the messages.
template <class T, class Probe> int noise_probe(wfs_handle *h, const char *fn, int64_t t0, int64_t n, T *out, Probe &&probe)
{
    if (n < 0 || n > ((i64)1 << 30) || (n > 0 && !out)) return h->fail(WFS_E_INVALID, std::string(fn) + ": n outside 0 .. 2^30 or null buffer");
    if (t0 > I64_MAX - n) return h->fail(WFS_E_INVALID, std::string(fn) + ": t0 + n overflows");
    if (n == 0) return WFS_OK;
    HIPCHK(hipSetDevice(h->device));
    DevArr<T> buf;
    TRY(ensure(h, buf, (size_t)n));
    TRY(probe(buf.p()));
    HIPCHK(hipGetLastError());
    TRY(copy_async(h, out, buf.p(), (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(h->stream));
    CHECK_LAUNCHES();
    return WFS_OK;
}

// a code that kernels raised in the device scalar block (WfsDevError) -> error code and message of the C ABI
int device_error(wfs_handle *h, i64 code)
{
    switch (code) {
    case WFS_DEV_WINDOW: return h->fail(WFS_E_CAPACITY, "Pulse cache too long (digitise window of 10^6 samples or more, rawdata.py:219)");
    case WFS_DEV_TIME_RANGE: return h->fail(WFS_E_CAPACITY, "photon time further than 2^31 ns from its instruction");
    case WFS_DEV_TILE_BUFFER: return h->fail(WFS_E_STATE, "internal: a tile of k_s2_tile did not fit its sample buffer");
    case WFS_DEV_OPT_CHANNEL: return h->fail(WFS_E_INVALID, "photon channel out of range");
    case WFS_DEV_OPT_TIME: return h->fail(WFS_E_CAPACITY, "photon time beyond 2^31 ns");
    default: return WFS_OK;
    }
}

// cum[i] = P(trunc(Y) <= vmin + i) for Y ~ N(mu, sigma) (trunc = C cast, toward zero)
static void normal_trunc_table(double mu, double sigma, std::vector<double> &cum, int &vmin)
{
    cum.clear();
    if (!(sigma > 0)) { vmin = (int)mu; cum.push_back(1.0); return; }
    const int lo = (int)floor(mu - 8.5 * sigma) - 1, hi = (int)ceil(mu + 8.5 * sigma) + 1;
    vmin = lo;
    for (int k = lo; k <= hi; k++) {
        const double x = ((k >= 0 ? k + 1 : k) - mu) / sigma;
        cum.push_back(0.5 * erfc(-x / 1.4142135623730951));
    }
    cum.back() = 1.0;
}

// Walker alias table of a discrete distribution given by its cumulative probabilities (Vose's construction, sequential and
// in a fixed order so that the CPU oracle -- which builds its own -- arrives at the same cells): K = 2^k >= max(n, 2) cells,
// q[i] = p[i] * K; "small" (q < 1) and "large" cells on two stacks filled in ascending index order; pop a small s, pair it
// with the large l on top: cell s = {thr = floor(q[s] * 2^32), alias = l}, q[l] = (q[l] + q[s]) - 1, l moves to the small
// stack when it drops below 1; what is left over keeps its own outcome.  Sampling: wfs_device.h alias_sample.
// (Cell: uint2, or the NoiseCell of wfs_noise.h, which has the same two words)
template <class Cell> static void build_alias(const std::vector<double> &cum, std::vector<Cell> &cell, int &shift)
{
    const size_t n = cum.size();
    size_t K = 2; int lg = 1;
    while (K < n) { K <<= 1; lg++; }
    shift = 32 - lg;
    std::vector<double> q(K, 0.0);
    for (size_t i = 0; i < n; i++) q[i] = (cum[i] - (i ? cum[i - 1] : 0.0)) * (double)K;
    std::vector<u32> small, large; small.reserve(K); large.reserve(K);
    for (size_t i = 0; i < K; i++) (q[i] < 1.0 ? small : large).push_back((u32)i);
    cell.assign(K, Cell{0xffffffffu, 0u});
    for (size_t i = 0; i < K; i++) cell[i].y = (u32)i;                       // default: own outcome with certainty
    while (!small.empty() && !large.empty()) {
        const u32 sidx = small.back(); small.pop_back();
        const u32 l = large.back();
        const double t = q[sidx] * 4294967296.0;
        cell[sidx].x = t >= 4294967295.0 ? 0xffffffffu : (u32)t; cell[sidx].y = l;
        q[l] = (q[l] + q[sidx]) - 1.0;
        if (q[l] < 1.0) { large.pop_back(); small.push_back(l); }
    }
}

static int upload_disc(wfs_handle *h, DevArr<uint2> &buf, const std::vector<double> &cum, int vmin, AliasTab &out)
{
    if (cum.size() > 65000) return h->fail(WFS_E_CAPACITY, "delay table too long (time constant above ~1.5 us)");
    std::vector<uint2> cell; int shift = 31;
    build_alias(cum, cell, shift);
    TRY(upload(h, buf, cell.data(), cell.size()));
    HIPCHK(hipStreamSynchronize(h->stream));
    out.cell = buf.p(); out.vmin = vmin; out.shift = shift;
    return WFS_OK;
}

// ---- delay of a photon = sum of independent, separately truncated terms: sampled from ONE uniform through
// the convolution of the terms' probability mass functions (same distribution as adding separately drawn terms)

static Pmf pmf_from_cum(const std::vector<double> &cum, long vmin)
{
    Pmf r; r.vmin = vmin; r.p.resize(cum.size());
    for (size_t i = 0; i < cum.size(); i++) r.p[i] = cum[i] - (i ? cum[i - 1] : 0.0);
    return r;
}
static Pmf pmf_normal(double mu, double sigma) { std::vector<double> cum; int vmin; normal_trunc_table(mu, sigma, cum, vmin); return pmf_from_cum(cum, vmin); }
// trunc(Exp * tau) (s1.py:193, pulse.py:341): P(X <= k) = 1 - exp(-(k + 1) / tau)
static Pmf pmf_exp(double tau)
{
    std::vector<double> cum;
    if (!(tau > 0)) cum.push_back(1.0);
    else for (long k = 0; k < 60000; k++) { const double v = -expm1(-(double)(k + 1) / tau); cum.push_back(v); if (v >= 1.0) break; }
    cum.back() = 1.0;
    return pmf_from_cum(cum, 0);
}
// trunc(np.interp(u, x, t)) (s2.py:338): P(L <= y) is the inverse of the increasing piecewise linear map u -> L
static Pmf pmf_luminescence(const std::vector<double> &x, const std::vector<double> &t)
{
    const int n = (int)x.size();
    if (n < 2) { Pmf r; r.p = {1.0}; return r; }
    auto cdf = [&](double y) {
        if (y < t[0]) return 0.0;
        if (y >= t[n - 1]) return 1.0;
        int lo = 0, hi = n - 1;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (t[mid] <= y) lo = mid; else hi = mid; }
        return x[lo] + (y - t[lo]) / (t[lo + 1] - t[lo]) * (x[lo + 1] - x[lo]);
    };
    const long lo = (long)floor(t[0]) - 1, hi = (long)ceil(t[n - 1]) + 1;
    std::vector<double> cum;
    for (long k = lo; k <= hi; k++) cum.push_back(cdf((double)(k >= 0 ? k + 1 : k)));      // the cast truncates toward zero
    cum.back() = 1.0;
    return pmf_from_cum(cum, lo);
}
static Pmf pmf_mix(const Pmf &a, double wa, const Pmf &b, double wb)
{
    Pmf r; r.vmin = std::min(a.vmin, b.vmin);
    const long hi = std::max(a.vmin + (long)a.p.size(), b.vmin + (long)b.p.size());
    r.p.assign((size_t)(hi - r.vmin), 0.0);
    for (size_t i = 0; i < a.p.size(); i++) r.p[(size_t)(a.vmin - r.vmin) + i] += wa * a.p[i];
    for (size_t i = 0; i < b.p.size(); i++) r.p[(size_t)(b.vmin - r.vmin) + i] += wb * b.p[i];
    return r;
}
static Pmf pmf_conv(const Pmf &a, const Pmf &b)
{
    Pmf r; r.vmin = a.vmin + b.vmin; r.p.assign(a.p.size() + b.p.size() - 1, 0.0);
    for (size_t i = 0; i < a.p.size(); i++) { const double ai = a.p[i]; if (ai == 0.0) continue; for (size_t j = 0; j < b.p.size(); j++) r.p[i + j] += ai * b.p[j]; }
    return r;
}
// cumulative table of a pmf: leading zeros dropped, cut where the running sum reaches 1 (the oracle does the same)
static void cum_of_pmf(const Pmf &a, std::vector<double> &cum, long &vmin)
{
    size_t first = 0; while (first + 1 < a.p.size() && a.p[first] == 0.0) first++;
    cum.clear(); double acc = 0;
    for (size_t i = first; i < a.p.size(); i++) { acc += a.p[i]; cum.push_back(acc); if (acc >= 1.0) break; }
    while (cum.size() > 1 && cum[cum.size() - 2] >= 1.0) cum.pop_back();
    cum.back() = 1.0;
    vmin = a.vmin + (long)first;
}
static int upload_pmf(wfs_handle *h, int slot, const Pmf &a, AliasTab &out)
{
    std::vector<double> cum; long vmin;
    cum_of_pmf(a, cum, vmin);
    return upload_disc(h, h->tt_alias[slot], cum, (int)vmin, out);
}

// tab_tts: transit time alone (photons that arrive with their times: RawDataOptical); tab_s1 / tab_s2: every delay term of
// an S1 / S2 photon relative to its emitter (s1.py:193-194, s2.py:338 + pulse.py:339-341 + s2.py:550, pulse.py:54-56)
int build_time_tables(wfs_handle *h)
{
    const wfs_config &c = h->cfg; WfsDev &d = h->dev;
    const Pmf tts = pmf_normal(c.tts_mean, c.tts_sigma);
    TRY(upload_pmf(h, 0, tts, d.tab_tts));
    Pmf s1; s1.p = {1.0};
    if (c.s1_simple) { s1 = pmf_exp(c.s1_decay_time); if (c.s1_decay_spread != 0.0) s1 = pmf_conv(s1, pmf_normal(0.0, c.s1_decay_spread)); }
    TRY(upload_pmf(h, 1, pmf_conv(s1, tts), d.tab_s1));
    const Pmf st = pmf_mix(pmf_exp(c.t1_gas), c.sf_gas, pmf_exp(c.t3_gas), 1.0 - c.sf_gas);
    Pmf s2 = pmf_conv(st, pmf_luminescence(h->h_lum_x, h->h_lum_t)), s2n = st;
    if (c.s2_time_model == 1 && c.s2_time_spread != 0.0) { s2 = pmf_conv(s2, pmf_normal(0.0, c.s2_time_spread)); s2n = pmf_conv(s2n, pmf_normal(0.0, c.s2_time_spread)); }
    TRY(upload_pmf(h, 2, pmf_conv(s2, tts), d.tab_s2));
    // bases of the model-variant tables (wfs_set_delay_models): 0 transit time, 1 S1 terms, 2 S2 terms, 3 S2 without luminescence
    h->base_pmf = {tts, pmf_conv(s1, tts), pmf_conv(s2, tts), pmf_conv(s2n, tts)};
    return WFS_OK;
}

// The device view, rebuilt from the config and the handle's switches.  The copy-outs of rows and intervals decode the last run with its
// row_slots, he_rows, sum_channel and noise_channels: when one of them moves, whichever wfs_set_* call it was, that run is no longer Complete.
void refresh_dev(wfs_handle *h)
{
    const wfs_config &c = h->cfg; WfsDev &d = h->dev;
    const i32 layout0[4] = {d.row_slots, d.he_rows, d.sum_channel, d.noise_channels};
    d.dt = c.dt; d.samples_before = c.samples_before; d.samples_after = c.samples_after; d.store_before = c.store_before;
    d.store_after = c.store_after; d.tlen = c.tlen; d.tw = c.trigger_window; d.baseline = c.baseline; d.n_rows = c.n_rows;
    d.n_tpc = c.n_tpc; d.n_top = c.n_top; d.he_first = c.he_first; d.he_factor = c.he_factor; d.last_bottom = c.last_bottom;
    d.detector_nt = c.detector_nt; d.s1_simple = c.s1_simple; d.s2_time_model = c.s2_time_model; d.enable_pmt_ap = c.enable_pmt_ap;
    d.c2a = c.c2a; d.tts_mean = c.tts_mean; d.tts_sigma = c.tts_sigma; d.p_dpe = c.p_dpe; d.s1_decay_time = c.s1_decay_time;
    d.s1_decay_spread = c.s1_decay_spread; d.sf_gas = c.sf_gas; d.t1_gas = c.t1_gas; d.t3_gas = c.t3_gas;
    d.s2_time_spread = c.s2_time_spread; d.trap_time = c.trap_time; d.gain_spread = c.gain_spread;
    d.pmt_ap_modifier = c.pmt_ap_modifier; d.pmt_ap_t_modifier = c.pmt_ap_t_modifier; d.rext = c.rext;
    d.k0 = (u32)c.seed; d.k1 = (u32)(c.seed >> 32);
    auto thr = [](double p) -> u64 { if (!(p > 0)) return 0; if (p >= 1) return 4294967296ull; return (u64)(p * 4294967296.0); };
    d.thr_dpe = thr(c.p_dpe); d.dpe_inv = d.thr_dpe ? (double)SPE_BINS / (double)d.thr_dpe : 0.0;
    // HE rows are only materialised when they can differ from a flat baseline: a non-zero int(factor)
    // (rawdata.py:242) or noise columns for the HE channels
    // a noise model takes precedence over the table, which stays where it is for wfs_set_noise_model(h, 0, ...)
    {   // the device view of the model: the state and the layouts of its two buffers (wfs_noise.h)
        const NoiseModelState &m = h->noise;
        const bool model = m.set(), colour = m.coloured(), slow = m.levels() > 0, grouped = colour && m.colour.groups > 0;
        const NoiseColourLayout cl(m.channels, m.colour.groups); const NoiseSlowLayout sl(m.channels, m.colour.groups, colour);
        const i32 *nc = h->nc_buf.p(), *ns = h->ns_buf.p();
        d.nm_cells = model ? (const uint2 *)h->nm_cells.p() : nullptr; d.nm_cells_per_ch = m.k; d.nm_shift = m.shift; d.nm_vmin = m.vmin;
        d.noise_channels = model ? m.channels : h->table_channels;
        // slow levels without a colour: the unit taps of the slow buffer are the taps
        d.nc_taps = colour ? nc + cl.taps : (slow ? ns + sl.unit_taps : nullptr); d.nc_n_taps = colour ? m.colour.n_taps : (slow ? 1 : 0);
        d.nc_groups = colour ? m.colour.groups : 0; d.nc_group = grouped ? nc + cl.group : nullptr; d.nc_mix = grouped ? nc + cl.mix : nullptr;
        d.ns_shift = slow ? ns + sl.shifts : nullptr; d.ns_amp = slow ? ns + sl.amps : nullptr; d.ns_levels = m.levels();
    }
    d.dk_channels = h->dark.channels; d.dk_thr = h->dark.set() ? h->dk_thr.p() : nullptr;
    const bool model = h->noise.set();
    d.enable_noise = (c.enable_noise && (model || d.noise != nullptr)) ? 1 : 0;
    bool he_noise = d.enable_noise && d.noise_channels > c.he_first;
    d.he_rows = (c.detector_nt && c.n_top > 0 && (c.he_factor != 0 || he_noise)) ? 1 : 0;
    d.row_slots = c.n_tpc + (d.he_rows ? c.n_top : 0);
    // the bottom-array sum row: one more slot per window, behind the TPC and HE slots (XENONnT only, rawdata.py:241)
    d.sum_channel = (h->sum_on && c.detector_nt) ? c.sum_channel : -1;
    if (d.sum_channel >= 0) d.row_slots += 1;
    d.full_readout = h->full_on ? 1 : 0;        // (no slot more or less: the layout the copy-outs decode with does not move)
    if (layout0[0] != d.row_slots || layout0[1] != d.he_rows || layout0[2] != d.sum_channel || layout0[3] != d.noise_channels) h->state().view_changed();
}

// the batch came through wfs_load_instructions: its photons are made on the device (run_generation)
bool from_generator(const wfs_handle *h) { return h->batch.kind == BatchKind::Instructions; }
// ... and has n instructions: what the per-instruction setters take
bool generator_batch_of(const wfs_handle *h, i64 n) { return from_generator(h) && n == h->batch.n_ins; }
// wfs_run came to its end: records, counts, truth, photons and pulses may be copied out
bool run_finished(const wfs_handle *h) { return h->run.stage >= RunStage::Finished; }
// ... and the device view still has the row layout it ran with: what is decoded with row_slots, he_rows or sum_channel may be too
bool run_complete(const wfs_handle *h) { return h->run.stage == RunStage::Complete; }
// the photons of a generator batch are made (a run that stopped after the generation, wfs_set_debug bit 2, counts)
bool generated(const wfs_handle *h) { return from_generator(h) && h->run.stage >= RunStage::Generated; }
// photons in front of the PMT afterpulse photons: made by the generator, or brought by the load
i64 n_primary_photons(const wfs_handle *h) { return from_generator(h) ? h->run.n_gen_photons : h->batch.n_photons; }

}  // namespace


// Exception firewall of the C ABI: every extern "C" entry point is a function-try-block, so that a std::bad_alloc /
// std::length_error from the host-side containers becomes an error code + wfs_last_error instead of std::terminate.
static int wfs_caught(wfs_handle *h, const char *fn) noexcept
{
    int code = WFS_E_INVALID; const char *what = "unknown C++ exception";
    char buf[256];
    try { throw; }
    catch (const WfsHipError &e) { return e.code; }      // (download: the message is on the handle already)
    catch (const std::bad_alloc &) { code = WFS_E_NOMEM; what = "out of host memory (std::bad_alloc)"; }
    catch (const std::exception &e) { snprintf(buf, sizeof buf, "%s", e.what()); what = buf; }
    catch (...) {}
    if (h) { try { h->err = std::string(fn) + ": " + what; } catch (...) {} }
    return code;
}
#define WFS_CATCH(h) catch (...) { return wfs_caught((h), __func__); }

extern "C" {

int wfs_device_count(int *n) try { return hipGetDeviceCount(n) == hipSuccess ? WFS_OK : WFS_E_HIP; } WFS_CATCH(nullptr)

int wfs_device_allocations(int64_t *buffers, int64_t *bytes)
{
    if (!buffers || !bytes) return WFS_E_INVALID;
    *buffers = wfs_dev_live_buffers.load(std::memory_order_relaxed); *bytes = wfs_dev_live_bytes.load(std::memory_order_relaxed);
    return WFS_OK;
}

int wfs_create(const wfs_config *cfg, int device, wfs_handle **out)
try {
    if (!cfg || !out) return WFS_E_INVALID;
    // (the fast kernels are specialised for 10 ns samples and 22-tap templates; any other geometry runs through k_pulse_generic)
    if (cfg->n_tpc <= 0 || cfg->n_tpc > WFS_MAX_CH || cfg->dt < 1 || cfg->dt > WFS_MAX_DT || cfg->tlen < 1 || cfg->tlen > WFS_MAX_TLEN
        || cfg->samples_before + cfg->samples_after != cfg->tlen) return WFS_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return WFS_E_HIP;      // fail loudly: no CPU fallback
    if (device < 0 || device >= ndev) return WFS_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WFS_E_HIP;
    std::unique_ptr<wfs_handle> owner(new wfs_handle());
    wfs_handle *h = owner.get();
    h->cfg = *cfg; h->device = device;
    h->generic_geom = cfg->dt != WFS_DT || cfg->tlen != 22;
    { hipDeviceProp_t prop; h->n_cus = (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256; }
    memset(&h->dev, 0, sizeof(h->dev));
    if (hipStreamCreate(&h->stream) != hipSuccess) return WFS_E_HIP;
    h->own_stream = true;
    if (hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&h->rec_copied[0], hipEventDisableTiming) != hipSuccess
        || hipEventCreateWithFlags(&h->rec_copied[1], hipEventDisableTiming) != hipSuccess) return WFS_E_HIP;
    // (a lower priority for the pack stream, with or without a higher one for the main stream, did not help the headline step: DESIGN 7)
    if (hipStreamCreateWithFlags(&h->pack_stream, hipStreamNonBlocking) != hipSuccess) return WFS_E_HIP;
    for (int a = 0; a < 2; a++)
        if (hipEventCreateWithFlags(&h->pack_go[a], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&h->rec_ready[a], hipEventDisableTiming) != hipSuccess) return WFS_E_HIP;
    { const char *e = getenv("WFS_PACK_SYNC"); h->pack_sync = e && atoi(e) != 0; }
    if (ensure(h, h->scal, 1) != WFS_OK) return WFS_E_HIP;
    {   // the host copy of the scalar block; mapped and coherent with the sequence word on the cache line behind it where the
        // device may write it (read_scal), else -- or with WFS_HOST_SYNC=copy, A/B runs -- page-locked for the copy as before
        const char *e = getenv("WFS_HOST_SYNC");
        const size_t bytes = sizeof(WfsScal) + 64;
        static_assert(sizeof(WfsScal) % 64 == 0, "the sequence word starts a cache line");
        void *dp = nullptr;
        if (!(e && !strcmp(e, "copy")) && hipHostMalloc((void **)&h->h_scal, bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
            if (hipHostGetDevicePointer(&dp, h->h_scal, 0) == hipSuccess && dp) h->publish = true;
            else { hipHostFree(h->h_scal); h->h_scal = nullptr; }
        }
        (void)hipGetLastError();
        if (!h->publish && hipHostMalloc((void **)&h->h_scal, bytes, hipHostMallocDefault) != hipSuccess) return WFS_E_HIP;
        memset(h->h_scal, 0, bytes);
        h->h_seq = (uint64_t *)(h->h_scal + 1);
        if (h->publish) { h->d_hscal = (WfsScal *)dp; h->d_hseq = (u64 *)(h->d_hscal + 1); }
    }
#ifdef WFS_STAMPS
    if (ensure(h, h->stamps, 4096 * 64) != WFS_OK) return WFS_E_HIP;
    hipMemset(h->stamps.p(), 0, 4096 * 64 * sizeof(unsigned long long)); h->dev.stamps = h->stamps.p();
#endif
    refresh_dev(h);
    if (const char *e = getenv("WFS_TAP_SPARSE_MAX")) h->tap_sparse_max = std::min(atoi(e), TAP_LIST_LEN - 1);      // tuning knob of tap_block (results do not depend on it)
    if (build_time_tables(h) != WFS_OK) return WFS_E_HIP;
    if (const char *e = getenv("WFS_ROW_RESIDENT")) h->res_env = atoi(e);          // 0 / 1 / 2 as the config switch (A/B runs)
    if (const char *e = getenv("WFS_FULL_READOUT_MAX_SAMPLES")) h->full_max_samples = std::max<i64>(0, atoll(e));      // capacity knob of full readout (tests)
    if (const char *e = getenv("WFS_RES_MAX_LEN")) h->res_max_len = std::max(256, std::min(atoi(e), RES_MAX_LEN)) / 256 * 256;      // tuning knob (results do not depend on it)
    {   // k_s2_bright: what the device grants one workgroup, less the SPE row, the afterpulse stage and the kernel's static arrays
        int granted = 0;
        if (hipDeviceGetAttribute(&granted, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || granted <= 0) granted = 64 * 1024;
        h->bright_lds = bright_lds_of_grant(granted);
        h->bright_max_bins = bright_bins_of_lds(h->bright_lds);
        if (const char *e = getenv("WFS_BRIGHT_MAX_BINS")) h->bright_max_bins = std::max(0, std::min(atoi(e), h->bright_max_bins));      // tuning knob (results do not depend on it)
    }
    // dynamic-LDS caps: every member with a cap of every family that declares one (k_s2_bright: the AP forms' layout, the largest)
    const int bright_cap = bright_lds_layout(h->bright_lds, true).total;
    FamilyBase::each([&](const FamilyBase &f) {
        for (int m = 0; m < f.size(); m++)
            if (const int cap = f.lds_cap(m)) hipFuncSetAttribute(f.address(m), hipFuncAttributeMaxDynamicSharedMemorySize, cap == LDS_CAP_GRANT ? bright_cap : cap);
    });
    *out = owner.release();
    return WFS_OK;
} WFS_CATCH(nullptr)

int wfs_destroy(wfs_handle *h)
try {
    if (!h) return WFS_OK;
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    if (h->pack_stream) hipStreamSynchronize(h->pack_stream);      // (packers that nobody read: the buffers go with the handle)

#ifdef WFS_STAMPS
    {   // diagnostic build: average cycles per workgroup and phase
        std::vector<unsigned long long> all((size_t)4096 * 64); unsigned long long v[64] = {0};
        if (copy_out(h, all.data(), h->stamps.p(), all.size()) == WFS_OK) {
            for (size_t r = 0; r < 4096; r++) for (int i = 0; i < 64; i++) v[i] += all[r * 64 + i];
            for (int i = 0; i < 32; i++) if (v[i + 32]) fprintf(stderr, "stamp %2d: %10.0f cycles/wg  (%llu wgs, %.3e cycles total)\n", i, (double)v[i] / (double)v[i + 32], v[i + 32], (double)v[i]);
        }
    }
#endif
    delete h;
    return WFS_OK;
} WFS_CATCH(nullptr)

const char *wfs_last_error(const wfs_handle *h) { return h ? h->err.c_str() : "null handle"; }

int wfs_set_stream(wfs_handle *h, void *s)
try {
    if (!h) return WFS_E_INVALID;
    TRY(pack_wait(h));          // (from here on the packers run on the caller's stream)
    if (h->own_stream) { hipStreamSynchronize(h->stream); hipStreamDestroy(h->stream); h->own_stream = false; }
    h->stream = (hipStream_t)s;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_synchronize(wfs_handle *h)
try {
    if (!h) return WFS_E_INVALID;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->pack_stream)); h->pack.host_waited();
    return WFS_OK;
} WFS_CATCH(h)
// a noise array of floats (resource.noise_data of a float dtype with non-integral values): add_noise (rawdata.py:436) adds it into
// the int64 row inside numba, which stores the TRUNCATED SUM -- not the sum with the truncated noise.  Replaces the int16 table.
int wfs_set_noise_float(wfs_handle *h, const double *noise, int32_t noise_len, int32_t noise_channels)
try {
    if (!h) return WFS_E_INVALID;
    if (!h->tables_set) return h->fail(WFS_E_STATE, "wfs_set_tables must be called first");
    if (!noise || noise_len <= 0 || noise_channels <= 0) return h->fail(WFS_E_INVALID, "wfs_set_noise_float: empty noise array");
    HIPCHK(hipSetDevice(h->device));
    TRY(pack_wait(h));          // (pending packers read the table this call replaces)
    const size_t stride = (size_t)noise_len + NOISE_PAD;        // (every row followed by its own first samples: wfs_device.h NOISE_PAD)
    std::vector<double> nt(stride * noise_channels);
    for (int64_t i = 0; i < (int64_t)stride; i++) for (int c = 0; c < noise_channels; c++) nt[(size_t)c * stride + i] = noise[(size_t)(i % noise_len) * noise_channels + c];
    TRY(upload(h, h->t_noise_f, nt.data(), nt.size()));
    HIPCHK(hipStreamSynchronize(h->stream));
    WfsDev &d = h->dev;
    d.noise_f = h->t_noise_f.p(); d.noise = (const int16_t *)d.noise_f; d.noise_len = noise_len; h->table_channels = noise_channels; d.noise_stride = (i32)stride;
    refresh_dev(h);
    return WFS_OK;
} WFS_CATCH(h)

int wfs_set_noise_offsets(wfs_handle *h, const int64_t *ix, int64_t n)
try {
    if (!h || n < 0 || (n > 0 && !ix)) return WFS_E_INVALID;
    TRY(pack_wait(h));
    h->n_noise_override = n;
    if (n) { TRY(upload(h, h->noise_override, ix, (size_t)n)); HIPCHK(hipStreamSynchronize(h->stream)); }
    return WFS_OK;
} WFS_CATCH(h)
int wfs_set_window_carry(wfs_handle *h, int32_t has, int64_t t) try { if (!h) return WFS_E_INVALID; h->carry_has = has; h->carry_runmax = t; return WFS_OK; } WFS_CATCH(h)
int wfs_copy_cluster_groups(wfs_handle *h, int32_t *group, int64_t cap)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    if (cap < h->batch.n_clusters) return h->fail(WFS_E_CAPACITY, "cluster buffer too small");
    TRY(copy_out(h, group, h->cl_group.p(), (size_t)h->batch.n_clusters));
    return WFS_OK;
} WFS_CATCH(h)
// (a mode that changes waits for pending packers; a call that leaves it as it is -- one per step is common -- does not)
int wfs_set_debug(wfs_handle *h, int32_t keep) try { if (!h) return WFS_E_INVALID; if (keep != h->debug_bits) TRY(pack_wait(h)); h->debug_bits = keep; return WFS_OK; } WFS_CATCH(h)
int wfs_set_profiling(wfs_handle *h, int32_t on) try { if (!h) return WFS_E_INVALID; if (on != h->profiling) TRY(pack_wait(h)); h->profiling = on; return WFS_OK; } WFS_CATCH(h)

int wfs_set_tables(wfs_handle *h, const double *templates, const double *spe, int32_t n_spe, const double *gains,
                   const double *thr_truth, const int64_t *thr_zle, const double *lum_x, const double *lum_t, int32_t n_lum,
                   const int16_t *noise, int32_t noise_len, int32_t noise_channels)
try {
    if (!h || !templates || !spe || !gains || !thr_truth || !thr_zle || n_spe < 1) return h ? h->fail(WFS_E_INVALID, "wfs_set_tables: null table") : WFS_E_INVALID;
    if (n_spe != 1 && n_spe < h->cfg.n_tpc) return h->fail(WFS_E_INVALID, "wfs_set_tables: n_spe must be 1 or >= n_tpc");
    HIPCHK(hipSetDevice(h->device));
    TRY(pack_wait(h));          // (pending packers read the noise table this call replaces)
    const wfs_config &c = h->cfg;
    TRY(upload(h, h->t_templates, templates, c.dt * c.tlen));
    TRY(upload(h, h->t_spe, spe, SPE_ROW_LEN * (size_t)n_spe));
    TRY(upload(h, h->t_gains, gains, c.n_tpc));
    TRY(upload(h, h->t_thr_truth, thr_truth, c.n_rows));
    TRY(upload(h, h->t_thr_zle, thr_zle, c.n_rows));
    WfsDev &d = h->dev;
    d.n_lum = 0; h->h_lum_x.clear(); h->h_lum_t.clear();
    if (lum_x && lum_t && n_lum >= 2) {
        for (int i = 0; i + 1 < n_lum; i++)
            if (!(lum_x[i + 1] >= lum_x[i]) || !(lum_t[i + 1] > lum_t[i])) return h->fail(WFS_E_INVALID, "luminescence table must be increasing");
        TRY(upload(h, h->t_lumx, lum_x, n_lum)); TRY(upload(h, h->t_lumt, lum_t, n_lum));
        d.n_lum = n_lum; h->h_lum_x.assign(lum_x, lum_x + n_lum); h->h_lum_t.assign(lum_t, lum_t + n_lum);
    }
    TRY(build_time_tables(h));         // the S2 delay table contains the luminescence term
    d.noise = nullptr; d.noise_f = nullptr; d.noise_len = 0; h->table_channels = 0; d.noise_stride = 0;
    if (noise && noise_len > 0 && noise_channels > 0) {
        // channel-major on the device ([channel][sample]; the reference's array is [sample][channel], rawdata.py:429): a row reads
        // consecutive samples of ONE channel -- time-major that is one cache line per sample
        // (and every row followed by its own first samples: wfs_device.h NOISE_PAD)
        const size_t stride = (size_t)noise_len + NOISE_PAD;
        std::vector<int16_t> nt(stride * noise_channels);
        for (int64_t i = 0; i < (int64_t)stride; i++) for (int c = 0; c < noise_channels; c++) nt[(size_t)c * stride + i] = noise[(size_t)(i % noise_len) * noise_channels + c];
        TRY(upload(h, h->t_noise, nt.data(), nt.size()));
        HIPCHK(hipStreamSynchronize(h->stream));
        d.noise = h->t_noise.p(); d.noise_len = noise_len; h->table_channels = noise_channels; d.noise_stride = (i32)stride;
    }
    d.templates = h->t_templates.p(); d.spe = h->t_spe.p(); d.n_spe = n_spe; d.gains = h->t_gains.p();
    d.thr_truth = h->t_thr_truth.p(); d.thr_zle = h->t_thr_zle.p(); d.lum_x = h->t_lumx.p(); d.lum_t = h->t_lumt.p();
    h->h_templates.assign(templates, templates + (size_t)c.dt * c.tlen);
    h->h_gains.assign(gains, gains + c.n_tpc);
    for (int r = 0; r < c.dt; r++) {                       // pulse.py:32 current_max
        double m = templates[r * c.tlen];
        for (int k = 1; k < c.tlen; k++) m = std::max(m, templates[r * c.tlen + k]);
        d.current_max[r] = m;
    }
    refresh_dev(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->tables_set = true;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_set_ap_element(wfs_handle *h, int32_t e, int32_t n_bins_delay, int32_t n_bins_amp, int32_t amp_2d, int32_t is_uniform,
                       double delay_bin, double amp_bin, const double *delay_cdf, const double *amp_cdf)
try {
    if (!h || e < 0 || e >= WFS_MAX_AP || !delay_cdf || !amp_cdf) return WFS_E_INVALID;
    ApElem &a = h->ap[e];
    a.n_bins_delay = n_bins_delay; a.n_bins_amp = n_bins_amp; a.amp_2d = amp_2d; a.is_uniform = is_uniform; a.delay_bin = delay_bin; a.amp_bin = amp_bin;
    TRY(upload(h, a.delay_cdf, delay_cdf, (size_t)h->cfg.n_tpc * n_bins_delay));
    TRY(upload(h, a.amp_cdf, amp_cdf, (size_t)(amp_2d ? h->cfg.n_tpc : 1) * n_bins_amp));
    // the probability column on its own (last entry of every channel's delay row): the generator keeps it in LDS
    std::vector<double> prob((size_t)h->cfg.n_tpc);
    for (int c = 0; c < h->cfg.n_tpc; c++) prob[c] = delay_cdf[(size_t)c * n_bins_delay + n_bins_delay - 1];
    TRY(upload(h, a.prob, prob.data(), prob.size()));
    a.prob_h = prob; a.thr_mod = -1.0;
    // non-decreasing rows (every cumulative distribution is): np.argmin(|cdf - u|) by bisection on the device
    auto rows_sorted = [](const double *c, size_t rows, int n) {
        for (size_t r = 0; r < rows; r++) for (int k = 1; k < n; k++) if (!(c[r * n + k] >= c[r * n + k - 1])) return 0;
        return 1;
    };
    a.delay_sorted = rows_sorted(delay_cdf, (size_t)h->cfg.n_tpc, n_bins_delay);
    a.amp_sorted = rows_sorted(amp_cdf, (size_t)(amp_2d ? h->cfg.n_tpc : 1), n_bins_amp);
    // guides of the sorted rows (ApGuide): for every cell of u * scale a bracket of "first entry >= u" that holds for every u the
    // device can put into the cell -- the cell's ends moved outwards by 2^-40 (the one rounding of u * scale is 2^-53)
    auto build_guides = [&](DevArr<ApGuide> &buf, const double *c, size_t rows, int n) -> int {
        buf.reset();
        if (n < 1 || n > 65535) return WFS_OK;
        std::vector<ApGuide> g(rows);
        const double margin = 9.094947017729282e-13;            // 2^-40
        for (size_t r = 0; r < rows; r++) {
            const double *row = c + r * n;
            auto first_ge = [&](double x) { return (int)(std::lower_bound(row, row + n, x) - row); };
            const double top = row[n - 1];
            g[r].scale = top > 0.0 ? (double)AP_GUIDE / top : 0.0;
            for (int j = 0; j < AP_GUIDE; j++) {
                if (!(g[r].scale > 0.0)) { g[r].lo[j] = 0; g[r].hi[j] = (unsigned short)n; continue; }
                const double x_lo = (double)j / g[r].scale * (1.0 - margin), x_hi = (double)(j + 1) / g[r].scale * (1.0 + margin);
                g[r].lo[j] = (unsigned short)first_ge(x_lo);
                g[r].hi[j] = j == AP_GUIDE - 1 ? (unsigned short)n : (unsigned short)first_ge(x_hi);       // (the last cell also takes every u above the row)
            }
        }
        TRY(upload(h, buf, g.data(), g.size()));
        HIPCHK(hipStreamSynchronize(h->stream));
        return WFS_OK;
    };
    if (a.delay_sorted) TRY(build_guides(a.delay_guide, delay_cdf, (size_t)h->cfg.n_tpc, n_bins_delay)); else a.delay_guide.reset();
    if (a.amp_sorted) TRY(build_guides(a.amp_guide, amp_cdf, (size_t)(amp_2d ? h->cfg.n_tpc : 1), n_bins_amp)); else a.amp_guide.reset();
    h->dev.n_ap = std::max(h->dev.n_ap, e + 1);
    HIPCHK(hipStreamSynchronize(h->stream));
    return WFS_OK;
} WFS_CATCH(h)

// ---------------------------------------------------------------------------------------------- batch input
static int load_clusters(wfs_handle *h, i64 n, const int32_t *cluster, const int64_t *tmin, const uint32_t *gid)
{
    // clusters are contiguous runs of the (sorted) input; first member gives the key and the noise stream id
    std::vector<i64> cl_tmin; std::vector<u32> cl_gid;
    for (i64 i = 0; i < n; i++) {
        if (cluster[i] < 0 || (i > 0 && (cluster[i] < cluster[i - 1] || cluster[i] > cluster[i - 1] + 1)) || (i == 0 && cluster[0] != 0))
            return h->fail(WFS_E_INVALID, "cluster ids must start at 0 and be non-decreasing without gaps");
        if ((i64)cl_tmin.size() <= cluster[i]) { cl_tmin.push_back(tmin[i]); cl_gid.push_back(gid ? gid[i] : (u32)i); }
        else cl_tmin[cluster[i]] = std::min(cl_tmin[cluster[i]], (i64)tmin[i]);
    }
    h->batch.n_clusters = (i64)cl_tmin.size();
    TRY(upload(h, h->cl_tmin, cl_tmin.data(), cl_tmin.size()));
    TRY(upload(h, h->cl_gid, cl_gid.data(), cl_gid.size()));
    HIPCHK(hipStreamSynchronize(h->stream));       // vectors go out of scope
    return WFS_OK;
}

int wfs_load_instructions(wfs_handle *h, int64_t n, const int8_t *type, const int64_t *time, const int32_t *amp, const uint32_t *gid,
                          const int32_t *cluster, const int64_t *tmin, const double *p_hit, const double *drift_mean,
                          const double *drift_spread, const double *sc_gain, const int32_t *cdf_row, const double *cdf_table, int32_t n_cdf,
                          const int32_t *run_set, int64_t n_run_sets, const uint32_t *em_base)
try {
    if (!h) return WFS_E_INVALID;
    if (!h->tables_set) return h->fail(WFS_E_STATE, "wfs_set_tables must be called first");
    if (n <= 0 || !type || !time || !amp || !gid || !cluster || !tmin || !p_hit || !drift_mean || !drift_spread || !sc_gain || !cdf_row || !cdf_table || n_cdf <= 0)
        return h->fail(WFS_E_INVALID, "wfs_load_instructions: null or empty input");
    HIPCHK(hipSetDevice(h->device));
    h->state().load_begins(); BatchState &b = h->batch;
    std::vector<i64> em_off((size_t)n + 1);
    em_off[0] = 0;
    for (i64 i = 0; i < n; i++) {
        if (type[i] != 1 && type[i] != 2 && type[i] != 4 && type[i] != 6)      // 4 / 6: electron afterpulses, simulated like an S2 (afterpulse.py:14, 94)
            return h->fail(WFS_E_INVALID, "instruction types: 1 (S1), 2 (S2), 4 / 6 (photo-ionisation / photo-electric electrons)");
        if (amp[i] < 0) return h->fail(WFS_E_INVALID, "negative amp");
        if (cdf_row[i] < -1 || cdf_row[i] >= n_cdf) return h->fail(WFS_E_INVALID, "cdf_row out of range");
        if (cdf_row[i] == -1 && !h->pmap[type[i] == 1 ? 0 : 1].set) return h->fail(WFS_E_STATE, "cdf_row -1 needs wfs_set_pattern_map for the instruction type");
        if (type[i] != 1 && h->dev.n_lum < 2) return h->fail(WFS_E_STATE, "S2 instructions need the luminescence table");
        em_off[i + 1] = em_off[i] + (type[i] == 1 ? 1 : (i64)amp[i]);
        if (type[i] != 1 && sc_gain[i] > 217.0) b.any_ptrs = true;         // POIS_LAM_MAX: the electrons of such an instruction draw with PTRS (k_s2_photons)
    }
    // pulse sets (one Pulse.__call__ each, rawdata.py:108-127): the caller's run sets, by default one per instruction
    std::vector<i32> ins_set((size_t)n);
    i64 PS = n;
    if (run_set) {
        if (n_run_sets <= 0 || n_run_sets > n) return h->fail(WFS_E_INVALID, "wfs_load_instructions: bad number of run sets");
        PS = n_run_sets;
        for (i64 i = 0; i < n; i++) { if (run_set[i] < 0 || run_set[i] >= PS) return h->fail(WFS_E_INVALID, "run set index out of range"); ins_set[i] = run_set[i]; }
    } else for (i64 i = 0; i < n; i++) ins_set[i] = (i32)i;
    std::vector<i64> set_off((size_t)PS + 1, 0); std::vector<i32> set_list((size_t)n);        // set -> its instructions (CSR)
    for (i64 i = 0; i < n; i++) set_off[ins_set[i] + 1]++;
    // (a run set may be empty: a caller that numbers the sets by their first instruction -- what lets single-instruction sets take the
    // tile-local generator next to the shared Pulse calls of electron afterpulses -- leaves the numbers of the other members unused)
    for (i64 q = 0; q < PS; q++) set_off[q + 1] += set_off[q];
    { std::vector<i64> cur(set_off.begin(), set_off.end() - 1); for (i64 i = 0; i < n; i++) set_list[cur[ins_set[i]]++] = (i32)i; }
    for (i64 q = 0; q < PS; q++)
        for (i64 k = set_off[q] + 1; k < set_off[q + 1]; k++)
            if (cluster[set_list[k]] != cluster[set_list[set_off[q]]] || type[set_list[k]] != type[set_list[set_off[q]]])
                return h->fail(WFS_E_INVALID, "the instructions of a run set must share cluster and type");
    // PMT afterpulses are a second pulse set per primary set (rawdata.py:176-178): set PS + q belongs to set q
    b.ap_sets = h->cfg.enable_pmt_ap && h->dev.n_ap > 0;
    const i64 S = b.ap_sets ? 2 * PS : PS;
    b.run_sets_given = run_set != nullptr;
    b.sets_aligned = PS == n;                     // every set carries the index of its first instruction
    for (i64 q = 0; q < PS && b.sets_aligned; q++) if (set_off[q + 1] > set_off[q] && set_list[set_off[q]] != (i32)q) b.sets_aligned = false;
    for (i64 i = 0; i < n; i++) if (type[i] == 2) { b.any_s2 = true; break; }
    b.n_ins = n; b.n_psets = PS; b.n_sets = S; b.n_emitters = em_off[n]; b.n_tiles = S * h->cfg.n_tpc;
    b.h_rs_off = set_off; b.h_rs_list = set_list;
    if (b.n_tiles > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, "too many tiles in one batch");
    TRY(upload(h, h->ins_type, type, (size_t)n)); TRY(upload(h, h->ins_time, time, (size_t)n)); TRY(upload(h, h->ins_amp, amp, (size_t)n));
    { std::vector<u32> eb((size_t)n, 0u); if (em_base) eb.assign(em_base, em_base + n); TRY(upload(h, h->ins_embase, eb.data(), (size_t)n)); HIPCHK(hipStreamSynchronize(h->stream)); }
    TRY(upload(h, h->ins_gid, gid, (size_t)n)); TRY(upload(h, h->ins_p, p_hit, (size_t)n)); TRY(upload(h, h->ins_dm, drift_mean, (size_t)n));
    TRY(upload(h, h->ins_ds, drift_spread, (size_t)n)); TRY(upload(h, h->ins_sc, sc_gain, (size_t)n));
    // rows -1: the channel CDF of the instruction comes from the device pattern map (wfs_eval_pattern_rows), stored behind the host rows
    b.h_ins_type.assign(type, type + n); b.n_host_rows = n_cdf;
    {
        std::vector<i32> rows(cdf_row, cdf_row + n);
        for (i64 i = 0; i < n; i++) if (rows[i] < 0) { rows[i] = (i32)(n_cdf + (i64)b.dev_row_ins.size()); b.dev_row_ins.push_back((i32)i); }
        b.dev_rows_pending = !b.dev_row_ins.empty();
        const size_t total = (size_t)n_cdf + b.dev_row_ins.size();
        TRY(ensure(h, h->cdf_table, total * h->cfg.n_tpc));
        TRY(upload(h, h->ins_cdfrow, rows.data(), (size_t)n)); HIPCHK(hipStreamSynchronize(h->stream));
    }
    TRY(upload(h, h->cdf_table, cdf_table, (size_t)n_cdf * h->cfg.n_tpc));
    TRY(upload(h, h->em_off, em_off.data(), em_off.size()));
    {
        std::vector<i32> sc((size_t)S), sm((size_t)S, 0); std::vector<i64> st((size_t)S);
        for (i64 q = 0; q < S; q++) {
            const i64 ps = q % PS;
            sm[q] = q >= PS ? 1 : 0;
            if (set_off[ps + 1] == set_off[ps]) { sc[q] = 0; st[q] = 0; continue; }      // an unused set number: no instructions, no photons, no tiles
            i64 t0 = time[set_list[set_off[ps]]];
            for (i64 k = set_off[ps]; k < set_off[ps + 1]; k++) t0 = std::min<i64>(t0, time[set_list[k]]);
            sc[q] = cluster[set_list[set_off[ps]]]; st[q] = t0;
        }
        TRY(upload(h, h->ins_set, ins_set.data(), (size_t)n)); TRY(upload(h, h->set_ins_off, set_off.data(), set_off.size()));
        TRY(upload(h, h->set_ins_list, set_list.data(), (size_t)n));
        TRY(upload(h, h->set_cluster, sc.data(), (size_t)S)); TRY(upload(h, h->set_t0, st.data(), (size_t)S));
        TRY(upload(h, h->set_mode, sm.data(), (size_t)S));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    TRY(load_clusters(h, n, cluster, tmin, gid));
    h->state().load_commits(BatchKind::Instructions);
    return WFS_OK;
} WFS_CATCH(h)

// ---- model variants of the photon delays: S1 'custom' recoil models and optical propagation (s1.py:162-260), S2 garfield
// luminescence and optical propagation (s2.py:380-557).  Each adds one independent integer-truncated term; the host builds
// its probability mass function, the table of the sum is the convolution with the terms wfs_config describes.
int wfs_set_delay_models(wfs_handle *h, int32_t n_tables, const int32_t *base, const int64_t *pmf_off, const double *pmf, const int32_t *vmin)
try {
    if (!h) return WFS_E_INVALID;
    if (!h->tables_set) return h->fail(WFS_E_STATE, "wfs_set_tables must be called first");
    if (n_tables < 0 || n_tables > 65536 || (n_tables > 0 && (!base || !pmf_off || !pmf || !vmin))) return h->fail(WFS_E_INVALID, "wfs_set_delay_models: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    h->x_alias.clear();
    h->x_alias.resize((size_t)n_tables);
    h->h_tabs.assign((size_t)n_tables + 2, AliasTab{});
    h->n_user_tabs = n_tables; h->batch.ins_models = false; h->state().option_changed();      // (the instructions' table numbers meant the tables before)
    for (int k = 0; k < n_tables; k++) {
        if (base[k] < 0 || base[k] > 3 || pmf_off[k + 1] <= pmf_off[k]) return h->fail(WFS_E_INVALID, "wfs_set_delay_models: bad base or empty pmf");
        Pmf e; e.vmin = vmin[k]; e.p.assign(pmf + pmf_off[k], pmf + pmf_off[k + 1]);
        std::vector<double> cum; long v0;
        cum_of_pmf(pmf_conv(h->base_pmf[base[k]], e), cum, v0);
        if (cum.size() > 65000) return h->fail(WFS_E_CAPACITY, "delay table too long");
        TRY(upload_disc(h, h->x_alias[k], cum, (int)v0, h->h_tabs[k]));
    }
    h->h_tabs[n_tables] = h->dev.tab_s1; h->h_tabs[n_tables + 1] = h->dev.tab_s2;       // "-1": the default table of the type
    TRY(upload(h, h->d_tabs, h->h_tabs.data(), h->h_tabs.size()));
    HIPCHK(hipStreamSynchronize(h->stream));
    return WFS_OK;
} WFS_CATCH(h)

// ---- pattern maps evaluated on the device (make_patternmap, load_resource.py:403-435; WeightedNearestNeighbors) ----
static int map_set_grid(wfs_handle *h, wfs_handle::PatternMap &m, int dims, int min_dims, const int32_t *n_nodes, const double *lo, const double *hi, size_t &nodes)
{
    if (dims < min_dims || dims > 3 || !n_nodes || !lo || !hi) return h->fail(WFS_E_INVALID, "map: bad number of dimensions / missing grid");
    nodes = 1; double diag2 = 0;
    for (int a = 0; a < 3; a++) { m.n[a] = 1; m.lo[a] = 0; m.hgrid[a] = 1; m.w[a] = 0; }
    for (int a = 0; a < dims; a++) {
        if (n_nodes[a] < 2 || !(hi[a] > lo[a])) return h->fail(WFS_E_INVALID, "map: every axis needs at least 2 nodes and hi > lo");
        m.n[a] = n_nodes[a]; m.lo[a] = lo[a]; m.hgrid[a] = (hi[a] - lo[a]) / (n_nodes[a] - 1); nodes *= (size_t)n_nodes[a];
        diag2 += m.hgrid[a] * m.hgrid[a];
    }
    // the 2 * dims nearest nodes lie within one cell diagonal (a cell has 2^dims >= 2 * dims corners): candidate block per axis
    for (int a = 0; a < dims; a++) m.w[a] = (i32)ceil(sqrt(diag2) / m.hgrid[a]) + 1;
    m.dims = dims; m.n_points = 0;
    return WFS_OK;
}

static void map_args(const wfs_handle::PatternMap &pm, MapArgs &m)
{
    m.dims = pm.dims; for (int q = 0; q < 3; q++) { m.n[q] = pm.n[q]; m.w[q] = pm.w[q]; m.lo[q] = pm.lo[q]; m.h[q] = pm.hgrid[q]; }
    m.n_points = pm.n_points; m.points = pm.n_points ? pm.points.p() : nullptr;
    m.values = pm.values.p(); m.n_map_ch = pm.n_map_ch;
    m.cell_start = pm.cnx ? pm.cell_start.p() : nullptr; m.cell_pts = pm.cnx ? pm.cell_pts.p() : nullptr;
    m.cnx = pm.cnx; m.cny = pm.cny; m.cell_lo[0] = pm.cell_lo[0]; m.cell_lo[1] = pm.cell_lo[1]; m.cell_h = pm.cell_h;
}

static int launch_neighbours(wfs_handle *h, const MapArgs &m)
{
    if (m.points) return launch(h, PLAIN(k_map_neighbours_points), per_wave(m.n_rows), m);
    return launch(h, PLAIN(k_map_neighbours), per_thread(m.n_rows, 128), m);
}

int wfs_set_pattern_map(wfs_handle *h, int32_t which, int32_t dims, const int32_t *n_nodes, const double *lo, const double *hi,
                        const float *values, int32_t n_map_channels)
try {
    if (!h) return WFS_E_INVALID;
    if (which != 1 && which != 2) return h->fail(WFS_E_INVALID, "wfs_set_pattern_map: which = 1 (S1 map) or 2 (S2 map)");
    auto &m = h->pmap[which - 1];
    if (dims == 0) { m.set = false; return WFS_OK; }
    if (!values || n_map_channels <= 0 || n_map_channels > h->cfg.n_tpc) return h->fail(WFS_E_INVALID, "wfs_set_pattern_map: at most n_tpc channels");
    HIPCHK(hipSetDevice(h->device));
    size_t nodes = 0;
    TRY(map_set_grid(h, m, dims, 2, n_nodes, lo, hi, nodes));
    m.n_map_ch = n_map_channels;
    TRY(upload(h, m.values, values, nodes * (size_t)n_map_channels));
    HIPCHK(hipStreamSynchronize(h->stream));
    m.set = true;
    return WFS_OK;
} WFS_CATCH(h)

// a pattern map on an irregular coordinate system (a list of points; straxen queries a KD-tree for the 2 * dims nearest)
int wfs_set_pattern_map_points(wfs_handle *h, int32_t which, int32_t dims, int64_t n_points, const double *points, const float *values, int32_t n_map_channels)
try {
    if (!h) return WFS_E_INVALID;
    if (which != 1 && which != 2) return h->fail(WFS_E_INVALID, "wfs_set_pattern_map_points: which = 1 (S1 map) or 2 (S2 map)");
    auto &m = h->pmap[which - 1];
    if (dims < 2 || dims > 3 || n_points < 2 * dims || !points || !values || n_map_channels <= 0 || n_map_channels > h->cfg.n_tpc)
        return h->fail(WFS_E_INVALID, "wfs_set_pattern_map_points: 2 or 3 dimensions, at least 2 * dims points, at most n_tpc channels");
    HIPCHK(hipSetDevice(h->device));
    m.dims = dims; m.n_points = n_points; m.n_map_ch = n_map_channels;
    TRY(upload(h, m.points, points, (size_t)n_points * dims));
    TRY(upload(h, m.values, values, (size_t)n_points * (size_t)n_map_channels));
    m.cnx = m.cny = 0;
    if (dims == 2) {
        // cell index for the per-electron searches of the transverse diffusion (k_diffuse_patterns): square cells of about two points
        double lo[2] = {points[0], points[1]}, hi[2] = {points[0], points[1]};
        for (i64 q = 0; q < n_points; q++) for (int a = 0; a < 2; a++) { lo[a] = std::min(lo[a], points[2 * q + a]); hi[a] = std::max(hi[a], points[2 * q + a]); }
        const double span = std::max(std::max(hi[0] - lo[0], hi[1] - lo[1]), 1e-9);
        const double ch = span / std::max<double>(1.0, std::ceil(std::sqrt((double)n_points / 2.0)));
        const i32 cnx = (i32)std::floor((hi[0] - lo[0]) / ch) + 1, cny = (i32)std::floor((hi[1] - lo[1]) / ch) + 1;
        std::vector<i32> start((size_t)cnx * cny + 1, 0), pts((size_t)n_points), cell((size_t)n_points);
        for (i64 q = 0; q < n_points; q++) {
            i32 cx = (i32)std::floor((points[2 * q] - lo[0]) / ch), cy = (i32)std::floor((points[2 * q + 1] - lo[1]) / ch);
            cx = std::min(std::max(cx, 0), cnx - 1); cy = std::min(std::max(cy, 0), cny - 1);
            cell[(size_t)q] = cx * cny + cy; start[(size_t)cell[(size_t)q] + 1]++;
        }
        for (size_t c = 0; c + 1 < start.size(); c++) start[c + 1] += start[c];
        { std::vector<i32> cur(start.begin(), start.end() - 1); for (i64 q = 0; q < n_points; q++) pts[(size_t)cur[(size_t)cell[(size_t)q]]++] = (i32)q; }      // (ascending point index inside a cell)
        TRY(upload(h, m.cell_start, start.data(), start.size())); TRY(upload(h, m.cell_pts, pts.data(), pts.size()));
        m.cnx = cnx; m.cny = cny; m.cell_lo[0] = lo[0]; m.cell_lo[1] = lo[1]; m.cell_h = ch;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    m.set = true;
    return WFS_OK;
} WFS_CATCH(h)

// s2_aft_sigma (s2.py:660-665): the skew-normal factor of every instruction of the loaded batch (NaN: none), applied to the
// rows the device evaluates.  Call between wfs_load_instructions and wfs_eval_pattern_rows.
int wfs_set_instruction_aft(wfs_handle *h, int64_t n, const double *factor)
try {
    if (!h) return WFS_E_INVALID;
    if (!generator_batch_of(h, n)) return h->fail(WFS_E_STATE, "wfs_set_instruction_aft follows wfs_load_instructions of the same batch");
    h->batch.ins_aft_set = false; h->state().option_changed();
    if (!factor) return WFS_OK;
    HIPCHK(hipSetDevice(h->device));
    TRY(upload(h, h->ins_aft, factor, (size_t)n));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->batch.ins_aft_set = true;
    return WFS_OK;
} WFS_CATCH(h)

// diffusion_constant_transverse with enable_field_dependencies['diffusion_transverse_map'] (S2.s2_pattern_map_diffuse, s2.py:560-613):
// sigma_r[i], sigma_a[i] = sqrt(2 D t) of instruction i along / across the radius (cm; NaN: not this path).  The pattern of such an
// instruction is averaged over its surviving electrons inside wfs_run (k_diffuse_patterns), not by wfs_eval_pattern_rows.
// Needs the S2 pattern map on the device (a 2-D regular grid or point list) and the instruction loaded with cdf_row = -1.
int wfs_set_instruction_diffusion(wfs_handle *h, int64_t n, const double *sigma_r, const double *sigma_a, double tpc_radius)
try {
    if (!h) return WFS_E_INVALID;
    if (!generator_batch_of(h, n) || !sigma_r || !sigma_a) return h->fail(WFS_E_STATE, "wfs_set_instruction_diffusion follows wfs_load_instructions of the same batch");
    const auto &pm = h->pmap[1];
    if (!pm.set || pm.dims != 2 || (pm.n_points && !pm.cnx)) return h->fail(WFS_E_STATE, "wfs_set_instruction_diffusion needs a two-dimensional S2 pattern map on the device (wfs_set_pattern_map / wfs_set_pattern_map_points)");
    HIPCHK(hipSetDevice(h->device));
    h->batch.ins_diff.assign((size_t)n, 0); h->state().option_changed();
    std::vector<char> is_dev((size_t)n, 0);
    for (i32 i : h->batch.dev_row_ins) is_dev[i] = 1;
    std::vector<i32> rows; std::vector<i64> ids;
    for (size_t k = 0; k < h->batch.dev_row_ins.size(); k++) {
        const i32 i = h->batch.dev_row_ins[k];
        if (h->batch.h_ins_type[i] == 1 || !(sigma_r[i] == sigma_r[i]) || !(sigma_a[i] == sigma_a[i])) continue;
        h->batch.ins_diff[i] = 1; rows.push_back(i); ids.push_back(h->batch.n_host_rows + (i64)k);
    }
    for (i64 i = 0; i < n; i++)
        if (h->batch.h_ins_type[i] != 1 && sigma_r[i] == sigma_r[i] && !is_dev[i]) return h->fail(WFS_E_STATE, "transverse diffusion: the instruction must take its pattern from the device map (cdf_row = -1)");
    h->batch.n_diff_rows = (i64)rows.size(); h->batch.diff_r2 = tpc_radius * tpc_radius;
    TRY(upload(h, h->ins_sigr, sigma_r, (size_t)n)); TRY(upload(h, h->ins_siga, sigma_a, (size_t)n));
    TRY(upload(h, h->diff_row_ins, rows.data(), rows.size())); TRY(upload(h, h->diff_row_id, ids.data(), ids.size()));
    HIPCHK(hipStreamSynchronize(h->stream));
    return WFS_OK;
} WFS_CATCH(h)

// ---- scalar maps on the device: LCE (s1.py:125), S2 correction / SE gain (s2.py:193-234), longitudinal diffusion (s2.py:170),
// field-dependence splines (s2.py:150, 248), field distortion maps (s2.py:41, 66) ----
static int smap_new(wfs_handle *h, std::unique_ptr<wfs_handle::ScalarMap> m, int32_t *map_id)
{
    HIPCHK(hipStreamSynchronize(h->stream));
    h->smaps.push_back(std::move(m));
    *map_id = (int32_t)h->smaps.size() - 1;
    return WFS_OK;
}

static int scalar_map_grid(wfs_handle *h, int kind, int32_t dims, const int32_t *n_nodes, const double *lo, const double *hi, const double *values, int32_t n_values, int32_t *map_id)
{
    if (!h || !map_id || !values) return WFS_E_INVALID;
    if (n_values < 1 || n_values > 4096) return h->fail(WFS_E_INVALID, "scalar map: 1 .. 4096 values per node");
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<wfs_handle::ScalarMap> m(new wfs_handle::ScalarMap()); size_t nodes = 0;
    m->kind = kind; m->nv = n_values;
    TRY(map_set_grid(h, m->g, dims, 1, n_nodes, lo, hi, nodes));
    TRY(upload(h, m->values, values, nodes * (size_t)n_values));
    return smap_new(h, std::move(m), map_id);
}

int wfs_scalar_map_grid(wfs_handle *h, int32_t dims, const int32_t *n_nodes, const double *lo, const double *hi, const double *values, int32_t *map_id)
try { return scalar_map_grid(h, 0, dims, n_nodes, lo, hi, values, 1, map_id); } WFS_CATCH(h)

int wfs_scalar_map_grid_array(wfs_handle *h, int32_t dims, const int32_t *n_nodes, const double *lo, const double *hi, const double *values, int32_t n_values, int32_t *map_id)
try { return scalar_map_grid(h, 0, dims, n_nodes, lo, hi, values, n_values, map_id); } WFS_CATCH(h)

int wfs_scalar_map_linear(wfs_handle *h, int32_t dims, const int32_t *n_nodes, const double *lo, const double *hi, const double *values, int32_t n_values, int32_t *map_id)
try { return scalar_map_grid(h, 3, dims, n_nodes, lo, hi, values, n_values, map_id); } WFS_CATCH(h)

static int scalar_map_points(wfs_handle *h, int32_t dims, int64_t n_points, const double *points, const double *values, int32_t n_values, int32_t *map_id)
{
    if (!h || !map_id || !values || !points || dims < 1 || dims > 3 || n_points < 2 * dims) return h ? h->fail(WFS_E_INVALID, "wfs_scalar_map_points: 1..3 dimensions, at least 2 * dims points") : WFS_E_INVALID;
    if (n_values < 1 || n_values > 4096) return h->fail(WFS_E_INVALID, "scalar map: 1 .. 4096 values per node");
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<wfs_handle::ScalarMap> m(new wfs_handle::ScalarMap());
    m->kind = 1; m->nv = n_values; m->g.dims = dims; m->g.n_points = n_points;
    TRY(upload(h, m->g.points, points, (size_t)n_points * dims));
    TRY(upload(h, m->values, values, (size_t)n_points * (size_t)n_values));
    return smap_new(h, std::move(m), map_id);
}

int wfs_scalar_map_points(wfs_handle *h, int32_t dims, int64_t n_points, const double *points, const double *values, int32_t *map_id)
try { return scalar_map_points(h, dims, n_points, points, values, 1, map_id); } WFS_CATCH(h)

int wfs_scalar_map_points_array(wfs_handle *h, int32_t dims, int64_t n_points, const double *points, const double *values, int32_t n_values, int32_t *map_id)
try { return scalar_map_points(h, dims, n_points, points, values, n_values, map_id); } WFS_CATCH(h)

int wfs_scalar_map_spline(wfs_handle *h, int32_t nx, const double *tx, int32_t ny, const double *ty, int32_t kx, int32_t ky, const double *c, int32_t *map_id)
try {
    if (!h || !map_id || !tx || !ty || !c) return WFS_E_INVALID;
    if (kx < 1 || kx > 5 || ky < 1 || ky > 5 || nx < 2 * kx + 2 || ny < 2 * ky + 2) return h->fail(WFS_E_INVALID, "wfs_scalar_map_spline: degrees 1..5, at least 2 (k + 1) knots per axis");
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<wfs_handle::ScalarMap> m(new wfs_handle::ScalarMap());
    m->kind = 2; m->nx = nx; m->ny = ny; m->kx = kx; m->ky = ky;
    TRY(upload(h, m->tx, tx, (size_t)nx)); TRY(upload(h, m->ty, ty, (size_t)ny));
    TRY(upload(h, m->c, c, (size_t)(nx - kx - 1) * (size_t)(ny - ky - 1)));
    return smap_new(h, std::move(m), map_id);
} WFS_CATCH(h)

static int scalar_map_eval(wfs_handle *h, int32_t map_id, int64_t n, const double *pos, double *out, int32_t n_values)
{
    if (!h) return WFS_E_INVALID;
    if (map_id < 0 || (size_t)map_id >= h->smaps.size() || n < 0 || (n && (!pos || !out))) return h->fail(WFS_E_INVALID, "wfs_scalar_map_eval: unknown map or missing arrays");
    const auto &sm = *h->smaps[map_id];
    if (sm.nv != n_values) return h->fail(WFS_E_INVALID, "wfs_scalar_map_eval: the map has another number of values per node (wfs_scalar_map_eval_array)");
    if (n == 0) return WFS_OK;
    HIPCHK(hipSetDevice(h->device));
    const int dims = sm.kind == 2 ? 2 : sm.g.dims, nv = sm.nv;
    TRY(upload(h, h->smap_pos, pos, (size_t)n * dims)); TRY(ensure(h, h->smap_out, (size_t)n * nv));
    if (sm.kind == 2) {
        SplineArgs a{sm.nx, sm.ny, sm.kx, sm.ky, sm.tx.p(), sm.ty.p(), sm.c.p(), n, h->smap_pos.p(), h->smap_out.p()};
        TRY(launch(h, PLAIN(k_map_spline), per_thread(n, 128), a));
    } else if (sm.kind == 3) {
        LinearMapArgs a{};
        a.dims = dims; a.nv = nv; a.values = sm.values.p(); a.n_rows = n; a.pos = h->smap_pos.p(); a.out = h->smap_out.p();
        for (int q = 0; q < 3; q++) { a.n[q] = sm.g.n[q]; a.lo[q] = sm.g.lo[q]; a.h[q] = sm.g.hgrid[q]; }
        TRY(launch(h, PLAIN(k_map_linear), per_thread(n * nv, 128), a));
    } else {
        TRY(ensure(h, h->smap_nb_idx, (size_t)n * MAP_K)); TRY(ensure(h, h->smap_nb_w, (size_t)n * MAP_K));
        MapArgs m{};
        map_args(sm.g, m);
        m.n_rows = n; m.pos = h->smap_pos.p(); m.nb_idx = h->smap_nb_idx.p(); m.nb_w = h->smap_nb_w.p();
        TRY(launch_neighbours(h, m));
        TRY(launch(h, PLAIN(k_map_scalar), per_thread(n * nv, 128), m, sm.values.p(), h->smap_out.p(), nv));
    }
    TRY(copy_async(h, out, h->smap_out.p(), (size_t)n * nv, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return WFS_OK;
}

int wfs_scalar_map_eval(wfs_handle *h, int32_t map_id, int64_t n, const double *pos, double *out)
try { return scalar_map_eval(h, map_id, n, pos, out, 1); } WFS_CATCH(h)

int wfs_scalar_map_eval_array(wfs_handle *h, int32_t map_id, int64_t n, const double *pos, double *out, int32_t n_values)
try { return scalar_map_eval(h, map_id, n, pos, out, n_values); } WFS_CATCH(h)

int wfs_eval_pattern_rows(wfs_handle *h, int64_t n, const float *x, const float *y, const float *z)
try {
    if (!h) return WFS_E_INVALID;
    if (!generator_batch_of(h, n) || !x || !y || !z) return h->fail(WFS_E_STATE, "wfs_eval_pattern_rows follows wfs_load_instructions of the same batch");
    if (h->batch.dev_row_ins.empty()) return WFS_OK;
    HIPCHK(hipSetDevice(h->device));
    const int nch = h->cfg.n_tpc;
    TRY(upload(h, h->map_x, x, (size_t)n)); TRY(upload(h, h->map_y, y, (size_t)n)); TRY(upload(h, h->map_z, z, (size_t)n));
    i64 first = h->batch.n_host_rows;
    // rows were numbered in instruction order; evaluate them map by map, each over its own (ordered) subset
    std::vector<i32> rows_of[2]; std::vector<i64> row_id[2];
    for (size_t k = 0; k < h->batch.dev_row_ins.size(); k++) {
        if (!h->batch.ins_diff.empty() && h->batch.ins_diff[h->batch.dev_row_ins[k]]) continue;       // averaged over its electrons inside wfs_run
        const int w = h->batch.h_ins_type[h->batch.dev_row_ins[k]] == 1 ? 0 : 1; rows_of[w].push_back(h->batch.dev_row_ins[k]); row_id[w].push_back(first + (i64)k);
    }
    for (int w = 0; w < 2; w++) {
        if (rows_of[w].empty()) continue;
        const auto &pm = h->pmap[w];
        const i64 nr = (i64)rows_of[w].size();
        TRY(upload(h, h->map_row_ins[w], rows_of[w].data(), (size_t)nr)); TRY(upload(h, h->map_row_id[w], row_id[w].data(), (size_t)nr));
        TRY(ensure(h, h->map_nb_idx[w], (size_t)nr * MAP_K)); TRY(ensure(h, h->map_nb_w[w], (size_t)nr * MAP_K));
        MapArgs m{};
        map_args(pm, m);
        m.n_rows = nr; m.row_ins = h->map_row_ins[w].p(); m.row_id = h->map_row_id[w].p();
        m.aft = (w == 1 && h->batch.ins_aft_set) ? h->ins_aft.p() : nullptr; m.n_top = h->cfg.n_top;
        m.x = h->map_x.p(); m.y = h->map_y.p(); m.z = h->map_z.p();
        m.nb_idx = h->map_nb_idx[w].p(); m.nb_w = h->map_nb_w[w].p();
        m.cdf_table = h->cdf_table.p(); m.gains = h->t_gains.p();
        TRY(launch_neighbours(h, m));
        TRY(launch(h, PLAIN(k_map_rows), per_group(nr, 256, (size_t)map_rows_lds(nch).total), m, nch));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    h->batch.dev_rows_pending = false; h->state().option_changed();
    return WFS_OK;
} WFS_CATCH(h)

// channel CDF rows of the loaded batch as the generator sees them (host rows followed by the device-evaluated ones)
int wfs_copy_cdf_rows(wfs_handle *h, int32_t *cdf_row, double *cdf_table, int64_t cap_rows)
try {
    if (!h || !from_generator(h)) return WFS_E_STATE;
    if (h->batch.dev_rows_pending) return h->fail(WFS_E_STATE, "wfs_eval_pattern_rows has not been called for this batch");
    const i64 total = h->batch.n_host_rows + (i64)h->batch.dev_row_ins.size();
    if (cap_rows < total) return h->fail(WFS_E_CAPACITY, "cdf row buffer too small");
    HIPCHK(hipSetDevice(h->device));
    if (cdf_row) TRY(copy_out(h, cdf_row, h->ins_cdfrow.p(), (size_t)h->batch.n_ins));
    if (cdf_table) TRY(copy_out(h, cdf_table, h->cdf_table.p(), (size_t)total * h->cfg.n_tpc));
    return WFS_OK;
} WFS_CATCH(h)

int wfs_set_s1_propagation(wfs_handle *h, int32_t nz, int32_t nu, double u0, double du, const double *top, const double *bottom)
try {
    if (!h) return WFS_E_INVALID;
    if (nz == 0) { h->prop_nz = 0; return WFS_OK; }
    if (nz < 2 || nu < 2 || !(du > 0) || !top || !bottom) return h->fail(WFS_E_INVALID, "wfs_set_s1_propagation: needs a grid of at least 2 x 2 nodes");
    HIPCHK(hipSetDevice(h->device));
    TRY(upload(h, h->prop_top, top, (size_t)nz * nu)); TRY(upload(h, h->prop_bot, bottom, (size_t)nz * nu));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->prop_nz = nz; h->prop_nu = nu; h->prop_u0 = u0; h->prop_du = du;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_set_instruction_models(wfs_handle *h, int64_t n, const int32_t *tab, const int32_t *tab_bottom, const int32_t *prop_zi, const double *prop_zf)
try {
    if (!h) return WFS_E_INVALID;
    if (!generator_batch_of(h, n)) return h->fail(WFS_E_STATE, "wfs_set_instruction_models follows wfs_load_instructions of the same batch");
    if (h->d_tabs.p() == nullptr) TRY(wfs_set_delay_models(h, 0, nullptr, nullptr, nullptr, nullptr));
    HIPCHK(hipSetDevice(h->device));
    const std::vector<int8_t> type = download(h, h->ins_type, (size_t)n);
    std::vector<i32> t((size_t)n), tb((size_t)n), zi((size_t)n, -1); std::vector<double> zf((size_t)n, 0.0);
    for (i64 i = 0; i < n; i++) {
        const i32 dflt = h->n_user_tabs + (type[i] == 1 ? 0 : 1);
        const i32 a = tab ? tab[i] : -1, b = tab_bottom ? tab_bottom[i] : a;
        if (a < -1 || a >= h->n_user_tabs || b < -1 || b >= h->n_user_tabs) return h->fail(WFS_E_INVALID, "delay table index out of range");
        t[i] = a < 0 ? dflt : a; tb[i] = b < 0 ? dflt : b;
        if (prop_zi && prop_zi[i] >= 0) {
            if (h->prop_nz < 2 || prop_zi[i] > h->prop_nz - 2 || !prop_zf) return h->fail(WFS_E_INVALID, "S1 propagation cell out of range (wfs_set_s1_propagation first)");
            zi[i] = prop_zi[i]; zf[i] = prop_zf[i];
        }
    }
    TRY(upload(h, h->ins_tab, t.data(), (size_t)n)); TRY(upload(h, h->ins_tabb, tb.data(), (size_t)n));
    TRY(upload(h, h->ins_pzi, zi.data(), (size_t)n)); TRY(upload(h, h->ins_pzf, zf.data(), (size_t)n));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->batch.ins_models = true; h->state().option_changed();
    return WFS_OK;
} WFS_CATCH(h)

// ---- s2_luminescence_model 'garfield_gas_gap' (s2.py:413-483, load_resource.py:284-291) ----
int wfs_set_gas_gap_model(wfs_handle *h, int32_t n_gas_gaps, int32_t n_points, const double *timing_inv_cdf)
try {
    if (!h) return WFS_E_INVALID;
    if (n_gas_gaps == 0) { h->gg_n = 0; return WFS_OK; }
    if (n_gas_gaps < 1 || n_points < 3 || !timing_inv_cdf) return h->fail(WFS_E_INVALID, "wfs_set_gas_gap_model: at least one table of at least 3 points");
    HIPCHK(hipSetDevice(h->device));
    TRY(upload(h, h->gg_inv, timing_inv_cdf, (size_t)n_gas_gaps * n_points));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->gg_n = n_gas_gaps; h->gg_L = n_points;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_set_instruction_gas_gap(wfs_handle *h, int64_t n, const int32_t *table, const double *weight)
try {
    if (!h) return WFS_E_INVALID;
    if (!generator_batch_of(h, n) || !table || !weight) return h->fail(WFS_E_STATE, "wfs_set_instruction_gas_gap follows wfs_load_instructions of the same batch");
    if (h->gg_n < 1) return h->fail(WFS_E_STATE, "wfs_set_gas_gap_model first");
    for (i64 i = 0; i < n; i++) if (table[i] < -1 || table[i] >= h->gg_n) return h->fail(WFS_E_INVALID, "gas gap table index out of range");
    HIPCHK(hipSetDevice(h->device));
    TRY(upload(h, h->ins_gg, table, (size_t)n)); TRY(upload(h, h->ins_ggw, weight, (size_t)n));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->batch.ins_gg_set = true; h->state().option_changed();
    return WFS_OK;
} WFS_CATCH(h)

int wfs_load_photons(wfs_handle *h, int64_t n_sets, const int32_t *set_cluster, const int64_t *set_tmin, const int64_t *set_off,
                     const int64_t *t, const int16_t *ch, const double *gain, const uint8_t *dpe)
try {
    if (!h) return WFS_E_INVALID;
    if (!h->tables_set) return h->fail(WFS_E_STATE, "wfs_set_tables must be called first");
    if (n_sets <= 0 || !set_cluster || !set_tmin || !set_off) return h->fail(WFS_E_INVALID, "wfs_load_photons: null or empty input");
    HIPCHK(hipSetDevice(h->device));
    h->state().load_begins(); BatchState &b = h->batch;
    const i64 P = set_off[n_sets]; const int nch = h->cfg.n_tpc;
    b.n_sets = n_sets; b.n_tiles = n_sets * nch; b.n_photons = P;
    if (b.n_tiles > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, "too many tiles in one batch");
    // host bucketing: the input is already channel sorted inside each set
    std::vector<i32> count((size_t)b.n_tiles, 0), tmn((size_t)b.n_tiles, 0x7fffffff), tmx((size_t)b.n_tiles, (i32)0x80000000), rel((size_t)P);
    std::vector<i64> t0((size_t)n_sets, 0);
    std::vector<i32> mode((size_t)n_sets, 1);
    for (i64 s = 0; s < n_sets; s++) {
        i64 a = set_off[s], b = set_off[s + 1];
        if (b < a) return h->fail(WFS_E_INVALID, "set_off must be non-decreasing");
        if (b == a) { t0[s] = set_tmin[s]; continue; }
        i64 mn = t[a];
        for (i64 p = a; p < b; p++) mn = std::min(mn, (i64)t[p]);
        t0[s] = mn;
        for (i64 p = a; p < b; p++) {
            if (ch[p] < 0 || ch[p] >= nch) return h->fail(WFS_E_INVALID, "photon channel out of range");
            if (h->h_gains[ch[p]] == 0) return h->fail(WFS_E_INVALID, "photon on a turned-off PMT (gain 0): drop it before wfs_load_photons (pulse.py:89-90)");
            if (p > a && ch[p] < ch[p - 1]) return h->fail(WFS_E_INVALID, "photons of a set must be sorted by channel");
            i64 r = t[p] - mn;
            if (r > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, "photon time span of a set exceeds 2^31 ns");
            rel[p] = (i32)r;
            size_t tile = (size_t)(s * nch + ch[p]);
            count[tile]++; tmn[tile] = std::min(tmn[tile], (i32)r); tmx[tile] = std::max(tmx[tile], (i32)r);
        }
    }
    b.h_set_off.assign(set_off, set_off + n_sets + 1);
    TRY(upload(h, h->set_cluster, set_cluster, (size_t)n_sets)); TRY(upload(h, h->set_t0, t0.data(), (size_t)n_sets));
    TRY(upload(h, h->set_mode, mode.data(), (size_t)n_sets));
    TRY(upload(h, h->tile_count, count.data(), count.size())); TRY(upload(h, h->tile_tmin, tmn.data(), tmn.size()));
    TRY(upload(h, h->tile_tmax, tmx.data(), tmx.size()));
    TRY(upload(h, h->ph_gain, gain, (size_t)P));
    {   // DPE flags ride in the code word (only the truth quirk pulse.py:255 reads them in explicit-gain mode)
        std::vector<PhotonRec> recs((size_t)P);
        for (i64 p = 0; p < P; p++) recs[p] = PhotonRec{rel[p], (dpe && dpe[p]) ? (1u << 16) : 0u};
        TRY(upload(h, h->ph, recs.data(), (size_t)P));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    TRY(load_clusters(h, n_sets, set_cluster, set_tmin, nullptr));
    h->state().load_commits(BatchKind::Photons);
    return WFS_OK;
} WFS_CATCH(h)

// capacity of the afterpulse lists of an optical batch of P photons: the generator's rule (gen_block_photons)
static i64 optical_ap_cap(i64 P) { return P / 8 + 65536; }

int wfs_load_optical(wfs_handle *h, int64_t n, const int64_t *time, const uint32_t *gid, const int32_t *cluster, const int64_t *tmin,
                     const int32_t *first, const int32_t *last, const int32_t *channels, const int64_t *timings, int64_t n_ph, int64_t cutoff)
try {
    if (!h) return WFS_E_INVALID;
    if (!h->tables_set) return h->fail(WFS_E_STATE, "wfs_set_tables must be called first");
    if (n <= 0 || !time || !gid || !cluster || !tmin || !first || !last || (n_ph > 0 && (!channels || !timings)))
        return h->fail(WFS_E_INVALID, "wfs_load_optical: null or empty input");
    HIPCHK(hipSetDevice(h->device));
    h->state().load_begins(); BatchState &b = h->batch;
    const int nch = h->cfg.n_tpc;
    // PMT afterpulses are a second pulse set per instruction (rawdata.py:176-178, behind every primary Pulse call): set n + i belongs to set i
    b.ap_sets = h->cfg.enable_pmt_ap && h->dev.n_ap > 0;
    const i64 S = b.ap_sets ? 2 * n : n;
    b.n_ins = n; b.n_psets = n; b.n_sets = S; b.n_tiles = S * nch;
    if (b.n_tiles > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, "too many tiles in one batch");
    i64 n_ranged = 0;        // photons the instructions name: ranges may overlap (rawdata.py:477 takes any), so this can exceed n_ph
    for (i64 i = 0; i < n; i++) {
        if (first[i] < 0 || last[i] < first[i] || last[i] > n_ph) return h->fail(WFS_E_INVALID, "_first/_last out of range");
        n_ranged += (i64)last[i] - first[i];
        if (b.ap_sets && (i64)last[i] - first[i] >= (1LL << 29))      // (the order key of an afterpulse holds 29 bits of its parent's index)
            return h->fail(WFS_E_CAPACITY, "an instruction of 2^29 or more supplied photons with PMT afterpulses on");
    }
    // the photons are bucketed by (instruction, channel) on the device: count, scan, place (k_optical_bucket) -- the primary tiles only
    const i64 T = n * nch;
    {
        std::vector<i32> mode((size_t)S, 0), sc((size_t)S); std::vector<i64> st((size_t)S); std::vector<u32> sg((size_t)S);
        for (i64 q = 0; q < S; q++) { sc[q] = cluster[q % n]; st[q] = time[q % n]; sg[q] = gid[q % n]; mode[q] = q >= n ? 1 : 0; }
        TRY(upload(h, h->set_cluster, sc.data(), (size_t)S)); TRY(upload(h, h->set_t0, st.data(), (size_t)S)); TRY(upload(h, h->set_mode, mode.data(), (size_t)S));
        TRY(upload(h, h->set_gid, sg.data(), (size_t)S)); TRY(upload(h, h->ins_time, time, (size_t)n));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    TRY(upload(h, h->opt_first, first, (size_t)n)); TRY(upload(h, h->opt_last, last, (size_t)n));
    TRY(upload(h, h->opt_ch, channels, (size_t)n_ph)); TRY(upload(h, h->opt_time, timings, (size_t)n_ph));
    TRY(ensure(h, h->tile_count, (size_t)b.n_tiles)); TRY(ensure(h, h->tile_cursor, (size_t)b.n_tiles)); TRY(ensure(h, h->tile_off, (size_t)(b.n_tiles + 1)));
    // (the bucketed copies hold a slot per photon of every instruction's range, not per entry of the flat arrays)
    TRY(ensure(h, h->opt_t, (size_t)n_ranged)); TRY(ensure(h, h->opt_item, (size_t)n_ranged));
    {
        FillGroup fg(h, "fills_optical");
        TRY(fg.zero(h->tile_count.p(), T)); TRY(fg.zero(h->tile_cursor.p(), T)); TRY(fg.zero(h->scal.p(), 1));
        TRY(fg.flush());
    }
    OptLoadArgs oa{n, h->opt_first.p(), h->opt_last.p(), h->opt_ch.p(), h->opt_time.p(), cutoff, h->t_gains.p(),
                   h->tile_count.p(), h->tile_off.p(), h->tile_cursor.p(), h->opt_t.p(), h->opt_item.p(), h->scal.p()};
    // (not timed: part of the load, whose entries wfs_run clears before anyone can read them)
    TRY(launch_untimed(h, K_OPTICAL_BUCKET(false), per_thread(n), h->dev, oa));
    TRY(scan_into(h, h->tile_count.p(), T, h->tile_off.p(), &WfsScal::n_tile_photons, 0));
    TRY(launch_untimed(h, K_OPTICAL_BUCKET(true), per_thread(n), h->dev, oa));      // (not timed: as the count pass above)
    TRY(read_scal(h));
    HIPCHK(hipGetLastError());
    TRY(device_error(h, h->h_scal->opt_error));
    const i64 P = b.n_photons = h->h_scal->n_tile_photons;
    // (with afterpulses the array also holds theirs, behind the primary photons: sized here, k_optical_finish writes into it)
    TRY(ensure(h, h->ph, (size_t)(P + (b.ap_sets ? optical_ap_cap(P) : 0))));
    TRY(ensure(h, h->tile_tmin, (size_t)b.n_tiles)); TRY(ensure(h, h->tile_tmax, (size_t)b.n_tiles));
    TRY(ensure(h, h->el_stat, (size_t)n * STAT_PER_INS)); TRY(ensure(h, h->el_minmax, (size_t)n * MINMAX));
    HIPCHK(hipMemsetAsync(h->el_stat.p(), 0, (size_t)n * STAT_PER_INS * sizeof(double), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    TRY(load_clusters(h, n, cluster, tmin, gid));
    h->state().load_commits(BatchKind::Optical);
    return WFS_OK;
} WFS_CATCH(h)

// ---------------------------------------------------------------------------------------------- run
// pulses made by k_s2_tile (wfs_tilegen.h): their tiles are on no work list
static bool tiles_made(const wfs_handle *h) { return from_generator(h) && h->run.fuse_full && h->run.n_fused_tiles + h->run.n_bright_tiles > 0; }
// tiles that drew their own photons, whichever kernel made them
static i64 n_tilegen_tiles(const wfs_handle *h) { return h->run.n_fused_tiles + h->run.n_gen_tiles + h->run.n_bright_tiles; }
// ph_gain holds the photons with an explicit gain only: every photon of an injected batch, or the PMT afterpulses, which follow the
// n_photons primary ones; the kernels index it by photon number
static const double *ph_gain_base(const wfs_handle *h) { return h->batch.ap_sets ? h->ph_gain.p() - n_primary_photons(h) : h->ph_gain.p(); }
// the templates as the pulse kernels take them by value: t[tap * dt + ns remainder]
static TemplateArg fill_template_arg(const wfs_handle *h)
{
    TemplateArg tp;
    for (int k = 0; k < 22; k++) for (int r = 0; r < WFS_DT; r++) tp.t[k * WFS_DT + r] = h->h_templates[(size_t)r * 22 + k];
    return tp;
}
// What crosses the stage boundaries of one run_generation (on its stack).
struct GenRun {
    GenArgs g{}; FuseArgs f{}; ApArgs ap{};
    bool ext = false, ap_on = false;      // timing-model variants per instruction; PMT afterpulses
    i64 TP = 0, P = 0, ap_cap = 0;        // primary tiles (afterpulse tiles follow); photons of the block generator; capacity of the afterpulse lists
};

// ---- generation 1: electrons, and which tiles make their own photons
static int gen_electrons(wfs_handle *h, GenRun &r, FillGroup &fg)
{
    const WfsDev &d = h->dev;
    GenArgs &g = r.g; FuseArgs &f = r.f;
    const i64 N = h->batch.n_ins, E = h->batch.n_emitters, T = h->batch.n_tiles;
    TRY(ensure(h, h->em_time, (size_t)E)); TRY(ensure(h, h->em_nph, (size_t)E)); TRY(ensure(h, h->em_ins, (size_t)E));
    TRY(ensure(h, h->el_stat, (size_t)N * STAT_PER_INS)); TRY(ensure(h, h->el_minmax, (size_t)N * MINMAX));
    // (fg: the fills at the head of the generation, behind the scalar block's of wfs_run; flushed in front of the first kernel)
    TRY(fg.zero(h->el_stat.p(), N * STAT_PER_INS));
    TRY(fg.pairs(h->el_minmax.p(), N * MINMAX, I64_MAX, I64_MIN));      // (min, max) pairs: (I64_MAX, I64_MIN)
    g.n_ins = N; g.n_psets = h->batch.n_psets; g.n_emitters = E;
    g.ins_embase = h->ins_embase.p(); g.ins_set = h->ins_set.p(); g.set_ins_off = h->set_ins_off.p(); g.set_ins_list = h->set_ins_list.p(); g.set_t0 = h->set_t0.p();
    g.ins_type = h->ins_type.p(); g.ins_time = h->ins_time.p(); g.ins_amp = h->ins_amp.p(); g.ins_gid = h->ins_gid.p();
    g.ins_p = h->ins_p.p(); g.ins_dm = h->ins_dm.p(); g.ins_ds = h->ins_ds.p(); g.ins_sc = h->ins_sc.p();
    g.ins_cdfrow = h->ins_cdfrow.p(); g.cdf_table = h->cdf_table.p(); g.em_off = h->em_off.p();
    g.em_time = h->em_time.p(); g.em_nph = h->em_nph.p(); g.em_ins = h->em_ins.p();
    g.el_stat = h->el_stat.p(); g.el_minmax = h->el_minmax.p(); g.scal = h->scal.p();
    const bool ext = r.ext = h->batch.ins_models;
    if (ext) {
        g.tabs = h->d_tabs.p(); g.ins_tab = h->ins_tab.p(); g.ins_tabb = h->ins_tabb.p();
        g.ins_pzi = h->ins_pzi.p(); g.ins_pzf = h->ins_pzf.p();
        if (h->prop_nz >= 2) { g.prop_top = h->prop_top.p(); g.prop_bot = h->prop_bot.p(); g.prop_nu = h->prop_nu; g.prop_u0 = h->prop_u0; g.prop_du = h->prop_du; }
        if (h->batch.ins_gg_set && h->gg_n >= 1) {
            TRY(ensure(h, h->ins_ggsum, (size_t)(N + 1))); TRY(fg.zero(h->ins_ggsum.p(), N + 1));
            g.gg_inv = h->gg_inv.p(); g.gg_n = h->gg_n; g.gg_L = h->gg_L; g.ins_gg = h->ins_gg.p(); g.ins_ggw = h->ins_ggw.p(); g.ins_ggsum = h->ins_ggsum.p();
        }
    }
    // em_zg is NaN wherever k_s2_electrons did not store a gain: k_s2_photons alone reads it, and it runs only with any_ptrs
    TRY(ensure(h, h->em_zg, (size_t)E)); if (h->batch.any_ptrs) TRY(fg.ones(h->em_zg.p(), E)); g.em_zg = h->em_zg.p();
    // tile-local generation (wfs_tilegen.h): which instructions take it is decided before the electrons are drawn -- theirs get no
    // photon numbers.  Debug modes that need the per-photon arrays (currents, generation only) run the generation half alone.
    // (PMT afterpulses of tile-generated photons are screened inside k_s2_tile)
    h->run.fuse_on = h->cfg.tile_gen && !h->generic_geom && h->batch.any_s2 && d.gain_spread == 0.0 && (!h->batch.run_sets_given || h->batch.sets_aligned) && h->batch.n_diff_rows == 0;
    h->run.fuse_full = h->run.fuse_on && !(h->debug_bits & (DBG_CURRENTS | DBG_GEN_ONLY));
    if (h->run.fuse_on) {
        f.lam_min = h->cfg.tile_gen_min; f.n_ins = N; f.nch = d.n_tpc; f.table_span = (i32)(1u << (32 - d.tab_s2.shift));
        f.set_ins_off = h->batch.run_sets_given ? h->set_ins_off.p() : nullptr;
        f.n_top = d.n_top;
        if (ext) {       // timing-model variants: the instruction's tables (the longest one bounds every tile buffer)
            f.tabs = g.tabs; f.ins_tab = g.ins_tab; f.ins_tabb = g.ins_tabb; f.ins_gg = g.gg_inv ? g.ins_gg : nullptr;
            for (const AliasTab &t : h->h_tabs) if (t.cell) f.table_span = std::max(f.table_span, (i32)(1u << (32 - t.shift)));
        }
        f.ins_type = g.ins_type; f.ins_amp = g.ins_amp; f.ins_sc = g.ins_sc; f.ins_embase = g.ins_embase; f.ins_gid = g.ins_gid; f.ins_cdfrow = g.ins_cdfrow;
        f.cdf_table = g.cdf_table; f.ins_time = g.ins_time; f.em_off = g.em_off; f.em_time = g.em_time; f.el_minmax = g.el_minmax; f.scal = g.scal;
        TRY(ensure(h, h->ins_fused, (size_t)N)); TRY(ensure(h, h->ins_nsurv, (size_t)N)); TRY(ensure(h, h->ins_bcap, (size_t)N));
        TRY(ensure(h, h->ins_bcap_all, (size_t)N)); TRY(ensure(h, h->et32, (size_t)E));
        TRY(fg.zero(h->ins_bcap.p(), N)); TRY(fg.zero(h->ins_bcap_all.p(), N));
        f.ins_fused = h->ins_fused.p(); f.ins_nsurv = h->ins_nsurv.p(); f.ins_bcap = h->ins_bcap.p(); f.ins_bcap_all = h->ins_bcap_all.p();
        f.et32 = h->et32.p();
        {
            const i64 n_rows = h->batch.n_host_rows + (i64)h->batch.dev_row_ins.size();
            TRY(ensure(h, h->row_pmax, (size_t)n_rows)); f.row_pmax = h->row_pmax.p();
            TRY(fg.flush());
            Timer t(h, "k_fuse_decide");
            TRY(launch_untimed(h, PLAIN(k_row_pmax), per_wave(n_rows), f.cdf_table, d.n_tpc, n_rows, h->row_pmax.p()));
            TRY(launch_untimed(h, PLAIN(k_fuse_decide), per_thread(N), f));
        }
        g.ins_fused = f.ins_fused;
    }
    TRY(fg.flush());
    TRY(launch(h, PLAIN(k_s1_hits), per_wave(N), d, g));
    {
        const i64 neb = (E + 255) / 256;
        TRY(ensure(h, h->eblk_ins, (size_t)(neb + 1))); g.eblk_ins = h->eblk_ins.p();
        TRY(launch(h, PLAIN(k_emitter_blocks), per_thread(neb + 1), g, neb));
        TRY(ensure(h, h->pois_cdf, (size_t)N * POIS_W)); TRY(ensure(h, h->pois_kmin, (size_t)N));
        g.pois_cdf = h->pois_cdf.p(); g.pois_kmin = h->pois_kmin.p();
        TRY(launch(h, PLAIN(k_poisson_tables), per_group(N, POIS_W), g, h->pois_cdf.p(), h->pois_kmin.p()));
        TRY(launch(h, PLAIN(k_s2_electrons), per_thread(E), d, g));
        if (h->batch.any_ptrs) TRY(launch(h, PLAIN(k_s2_photons), per_thread(E), d, g));
    }
    if (h->batch.n_diff_rows > 0) {
        // transverse diffusion maps: the pattern of these instructions is the average over their surviving electrons (s2.py:560-613)
        const auto &pm = h->pmap[1];
        const i64 nr = h->batch.n_diff_rows;
        TRY(ensure(h, h->diff_pre, (size_t)nr * pm.n_map_ch));
        MapArgs m{};
        map_args(pm, m);
        m.n_rows = nr; m.row_ins = h->diff_row_ins.p(); m.row_id = h->diff_row_id.p();
        m.x = h->map_x.p(); m.y = h->map_y.p(); m.z = h->map_z.p();
        m.cdf_table = h->cdf_table.p(); m.gains = h->t_gains.p();
        m.aft = h->batch.ins_aft_set ? h->ins_aft.p() : nullptr; m.n_top = h->cfg.n_top;
        DiffArgs q{nr, m.row_ins, h->ins_sigr.p(), h->ins_siga.p(), h->batch.diff_r2, h->diff_pre.p()};
        TRY(launch(h, PLAIN(k_diffuse_patterns), per_group(nr), d, g, m, q));
        m.pre = h->diff_pre.p();
        TRY(launch(h, PLAIN(k_map_rows), per_group(nr, 256, (size_t)map_rows_lds(d.n_tpc).total), m, d.n_tpc));
    }
    const i64 TP = r.TP = h->batch.n_psets * d.n_tpc;
    TRY(ensure(h, h->tile_count, (size_t)T)); TRY(ensure(h, h->tile_cursor, (size_t)T));
    TRY(ensure(h, h->tile_tmin, (size_t)T)); TRY(ensure(h, h->tile_tmax, (size_t)T));
    {
        FillGroup ft(h, "fills_tiles");
        TRY(ft.zero(h->tile_count.p(), T)); TRY(ft.zero(h->tile_cursor.p(), T));
        TRY(ft.fill(h->tile_tmin.p(), T, 0x7fffffff)); TRY(ft.fill(h->tile_tmax.p(), T, (i32)0x80000000));
        TRY(ft.flush());
    }
    TRY(ensure(h, h->tile_off, (size_t)(T + 1)));
    if (h->run.fuse_on) {
        // surviving electrons compacted per instruction, tile buffers sized from their time range, photons per tile (Poisson)
        TRY(launch(h, PLAIN(k_fuse_electrons), per_group(N), d, f));
        TRY(scan(h, h->ins_bcap_all.p(), N, h->ins_boff, &WfsScal::n_tbuf_samples));
        // (the work list: TP entries for the tiles of k_s2_tile, from the front and from the back, and TP more for those of k_s2_bright)
        TRY(ensure(h, h->ftiles, (size_t)2 * TP)); TRY(ensure(h, h->tile_done, (size_t)TP)); TRY(ensure(h, h->tile_kind, (size_t)TP));
        f.ins_boff = h->ins_boff.p(); f.tile_count = h->tile_count.p(); f.tiles = h->ftiles.p();
        f.tile_done = h->tile_done.p(); f.full = h->run.fuse_full ? 1 : 0; f.n_list = TP;
        BrightArgs &b = h->bright_args;
        b.on = (h->run.fuse_full && h->bright_on && h->bright_max_bins > 0) ? 1 : 0; b.lds_bytes = h->bright_lds; b.max_bins = h->bright_max_bins; b.pad = 0;
        b.list_first = TP; b.tile_kind = h->tile_kind.p();
        TRY(launch(h, PLAIN(k_tile_counts), per_thread(TP), d, f, b));
    }
    TRY(scan(h, h->em_nph.p(), E, h->em_ph_off, &WfsScal::n_block_photons));
    TRY(read_scal(h));
    const WfsScal &sc = *h->h_scal;
    r.P = sc.n_block_photons;                   // the tiles' own photons come on top
    if (h->run.fuse_on) { h->run.p_fused = sc.n_tilegen_photons; h->run.n_fused_tiles = sc.n_full_tiles; h->run.n_gen_tiles = sc.n_gen_tiles; h->run.n_bright_tiles = sc.n_bright_tiles; }
    if (h->run.fuse_on && getenv("WFS_BRIGHT_STATS")) {
        fprintf(stderr, "bright tiles: %lld by k_s2_bright, %lld generation only, %lld of up to %d photons; widest H table of a tile above that: %lld start bins (budget %d bins, %d bytes)\n",
                (long long)h->run.n_bright_tiles, (long long)h->run.n_gen_tiles, (long long)h->run.n_fused_tiles, TILE_MAX_PHOTONS, (long long)sc.max_bright_bins, h->bright_max_bins, h->bright_lds);
    }
    h->run.n_gen_photons = r.P + h->run.p_fused;
    return WFS_OK;
}

// the afterpulse kernels' arguments: element tables, acceptance probabilities, screening thresholds of the current modifier and the
// candidate / photon lists of ap_cap entries (ph_gain: the explicit gains of the afterpulse photons, which follow the primary ones)
static int fill_ap_args(wfs_handle *h, ApArgs &ap, i64 ap_cap)
{
    const WfsDev &d = h->dev;
    ap.n = d.n_ap;
    for (int e = 0; e < d.n_ap; e++) {
        const ApElem &s = h->ap[e];
        ap.el[e] = ApElemDev{s.n_bins_delay, s.n_bins_amp, s.amp_2d, s.is_uniform, s.delay_bin, s.amp_bin, s.delay_cdf.p(), s.amp_cdf.p(),
                             s.delay_sorted, s.amp_sorted, s.delay_guide.p(), s.amp_guide.p()};
        ap.prob[e] = s.prob.p();
        ApElem &sm = h->ap[e];
        if (sm.thr_mod != d.pmt_ap_modifier || !sm.thr.p()) {           // screening thresholds of the generator (ap_threshold), once per modifier
            std::vector<u32> th(sm.prob_h.size() * 2);
            for (size_t c = 0; c < sm.prob_h.size(); c++) for (int dpe = 0; dpe < 2; dpe++) th[2 * c + dpe] = ap_threshold(sm.prob_h[c], d.pmt_ap_modifier, dpe != 0);
            TRY(upload(h, sm.thr, th.data(), th.size()));
            HIPCHK(hipStreamSynchronize(h->stream));
            sm.thr_mod = d.pmt_ap_modifier;
        }
        ap.thr[e] = sm.thr.p();
    }
    TRY(ensure(h, h->ap_ins, (size_t)ap_cap)); TRY(ensure(h, h->ap_ch, (size_t)ap_cap)); TRY(ensure(h, h->ap_t, (size_t)ap_cap));
    TRY(ensure(h, h->ap_gain, (size_t)ap_cap)); TRY(ensure(h, h->ph_gain, (size_t)ap_cap)); TRY(ensure(h, h->ap_key, (size_t)ap_cap));
    ap.ap_key = h->ap_key.p();
    ap.cap = ap_cap; ap.ap_ins = h->ap_ins.p(); ap.ap_ch = h->ap_ch.p(); ap.ap_t = h->ap_t.p(); ap.ap_gain = h->ap_gain.p();
    ap.count = &h->scal.p()->n_ap_candidates;
    TRY(ensure(h, h->ap_cand, (size_t)ap_cap)); ap.cand = h->ap_cand.p();
    return WFS_OK;
}

// ---- generation 2: the photons of the block generator, bucketed by tile
static int gen_block_photons(wfs_handle *h, GenRun &r)
{
    const WfsDev &d = h->dev;
    GenArgs &g = r.g; ApArgs &ap = r.ap;
    const i64 N = h->batch.n_ins, P = r.P, TP = r.TP;
    const bool ext = r.ext;
    g.em_ph_off = h->em_ph_off.p(); g.n_photons = P;
    const bool ap_on = r.ap_on = h->batch.ap_sets;
    const i64 ap_cap = r.ap_cap = ap_on ? (P + h->run.p_fused) / 8 + 65536 : 0;
    TRY(ensure(h, h->ph, (size_t)(P + h->run.p_fused + ap_cap)));
    TRY(ensure(h, h->ph_idx, (size_t)(P + h->run.p_fused + ap_cap))); g.ph_idx = h->ph_idx.p();
    g.tile_count = h->tile_count.p(); g.tile_cursor = h->tile_cursor.p(); g.tile_tmin = h->tile_tmin.p();
    g.tile_tmax = h->tile_tmax.p(); g.ph = h->ph.p();
    g.tile_off = h->tile_off.p();
    if (ap_on) TRY(fill_ap_args(h, ap, ap_cap));
    TRY(ensure(h, h->ins_ph0, (size_t)(N + 1))); g.ins_ph0 = h->ins_ph0.p();
    TRY(launch(h, PLAIN(k_ins_ph0), per_thread(N + 1), g));
    TRY(ensure(h, h->ins_sbase, (size_t)N)); g.ins_sbase = h->ins_sbase.p();
    TRY(ensure(h, h->ins_fullsort, (size_t)N)); g.ins_fullsort = h->ins_fullsort.p();
    TRY(ensure(h, h->tile_tail, (size_t)TP)); TRY(ensure(h, h->tile_tailbase, (size_t)TP));
    {
        FillGroup fg(h, "fills_block_photons");
        TRY(fg.zero(h->tile_tail.p(), TP)); TRY(fg.zero(h->tile_tailbase.p(), TP));
        TRY(fg.flush());
    }
    g.tile_tail = h->tile_tail.p(); g.tile_tailbase = h->tile_tailbase.p();
    TRY(launch(h, PLAIN(k_set_bases), per_thread(h->batch.n_psets), g));
    if (P > 0) {
        const unsigned nb = (unsigned)((P + GEN_BLOCK - 1) / GEN_BLOCK);
        g.n_blocks = nb;
        TRY(ensure(h, h->blk_e, (size_t)nb * MINMAX)); TRY(ensure(h, h->blk_base, (size_t)nb * d.n_tpc)); TRY(ensure(h, h->blk_cnt, (size_t)nb * d.n_tpc)); TRY(ensure(h, h->blk_ins, (size_t)nb));
        g.blk_e = h->blk_e.p(); g.blk_base = h->blk_base.p(); g.blk_cnt = h->blk_cnt.p(); g.blk_ins = h->blk_ins.p();
        TRY(ensure(h, h->blk_desc, (size_t)nb)); g.blk_desc = h->blk_desc.p();
        TRY(launch(h, PLAIN(k_block_emitters), per_thread(nb), g));
        // XCD x (workgroup id % 8) walks the photon blocks [x * chunk, (x + 1) * chunk) in order: the blocks that share
        // cache lines of a tile (consecutive ranges, k_block_ranges) run close together in time on the same L2
        g.xcd_chunk = (nb + 7) / 8;
        const unsigned nbx = (unsigned)(g.xcd_chunk * 8);
        {   // alias cells of every channel CDF row (host rows + rows from the device maps, the electron-averaged ones included)
            const i64 n_rows = h->batch.n_host_rows + (i64)h->batch.dev_row_ins.size();
            int lg = 1; while ((1 << lg) < d.n_tpc) lg++;
            TRY(ensure(h, h->chan_alias, (size_t)n_rows << lg));
            g.chan_alias = h->chan_alias.p(); g.ch_lg = lg;
            TRY(launch(h, PLAIN(k_chan_alias), per_group(n_rows, 64), g.cdf_table, d.n_tpc, lg, h->chan_alias.p()));
        }
        if (g.gg_inv) TRY(launch(h, PLAIN(k_gg_sum), Shape(dim3(nb), dim3(256)), d, g));
        TRY(launch(h, PLAIN(k_photon_count), Shape(dim3(nbx), dim3(COUNT_TPB), (size_t)count_lds(d.n_tpc, g.ch_lg).total), d, g));
        TRY(launch(h, PLAIN(k_block_ranges), per_thread(TP), d, g));
        TRY(scan_into(h, h->tile_count.p(), TP, h->tile_off.p(), &WfsScal::n_tile_photons, 0));
        const size_t gen_lds = (size_t)gen_fill_lds(d.n_tpc, g.ch_lg, ap_on).total;
        TRY(launch(h, K_PHOTON_FILL(ap_on, ext), Shape(dim3(nbx), dim3(FILL_TPB), gen_lds), d, g, ap));
    } else {
        TRY(scan_into(h, h->tile_count.p(), TP, h->tile_off.p(), &WfsScal::n_tile_photons, 0));
    }
    return WFS_OK;
}

// ---- generation 3: the tiles that make their own photons (k_s2_tile) -- before the geometry: the tile time ranges come out of this kernel
static int gen_tile_photons(wfs_handle *h, GenRun &r)
{
    const WfsDev &d = h->dev;
    FuseArgs &f = r.f; ApArgs &ap = r.ap;
    const i64 T = h->batch.n_tiles, TP = r.TP;
    const bool ap_on = r.ap_on;
    // (photon counts only -- wfs_set_debug bit 2 without bit 4, the electron-afterpulse pre-pass: the tiles' photon numbers are drawn
    // (k_tile_counts) and single photons are recomputed on request (wfs_gather_photon_times); no photon of a tile is generated)
    const bool counts_only = (h->debug_bits & DBG_GEN_ONLY) && !(h->debug_bits & DBG_KEEP_PHOTONS);
    if (h->run.fuse_on && n_tilegen_tiles(h) > 0 && !counts_only) {
        TRY(pack_fence(h));         // the tile buffers: the first write of a run to what the previous batch's packers read
        TRY(ensure(h, h->tbuf, (size_t)h->h_scal->n_tbuf_samples + 16));
        TRY(ensure(h, h->tile_truth, (size_t)T * TRUTH_PER_TILE));
        f.tile_off = h->tile_off.p(); f.tile_tmin = h->tile_tmin.p(); f.tile_tmax = h->tile_tmax.p(); f.tile_truth = h->tile_truth.p();
        f.tbuf = h->tbuf.p(); f.ph = h->ph.p(); f.keep_ph = (h->debug_bits & DBG_KEEP_PHOTONS) ? 1 : 0;
        const TemplateArg tp = fill_template_arg(h);
        const bool fma = h->cfg.fma != 0;
        const size_t lds = (size_t)tile_lds(fma, ap_on).total;
        const ApArgs *app = nullptr;
        if (ap_on) {
            TRY(ensure(h, h->ap_seg, (size_t)n_tilegen_tiles(h))); ap.seg = h->ap_seg.p(); ap.n_seg = n_tilegen_tiles(h);      // (one segment per tile of every class)
            f.n_ptiles = TP;
            TRY(upload(h, h->ap_args_dev, &ap, 1)); app = h->ap_args_dev.p();      // (`ap` outlives the copy: read_scal of gen_afterpulses)
        }
        f.sparse_max = h->tap_sparse_max;
        // tiles of up to 2048 photons: photons and pulse in one workgroup (listed from the front); brighter ones -- and every tile in the
        // debug modes -- generation only (listed from the back), their pulses are made by the ordinary kernels below
        if (h->run.n_fused_tiles > 0) {
            TRY(launch(h, K_S2_TILE(ap_on, fma), per_group(h->run.n_fused_tiles, 256, lds), d, f, tp, app));
        }
        if (h->run.n_gen_tiles > 0) {
            TRY(launch(h, K_S2_TILE_GEN(ap_on), per_group(h->run.n_gen_tiles, 256, (size_t)tile_gen_lds(ap_on).total), d, f, app, (int)h->run.n_fused_tiles));
        }
        // tiles above 2048 photons whose H table fits the LDS as a whole: photons and pulse in one workgroup of 1024 threads, no photon array
        if (h->run.n_bright_tiles > 0) {
            const size_t blds = (size_t)bright_lds_layout(h->bright_lds, ap_on).total;
            const int seg_first = (int)(h->run.n_fused_tiles + h->run.n_gen_tiles);
            TRY(launch(h, K_S2_BRIGHT(ap_on, fma), per_group(h->run.n_bright_tiles, BRIGHT_TPB, blds), d, f, h->bright_args, tp, app, seg_first));
        }
    }
    h->fuse_args = f;
    return WFS_OK;
}

// ---- generation 4: PMT afterpulse photons: count per tile of the afterpulse sets, offsets behind the primary photons, place
static int gen_afterpulses(wfs_handle *h, GenRun &r)
{
    const WfsDev &d = h->dev;
    const GenArgs &g = r.g; const ApArgs &ap = r.ap;
    const i64 P = r.P, TP = r.TP, ap_cap = r.ap_cap;
    TRY(launch(h, PLAIN(k_ap_finish), per_thread(ap_cap), d, g, ap));
    { Timer t(h, "k_ap_count"); TRY(launch_untimed(h, PLAIN(k_ap_count), per_thread(ap_cap), d, g, ap));
      if (ap.n_seg > 0) TRY(launch_untimed(h, K_AP_SEG(false), per_wave(ap.n_seg), d, g, ap, (double *)nullptr)); }
    TRY(scan_into(h, h->tile_count.p() + TP, TP, h->tile_off.p() + TP, &WfsScal::n_ap_photons, P + h->run.p_fused));      // (behind the slots of every primary tile, the tile-generated ones included)
    { Timer t(h, "k_ap_place"); TRY(launch_untimed(h, PLAIN(k_ap_place), per_thread(ap_cap), d, g, ap, h->ph_gain.p() - (P + h->run.p_fused)));
      if (ap.n_seg > 0) TRY(launch_untimed(h, K_AP_SEG(true), per_wave(ap.n_seg), d, g, ap, h->ph_gain.p() - (P + h->run.p_fused))); }
    TRY(read_scal(h));
    if (h->h_scal->n_ap_candidates > ap_cap) return h->fail(WFS_E_CAPACITY, "more PMT afterpulse photons than 1/8 of the primary photons: afterpulse probability unreasonably high");
    h->run.n_ap_photons = h->h_scal->n_ap_photons;                   // (the accepted candidates: total of the afterpulse tiles' counts, the scan above)
    return WFS_OK;
}

// the order pass over the tiles oa describes: scan, then every listed range by the kernel of its class
static int order_ranges(wfs_handle *h, const OrderArgs &oa)
{
    const i64 T = oa.n_tiles;
    TRY(launch(h, PLAIN(k_tile_order_scan), per_thread(T), oa));
    TRY(read_scal(h));
    const i64 n_wave = h->h_scal->n_order_wave, n_big = h->h_scal->n_order_big;
    if (n_wave > 0) TRY(launch(h, PLAIN(k_tile_order), per_wave(n_wave), oa, n_wave));
    if (n_big > 0) {
        TRY(launch(h, K_TILE_ORDER_BIG(0), per_group(n_big, 256, (size_t)order_lds(TILE_ORDER_MAX).total), oa));
    }
    const i64 n_huge = h->h_scal->n_order_huge;
    if (n_huge > 0) {
        // ranges beyond the workgroup sort: compact copies, one segmented radix sort over (order key, position), records to their ranks
        std::vector<OrderRange> rg((size_t)n_huge);
        TRY(copy_out(h, rg.data(), oa.big_list + (2 * T - n_huge), (size_t)n_huge));
        std::sort(rg.begin(), rg.end(), [](const OrderRange &x, const OrderRange &y) { return x.start < y.start; });      // (appended with atomics: a fixed order for the offsets)
        std::vector<i64> start((size_t)n_huge), cbeg((size_t)n_huge + 1, 0);
        for (i64 k = 0; k < n_huge; k++) { start[(size_t)k] = rg[(size_t)k].start; cbeg[(size_t)k + 1] = cbeg[(size_t)k] + rg[(size_t)k].n; }
        const i64 tot = cbeg[(size_t)n_huge];
        if (tot > 0xffffffffLL) return h->fail(WFS_E_CAPACITY, "more than 2^32 photons in tiles beyond 4096 photons");
        TRY(upload(h, h->huge_start, start.data(), start.size())); TRY(upload(h, h->huge_cbeg, cbeg.data(), cbeg.size()));
        TRY(ensure(h, h->huge_keys, (size_t)tot)); TRY(ensure(h, h->huge_keys2, (size_t)tot)); TRY(ensure(h, h->huge_vals, (size_t)tot)); TRY(ensure(h, h->huge_vals2, (size_t)tot));
        TRY(ensure(h, h->huge_rec, (size_t)tot)); TRY(ensure(h, h->huge_gain, (size_t)tot));
        HugeOrderArgs ha{n_huge, tot, h->huge_start.p(), h->huge_cbeg.p(), oa.ph, oa.ph_idx, oa.ph_gain, oa.gain_first,
                         h->huge_keys.p(), h->huge_vals.p(), h->huge_rec.p(), h->huge_gain.p()};
        Timer t(h, "k_tile_order_huge");
        TRY(launch_untimed(h, PLAIN(k_order_huge_pack), per_thread(tot), ha));
        TRY(two_step(h, "tile order sort", [&](void *tmp, size_t &bytes) {
            return rocprim::segmented_radix_sort_pairs(tmp, bytes, h->huge_keys.p(), h->huge_keys2.p(), h->huge_vals.p(), h->huge_vals2.p(),
                                                       (unsigned)tot, (unsigned)n_huge, h->huge_cbeg.p(), h->huge_cbeg.p() + 1, 0u, 32u, h->stream); }));
        TRY(launch_untimed(h, PLAIN(k_order_huge_apply), per_thread(tot), ha, h->huge_keys2.p(), h->huge_vals2.p(), h->ph.p(), h->ph_idx.p(), oa.ph_gain));
    }
    return WFS_OK;
}

// ---- generation 5: every tile of the block generator into generation order (k_tile_order): the order the reference's Pulse call sees
static int gen_order(wfs_handle *h, GenRun &r)
{
    const WfsDev &d = h->dev;
    const i64 T = h->batch.n_tiles, P = r.P, TP = r.TP;
    const bool ap_on = r.ap_on;
    TRY(ensure(h, h->order_list, (size_t)T * 2)); TRY(ensure(h, h->order_list2, (size_t)T * 2));
    OrderArgs oa{T, TP, h->tile_count.p(), h->tile_off.p(), h->ph.p(), h->ph_idx.p(),
                 ap_on ? h->ph_gain.p() : nullptr, P + h->run.p_fused, h->order_list.p(), h->order_list2.p(), h->scal.p(),
                 (h->run.fuse_on && n_tilegen_tiles(h) > 0) ? h->ins_fused.p() : nullptr, d.n_tpc,
                 h->tile_cursor.p(), h->tile_tailbase.p(), h->ins_fullsort.p(), h->set_ins_off.p(), h->set_ins_list.p()};
    return order_ranges(h, oa);
}

static int run_generation(wfs_handle *h, FillGroup &fg)
{
    GenRun r;
    TRY(gen_electrons(h, r, fg));
    TRY(gen_block_photons(h, r));
    TRY(gen_tile_photons(h, r));
    if (r.ap_on) TRY(gen_afterpulses(h, r));
    if (r.P > 0 || r.ap_on) TRY(gen_order(h, r));
    h->gen_args = r.g;
    return WFS_OK;
}

// What crosses the stage boundaries of one wfs_run (on its stack).
struct RunState {
    GeomArgs ga{}; PulseArgs pa{}; ZleArgs za{};
    bool tiles_done = false;                                // pulses made by k_s2_tile (wfs_tilegen.h)
    i64 CG = 0, RS = 0;                                     // group slots; row slots
    i64 first_sparse = 0, first_dense = 0, first_wave = 0;  // the one work list: tiny tiles, then sparse, dense, wave
    int noise_kind = 0;                                     // the nk axis of the row kernels' families
    bool dark = false;                                      // their dk axis: PMT dark counts are on
};

// ---- PMT afterpulses of an optical batch: the supplied photons are screened (k_optical_ap_screen), the candidates go through the
// generator's stages (gen_afterpulses) into the tiles of the afterpulse sets, and those tiles into generation order.  The primary
// tiles are in item order as k_optical_bucket wrote them and are on none of the lists the order pass reads for a generator batch:
// the pass is given the afterpulse tiles alone.
static int optical_afterpulses(wfs_handle *h)
{
    const WfsDev &d = h->dev;
    const i64 P = h->batch.n_photons, TP = h->batch.n_ins * d.n_tpc, ap_cap = optical_ap_cap(P);
    GenArgs g{}; ApArgs ap{};
    TRY(fill_ap_args(h, ap, ap_cap));
    TRY(ensure(h, h->ph_idx, (size_t)(P + ap_cap)));
    g.n_psets = h->batch.n_psets; g.tile_count = h->tile_count.p(); g.tile_cursor = h->tile_cursor.p(); g.tile_off = h->tile_off.p();
    g.tile_tmin = h->tile_tmin.p(); g.tile_tmax = h->tile_tmax.p(); g.ph = h->ph.p(); g.ph_idx = h->ph_idx.p();
    g.scal = h->scal.p();
    if (P > 0) {
        OptApArgs sa{P, TP, h->tile_off.p(), h->set_gid.p(), h->set_t0.p(), h->opt_item.p(), h->ph.p()};
        TRY(launch(h, PLAIN(k_optical_ap_screen), per_thread(P), d, sa, ap));
    }
    double *const gain_base = h->ph_gain.p() - P;
    TRY(launch(h, PLAIN(k_ap_finish), per_thread(ap_cap), d, g, ap));
    TRY(launch(h, PLAIN(k_ap_count), per_thread(ap_cap), d, g, ap));
    TRY(scan_into(h, h->tile_count.p() + TP, TP, h->tile_off.p() + TP, &WfsScal::n_ap_photons, P));
    TRY(launch(h, PLAIN(k_ap_place), per_thread(ap_cap), d, g, ap, gain_base));
    TRY(read_scal(h));
    if (h->h_scal->n_ap_candidates > ap_cap) return h->fail(WFS_E_CAPACITY, "more PMT afterpulse photons than 1/8 of the primary photons: afterpulse probability unreasonably high");
    h->run.n_ap_photons = h->h_scal->n_ap_photons;
    TRY(ensure(h, h->order_list, (size_t)TP * 2)); TRY(ensure(h, h->order_list2, (size_t)TP * 2));
    OrderArgs oa{TP, 0, h->tile_count.p() + TP, h->tile_off.p() + TP, h->ph.p(), h->ph_idx.p(), h->ph_gain.p(), P,
                 h->order_list.p(), h->order_list2.p(), h->scal.p(), nullptr, d.n_tpc, nullptr, nullptr, nullptr, nullptr, nullptr};
    return order_ranges(h, oa);
}

// ---- input: photons bucketed by tile, whichever way the batch was loaded
static int run_input(wfs_handle *h)
{
    const WfsDev &d = h->dev;
    // the scalar block is cleared with the first fills of the run: the generator's (gen_electrons), or alone
    FillGroup fg(h, from_generator(h) ? "fills_electrons" : "fills_input");
    TRY(fg.zero(h->scal.p(), 1));
    if (from_generator(h)) return run_generation(h, fg);
    const bool optical = h->batch.kind == BatchKind::Optical;
    if (optical && h->batch.ap_sets) {
        // the afterpulse tiles start every run empty (the primary tiles keep the counts and offsets of wfs_load_optical)
        const i64 TP = h->batch.n_ins * d.n_tpc;
        TRY(fg.zero(h->tile_count.p() + TP, TP)); TRY(fg.zero(h->tile_cursor.p() + TP, TP));
        TRY(fg.fill(h->tile_tmin.p() + TP, TP, 0x7fffffff)); TRY(fg.fill(h->tile_tmax.p() + TP, TP, (i32)0x80000000));
    }
    TRY(fg.flush());
    if (optical) {
        const i64 T = h->batch.n_ins * d.n_tpc;                    // the primary tiles (afterpulse tiles follow them)
        OpticalArgs oa{T, h->tile_count.p(), h->tile_off.p(), h->tile_tmin.p(), h->tile_tmax.p(), h->set_gid.p(),
                       h->opt_t.p(), h->opt_item.p(), h->ph.p(), h->scal.p()};
        TRY(launch(h, PLAIN(k_optical_finish), per_thread(T), d, oa));
        if (h->batch.ap_sets) TRY(optical_afterpulses(h));
    }
    else { TRY(scan(h, h->tile_count.p(), h->batch.n_tiles, h->tile_off, &WfsScal::n_tile_photons)); }
    return WFS_OK;
}

// ---- geometry: tiles -> clusters -> groups -> rows; the counters of the batch come back and size everything that follows
static int run_geometry(wfs_handle *h, RunState &r)
{
    const WfsDev &d = h->dev;
    GeomArgs &ga = r.ga;
    const i64 T = h->batch.n_tiles, S = h->batch.n_sets, C = h->batch.n_clusters;
    const i64 CG = r.CG = C + 1;
    FillGroup fg(h, "fills_geometry");
    TRY(ensure(h, h->cl_end, (size_t)C)); TRY(fg.fill(h->cl_end.p(), C, I64_MIN)); TRY(ensure(h, h->cl_group, (size_t)C));
    TRY(ensure(h, h->grp_lo, (size_t)CG)); TRY(ensure(h, h->grp_hi, (size_t)CG));
    TRY(fg.fill(h->grp_lo.p(), CG, I64_MAX)); TRY(fg.fill(h->grp_hi.p(), CG, I64_MIN));
    TRY(ensure(h, h->grp_left, (size_t)CG)); TRY(ensure(h, h->grp_right, (size_t)CG)); TRY(ensure(h, h->grp_ixrand, (size_t)CG));
    TRY(ensure(h, h->grp_gid, (size_t)CG)); TRY(fg.ones(h->grp_gid.p(), CG));
    TRY(ensure(h, h->row_lo, (size_t)CG * d.n_tpc)); TRY(ensure(h, h->row_hi, (size_t)CG * d.n_tpc));
    TRY(fg.fill(h->row_lo.p(), CG * d.n_tpc, I64_MAX)); TRY(fg.fill(h->row_hi.p(), CG * d.n_tpc, I64_MIN));
    TRY(ensure(h, h->acc_len, (size_t)CG * d.n_tpc)); TRY(fg.zero(h->acc_len.p(), CG * d.n_tpc));
    TRY(ensure(h, h->itv_cap, (size_t)CG * d.row_slots)); TRY(ensure(h, h->active_rows, (size_t)CG * d.row_slots));
    TRY(ensure(h, h->active_tiles, (size_t)T)); TRY(ensure(h, h->sparse_tiles, (size_t)T)); TRY(ensure(h, h->dense_tiles, (size_t)T)); TRY(ensure(h, h->wave_tiles, (size_t)T));
    ga.n_sets = S; ga.n_tiles = T; ga.n_clusters = C; ga.n_gslots = CG;
    ga.tile_count = h->tile_count.p(); ga.tile_tmin = h->tile_tmin.p(); ga.tile_tmax = h->tile_tmax.p();
    ga.set_cluster = h->set_cluster.p(); ga.set_t0 = h->set_t0.p(); ga.cl_tmin = h->cl_tmin.p(); ga.cl_gid = h->cl_gid.p();
    ga.cl_end = h->cl_end.p(); ga.cl_group = h->cl_group.p(); ga.grp_lo = h->grp_lo.p(); ga.grp_hi = h->grp_hi.p();
    ga.grp_left = h->grp_left.p(); ga.grp_right = h->grp_right.p(); ga.grp_ixrand = h->grp_ixrand.p(); ga.grp_gid = h->grp_gid.p();
    ga.row_lo = h->row_lo.p(); ga.row_hi = h->row_hi.p(); ga.acc_len = h->acc_len.p(); ga.itv_cap = h->itv_cap.p();
    ga.active_rows = h->active_rows.p(); ga.scal = h->scal.p(); ga.active_tiles = h->active_tiles.p(); ga.sparse_tiles = h->sparse_tiles.p(); ga.dense_tiles = h->dense_tiles.p(); ga.wave_tiles = h->wave_tiles.p(); ga.force_dense = ((h->debug_bits & DBG_FORCE_DENSE) || h->generic_geom) ? 1 : 0; ga.init_has = h->carry_has; ga.init_runmax = h->carry_runmax;
    ga.noise_override = h->n_noise_override ? h->noise_override.p() : nullptr; ga.n_noise_override = h->n_noise_override;
    if (d.sum_channel >= 0) {
        TRY(ensure(h, h->sum_lo, (size_t)CG)); TRY(ensure(h, h->sum_hi, (size_t)CG));
        TRY(fg.fill(h->sum_lo.p(), CG, I64_MAX)); TRY(fg.fill(h->sum_hi.p(), CG, I64_MIN));
        TRY(ensure(h, h->sum_len, (size_t)CG)); TRY(ensure(h, h->sum_nchunk, (size_t)CG));
        TRY(fg.zero(h->sum_len.p(), CG)); TRY(fg.zero(h->sum_nchunk.p(), CG));
        ga.sum_lo = h->sum_lo.p(); ga.sum_hi = h->sum_hi.p(); ga.sum_len = h->sum_len.p(); ga.sum_nchunk = h->sum_nchunk.p();
    }
    if (d.full_readout) {
        TRY(ensure(h, h->fr_len, (size_t)CG * d.row_slots)); TRY(ensure(h, h->empty_rows, (size_t)CG * d.row_slots));
        TRY(fg.zero(h->fr_len.p(), CG * d.row_slots));
        ga.fr_len = h->fr_len.p(); ga.empty_rows = h->empty_rows.p();
    }
    const bool tiles_done = r.tiles_done = tiles_made(h);
    // resident rows (k_row_pulse): the usual digitiser geometry, a hold-off of at least a chunk and a noise table the fast row loads
    // can walk (as the fast path of k_zle), no HE rows, no debug copies of currents or rows
    // 2 (auto, the default): on when the batch holds at least two photons per (pulse set, channel) slot -- rows that collect several
    // pulses are where the accumulators cost (memset, atomics, two more reads); a batch of sparse S1 or nVeto hits is as fast through
    // them, and the resident path's extra pass over the tiles does not pay there
    // (photons in the photon array: the tiles k_s2_tile made in one go hold theirs in their sample buffers and can never be resident)
    const i64 p_all = n_primary_photons(h) - (h->run.fuse_full ? h->run.p_fused : 0) + h->run.n_ap_photons;
    const bool res_auto = T > 0 && p_all >= 2 * T;
    const int res_mode = h->res_env >= 0 ? h->res_env : h->cfg.row_resident;
    h->run.res_on = (res_mode == 2 ? res_auto : res_mode != 0) && !(h->debug_bits & (DBG_CURRENTS | DBG_FORCE_DENSE)) && !h->generic_geom && !d.he_rows && zle_holdoff(d.tw) >= ZLE_FAST_HOLD
                && (!d.enable_noise || d.nm_cells || d.noise_len >= NOISE_MIN_FAST);
    if (tiles_done || h->run.res_on) {
        TRY(ensure(h, h->row_cnt, (size_t)CG * d.n_tpc)); TRY(ensure(h, h->row_tile, (size_t)CG * d.n_tpc));
        TRY(fg.zero(h->row_cnt.p(), CG * d.n_tpc));
        ga.row_cnt = h->row_cnt.p(); ga.row_tile = h->row_tile.p();
    }
    if (tiles_done) {
        ga.tile_done = h->tile_done.p(); ga.n_done = h->batch.n_psets * d.n_tpc;
        ga.ins_bcap = h->ins_bcap.p(); ga.ins_boff = h->ins_boff.p();
    }
    if (h->run.res_on) {
        const size_t nr = (size_t)CG * d.n_tpc;
        TRY(ensure(h, h->row_bad, nr)); TRY(ensure(h, h->fin_len, nr)); TRY(ensure(h, h->res_cnt, nr));
        TRY(fg.zero(h->row_bad.p(), nr)); TRY(fg.zero(h->fin_len.p(), nr)); TRY(fg.zero(h->res_cnt.p(), nr));
        ga.res_on = 1; ga.res_max_len = h->res_max_len; ga.row_bad = h->row_bad.p(); ga.fin_len = h->fin_len.p(); ga.res_cnt = h->res_cnt.p();
        ga.rows_cap = CG * d.row_slots;
        TRY(ensure(h, h->res_long, nr)); ga.res_long = h->res_long.p();
    }
    TRY(fg.flush());
    TRY(launch(h, PLAIN(k_tile_geom), per_thread(T, 1024), d, ga));
    TRY(launch(h, PLAIN(k_groups), Shape(dim3(1), dim3(GROUPS_TPB)), d, ga));
    TRY(launch(h, PLAIN(k_tile_rows), per_thread(T), d, ga));
    TRY(launch(h, PLAIN(k_group_final), per_thread(CG), d, ga));
    if (d.full_readout) TRY(launch(h, PLAIN(k_rows_widen), per_thread(CG * d.n_tpc), d, ga));
    TRY(launch(h, PLAIN(k_row_len), per_thread(CG * d.row_slots, 1024), d, ga));
    TRY(scan(h, h->acc_len.p(), CG * d.n_tpc, h->acc_off, &WfsScal::n_acc_samples));
    TRY(scan(h, h->itv_cap.p(), CG * d.row_slots, h->itv_off, &WfsScal::n_itv_slots));
    if (d.sum_channel >= 0) {
        TRY(scan(h, h->sum_len.p(), CG, h->sum_off, &WfsScal::n_sum_samples));
        TRY(scan(h, h->sum_nchunk.p(), CG, h->sum_chunk_off, &WfsScal::n_sum_chunks));
    }
    if (d.full_readout) TRY(scan(h, h->fr_len.p(), CG * d.row_slots, h->fr_off, &WfsScal::n_empty_samples));
    if (h->run.res_on) {
        TRY(scan(h, h->fin_len.p(), CG * d.n_tpc, h->fin_off, &WfsScal::n_fin_samples)); TRY(scan(h, h->res_cnt.p(), CG * d.n_tpc, h->res_toff, &WfsScal::n_res_tiles));
        // rows are known: tiles onto their row's list or the work list of their class.  res_desc holds a descriptor slot for EVERY
        // tile of the batch (T * sizeof(TileDesc) bytes) although only the resident ones are written: their number (n_res_tiles) is
        // still on the device here, and sizing from it would cost one more host round trip before k_tile_assign
        TRY(ensure(h, h->res_desc, (size_t)std::max<i64>(T, 1)));
        ga.res_toff = h->res_toff.p(); ga.res_desc = h->res_desc.p();
        DescArgs da{}; da.tile_off = h->tile_off.p(); da.set_mode = h->set_mode.p();
        TRY(ensure(h, h->tile_truth, (size_t)T * TRUTH_PER_TILE));
        PulseArgs pt{}; pt.ph = h->ph.p(); pt.tile_truth = h->tile_truth.p();
        pt.ph_gain = ph_gain_base(h);
        TRY(launch(h, PLAIN(k_tile_assign), per_thread(T), d, ga, da, pt));
    }
    TRY(read_scal(h));
    const WfsScal &sc = *h->h_scal;
    TRY(device_error(h, sc.error));
    h->run.n_groups = sc.n_groups;
    h->run.n_front_rows = sc.n_front_rows;
    h->run.n_short_rows = h->run.res_on ? sc.n_short_rows : 0;
    h->run.n_res_rows = h->run.res_on ? sc.n_short_rows + sc.n_long_rows : 0;
    h->run.n_active_rows = h->run.n_front_rows + h->run.n_res_rows + n_empty_rows(h);
    // full readout sizes its buffers from groups x row slots x window length: a batch beyond the cap ends here, before any of them is asked for
    if (s_empty(h) > h->full_max_samples)
        return h->fail(WFS_E_CAPACITY, "full readout: " + std::to_string(n_empty_rows(h)) + " rows without a pulse need " + std::to_string(s_empty(h)) + " finished samples, more than the "
                       + std::to_string(h->full_max_samples) + " of one batch (WFS_FULL_READOUT_MAX_SAMPLES): load fewer windows per batch");
    h->run.max_res_len = sc.max_res_len;
    h->run.s_fin = h->run.res_on ? sc.n_fin_samples : 0;
    h->run.n_res_tiles = h->run.res_on ? sc.n_res_tiles : 0;
    h->run.s_res = h->run.res_on ? sc.n_res_samples : 0;
    h->run.n_tiny_tiles = sc.n_tiny_tiles;
    h->run.n_sparse_tiles = sc.n_sparse_tiles; h->run.max_nb = sc.max_nb_sparse; h->run.max_tile = sc.max_ph_sparse;
    h->run.n_dense_tiles = sc.n_dense_tiles; h->run.max_nb_dense = sc.max_nb_dense; h->run.max_tile_dense = sc.max_ph_dense;
    h->run.n_wave_tiles = sc.n_wave_tiles;
    h->run.n_active_tiles = h->run.n_tiny_tiles + h->run.n_sparse_tiles + h->run.n_dense_tiles + h->run.n_wave_tiles;
    r.first_sparse = h->run.n_tiny_tiles; r.first_dense = r.first_sparse + h->run.n_sparse_tiles; r.first_wave = r.first_dense + h->run.n_dense_tiles;
    h->run.s_raw = sc.n_acc_samples; h->run.n_itv_slots = sc.n_itv_slots;
    h->run.s_sum = d.sum_channel >= 0 ? sc.n_sum_samples : 0; h->run.n_sum_chunks = d.sum_channel >= 0 ? sc.n_sum_chunks : 0;
    h->run.sum_base = (h->run.s_raw + 3) & ~(i64)3;
    h->run.s_raw_direct = tiles_done ? sc.n_direct_samples : 0;      // samples of the rows that are read from a tile buffer in place
    if (h->run.res_on && getenv("WFS_RES_STATS")) {
        fprintf(stderr, "resident rows: %lld short + %lld long of %lld rows, %lld tiles of %lld listed + resident, longest %lld samples, %lld finished samples, accumulators %lld samples\n",
                (long long)h->run.n_short_rows, (long long)(h->run.n_res_rows - h->run.n_short_rows), (long long)h->run.n_active_rows, (long long)h->run.n_res_tiles,
                (long long)(h->run.n_res_tiles + h->run.n_active_tiles), (long long)h->run.max_res_len, (long long)h->run.s_fin, (long long)h->run.s_raw);
    }
    // one work list: the sparse, dense and wave tiles behind the tiny ones
    if (h->run.n_sparse_tiles > 0) TRY(copy_async(h, h->active_tiles.p() + r.first_sparse, h->sparse_tiles.p(), (size_t)h->run.n_sparse_tiles, hipMemcpyDeviceToDevice));
    if (h->run.n_dense_tiles > 0) TRY(copy_async(h, h->active_tiles.p() + r.first_dense, h->dense_tiles.p(), (size_t)h->run.n_dense_tiles, hipMemcpyDeviceToDevice));
    if (h->run.n_wave_tiles > 0) TRY(copy_async(h, h->active_tiles.p() + r.first_wave, h->wave_tiles.p(), (size_t)h->run.n_wave_tiles, hipMemcpyDeviceToDevice));
    return WFS_OK;
}

// ---- pulses: every listed tile into its row's accumulators, by the kernel of its class
static int run_pulses(wfs_handle *h, RunState &r)
{
    const WfsDev &d = h->dev;
    PulseArgs &pa = r.pa;
    const i64 T = h->batch.n_tiles, S = h->batch.n_sets;
    const bool fma = h->cfg.fma != 0;
    TRY(pack_fence(h));             // the accumulators are the first such write of a run without tile buffers (with them: gen_tile_photons)
    // (+16 samples, 64 bytes: a lane of k_zle reads 4 samples from its first valid one; the sum rows behind the accumulators are written whole by k_sum_signal)
    TRY(ensure_rows(h, h->raw, (size_t)(h->run.s_sum > 0 ? h->run.sum_base + h->run.s_sum : h->run.s_raw) + 16, "the row accumulators"));
    TRY(ensure(h, h->truth, (size_t)S * TRUTH_PER_SET));
    {
        FillGroup fg(h, "fills_pulses");
        TRY(fg.zero(h->raw.p(), h->run.s_raw)); TRY(fg.zero(h->truth.p(), S * TRUTH_PER_SET));
        TRY(fg.flush());
    }
    TRY(ensure(h, h->tminmax, (size_t)S * MINMAX)); TRY(ensure(h, h->tile_truth, (size_t)T * TRUTH_PER_TILE));
    pa.ph = h->ph.p();
    pa.ph_gain = ph_gain_base(h);
    pa.raw = h->raw.p();
    pa.tile_truth = h->tile_truth.p();
    if ((h->debug_bits & DBG_CURRENTS) && h->run.n_active_tiles > 0) {
        // debug: tile lengths in work-list order -> offsets
        HIPCHK(hipStreamSynchronize(h->stream));
        const ListedTiles lt = listed_tiles(h);
        h->run.cur_total = lt.off.back();
        TRY(upload(h, h->cur_off, lt.off.data(), lt.off.size()));
        TRY(ensure(h, h->currents, (size_t)h->run.cur_total));
        HIPCHK(hipStreamSynchronize(h->stream));
        pa.currents = h->currents.p(); pa.cur_off = h->cur_off.p();
    }
    if (h->run.n_active_tiles > 0) {        // tile descriptors of the whole work list (read by every pulse kernel)
        TRY(ensure(h, h->tile_desc, (size_t)h->run.n_active_tiles));
        DescArgs da{h->active_tiles.p(), h->run.n_active_tiles, h->tile_count.p(), h->tile_tmin.p(), h->tile_tmax.p(), h->tile_off.p(),
                    h->set_cluster.p(), h->set_t0.p(), h->set_mode.p(), h->cl_group.p(), h->row_lo.p(), h->acc_off.p(),
                    h->tile_desc.p()};
        TRY(launch(h, PLAIN(k_tile_desc), per_thread(h->run.n_active_tiles), d, da));
    }
    if (h->run.n_tiny_tiles > 0) {
        PulseArgs pt = pa;
        pt.desc = h->tile_desc.p();
        TRY(launch(h, K_PULSE_TINY(fma), per_thread(h->run.n_tiny_tiles * TINY_LANES), d, pt, h->run.n_tiny_tiles));
    }
    if (h->run.n_wave_tiles > 0) {
        PulseArgs pw = pa;
        pw.desc = h->tile_desc.p() + r.first_wave;
        if (pw.cur_off) pw.cur_off += r.first_wave;
        TRY(launch(h, K_PULSE_WAVE(fma), per_wave(h->run.n_wave_tiles), d, pw, h->run.n_wave_tiles));
    }
    if (h->run.n_sparse_tiles > 0) {
        PulseArgs ps = pa;
        ps.desc = h->tile_desc.p() + r.first_sparse;
        if (ps.cur_off) ps.cur_off += r.first_sparse;
        ps.W = (int)((h->run.max_nb + 7) / 8 * 8); ps.NP = (int)((h->run.max_tile + 7) / 8 * 8);
        // (tile_class lists a tile here with at most SPARSE_MAX_PHOTONS photons in at most SPARSE_MAX_BINS start bins: one form, 64 threads)
        const size_t lds = (size_t)sparse_lds(ps.NP, ps.W, SPARSE_TPB).total;
        TRY(launch(h, K_PULSE_SPARSE(fma), per_group(h->run.n_sparse_tiles, SPARSE_TPB, lds), d, ps));
    }
    if (h->run.n_dense_tiles > 0 && h->generic_geom) {        // any digitiser geometry: one kernel for every tile
        PulseArgs pd = pa;
        pd.desc = h->tile_desc.p() + r.first_dense;
        if (pd.cur_off) pd.cur_off += r.first_dense;
        // two H tables (order-independent merge of the gains of one cell) where they fit, one otherwise
        pd.n_win = generic_lds_split(d.dt, d.tlen) ? 1 : 0;
        const size_t lds = (size_t)generic_lds(d.dt, d.tlen, pd.n_win != 0).total;
        if (lds > (size_t)LDS_CAP_GENERIC) return h->fail(WFS_E_CAPACITY, "sample_duration x template length too large for the LDS tables of k_pulse_generic");
        TRY(launch(h, K_PULSE_GENERIC(fma), per_group(h->run.n_dense_tiles, 256, lds), d, pd));
    } else if (h->run.n_dense_tiles > 0) {
        PulseArgs pd = pa;
        pd.desc = h->tile_desc.p() + r.first_dense;
        if (pd.cur_off) pd.cur_off += r.first_dense;
        // chunks of TPB live samples per pass (TPB + 21 start-bin rows of 80 bytes in LDS: 22 KB for 256 -> 7 workgroups per CU)
        const i64 n_live_max = h->run.max_nb_dense + d.tlen - 1;
        const bool small = n_live_max <= 128;
        const int tpb = small ? 128 : 256;
        const int NWIN_MAX = 8;
        // tiles that fit one register batch: one workgroup per tile walks the chunks with the photons resident in
        // registers; longer tiles: several workgroups per tile (each re-reads the tile's photons for its chunks)
        // (the resident form holds at most tpb x DENSE_PPT photons: a longer tile must take the windowed form even when its live samples
        // fit one chunk and n_win comes out as 1 -- choosing the form by n_win dropped the photons behind the register batch)
        const bool resident = h->run.max_tile_dense <= (i64)tpb * DENSE_PPT;
        pd.n_win = resident ? 1 : (int)std::min<i64>(NWIN_MAX, std::max<i64>(1, (n_live_max + tpb - 1) / tpb));
        pd.W = tpb;
        const TemplateArg tp = fill_template_arg(h);
        const size_t lds = (size_t)pulse_lds(tpb).total;
        pd.sparse_max = (h->debug_bits & DBG_FORCE_DENSE) ? -1 : h->tap_sparse_max;      // (force_dense: every wave takes the dense gather)
        pd.spe_lds = ((size_t)(tpb + d.tlen - 1) * d.dt >= SPE_ROW_LEN) ? 1 : 0;
        TRY(launch(h, K_PULSE(!small, resident, fma), per_group(h->run.n_dense_tiles * pd.n_win, tpb, lds), d, pd, tp));
    }

    if (r.tiles_done && (h->h_scal->n_shared_rows > 0 || d.full_readout)) {      // (full readout: no row is its tile, every one of them is added)   // tiles of k_s2_tile that share their row with other pulses: added into the row's accumulators
        TileAddArgs ta{h->set_cluster.p(), h->cl_group.p(), h->row_lo.p(), h->acc_off.p(), h->row_cnt.p(), h->raw.p()};
        Timer t(h, "k_tile_add");
        if (h->run.n_fused_tiles > 0) TRY(launch_untimed(h, PLAIN(k_tile_add), per_group(h->run.n_fused_tiles), d, h->fuse_args, ta));
        if (h->run.n_bright_tiles > 0) {                       // (the tiles of k_s2_bright: their own stretch of the work list)
            FuseArgs fb = h->fuse_args; fb.tiles += h->bright_args.list_first;
            TRY(launch_untimed(h, PLAIN(k_tile_add), per_group(h->run.n_bright_tiles), d, fb, ta));
        }
    }
    return WFS_OK;
}

// ---- rows: resident rows (pulses, finished samples and intervals in one kernel), truth, ZLE of the accumulator rows
static int run_rows(wfs_handle *h, RunState &r)
{
    const WfsDev &d = h->dev;
    const GeomArgs &ga = r.ga; const PulseArgs &pa = r.pa; ZleArgs &za = r.za;
    const i64 S = h->batch.n_sets, CG = r.CG;
    const i64 RS = r.RS = CG * d.row_slots;
    TRY(ensure_rows(h, h->itv_left, (size_t)h->run.n_itv_slots + 2, "the interval slots")); TRY(ensure_rows(h, h->itv_right, (size_t)h->run.n_itv_slots + 2, "the interval slots"));      // (+2: k_pack reads the first two slots of a row whatever its capacity)
    TRY(ensure(h, h->itv_n, (size_t)RS)); TRY(ensure(h, h->row_nrec, (size_t)RS));
    FillGroup fg(h, "fills_rows");
    TRY(fg.zero(h->itv_n.p(), RS)); TRY(fg.zero(h->row_nrec.p(), RS));
    za.active_rows = h->active_rows.p(); za.n_active_rows = h->run.n_active_rows; za.row_lo = h->row_lo.p(); za.row_hi = h->row_hi.p();
    za.acc_off = h->acc_off.p(); za.raw = h->raw.p(); za.grp_left = h->grp_left.p(); za.grp_ixrand = h->grp_ixrand.p();
    za.itv_off = h->itv_off.p(); za.itv_left = h->itv_left.p(); za.itv_right = h->itv_right.p();
    za.itv_n = h->itv_n.p(); za.row_nrec = h->row_nrec.p(); za.spr = WFS_SPR;
    if (r.tiles_done) { za.tile_done = ga.tile_done; za.n_done = ga.n_done; za.row_cnt = ga.row_cnt; za.row_tile = ga.row_tile; za.ins_bcap = ga.ins_bcap; za.ins_boff = ga.ins_boff; za.tbuf = h->tbuf.p(); }
    za.n_front = h->run.n_front_rows; za.rows_cap = CG * d.row_slots;
    if (d.sum_channel >= 0) { za.sum_lo = h->sum_lo.p(); za.sum_hi = h->sum_hi.p(); za.sum_off = h->sum_off.p(); za.sum_base = h->run.sum_base; }
    za.n_res = h->run.n_res_rows;
    if (h->run.n_res_rows > 0 || n_empty_rows(h) > 0) {      // finished 16-bit samples: the resident rows', then those of the rows without a pulse
        TRY(ensure_rows(h, h->fin, (size_t)(h->run.s_fin + s_empty(h)) + 8, "the finished samples of the rows without a pulse"));
        za.fin = h->fin.p();
    }
    if (h->run.n_res_rows > 0) {
        TRY(ensure(h, h->res_rows, (size_t)h->run.n_res_rows));
        za.res_toff = h->res_toff.p(); za.fin_off = h->fin_off.p();
        za.n_short = h->run.n_short_rows; za.res_long = h->res_long.p(); za.res_rows = h->res_rows.p();
    }
    if (n_empty_rows(h) > 0) {
        za.fin_base = h->run.s_fin; za.empty_rows = h->empty_rows.p(); za.fr_off = h->fr_off.p(); za.grp_lo = h->grp_lo.p(); za.grp_hi = h->grp_hi.p();
    }
    if ((h->debug_bits & DBG_CURRENTS) && h->run.n_active_rows > 0) {
        const ListedRows lr = listed_rows(h);
        h->run.row_dbg_total = lr.off.back();
        TRY(upload(h, h->row_dbg_off, lr.off.data(), lr.off.size()));
        TRY(ensure(h, h->row_dbg, (size_t)h->run.row_dbg_total));
        HIPCHK(hipStreamSynchronize(h->stream));
        za.row_dbg = h->row_dbg.p(); za.row_dbg_off = h->row_dbg_off.p();
    }
    TRY(ensure(h, h->row_desc, (size_t)h->run.n_active_rows)); za.desc = h->row_desc.p();
    if (h->sort_records) {      // key_origin / key_end: first sample / end of the last row of the batch (k_row_desc): origin and span of the sort keys
        za.key_base = h->scal.p();
        TRY(fg.fill(&za.key_base->key_origin, 1, I64_MAX)); TRY(fg.fill(&za.key_base->key_end, 1, I64_MIN));
    }
    TRY(fg.flush());
    if (h->run.n_active_rows > 0) TRY(launch(h, PLAIN(k_row_desc), per_thread(h->run.n_active_rows), d, za));
    r.noise_kind = d.enable_noise ? noise_kind_of(d) : NOISE_NONE;
    r.dark = d.dk_thr != nullptr;
    if (h->run.n_res_rows > 0) {        // resident rows: pulses, finished samples and intervals by one wave per row
        PulseArgs pr = pa;
        pr.desc = h->res_desc.p(); pr.currents = nullptr; pr.cur_off = nullptr;
        // two launches: the rows of at most RES_SHORT_LEN samples at full occupancy, the longer ones with LDS for the longest of them
        Timer t(h, "k_row_pulse");
        for (int part = 0; part < 2; part++) {
            const i64 first = part == 0 ? 0 : h->run.n_short_rows, n_rows = part == 0 ? h->run.n_short_rows : h->run.n_res_rows - h->run.n_short_rows;
            if (n_rows <= 0) continue;
            const i32 region = part == 0 ? RES_SHORT_LEN : (i32)((std::min<i64>(h->run.max_res_len, h->res_max_len) + 255) / 256 * 256);
            const size_t lds = (size_t)row_pulse_lds(region).total;
            TRY(launch_untimed(h, K_ROW_PULSE(r.noise_kind, h->cfg.fma != 0, part == 1, r.dark), per_wave(n_rows, lds), d, pr, za, first, n_rows, region));
        }
    }
    if (n_empty_rows(h) > 0) {      // full readout: the rows without a pulse, finished samples and intervals by one wave per row
        const i64 first = h->run.n_front_rows + h->run.n_res_rows;
        TRY(launch(h, K_ROW_EMPTY(r.noise_kind, r.dark), per_wave(n_empty_rows(h)), d, za, first, n_empty_rows(h)));
    }
    {   // truth accumulators of every pulse set from the per-tile partial sums
        TruthArgs ta{S, h->tile_count.p(), h->tile_tmin.p(), h->tile_tmax.p(), h->set_t0.p(), h->tile_truth.p(),
                     h->truth.p(), h->tminmax.p()};
        TRY(launch(h, PLAIN(k_truth_reduce), per_wave(S), d, ta));
    }

    // (WFS_SUM_SKIP_KERNEL: A/B runs that price what the switch costs apart from the kernel -- bottom rows off the resident path, one
    // more row per window through k_zle / k_pack; the sum rows then hold whatever the buffer held)
    if (h->run.n_sum_chunks > 0 && !getenv("WFS_SUM_SKIP_KERNEL")) {      // the windows' sum rows from their bottom rows: every accumulator and tile buffer is complete here (k_tile_add included)
        if (h->run.n_sum_chunks > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, "more than 2^31 chunks of sum rows in one batch");
        SumArgs sa{h->sum_chunk_off.p(), CG, h->sum_lo.p(), h->sum_off.p(), h->sum_len.p(),
                   h->row_lo.p(), h->row_hi.p(), h->acc_off.p(), h->raw.p(), r.tiles_done ? h->tbuf.p() : nullptr,
                   r.tiles_done ? ga.tile_done : nullptr, ga.row_cnt, ga.row_tile, ga.ins_bcap, ga.ins_boff, ga.n_done, h->raw.p() + h->run.sum_base};
        TRY(launch(h, PLAIN(k_sum_signal), per_group(h->run.n_sum_chunks), d, sa));
    }
    if (h->run.n_front_rows > 0) {
        TRY(launch(h, K_ZLE(r.noise_kind, r.dark), per_wave(h->run.n_front_rows), d, za));
    }
    return WFS_OK;
}

// ---- records: how many, where (sorted by time and channel on request), packing; the totals of wfs_get_counts
static int run_records(wfs_handle *h, RunState &r)
{
    const WfsDev &d = h->dev;
    ZleArgs &za = r.za;
    const i64 RS = r.RS;
    // the packers keep their place on the main stream, in front of the last boundary, in a profiled step (kernel_times lists them), in
    // the debug modes, on a caller's stream and under WFS_PACK_SYNC=1
    const bool defer = h->own_stream && !h->profiling && h->debug_bits == 0 && !h->pack_sync;
    TRY(scan(h, h->row_nrec.p(), RS, h->rec_off, &WfsScal::n_records));
    TRY(read_scal(h));
    h->run.n_records = h->h_scal->n_records;
    // the other arena: the previous batch's records may still be on their way to the host
    h->rec_cur ^= 1;
    if (h->rec_pending[h->rec_cur]) { HIPCHK(hipEventSynchronize(h->rec_copied[h->rec_cur])); h->rec_pending[h->rec_cur] = false; }
    TRY(ensure_rows(h, h->records_buf(), (size_t)h->run.n_records * WFS_RECORD_BYTES, "the records"));
    za.rec_off = h->rec_off.p(); za.records = h->records_buf().as<uint8_t>(); za.rec_capacity = h->run.n_records;
    if (h->sort_records && h->run.n_records > 1 && h->run.n_active_rows > 0)      // records by (time, channel): the packers write to the sorted slots
        TRY(order_records(h, h->rec, za, h->run.n_active_rows, h->run.n_records, h->h_scal->key_origin, h->h_scal->key_end, "more than 2^31 records in one batch (the device sort takes an int count)", "record_sort"));
    if (h->run.n_active_rows > 0 && h->run.n_records > 0) {
        TRY(ensure(h, h->pack_desc, (size_t)h->run.n_active_rows)); za.pdesc = h->pack_desc.p();
        // Nothing wfs_run returns depends on the packers: they go to the pack stream, behind everything on the main stream up to here,
        // and run under the front end of the next wfs_run, which fences them in front of its first write to what they read
        // (pack_fence).  Readers of the records wait for the arena's ready event.  (The timers are idle then: profiled steps are serial.)
        hipStream_t ps = h->stream;
        if (defer) {
            HIPCHK(hipEventRecord(h->pack_go[h->rec_cur], h->stream));
            HIPCHK(hipStreamWaitEvent(h->pack_stream, h->pack_go[h->rec_cur], 0));
            ps = h->pack_stream;
        }
        // (rows that exist as finished samples: resident, without a pulse; behind the front rows of the list)
        TRY(pack_finished_rows(h, za, h->run.n_active_rows, h->fin.p(), h->run.n_front_rows, h->run.n_res_rows + n_empty_rows(h), ps));
        if (h->run.n_front_rows > 0) {
            TRY(launch(h, K_PACK(r.noise_kind, r.dark), per_wave(h->run.n_front_rows).on(ps), d, za));
        }
        if (defer) {
            HIPCHK(hipEventRecord(h->rec_ready[h->rec_cur], h->pack_stream));
            h->pack.deferred(h->rec_cur);
        }
    }
    {   // totals of wfs_get_counts: afterpulse sets carry no truth (rawdata.py:322-323)
        const i64 n_prim = h->batch.ap_sets ? h->batch.n_psets : h->batch.n_sets;
        const i64 work = std::max<i64>(RS, n_prim);
        // (not timed, as ever: an entry would change the (name, launches) list that profiled steps are compared by, and tools/make_profiles.py
        // counts the runs of a trace by this kernel, not by an entry)
        TRY(launch_untimed(h, PLAIN(k_counts), Shape(dim3((unsigned)std::min<i64>(nblocks(work, 256), 128)), dim3(256)), h->itv_n.p(), RS, h->truth.p(), n_prim, h->scal.p()));
    }
    TRY(read_scal(h));
    HIPCHK(hipGetLastError());
    CHECK_LAUNCHES();
    return WFS_OK;
}

int wfs_run(wfs_handle *h)
try {
    if (!h) return WFS_E_INVALID;
    if (h->batch.kind == BatchKind::None) return h->fail(WFS_E_STATE, "no batch loaded");
    if (h->batch.dev_rows_pending) return h->fail(WFS_E_STATE, "instructions with cdf_row -1: call wfs_eval_pattern_rows before wfs_run");
    h->state().run_begins();
    HIPCHK(hipSetDevice(h->device));
    clear_times(h->times);
    TRY(run_input(h));
    h->state().generation_done();
    if (h->debug_bits & DBG_GEN_ONLY) { HIPCHK(hipStreamSynchronize(h->stream)); return WFS_OK; }      // wfs_set_debug bit 2: photon generation only
    RunState r;
    TRY(run_geometry(h, r));
    TRY(run_pulses(h, r));
    TRY(run_rows(h, r));
    TRY(run_records(h, r));
    h->state().run_complete();
    return WFS_OK;
} WFS_CATCH(h)

int wfs_get_counts(wfs_handle *h, wfs_counts *out)
try {
    if (!h || !out) return WFS_E_INVALID;
    if (!run_finished(h)) return h->fail(WFS_E_STATE, "wfs_run has not completed");
    wfs_counts c{};
    c.n_instructions = h->batch.n_ins; c.n_pulse_sets = h->batch.n_sets; c.n_emitters = h->batch.n_emitters; c.n_photons = n_primary_photons(h) + h->run.n_ap_photons;
    const bool tiles_done = tiles_made(h);
    c.n_tiles = h->run.n_active_tiles + (tiles_done ? h->run.n_fused_tiles : 0) + h->run.n_res_tiles; c.n_groups = h->run.n_groups; c.n_rows = h->run.n_active_rows;
    c.n_raw_samples = h->run.s_raw + (tiles_done ? h->run.s_raw_direct : 0) + h->run.s_res + h->run.s_sum;      // (full readout: rows without a pulse have no raw sample)
    c.n_records = h->run.n_records;
    c.n_intervals = h->h_scal->n_intervals; c.n_pe = h->h_scal->n_pe;          // reduced on the device at the end of wfs_run (k_counts)
    *out = c;
    return WFS_OK;
} WFS_CATCH(h)

const void *wfs_records_dev_ptr(wfs_handle *h) { return h ? h->records_buf().p : nullptr; }

int wfs_copy_records(wfs_handle *h, void *dst, int64_t cap)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    if (cap < h->run.n_records) return h->fail(WFS_E_CAPACITY, "record buffer too small");
    TRY(pack_wait(h));
    if (h->run.n_records) HIPCHK(hipMemcpy(dst, h->records_buf().p, (size_t)h->run.n_records * WFS_RECORD_BYTES, hipMemcpyDeviceToHost));
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_records_range(wfs_handle *h, void *dst, int64_t first, int64_t count)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    if (first < 0 || count < 0 || first + count > h->run.n_records) return h->fail(WFS_E_INVALID, "record range outside the batch");
    TRY(pack_wait(h));
    if (count) HIPCHK(hipMemcpy(dst, (const uint8_t *)h->records_buf().p + (size_t)first * WFS_RECORD_BYTES, (size_t)count * WFS_RECORD_BYTES, hipMemcpyDeviceToHost));
    return WFS_OK;
} WFS_CATCH(h)

// Pinned host memory + the copy stream: the records of a batch travel to the host while the next batch's kernels run
// (strax_interface.py:360-364: the caller owns the record buffer; pinning it once removes the staging copy of pageable
// transfers -- 15 GB/s -- and lets the transfer overlap).  wfs_run leaves the records of the last TWO batches intact.
int wfs_host_register(void *ptr, int64_t bytes)
try {
    if (!ptr || bytes <= 0) return WFS_E_INVALID;
    return hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault) == hipSuccess ? WFS_OK : WFS_E_HIP;
} WFS_CATCH(nullptr)
int wfs_host_unregister(void *ptr) try { return (ptr && hipHostUnregister(ptr) == hipSuccess) ? WFS_OK : WFS_E_HIP; } WFS_CATCH(nullptr)

int wfs_copy_records_range_async(wfs_handle *h, void *dst, int64_t first, int64_t count)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    if (first < 0 || count < 0 || first + count > h->run.n_records) return h->fail(WFS_E_INVALID, "record range outside the batch");
    HIPCHK(hipSetDevice(h->device));
    // (the copy stream waits for the packers of this arena; the host does not, and the pack stays pending for the next run's fence)
    if (h->pack.must_wait()) HIPCHK(hipStreamWaitEvent(h->copy_stream, h->rec_ready[h->pack.arena], 0));
    if (count) HIPCHK(hipMemcpyAsync(dst, (const uint8_t *)h->records_buf().p + (size_t)first * WFS_RECORD_BYTES, (size_t)count * WFS_RECORD_BYTES, hipMemcpyDeviceToHost, h->copy_stream));
    HIPCHK(hipEventRecord(h->rec_copied[h->rec_cur], h->copy_stream));
    h->rec_pending[h->rec_cur] = true;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_wait_records(wfs_handle *h)
try {
    if (!h) return WFS_E_INVALID;
    // May be called from the consumer's thread while a worker thread is inside wfs_run for the next batch (RawData.iter_batches):
    // it only waits for the copy stream and leaves the handle's state alone -- rec_pending stays with the thread that runs and copies
    // (wfs_run's own wait on an event that has completed returns at once).
    if (hipStreamSynchronize(h->copy_stream) != hipSuccess) return WFS_E_HIP;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_records_dev(wfs_handle *h, void *dst, int64_t cap)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    if (cap < h->run.n_records) return h->fail(WFS_E_CAPACITY, "record buffer too small");
    TRY(pack_wait(h));
    if (h->run.n_records) { HIPCHK(hipMemcpyAsync(dst, h->records_buf().p, (size_t)h->run.n_records * WFS_RECORD_BYTES, hipMemcpyDeviceToDevice, h->stream)); HIPCHK(hipStreamSynchronize(h->stream)); }
    return WFS_OK;
} WFS_CATCH(h)

// records of a batch in the order strax.sort_by_time gives them ((time, channel); strax_interface.py:453) instead of the
// order the reference yields pulses (window, channel, interval)
int wfs_set_record_order(wfs_handle *h, int32_t by_time)
try {
    if (!h) return WFS_E_INVALID;
    h->sort_records = by_time != 0;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_groups(wfs_handle *h, int64_t *left, int64_t *right, int64_t *first_record, int64_t *ix_rand)
try {
    if (!h || !run_complete(h)) return WFS_E_STATE;
    const i64 G = h->run.n_groups;
    if (left) TRY(copy_out(h, left, h->grp_left.p(), (size_t)G));
    if (right) TRY(copy_out(h, right, h->grp_right.p(), (size_t)G));
    if (ix_rand) TRY(copy_out(h, ix_rand, h->grp_ixrand.p(), (size_t)G));
    if (first_record && G > 0)      // rec_off[g * row_slots]: a strided copy of one value per window (the whole array is 6 KB per cluster)
        HIPCHK(hipMemcpy2D(first_record, sizeof(i64), h->rec_off.p(), (size_t)h->dev.row_slots * sizeof(i64), sizeof(i64), (size_t)G, hipMemcpyDeviceToHost));
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_intervals(wfs_handle *h, int32_t *group, int32_t *channel, int64_t *left, int64_t *right, int64_t *data_off, int64_t cap)
try {
    if (!h || !run_complete(h)) return WFS_E_STATE;
    const WfsDev &d = h->dev;
    const i64 RS = (h->batch.n_clusters + 1) * d.row_slots;
    const std::vector<i32> n = download(h, h->itv_n, (size_t)RS);
    const std::vector<i64> off = download(h, h->itv_off, (size_t)RS + 1);
    const std::vector<i64> L = download(h, h->itv_left, (size_t)h->run.n_itv_slots), R = download(h, h->itv_right, (size_t)h->run.n_itv_slots);
    i64 k = 0, doff = 0;
    for (i64 idx = 0; idx < RS; idx++) {
        const RowSlot s = row_slot(d, idx);
        for (i32 q = 0; q < n[idx]; q++) {
            if (k >= cap) return h->fail(WFS_E_CAPACITY, "interval buffer too small");
            i64 l = L[off[idx] + q], r = R[off[idx] + q];
            group[k] = (i32)s.g; channel[k] = s.channel; left[k] = l; right[k] = r; data_off[k] = doff;
            doff += (r - l + 1 > 0) ? r - l + 1 : 0; k++;
        }
    }
    if (k < cap) data_off[k] = doff;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_interval_data(wfs_handle *h, int16_t *data, int64_t cap)
try {
    // unpack the records: fragments of one interval are consecutive
    if (!h || !run_finished(h)) return WFS_E_STATE;
    std::vector<uint8_t> rec((size_t)h->run.n_records * WFS_RECORD_BYTES);
    TRY(pack_wait(h));
    if (h->run.n_records) HIPCHK(hipMemcpy(rec.data(), h->records_buf().p, rec.size(), hipMemcpyDeviceToHost));
    i64 k = 0;
    for (i64 r = 0; r < h->run.n_records; r++) {
        i32 len; memcpy(&len, &rec[(size_t)r * WFS_RECORD_BYTES + REC_LENGTH_BYTE], 4);
        if (k + len > cap) return h->fail(WFS_E_CAPACITY, "interval data buffer too small");
        memcpy(data + k, &rec[(size_t)r * WFS_RECORD_BYTES + REC_DATA_BYTE], (size_t)len * 2);
        k += len;
    }
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_pulses(wfs_handle *h, int32_t *set, int32_t *channel, int64_t *left, int64_t *right, int64_t *nph, int64_t *cur_off, int64_t cap)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    const WfsDev &d = h->dev;
    const i64 A = h->run.n_active_tiles;
    if (cap < A) return h->fail(WFS_E_CAPACITY, "pulse buffer too small");
    const ListedTiles lt = listed_tiles(h);
    const std::vector<i32> cnt = download(h, h->tile_count, (size_t)h->batch.n_tiles);
    for (i64 k = 0; k < A; k++) {
        const i64 tile = lt.tile[k], s = tile / d.n_tpc;
        set[k] = (i32)s; channel[k] = (i32)(tile - s * d.n_tpc);
        left[k] = lt.win[k].left; right[k] = lt.win[k].right;
        nph[k] = cnt[tile]; cur_off[k] = lt.off[k];
    }
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_currents(wfs_handle *h, double *cur, int64_t cap)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    if (!(h->debug_bits & DBG_CURRENTS)) return h->fail(WFS_E_STATE, "wfs_set_debug(h, 1) before wfs_run");
    if (cap < h->run.cur_total) return h->fail(WFS_E_CAPACITY, "current buffer too small");
    if (h->run.cur_total) TRY(copy_out(h, cur, h->currents.p(), (size_t)h->run.cur_total));
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_rows(wfs_handle *h, int32_t *group, int32_t *channel, int64_t *left, int64_t *right, int64_t *data_off, int64_t cap)
try {
    if (!h || !run_complete(h)) return WFS_E_STATE;
    if (!(h->debug_bits & DBG_CURRENTS)) return h->fail(WFS_E_STATE, "wfs_set_debug(h, 1) before wfs_run");
    const WfsDev &d = h->dev;
    const i64 A = h->run.n_active_rows - n_empty_rows(h);      // (full readout: the rows without a pulse never exist unfinished)
    if (cap < A) return h->fail(WFS_E_CAPACITY, "row buffer too small");
    const ListedRows lr = listed_rows(h);
    const std::vector<i64> gl = download(h, h->grp_left, (size_t)h->run.n_groups);
    for (i64 k = 0; k < A; k++) {
        const RowSlot &s = lr.slot[k];
        group[k] = (i32)s.g; channel[k] = s.channel;
        // relative to the window like the reference's channel mask (rawdata.py:258-259)
        const RowSpan sp = row_span(lr.lo[k] - gl[s.g], lr.hi[k] - gl[s.g], d.tw);
        left[k] = sp.left; right[k] = sp.right;
        data_off[k] = lr.off[k];
    }
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_row_data(wfs_handle *h, int32_t *data, int64_t cap)
try {
    if (!h || !run_complete(h)) return WFS_E_STATE;
    if (cap < h->run.row_dbg_total) return h->fail(WFS_E_CAPACITY, "row data buffer too small");
    if (h->run.row_dbg_total) TRY(copy_out(h, data, h->row_dbg.p(), (size_t)h->run.row_dbg_total));
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_photons(wfs_handle *h, int64_t *set_off, int64_t *t, int16_t *ch, double *gain, uint8_t *dpe, int64_t cap)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    if (tiles_made(h) && !(h->debug_bits & DBG_KEEP_PHOTONS))
        return h->fail(WFS_E_STATE, "the photons of tile-generated instructions were not kept: wfs_set_debug bit 4 before wfs_run");
    const WfsDev &d = h->dev;
    const i64 n_prim = n_primary_photons(h), P = n_prim + h->run.n_ap_photons, T = h->batch.n_tiles;
    if (cap < P) return h->fail(WFS_E_CAPACITY, "photon buffer too small");
    const std::vector<i64> off = download(h, h->tile_off, (size_t)T + 1), t0 = download(h, h->set_t0, (size_t)h->batch.n_sets);
    const std::vector<PhotonRec> recs = download(h, h->ph, (size_t)P);
    const std::vector<double> gains = download(h, h->t_gains, (size_t)d.n_tpc), spe = download(h, h->t_spe, (size_t)SPE_ROW_LEN * d.n_spe);
    const i64 gain_first = h->batch.kind == BatchKind::Photons ? 0 : n_prim;        // ph_gain covers the explicit-gain photons only
    const std::vector<double> pg = download(h, h->ph_gain, (size_t)std::max<i64>(P - gain_first, 0));
    if (off[(size_t)T] != P) { char msg[160]; snprintf(msg, sizeof msg, "wfs_copy_photons: tile offsets end at %lld, %lld photons (T %lld, sets %lld)", (long long)off[(size_t)T], (long long)P, (long long)T, (long long)h->batch.n_sets); return h->fail(WFS_E_STATE, msg); }
    for (i64 s = 0; s <= h->batch.n_sets; s++) set_off[s] = off[(size_t)s * d.n_tpc];
    for (i64 tile = 0; tile < T; tile++) {
        i64 s = tile / d.n_tpc; int c = (int)(tile - s * d.n_tpc);
        const double *row = &spe[(size_t)(d.n_spe > 1 ? c : 0) * SPE_ROW_LEN];
        for (i64 p = off[tile]; p < off[tile + 1]; p++) {
            t[p] = t0[s] + recs[p].t; ch[p] = (int16_t)c;
            u32 g1 = recs[p].code & 0xffffu, g2 = recs[p].code >> 16;
            if (p >= gain_first) { gain[p] = pg[(size_t)(p - gain_first)]; dpe[p] = g2 != 0; }
            else { gain[p] = spe_gain(gains[c], row[g1], row[g2], recs[p].code); dpe[p] = g2 != 0; }
        }
    }
    return WFS_OK;
} WFS_CATCH(h)

// Generation order of a batch's photons as the electron-afterpulse pre-pass sees it (rawdata.py:133-145 hands the parent S2's photons to
// afterpulse.py): instruction by instruction; the photons of an instruction of the per-electron generator in its generation order, those
// of a tile-generated instruction tile by tile (channel ascending), photon q of a tile at position q.  Host-side tables of that order,
// built once per generation.
static int gen_order_tables(wfs_handle *h)
{
    if (h->run.gen_order_ready) return WFS_OK;
    const i64 N = h->batch.n_ins; const int nch = h->dev.n_tpc;
    const std::vector<i64> emo = download(h, h->em_off, (size_t)N + 1), epo = download(h, h->em_ph_off, (size_t)h->batch.n_emitters + 1);
    h->run.go_fused.assign((size_t)N, 0); h->run.go_tile_count.clear();
    const bool any_fused = h->run.fuse_on && n_tilegen_tiles(h) > 0;
    if (any_fused) {
        h->run.go_fused = download(h, h->ins_fused, (size_t)N);
        h->run.go_tile_count = download(h, h->tile_count, (size_t)N * nch);      // (one pulse set per instruction: tile = instruction * n_tpc + channel)
    }
    h->run.go_off.assign((size_t)N + 1, 0); h->run.go_block0.assign((size_t)N, 0);
    for (i64 i = 0; i < N; i++) {
        i64 n = epo[(size_t)emo[i + 1]] - epo[(size_t)emo[i]];           // (0 for a tile-generated instruction: its electrons carry no photon numbers)
        h->run.go_block0[i] = epo[(size_t)emo[i]];
        if (any_fused && h->run.go_fused[i]) for (int c = 0; c < nch; c++) n += h->run.go_tile_count[(size_t)i * nch + c];
        h->run.go_off[i + 1] = h->run.go_off[i] + n;
    }
    h->run.gen_order_ready = true;
    return WFS_OK;
}

int wfs_copy_instruction_photon_offsets(wfs_handle *h, int64_t *off, int64_t cap)
try {
    if (!h || !generated(h)) return WFS_E_STATE;
    const i64 N = h->batch.n_ins;
    if (cap < N + 1) return h->fail(WFS_E_CAPACITY, "offset buffer too small");
    TRY(gen_order_tables(h));
    for (i64 i = 0; i <= N; i++) off[i] = h->run.go_off[(size_t)i];
    return WFS_OK;
} WFS_CATCH(h)

int wfs_gather_photon_times(wfs_handle *h, int64_t n, const int64_t *index, int64_t *t_out)
try {
    if (!h || !generated(h)) return WFS_E_STATE;
    if (n <= 0) return WFS_OK;
    if (!index || !t_out) return h->fail(WFS_E_INVALID, "wfs_gather_photon_times: null argument");
    TRY(gen_order_tables(h));
    const i64 N = h->batch.n_ins; const int nch = h->dev.n_tpc;
    for (i64 i = 0; i < n; i++) if (index[i] < 0 || index[i] >= h->run.go_off[(size_t)N]) return h->fail(WFS_E_INVALID, "photon index out of range");
    HIPCHK(hipSetDevice(h->device));
    // requests of the per-electron generator (index in ITS photon order) and of tile-generated instructions (instruction, channel, q)
    std::vector<i64> blk_idx, blk_pos, tile_pos; std::vector<TileTimeReq> treq;
    for (i64 k = 0; k < n; k++) {
        const i64 i = (i64)(std::upper_bound(h->run.go_off.begin(), h->run.go_off.end(), (i64)index[k]) - h->run.go_off.begin()) - 1;
        i64 local = index[k] - h->run.go_off[(size_t)i];
        if (!h->run.go_fused[(size_t)i]) { blk_idx.push_back(h->run.go_block0[(size_t)i] + local); blk_pos.push_back(k); continue; }
        int c = 0;
        const i32 *cnt = &h->run.go_tile_count[(size_t)i * nch];
        while (c < nch - 1 && local >= cnt[c]) { local -= cnt[c]; c++; }
        treq.push_back(TileTimeReq{(i32)i, (i32)c, (i32)local, 0}); tile_pos.push_back(k);
    }
    std::vector<i64> got;
    if (!blk_idx.empty()) {
        const i64 m = (i64)blk_idx.size();
        TRY(upload(h, h->gather_idx, blk_idx.data(), (size_t)m)); TRY(ensure(h, h->gather_out, (size_t)m));
        // (not timed: a copy-out after the run, whose entry would lengthen the list of the last profiled step)
        TRY(launch_untimed(h, PLAIN(k_photon_times), per_thread(m), h->dev, h->gen_args, m, h->gather_idx.p(), h->gather_out.p()));
        got.resize((size_t)m);
        TRY(copy_async(h, got.data(), h->gather_out.p(), (size_t)m, hipMemcpyDeviceToHost));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (i64 k = 0; k < m; k++) t_out[blk_pos[(size_t)k]] = got[(size_t)k];
    }
    if (!treq.empty()) {
        const i64 m = (i64)treq.size();
        TRY(upload(h, h->gather_req, treq.data(), (size_t)m)); TRY(ensure(h, h->gather_out, (size_t)m));
        // (not timed: as k_photon_times above)
        TRY(launch_untimed(h, PLAIN(k_tile_photon_times), per_thread(m), h->dev, h->fuse_args, m, h->gather_req.p(), h->gather_out.p()));
        got.resize((size_t)m);
        TRY(copy_async(h, got.data(), h->gather_out.p(), (size_t)m, hipMemcpyDeviceToHost));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (i64 k = 0; k < m; k++) t_out[tile_pos[(size_t)k]] = got[(size_t)k];
    }
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_truth(wfs_handle *h, double *acc12, double *tstat5, int64_t cap)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    const i64 S = h->batch.n_sets;
    if (cap < S) return h->fail(WFS_E_CAPACITY, "truth buffer too small");
    const std::vector<double> tr = download(h, h->truth, (size_t)S * TRUTH_PER_SET);
    const std::vector<i64> mm = download(h, h->tminmax, (size_t)S * MINMAX), t0 = download(h, h->set_t0, (size_t)S);
    for (i64 s = 0; s < S; s++) {
        for (int f = 0; f < 12; f++) acc12[s * 12 + f] = tr[s * 16 + f];
        stat5(tstat5 + s * 5, tr[s * 16 + 12], tr[s * 16 + 13], tr[s * 16 + 14], (double)t0[s], mm[2 * s], mm[2 * s + 1]);
    }
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_truth_per_pmt(wfs_handle *h, double *acc6, int64_t cap)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    const i64 S = h->batch.n_sets, nch = h->cfg.n_tpc, T = S * nch;
    if (cap < S) return h->fail(WFS_E_CAPACITY, "per-PMT truth buffer too small");
    const std::vector<double> tt = download(h, h->tile_truth, (size_t)T * TRUTH_PER_TILE), gains = download(h, h->t_gains, (size_t)nch);
    const std::vector<i32> cnt = download(h, h->tile_count, (size_t)T);
    for (i64 t = 0; t < T; t++) {
        double *o = acc6 + t * 6;
        if (cnt[t] <= 0) { for (int q = 0; q < 6; q++) o[q] = 0.0; continue; }     // tiles without photons were never written
        const double *p = tt.data() + t * 8, G = gains[t % nch];
        o[0] = p[0]; o[1] = p[0] + p[1]; o[2] = p[2]; o[3] = p[2] + p[3]; o[4] = p[4] / G; o[5] = p[5] / G;       // pulse.py:259-271
    }
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_electron_stats(wfs_handle *h, double *estat5, int64_t cap)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    const i64 N = h->batch.n_ins;
    if (h->batch.kind == BatchKind::Optical) { for (i64 i = 0; i < N && i < cap; i++) { estat5[i * 5] = 0; for (int q = 1; q < 5; q++) estat5[i * 5 + q] = NAN; } return WFS_OK; }
    const i64 PS = h->batch.n_psets;
    if (cap < PS) return h->fail(WFS_E_CAPACITY, "electron stats buffer too small");
    if (N == 0) return WFS_OK;
    const std::vector<double> st = download(h, h->el_stat, (size_t)N * STAT_PER_INS);
    const std::vector<i64> mm = download(h, h->el_minmax, (size_t)N * MINMAX), t0 = download(h, h->ins_time, (size_t)N);
    for (i64 q = 0; q < PS; q++) {
        // moments of the electrons of all instructions of the run set (rawdata.py:334-341), about the first instruction's time
        const i64 ref = h->batch.h_rs_off[q + 1] > h->batch.h_rs_off[q] ? t0[h->batch.h_rs_list[h->batch.h_rs_off[q]]] : 0;      // (an unused set number: no instructions, zero electrons)
        double n = 0, s1 = 0, s2 = 0; i64 lo = I64_MAX, hi = I64_MIN;
        for (i64 k = h->batch.h_rs_off[q]; k < h->batch.h_rs_off[q + 1]; k++) {
            const i64 i = h->batch.h_rs_list[k];
            const double ni = st[i * 4], a1 = st[i * 4 + 1], a2 = st[i * 4 + 2], dlt = (double)(t0[i] - ref);
            if (!(ni > 0)) continue;
            n += ni; s1 += a1 + ni * dlt; s2 += a2 + 2 * dlt * a1 + ni * dlt * dlt;
            lo = std::min(lo, mm[2 * i]); hi = std::max(hi, mm[2 * i + 1]);
        }
        stat5(estat5 + q * 5, n, s1, s2, (double)ref, lo, hi);
    }
    return WFS_OK;
} WFS_CATCH(h)

int wfs_set_bright_tiles(wfs_handle *h, int32_t on)
try {
    if (!h) return WFS_E_INVALID;
    h->bright_on = on != 0;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_set_sum_signal(wfs_handle *h, int32_t on)
try {
    if (!h) return WFS_E_INVALID;
    const wfs_config &c = h->cfg;
    if (on && c.detector_nt) {
        // the row takes the noise column, the threshold and the record channel of sum_channel: a channel of its own
        if (c.sum_channel < 0 || c.sum_channel >= c.n_rows) return h->fail(WFS_E_INVALID, "wfs_set_sum_signal: sum_channel outside the rows of the digitiser array");
        if (c.sum_channel < c.n_tpc || (c.sum_channel >= c.he_first && c.sum_channel < c.he_first + c.n_top))
            return h->fail(WFS_E_INVALID, "wfs_set_sum_signal: sum_channel lies inside the TPC or the high-energy channel range");
        if (c.n_top < 0 || c.last_bottom >= c.n_tpc) return h->fail(WFS_E_INVALID, "wfs_set_sum_signal: bottom array outside the TPC channels");
    }
    h->sum_on = on != 0;
    refresh_dev(h);             // (a switch that changes the row slots: run again before copying rows)
    return WFS_OK;
} WFS_CATCH(h)

// Every digitise window read out in full (include/wfsim_amd.h).  A change of mode: pending packers are waited for, like the other
// setters that change what a run lays out; the row SLOTS stay, so the last run's copies still decode.
int wfs_set_full_readout(wfs_handle *h, int32_t on)
try {
    if (!h) return WFS_E_INVALID;
    if ((on != 0) != h->full_on) TRY(pack_wait(h));
    h->full_on = on != 0;
    refresh_dev(h);
    return WFS_OK;
} WFS_CATCH(h)

// Parity entry: the sum rows before they are finished, S[t] = int(he_factor) * sum of the bottom rows (64 bits)
int wfs_copy_sum_signal(wfs_handle *h, int32_t *group, int64_t *left, int64_t *right, int64_t *data_off, int64_t *data, int64_t cap_rows, int64_t cap_samples)
try {
    if (!h || !run_complete(h)) return WFS_E_STATE;
    const WfsDev &d = h->dev;
    if (d.sum_channel < 0 || h->run.n_groups == 0) { if (cap_rows > 0 && data_off) data_off[0] = 0; return WFS_OK; }
    const i64 G = h->run.n_groups;
    const std::vector<i64> lo = download(h, h->sum_lo, (size_t)G), hi = download(h, h->sum_hi, (size_t)G), off = download(h, h->sum_off, (size_t)G + 1);
    std::vector<i32> acc((size_t)h->run.s_sum);
    if (h->run.s_sum) TRY(copy_out(h, acc.data(), h->raw.p() + h->run.sum_base, acc.size()));
    i64 k = 0, doff = 0;
    for (i64 g = 0; g < G; g++) {
        if (lo[g] == I64_MAX) continue;
        const RowSpan sp = row_span(lo[g], hi[g], d.tw); const i64 len = sp.len;
        if (k >= cap_rows || doff + len > cap_samples) return h->fail(WFS_E_CAPACITY, "sum signal buffer too small");
        group[k] = (i32)g; left[k] = sp.left; right[k] = sp.right; data_off[k] = doff;
        for (i64 i = 0; i < len; i++) data[doff + i] = (i64)acc[(size_t)(off[g] + i)] * d.he_factor;
        doff += len; k++;
    }
    if (k < cap_rows) data_off[k] = doff;
    return WFS_OK;
} WFS_CATCH(h)

// The noise model: one Walker table per channel from its probability mass function, all of one size (build_alias, the construction of
// the delay tables), sampled by the row kernels from the Philox word of the sample (wfs_device.h SITE_NOISE_SAMPLE).
// The three setters check and pack through wfs_noise.h, upload, and then move the state through its transitions.
static_assert(sizeof(NoiseCell) == sizeof(uint2) && sizeof(NoiseCell) == 2 * sizeof(u32) && offsetof(NoiseCell, y) == sizeof(u32) && alignof(NoiseCell) <= alignof(uint2),
              "the host's cells are uploaded as the uint2 {x, y} the kernels read");
// the alias cells of n_rows cumulative rows of n_values, appended to cells
static void append_alias_rows(const std::vector<double> &cum, i32 n_rows, i32 n_values, std::vector<NoiseCell> &cells, int &shift)
{
    std::vector<NoiseCell> cell;
    for (i32 r = 0; r < n_rows; r++) {
        build_alias(std::vector<double>(cum.begin() + (size_t)r * n_values, cum.begin() + (size_t)(r + 1) * n_values), cell, shift);
        cells.insert(cells.end(), cell.begin(), cell.end());
    }
}

int wfs_set_noise_model(wfs_handle *h, int32_t n_channels, int32_t n_values, int32_t vmin, const double *pmf)
try {
    if (!h) return WFS_E_INVALID;
    HIPCHK(hipSetDevice(h->device));
    TRY(pack_wait(h));          // (pending packers read the tables this call replaces)
    if (n_channels == 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        h->noise_moves(h->noise_state().model_cleared());
        h->lone.noise_hits = false;         // (no model, no value at an absolute sample: wfs_set_lone_noise_hits)
        refresh_dev(h);
        return WFS_OK;
    }
    std::vector<double> cum; std::string err;
    if (!noise_model_check(n_channels, h->cfg.n_rows, n_values, vmin, pmf, cum, err)) return h->fail(WFS_E_INVALID, err);
    std::vector<NoiseCell> cells; int shift = 31;
    append_alias_rows(cum, n_channels, n_values, cells, shift);
    const i32 K = (i32)(cells.size() / (size_t)n_channels);
    TRY(upload(h, h->nm_cells, cells.data(), cells.size()));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->noise_moves(h->noise_state().model_set(n_channels, K, shift, vmin, n_values, std::move(cells)));
    refresh_dev(h);             // (HE rows may appear or go with the model's channel count: run again before copying rows)
    return WFS_OK;
} WFS_CATCH(h)

int wfs_noise_model_samples(wfs_handle *h, int32_t channel, int64_t t0, int64_t n, int16_t *out)
try {
    if (!h) return WFS_E_INVALID;
    if (!h->noise.set()) return h->fail(WFS_E_STATE, "wfs_noise_model_samples: no noise model is set");
    if (channel < 0 || channel >= h->noise.channels) return h->fail(WFS_E_INVALID, "wfs_noise_model_samples: channel outside the model");
    return noise_probe(h, __func__, t0, n, out, [&](int16_t *buf) {
        const NoiseKind kind = noise_kind_of(h->dev);
        // (the coloured forms: a wave takes 256 samples)
        if (kind == NOISE_SLOW || kind == NOISE_COLOUR) return launch(h, K_NOISE_COLOUR_SAMPLES(kind == NOISE_SLOW), per_wave((n + 255) / 256), h->dev, channel, t0, n, buf);
        return launch(h, PLAIN(k_noise_model_samples), per_thread((n + 3) / 4), h->dev, channel, t0, n, buf);
    });
} WFS_CATCH(h)

// PMT dark counts (wfs_dark.h): the rates become the thresholds of the cells' Poisson counts, checked and computed by
// dark_check; the row kernels draw the photons where they finish a sample.  Rates that are all zero are the feature switched off.
int wfs_set_dark_counts(wfs_handle *h, int32_t n_channels, const double *rate_hz)
try {
    if (!h) return WFS_E_INVALID;
    HIPCHK(hipSetDevice(h->device));
    std::vector<u32> thr; std::string err;
    if (!dark_check(n_channels, h->cfg.n_tpc, rate_hz, h->cfg.dt, thr, err)) return h->fail(WFS_E_INVALID, err);
    TRY(pack_wait(h));          // (pending packers read the thresholds this call replaces)
    bool any = false;
    for (u32 t : thr) any = any || t != 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!any) { h->dark = DarkState{}; h->dk_thr.reset(); refresh_dev(h); return WFS_OK; }
    TRY(upload(h, h->dk_thr, thr.data(), thr.size()));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->dark = DarkState{}; h->dark.channels = n_channels; h->dark.thr = std::move(thr);
    refresh_dev(h);
    return WFS_OK;
} WFS_CATCH(h)

// the checks the three read-backs share; fn: the entry point, for the messages
static int dark_probe_check(wfs_handle *h, const char *fn, int32_t channel, int64_t t0, int64_t n)
{
    const std::string f = std::string(fn) + ": ";
    if (!h->dark.set()) return h->fail(WFS_E_STATE, f + "no dark-count rates are set");
    if (!h->tables_set) return h->fail(WFS_E_STATE, f + "tables not set");
    if (channel < 0 || channel >= h->dark.channels) return h->fail(WFS_E_INVALID, f + "channel outside the given rates");
    if (t0 < -((i64)1 << 48) || t0 > ((i64)1 << 48)) return h->fail(WFS_E_INVALID, f + "t0 beyond 2^48 in magnitude");
    if (n < 0 || n > ((i64)1 << 30)) return h->fail(WFS_E_INVALID, f + "n outside 0 .. 2^30");
    return WFS_OK;
}

int wfs_dark_count_samples(wfs_handle *h, int32_t channel, int64_t t0, int64_t n, int32_t *out)
try {
    if (!h) return WFS_E_INVALID;
    TRY(dark_probe_check(h, __func__, channel, t0, n));
    return noise_probe(h, __func__, t0, n, out, [&](i32 *buf) {
        return launch(h, PLAIN(k_dark_samples), per_wave((n + 255) / 256), h->dev, channel, t0, n, buf);
    });
} WFS_CATCH(h)

int wfs_dark_count_photons(wfs_handle *h, int32_t channel, int64_t t0, int64_t n, int64_t *t_ns, double *gain, int64_t capacity, int64_t *count)
try {
    if (!h) return WFS_E_INVALID;
    TRY(dark_probe_check(h, __func__, channel, t0, n));
    if (!count || capacity < 0 || (capacity > 0 && (!t_ns || !gain))) return h->fail(WFS_E_INVALID, "wfs_dark_count_photons: null count, negative capacity or null buffers");
    *count = 0;
    if (n == 0) return WFS_OK;
    HIPCHK(hipSetDevice(h->device));
    // a photon's start bin lies in its own cell: the cells of the samples t0 .. t0 + n - 1
    const i64 m0 = t0 >> DK_CELL_SHIFT, n_cells = ((t0 + n - 1) >> DK_CELL_SHIFT) - m0 + 1;
    DevArr<i32> d_cnt; DevArr<i64> d_t; DevArr<double> d_g;
    TRY(ensure(h, d_cnt, (size_t)n_cells)); TRY(ensure(h, d_t, (size_t)n_cells * DK_MAX)); TRY(ensure(h, d_g, (size_t)n_cells * DK_MAX));
    TRY(launch(h, PLAIN(k_dark_photons), per_thread(n_cells), h->dev, channel, m0, n_cells, d_cnt.p(), d_t.p(), d_g.p()));
    HIPCHK(hipGetLastError());
    std::vector<i32> cnt((size_t)n_cells); std::vector<i64> tt((size_t)n_cells * DK_MAX); std::vector<double> gg((size_t)n_cells * DK_MAX);
    TRY(copy_async(h, cnt.data(), d_cnt.p(), cnt.size(), hipMemcpyDeviceToHost));
    TRY(copy_async(h, tt.data(), d_t.p(), tt.size(), hipMemcpyDeviceToHost));
    TRY(copy_async(h, gg.data(), d_g.p(), gg.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(h->stream));
    CHECK_LAUNCHES();
    // time order: cells ascend, inside a cell a stable sort by time (equal times keep the order of j)
    const i64 dt = h->cfg.dt;
    i64 k = 0;
    for (i64 c = 0; c < n_cells; c++) {
        std::vector<std::pair<i64, double>> ph;
        for (int j = 0; j < cnt[(size_t)c] && j < DK_MAX; j++) {
            const i64 t = tt[(size_t)c * DK_MAX + j], idx = floordiv(t, dt);
            if (idx >= t0 && idx < t0 + n) ph.emplace_back(t, gg[(size_t)c * DK_MAX + j]);
        }
        std::stable_sort(ph.begin(), ph.end(), [](const std::pair<i64, double> &a, const std::pair<i64, double> &b) { return a.first < b.first; });
        for (const auto &q : ph) { if (k < capacity) { t_ns[k] = q.first; gain[k] = q.second; } k++; }
    }
    *count = k;
    if (k > capacity) return h->fail(WFS_E_CAPACITY, "wfs_dark_count_photons: " + std::to_string(k) + " photons, capacity " + std::to_string(capacity));
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_dark_counts(wfs_handle *h, int32_t channel, uint32_t thr[4])
try {
    if (!h || !thr) return WFS_E_INVALID;
    if (!h->dark.set()) return h->fail(WFS_E_STATE, "wfs_copy_dark_counts: no dark-count rates are set");
    if (channel < 0 || channel >= h->dark.channels) return h->fail(WFS_E_INVALID, "wfs_copy_dark_counts: channel outside the given rates");
    HIPCHK(hipSetDevice(h->device));
    const std::vector<u32> all = download(h, h->dk_thr, (size_t)h->dark.channels * DK_MAX);
    for (int k = 0; k < DK_MAX; k++) thr[k] = all[(size_t)channel * DK_MAX + k];
    return WFS_OK;
} WFS_CATCH(h)

// Lone-hit rows (wfs_lone.h): one pass over the starts [s0, s1) against the rows of the last wfs_run, or against no rows
// when none is finished.  The seeds: lone dark photons where rates are set, noise-hit seeds where wfs_set_lone_noise_hits is on.  Everything the pass writes is a buffer of wfs_handle::lone and a counter block of its own; of the run it
// reads the rows' ranges alone.  The work goes to the main stream behind the batch's packers.
static int lone_windows(wfs_handle *h, std::vector<i64> &wl, std::vector<i64> &wr, std::vector<i32> &wg)
{
    if (!run_finished(h) || h->run.n_groups == 0) return WFS_OK;
    const WfsDev &d = h->dev;
    const std::vector<i64> lo = download(h, h->grp_lo, (size_t)h->run.n_groups), hi = download(h, h->grp_hi, (size_t)h->run.n_groups);
    for (i64 g = 0; g < h->run.n_groups; g++) {
        if (lo[(size_t)g] == I64_MAX) continue;         // (a window without a pulse has no row)
        const RowSpan sp = full_row_span(lo[(size_t)g], hi[(size_t)g], d.tw);
        if (!wl.empty() && !lone_windows_apart(wr.back(), sp.left, d.tlen, d.tw))
            return h->fail(WFS_E_STATE, "wfs_lone_hits: two digitise windows of the last run lie within tlen + 2 tw samples of each other (right_raw_extension below (2 G + 64) dt)");
        wl.push_back(sp.left); wr.push_back(sp.right); wg.push_back((i32)g);
    }
    return WFS_OK;
}

// What crosses the stage boundaries of one wfs_lone_hits (on its stack).
struct LoneRun {
    LoneArgs a{}; ZleArgs za{}; WfsScal sc{}; i64 NK = 0, NR = 0, NREC = 0;      // (sc: the pass's counter block as last read; seeds, lone rows, records)
    bool photons = false, noise_hits = false; int kind = 0, noise_ch = 0;       // the seeds: dark photons, noise hits; the nk axis; PMT channels inside the model (noise hits)
};

// ---- lone 1: the seeds -- the windows of the run, the scans into a list (once more with room when it overflowed), the sort by (channel, start, kind)
static int lone_seeds(wfs_handle *h, LoneRun &r)
{
    const WfsDev &d = h->dev; auto &L = h->lone; LoneArgs &a = r.a;
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<i64> wl, wr; std::vector<i32> wg; TRY(lone_windows(h, wl, wr, wg));
    if (h->pack.must_wait()) HIPCHK(hipStreamWaitEvent(h->stream, h->rec_ready[h->pack.arena], 0));      // behind the batch's packers (the fence state stays as it is)
    TRY(upload(h, L.win_l, wl.data(), wl.size())); TRY(upload(h, L.win_r, wr.data(), wr.size())); TRY(upload(h, L.win_g, wg.data(), wg.size()));
    TRY(ensure(h, L.scal, 1)); a.scal = L.scal.p();
    a.a0 = a.s0 - lone_gap(d.tlen, d.tw); a.m0 = lone_first_cell(a.a0, d.samples_before); a.n_cells = lone_last_cell(a.s_limit, d.samples_before) - a.m0 + 1;
    a.n_blocks = r.noise_hits ? lone_noise_blocks(a.a0, a.s_limit) : 0;
    a.n_win = (i64)wl.size(); a.win_l = L.win_l.p(); a.win_r = L.win_r.p(); a.win_g = L.win_g.p(); a.row_lo = h->row_lo.p(); a.row_hi = h->row_hi.p();
    // the list: twice the expected photons of the scanned cells and room for a small pass; a pass that finds more is scanned again with
    // room (the number of noise hits cannot be had from the model cheaply: they come out of that room or out of the second scan)
    double expect = 0;
    for (int c = 0; c < h->dark.channels; c++) expect += (double)h->dark.thr[(size_t)c * DK_MAX] / 4294967296.0 * 1.2 * (double)a.n_cells;
    i64 cap = (i64)(2.0 * expect) + 4096;
    for (int attempt = 0; ; attempt++) {
        TRY(ensure_each(h, (size_t)cap, L.keys, L.keys2));
        a.keys = L.keys.p(); a.key_cap = cap;
        HIPCHK(hipMemsetAsync(L.scal.p(), 0, sizeof(WfsScal), h->stream));
        const i64 nb = (a.n_cells + LONE_SCAN_CELLS - 1) / LONE_SCAN_CELLS;
        if (nb > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, "wfs_lone_hits: lone hits: a pass of more than 2^39 cells per channel, split it");
        if (r.photons) TRY(launch(h, PLAIN(k_lone_scan), Shape(dim3((unsigned)nb, (unsigned)h->dark.channels), dim3(LONE_SCAN_CELLS)), d, a));
        if (r.noise_hits && r.noise_ch > 0 && a.n_blocks > 0)
            TRY(launch(h, K_LONE_NOISE_SCAN(r.kind - (int)NOISE_MODEL, r.photons), Shape(dim3((unsigned)((a.n_blocks + 3) / 4), (unsigned)r.noise_ch), dim3(256)), d, a));
        TRY(read_block(h, r.sc, L.scal.p()));
        if (r.sc.n_lone_seeds <= cap) break;
        if (attempt > 0) return h->fail(WFS_E_STATE, "wfs_lone_hits: internal: the seed list overflowed twice");
        cap = r.sc.n_lone_seeds;
    }
    const i64 NK = r.NK = a.n_keys = r.sc.n_lone_seeds; if (NK == 0) return WFS_OK;
    if (NK > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, "wfs_lone_hits: lone hits: more than 2^31 seeds (lone photons and noise hits) in one pass, split it");
    const unsigned end_bit = lone_key_end_bit(std::max(h->dark.channels, r.noise_ch));      // the key bits in use: of the channels that can have a seed
    TRY(two_step(h, "seed sort", [&](void *tmp, size_t &bytes) { return rocprim::radix_sort_keys(tmp, bytes, L.keys.p(), L.keys2.p(), (size_t)NK, 0u, end_bit, h->stream); }));
    a.keys = L.keys2.p();
    return WFS_OK;
}

// ---- lone 2: the rows -- chains of seeds, their places, descriptors and listing, and (k_row_empty: from there on like a batch's rows without a pulse) samples and intervals
static int lone_rows(wfs_handle *h, LoneRun &r)
{
    const WfsDev &d = h->dev; auto &L = h->lone; LoneArgs &a = r.a; ZleArgs &za = r.za; const i64 NK = r.NK;
    TRY(ensure_each(h, (size_t)NK, L.flag, L.cap, L.flen));
    a.flag = L.flag.p(); a.cap = L.cap.p(); a.flen = L.flen.p();
    TRY(launch(h, PLAIN(k_lone_rows), per_thread(NK), d, a));
    TRY(scan(h, L.flag.p(), NK, L.row_of, &WfsScal::n_lone_rows, L.scal.p()));
    TRY(scan(h, L.cap.p(), NK, L.itv_off, &WfsScal::n_itv_slots, L.scal.p()));
    TRY(scan(h, L.flen.p(), NK, L.fin_off, &WfsScal::n_empty_samples, L.scal.p()));
    TRY(read_block(h, r.sc, L.scal.p()));
    if (r.sc.lone_error) return h->fail(WFS_E_CAPACITY, "wfs_lone_hits: lone hits: a lone row of more than 2^19 samples (a chain of dark photons that long, or with noise hits on a baseline that stays across the threshold: lower the rate, the threshold or s_limit)");
    const i64 NR = r.NR = r.sc.n_lone_rows;
    if (NR > LONE_MAX_ROWS) return h->fail(WFS_E_CAPACITY, "wfs_lone_hits: lone hits: more than 2^24 lone rows in one pass, split it");
    if (NR == 0) return WFS_OK;
    TRY(ensure_each(h, (size_t)NR, L.desc, L.pdesc, L.out_channel, L.out_nph, L.out_nnz, L.out_left, L.out_right, L.out_ixr));
    TRY(ensure_each(h, (size_t)r.sc.n_itv_slots + 2, L.itv_left, L.itv_right));
    TRY(ensure_each(h, (size_t)NR, L.itv_n, L.row_nrec));
    TRY(ensure(h, L.fin, (size_t)r.sc.n_empty_samples + 8));
    FillGroup fg(h, "fills_lone");
    TRY(fg.zero(L.itv_n.p(), NR)); TRY(fg.zero(L.row_nrec.p(), NR));
    TRY(fg.fill(&L.scal.p()->key_origin, 1, I64_MAX)); TRY(fg.fill(&L.scal.p()->key_end, 1, I64_MIN));
    TRY(fg.flush());
    a.row_of = L.row_of.p(); a.itv_off = L.itv_off.p(); a.fin_off = L.fin_off.p();
    a.out_channel = L.out_channel.p(); a.out_nph = L.out_nph.p(); a.out_nnz = L.out_nnz.p(); a.out_left = L.out_left.p(); a.out_right = L.out_right.p(); a.out_ixr = L.out_ixr.p();
    TRY(launch(h, PLAIN(k_lone_desc), per_thread(NK), d, a, L.desc.p()));
    za.n_active_rows = NR; za.desc = L.desc.p(); za.fin = L.fin.p(); za.itv_left = L.itv_left.p(); za.itv_right = L.itv_right.p();
    za.itv_n = L.itv_n.p(); za.row_nrec = L.row_nrec.p(); za.spr = WFS_SPR; za.key_base = L.scal.p(); za.pdesc = L.pdesc.p();
    return launch(h, K_ROW_EMPTY(r.kind, r.photons), per_wave(NR), d, za, (i64)0, NR);
}

// ---- lone 3: the records -- how many, their order by (time, channel) and the packers, as run_records has them for the rows of a batch
static int lone_records(wfs_handle *h, LoneRun &r)
{
    auto &L = h->lone; ZleArgs &za = r.za;
    TRY(scan(h, L.row_nrec.p(), r.NR, L.rec_off, &WfsScal::n_records, L.scal.p()));
    TRY(read_block(h, r.sc, L.scal.p()));
    const i64 NREC = r.NREC = r.sc.n_records; L.n_rows = r.NR;
    if (NREC == 0) return WFS_OK;
    za.rec_off = L.rec_off.p(); za.rec_capacity = NREC;
    // (the order comes in front of the record arena: its count check is what a pass of too many records meets, whatever memory there is)
    if (NREC > 1) TRY(order_records(h, L.rec, za, r.NR, NREC, r.sc.key_origin, r.sc.key_end, "wfs_lone_hits: lone hits: more than 2^31 records in one pass, split it"));
    TRY(ensure(h, L.records_buf(), (size_t)NREC * WFS_RECORD_BYTES)); za.records = L.records_buf().as<uint8_t>();
    return pack_finished_rows(h, za, r.NR, L.fin.p(), 0, r.NR, h->stream);
}

int wfs_lone_hits(wfs_handle *h, int64_t s0, int64_t s1, int64_t s_limit, int64_t *n_records)
try {
    if (!h) return WFS_E_INVALID;
    if (!h->dark.set() && !h->lone.noise_hits) return h->fail(WFS_E_STATE, "wfs_lone_hits: no dark-count rates are set");
    if (!h->tables_set) return h->fail(WFS_E_STATE, "wfs_lone_hits: tables not set");
    if (!n_records) return h->fail(WFS_E_INVALID, "wfs_lone_hits: null n_records");
    const WfsDev &d = h->dev; auto &L = h->lone; LoneRun r;
    r.photons = h->dark.set(); r.noise_hits = L.noise_hits;
    r.kind = d.enable_noise ? (int)noise_kind_of(d) : (int)NOISE_NONE;
    if (r.noise_hits && r.kind < (int)NOISE_MODEL) return h->fail(WFS_E_STATE, "wfs_lone_hits: noise hits are on without a drawn noise model");
    r.noise_ch = r.noise_hits ? std::min((int)d.noise_channels, (int)d.n_tpc) : 0;
    std::string err;
    if (const int bad = lone_check(s0, s1, s_limit, h->dark.channels, d.tlen, d.tw, d.samples_before, err)) return h->fail(bad == 1 ? WFS_E_INVALID : WFS_E_CAPACITY, err);
    if (r.noise_hits) if (const int bad = lone_noise_check(s0, s_limit, d.tlen, d.tw, err)) return h->fail(bad == 1 ? WFS_E_INVALID : WFS_E_CAPACITY, err);
    HIPCHK(hipSetDevice(h->device)); L.n_rows = 0; L.n_records = 0; *n_records = 0;
    if (s1 == s0) return WFS_OK;
    r.a.s0 = s0; r.a.s1 = s1; r.a.s_limit = s_limit;
    TRY(lone_seeds(h, r));
    if (r.NK == 0) return WFS_OK;
    TRY(lone_rows(h, r));
    if (r.NR == 0) return WFS_OK;
    TRY(lone_records(h, r));
    TRY(pass_done(h));
    L.n_records = r.NREC; *n_records = r.NREC;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_lone_records(wfs_handle *h, void *dst, int64_t capacity)
try {
    if (!h) return WFS_E_INVALID;
    if (capacity < h->lone.n_records || (h->lone.n_records > 0 && !dst)) return h->fail(WFS_E_CAPACITY, "wfs_copy_lone_records: record buffer too small");
    HIPCHK(hipSetDevice(h->device));
    if (h->lone.n_records) HIPCHK(hipMemcpy(dst, h->lone.records_buf().p, (size_t)h->lone.n_records * WFS_RECORD_BYTES, hipMemcpyDeviceToHost));
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_lone_rows(wfs_handle *h, int32_t *channel, int64_t *left, int64_t *right, int64_t *ix_rand, int32_t *n_photons, int64_t capacity, int64_t *count)
try {
    if (!h || !count) return WFS_E_INVALID;
    const i64 n = h->lone.n_rows;
    *count = n;
    if (capacity < n) return h->fail(WFS_E_CAPACITY, "wfs_copy_lone_rows: " + std::to_string(n) + " lone rows, capacity " + std::to_string(capacity));
    if (n == 0) return WFS_OK;
    if (!channel || !left || !right || !ix_rand || !n_photons) return h->fail(WFS_E_INVALID, "wfs_copy_lone_rows: null buffers");
    HIPCHK(hipSetDevice(h->device));
    auto &L = h->lone;
    TRY(copy_out(h, channel, L.out_channel.p(), (size_t)n)); TRY(copy_out(h, n_photons, L.out_nph.p(), (size_t)n));
    TRY(copy_out(h, left, L.out_left.p(), (size_t)n)); TRY(copy_out(h, right, L.out_right.p(), (size_t)n)); TRY(copy_out(h, ix_rand, L.out_ixr.p(), (size_t)n));
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_lone_row_noise_hits(wfs_handle *h, int32_t *n_noise_hits, int64_t capacity, int64_t *count)
try {
    if (!h || !count) return WFS_E_INVALID;
    const i64 n = h->lone.n_rows;
    *count = n;
    if (capacity < n) return h->fail(WFS_E_CAPACITY, "wfs_copy_lone_row_noise_hits: " + std::to_string(n) + " lone rows, capacity " + std::to_string(capacity));
    if (n == 0) return WFS_OK;
    if (!n_noise_hits) return h->fail(WFS_E_INVALID, "wfs_copy_lone_row_noise_hits: null buffer");
    HIPCHK(hipSetDevice(h->device));
    TRY(copy_out(h, n_noise_hits, h->lone.out_nnz.p(), (size_t)n));
    return WFS_OK;
} WFS_CATCH(h)

// The overlay pass (wfs_overlay.h): the records of two streams merged per channel into one valid stream in (time, channel)
// order.  A: sim_host, or the records of the last wfs_run where they lie; B: bg_host.  Everything the pass writes is a buffer of
// wfs_handle::overlay; of the run it reads the record arena alone.  The work goes to the main stream behind the batch's packers.
// What crosses the stage boundaries of one wfs_overlay_records (on its stack); records, pulses, merged pulses, output records: a's n, n_pulses, n_merged, n_out
struct OverlayRun { OverlayArgs a{}; OverlayScal sc{}; int key_bits = 0; };      // (sc: the counter block as last read; key_bits: of the record and pulse keys)
static int overlay_invalid(wfs_handle *h, const OverlayRun &r)
{
    const i64 i = (i64)(r.sc.first_bad >> 8);
    return h->fail(WFS_E_INVALID, std::string("wfs_overlay_records: ") + (i < r.a.n_a ? "simulated record " + std::to_string(i) : "background record " + std::to_string(i - r.a.n_a)) + ": " +
                   ov_bad_name((int)(r.sc.first_bad & 0xffu)) + " (" + std::to_string(r.sc.n_bad) + " records in all)");
}
// ---- overlay 1: the two streams and the recorded baselines on the device, every record checked on its own (k_ov_check), the key bits
static int overlay_load(wfs_handle *h, OverlayRun &r, const void *sim_host, const void *bg_host, const int32_t *bg_baseline)
{
    auto &O = h->overlay; OverlayArgs &a = r.a;
    if (h->pack.must_wait()) HIPCHK(hipStreamWaitEvent(h->stream, h->rec_ready[h->pack.arena], 0));      // behind the batch's packers (the fence state stays as it is)
    if (sim_host) { TRY(upload(h, O.src_a, (const u32 *)sim_host, (size_t)a.n_a * REC_DWORDS)); a.src_a = O.src_a.p(); }
    else a.src_a = (const u32 *)h->records_buf().p;
    TRY(upload(h, O.src_b, (const u32 *)bg_host, (size_t)(a.n - a.n_a) * REC_DWORDS)); a.src_b = O.src_b.p();
    std::vector<i32> base((size_t)a.n_rows, a.baseline);
    if (bg_baseline) base.assign(bg_baseline, bg_baseline + a.n_rows);
    TRY(upload(h, O.base, base.data(), base.size())); a.base = O.base.p();
    HIPCHK(hipStreamSynchronize(h->stream));                // (the copy reads host memory that is a local)
    TRY(ensure(h, O.scal, 1)); a.scal = O.scal.p();
    r.sc = OverlayScal{}; r.sc.smin = I64_MAX; r.sc.smax = I64_MIN; r.sc.first_bad = ~0ull;
    TRY(copy_async(h, O.scal.p(), &r.sc, 1, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(h->stream));                // (sc is written below)
    TRY(launch(h, PLAIN(k_ov_check), per_thread(a.n), a));
    TRY(read_block(h, r.sc, O.scal.p()));
    if (r.sc.n_bad) return overlay_invalid(h, r);
    a.smin = r.sc.smin; a.bits.sbits = ov_bits_of((u64)r.sc.smax - (u64)r.sc.smin + 1ull); a.bits.chbits = ov_bits_of((u64)std::max(a.n_rows - 1, 1));
    if (!ov_bits_fit(a.bits)) return h->fail(WFS_E_CAPACITY, "wfs_overlay_records: overlay: the records span more samples than the sort keys hold beside the channel (2^" + std::to_string(63 - a.bits.chbits) + "), split the pass");
    r.key_bits = a.bits.sbits + a.bits.chbits + 1; return WFS_OK;
}

// ---- overlay 2: records to pulses -- the records by (stream, channel, time), each against the one in front (k_ov_valid), a pulse per first fragment
static int overlay_pulses(wfs_handle *h, OverlayRun &r)
{
    auto &O = h->overlay; OverlayArgs &a = r.a; const i64 N = a.n;
    TRY(ensure_each(h, (size_t)N, O.key, O.key2, O.val, O.val2, O.flag, O.pulse_of));
    a.key = O.key.p(); a.val = O.val.p();
    TRY(launch(h, PLAIN(k_ov_keys), per_thread(N), a));
    TRY(sort_pairs(h, "overlay record sort", O.key.p(), O.key2.p(), O.val.p(), O.val2.p(), N, (unsigned)r.key_bits));
    a.key = O.key2.p(); a.val = O.val2.p(); a.flag = O.flag.p();
    TRY(launch(h, PLAIN(k_ov_valid), per_thread(N), a));
    TRY(scan_inclusive(h, "overlay pulse scan", O.flag.p(), O.pulse_of.p(), N, rocprim::plus<i32>()));
    a.pulse_of = O.pulse_of.p(); i32 n_pulses = 0;
    TRY(read_block(h, r.sc, O.scal.p(), n_pulses, O.pulse_of.p() + (N - 1)));
    if (r.sc.n_bad) return overlay_invalid(h, r);
    if ((a.n_pulses = n_pulses) <= 0) return h->fail(WFS_E_STATE, "wfs_overlay_records: internal: valid records without a pulse");
    return WFS_OK;
}

// ---- overlay 3: pulses to merged pulses -- the pulses by (channel, start, stream), the running maximum of their ends, a merged pulse per head
static int overlay_merge(wfs_handle *h, OverlayRun &r)
{
    auto &O = h->overlay; OverlayArgs &a = r.a; const i64 N = a.n, P = a.n_pulses;
    TRY(ensure_each(h, (size_t)P, O.pkey, O.pkey2, O.plen, O.plen2, O.ekey, O.run_max, O.head, O.merged_of));
    a.pkey = O.pkey.p(); a.plen = O.plen.p();
    TRY(launch(h, PLAIN(k_ov_pulses), per_thread(N), a));
    TRY(sort_pairs(h, "overlay pulse sort", O.pkey.p(), O.pkey2.p(), O.plen.p(), O.plen2.p(), P, (unsigned)r.key_bits));
    a.pkey = O.pkey2.p(); a.plen = O.plen2.p(); a.ekey = O.ekey.p();
    TRY(launch(h, PLAIN(k_ov_ends), per_thread(P), a));
    TRY(scan_inclusive(h, "overlay end scan", O.ekey.p(), O.run_max.p(), P, rocprim::maximum<u64>()));
    a.run_max = O.run_max.p(); a.head = O.head.p();
    TRY(launch(h, PLAIN(k_ov_heads), per_thread(P), a));
    TRY(scan_inclusive(h, "overlay head scan", O.head.p(), O.merged_of.p(), P, rocprim::plus<i32>()));
    a.merged_of = O.merged_of.p(); i32 n_merged = 0;
    TRY(read_block(h, n_merged, O.merged_of.p() + (P - 1)));
    const i64 M = a.n_merged = n_merged;
    if (M <= 0 || M > P) return h->fail(WFS_E_STATE, "wfs_overlay_records: internal: the merged pulses do not follow from the pulses");
    TRY(ensure_each(h, (size_t)M, O.m_first, O.m_last, O.m_nrec, O.rec_end));
    a.m_first = O.m_first.p(); a.m_last = O.m_last.p(); a.m_nrec = O.m_nrec.p();
    return launch(h, PLAIN(k_ov_merged), per_thread(P), a);
}

// ---- overlay 4: the output records -- how many per merged pulse, their keys, the sort by (time, channel), each filled in its sorted slot
static int overlay_output(wfs_handle *h, OverlayRun &r)
{
    auto &O = h->overlay; OverlayArgs &a = r.a; const i64 M = a.n_merged;
    TRY(launch(h, PLAIN(k_ov_count), per_thread(M), a));
    TRY(scan_inclusive(h, "overlay record scan", O.m_nrec.p(), O.rec_end.p(), M, rocprim::plus<i64>()));
    a.rec_end = O.rec_end.p(); i64 n_out = 0;
    TRY(read_block(h, r.sc, O.scal.p(), n_out, O.rec_end.p() + (M - 1)));
    if (r.sc.too_long) return h->fail(WFS_E_CAPACITY, "wfs_overlay_records: overlay: a merged pulse of more than 2^31 - 1 samples");
    if (n_out > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, "wfs_overlay_records: overlay: more than 2^31 records come out of one pass, split it");
    const i64 NO = a.n_out = n_out;
    if (NO <= 0) return h->fail(WFS_E_STATE, "wfs_overlay_records: internal: merged pulses without a record");
    TRY(ensure_each(h, (size_t)NO, O.okey, O.okey2, O.oval, O.oval2)); TRY(ensure(h, O.out, (size_t)NO * REC_DWORDS));
    a.okey = O.okey.p(); a.oval = O.oval.p();
    TRY(launch(h, PLAIN(k_ov_out_keys), per_thread(M), a));
    TRY(sort_pairs(h, "overlay output sort", O.okey.p(), O.okey2.p(), O.oval.p(), O.oval2.p(), NO, (unsigned)(a.bits.sbits + a.bits.chbits)));
    a.okey = O.okey2.p(); a.oval = O.oval2.p(); a.out = O.out.p();
    return launch(h, PLAIN(k_ov_fill), per_wave(NO), a);
}

int wfs_overlay_records(wfs_handle *h, const void *sim_host, int64_t n_sim, const void *bg_host, int64_t n_bg, const int32_t *bg_baseline, int64_t *n_records)
try {
    if (!h) return WFS_E_INVALID;
    if (!n_records) return h->fail(WFS_E_INVALID, "wfs_overlay_records: null n_records");
    if (n_bg < 0 || (n_bg > 0 && !bg_host)) return h->fail(WFS_E_INVALID, "wfs_overlay_records: n_bg is negative or bg_host is null");
    if (sim_host && n_sim < 0) return h->fail(WFS_E_INVALID, "wfs_overlay_records: n_sim is negative");
    if (!sim_host && !run_finished(h)) return h->fail(WFS_E_STATE, "wfs_overlay_records: no simulated records: wfs_run has not completed and sim_host is null");
    const WfsDev &d = h->dev; auto &O = h->overlay;
    if (!sim_host && n_sim > h->run.n_records) return h->fail(WFS_E_INVALID, "wfs_overlay_records: n_sim beyond the records of the last run");
    const i64 NA = sim_host ? n_sim : (n_sim < 0 ? h->run.n_records : n_sim), N = NA + n_bg;
    O.n_records = 0; *n_records = 0;
    if (NA > 0x7fffffffLL || n_bg > 0x7fffffffLL || N > 0x7fffffffLL) return h->fail(WFS_E_CAPACITY, "wfs_overlay_records: overlay: more than 2^31 records in one pass, split it");
    if (N == 0) return WFS_OK;
    HIPCHK(hipSetDevice(h->device));
    OverlayRun r; r.a.n_a = NA; r.a.n = N; r.a.dt = (i32)d.dt; r.a.n_rows = (i32)h->cfg.n_rows; r.a.baseline = (i32)d.baseline;
    TRY(overlay_load(h, r, sim_host, bg_host, bg_baseline));
    TRY(overlay_pulses(h, r));
    TRY(overlay_merge(h, r));
    TRY(overlay_output(h, r));
    TRY(pass_done(h));
    O.n_records = r.a.n_out; *n_records = r.a.n_out;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_overlay_records(wfs_handle *h, void *dst, int64_t capacity_records)
try {
    if (!h) return WFS_E_INVALID;
    if (capacity_records < h->overlay.n_records || (h->overlay.n_records > 0 && !dst)) return h->fail(WFS_E_CAPACITY, "wfs_copy_overlay_records: record buffer too small");
    HIPCHK(hipSetDevice(h->device));
    if (h->overlay.n_records) HIPCHK(hipMemcpy(dst, h->overlay.out.p(), (size_t)h->overlay.n_records * WFS_RECORD_BYTES, hipMemcpyDefault));
    return WFS_OK;
} WFS_CATCH(h)

// Noise-hit seeds of the lone-hit passes (include/wfsim_amd.h).  The switch changes nothing a run lays out: no packer is waited for.
int wfs_set_lone_noise_hits(wfs_handle *h, int32_t on)
try {
    if (!h) return WFS_E_INVALID;
    if (on) {
        if (!h->noise.set()) return h->fail(WFS_E_STATE, "wfs_set_lone_noise_hits: no drawn noise model is set (wfs_set_noise_model; a noise table has no value at an absolute sample)");
        if (!h->cfg.enable_noise) return h->fail(WFS_E_STATE, "wfs_set_lone_noise_hits: enable_noise is off");
    }
    h->lone.noise_hits = on != 0;
    return WFS_OK;
} WFS_CATCH(h)

// The colour of the noise model: FIR taps per stream and common streams shared by groups of channels.  Everything the
// kernels rely on is checked in noise_colour_pack: the tap count, the bound that keeps the int32 sums of the kernels exact, groups and gains.
int wfs_set_noise_colour(wfs_handle *h, int32_t n_taps, const int32_t *taps_q, int32_t n_groups, const int32_t *group, const int32_t *mix_q, const double *common_pmf)
try {
    if (!h) return WFS_E_INVALID;
    const NoiseModelState &m = h->noise;
    if (!m.set()) return h->fail(WFS_E_STATE, "wfs_set_noise_colour: no noise model is set");
    HIPCHK(hipSetDevice(h->device));
    TRY(pack_wait(h));          // (pending packers read the tables this call replaces)
    if (n_taps == 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        // (the cells of the common streams leave the device with them)
        if (m.colour.groups > 0) { TRY(upload(h, h->nm_cells, m.cells.data(), m.cells.size())); HIPCHK(hipStreamSynchronize(h->stream)); }
        h->noise_moves(h->noise_state().colour_cleared());
        refresh_dev(h);
        return WFS_OK;
    }
    std::vector<i32> buf; std::vector<i64> tapsum; std::vector<double> cum; std::string err;
    if (!noise_colour_pack(m, n_taps, taps_q, n_groups, group, mix_q, common_pmf, buf, tapsum, cum, err)) return h->fail(WFS_E_INVALID, err);
    std::vector<NoiseCell> cells(m.cells); int shift = 31;
    append_alias_rows(cum, n_groups, m.values, cells, shift);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (n_groups > 0 || m.colour.groups > 0) TRY(upload(h, h->nm_cells, cells.data(), cells.size()));
    TRY(upload(h, h->nc_buf, buf.data(), buf.size()));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->noise_moves(h->noise_state().colour_set(n_taps, n_groups, std::move(tapsum)));
    refresh_dev(h);
    return WFS_OK;
} WFS_CATCH(h)

// The slow levels of the noise model: interpolated knot sequences per stream, octaves apart.  The bound of the colour with
// the slow amplitudes added (noise_slow_pack) keeps every int32 sum of the kernels exact.
int wfs_set_noise_slow(wfs_handle *h, int32_t n_levels, const int32_t *shifts, const int32_t *slow_q)
try {
    if (!h) return WFS_E_INVALID;
    if (!h->noise.set()) return h->fail(WFS_E_STATE, "wfs_set_noise_slow: no noise model is set");
    HIPCHK(hipSetDevice(h->device));
    TRY(pack_wait(h));          // (pending packers read the tables this call replaces)
    if (n_levels == 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        h->noise_moves(h->noise_state().slow_cleared());
        refresh_dev(h);
        return WFS_OK;
    }
    std::vector<i32> buf; std::string err;
    if (!noise_slow_pack(h->noise, n_levels, shifts, slow_q, buf, err)) return h->fail(WFS_E_INVALID, err);
    HIPCHK(hipStreamSynchronize(h->stream));
    TRY(upload(h, h->ns_buf, buf.data(), buf.size()));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->noise_moves(h->noise_state().slow_set(n_levels));
    refresh_dev(h);
    return WFS_OK;
} WFS_CATCH(h)

int wfs_noise_slow_samples(wfs_handle *h, int32_t row, int64_t t0, int64_t n, int32_t *out)
try {
    if (!h) return WFS_E_INVALID;
    if (h->noise.levels() <= 0) return h->fail(WFS_E_STATE, "wfs_noise_slow_samples: no noise model with slow levels is set");
    if (row < 0 || row >= h->noise.rows()) return h->fail(WFS_E_INVALID, "wfs_noise_slow_samples: row outside the model's channels and common streams");
    return noise_probe(h, __func__, t0, n, out, [&](int32_t *buf) {
        return launch(h, PLAIN(k_noise_slow_samples), per_wave((n + 255) / 256), h->dev, row, t0, n, buf);
    });
} WFS_CATCH(h)

int wfs_noise_white_samples(wfs_handle *h, int32_t row, int64_t t0, int64_t n, int16_t *out)
try {
    if (!h) return WFS_E_INVALID;
    if (!h->noise.set()) return h->fail(WFS_E_STATE, "wfs_noise_white_samples: no noise model is set");
    if (row < 0 || row >= h->noise.rows()) return h->fail(WFS_E_INVALID, "wfs_noise_white_samples: row outside the model's channels and common streams");
    return noise_probe(h, __func__, t0, n, out, [&](int16_t *buf) {
        return launch(h, PLAIN(k_noise_white_samples), per_thread(n), h->dev, row, t0, n, buf);
    });
} WFS_CATCH(h)

int wfs_copy_noise_model(wfs_handle *h, int32_t channel, uint32_t *thr, uint32_t *alias, int32_t capacity_cells, int32_t *n_cells, int32_t *shift, int32_t *vmin)
try {
    if (!h) return WFS_E_INVALID;
    const NoiseModelState &m = h->noise;
    if (!m.set()) return h->fail(WFS_E_STATE, "wfs_copy_noise_model: no noise model is set");
    if (channel < 0 || channel >= m.channels) return h->fail(WFS_E_INVALID, "wfs_copy_noise_model: channel outside the model");
    if (!thr || !alias || !n_cells || !shift || !vmin) return h->fail(WFS_E_INVALID, "wfs_copy_noise_model: null argument");
    if (capacity_cells < m.k) return h->fail(WFS_E_CAPACITY, "wfs_copy_noise_model: cell buffers too small");
    HIPCHK(hipSetDevice(h->device));
    std::vector<NoiseCell> cell((size_t)m.k);            // what the device samples from, not the host copy
    TRY(copy_out(h, cell.data(), h->nm_cells.p() + (size_t)channel * m.k, cell.size()));
    for (i32 k = 0; k < m.k; k++) { thr[k] = cell[(size_t)k].x; alias[k] = cell[(size_t)k].y; }
    *n_cells = m.k; *shift = m.shift; *vmin = m.vmin;
    return WFS_OK;
} WFS_CATCH(h)

int wfs_copy_tile_kernels(wfs_handle *h, int8_t *kind, int64_t capacity)
try {
    if (!h || !run_finished(h)) return WFS_E_STATE;
    if (!kind) return h->fail(WFS_E_INVALID, "wfs_copy_tile_kernels: null argument");
    const i64 TP = (from_generator(h) ? h->batch.n_psets : h->batch.n_sets) * h->cfg.n_tpc;      // (a batch of loaded photons has primary sets only)
    if (capacity < TP) return h->fail(WFS_E_CAPACITY, "tile kernel buffer too small");
    if (!from_generator(h) || !h->run.fuse_on || TP == 0) { memset(kind, 0, (size_t)TP); return WFS_OK; }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    TRY(copy_out(h, kind, h->tile_kind.p(), (size_t)TP));
    return WFS_OK;
} WFS_CATCH(h)

int wfs_kernel_times(wfs_handle *h, char *names, int64_t names_cap, float *ms, int32_t *n_launches, int32_t *n_kernels)
try {
    if (!h) return WFS_E_INVALID;
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<std::string> uniq; std::vector<float> tot; std::vector<int> cnt;
    for (auto &t : h->times) {
        float m = 0; hipEventElapsedTime(&m, t.a, t.b);
        size_t k = 0; for (; k < uniq.size(); k++) if (uniq[k] == t.name) break;
        if (k == uniq.size()) { uniq.push_back(t.name); tot.push_back(0); cnt.push_back(0); }
        tot[k] += m; cnt[k]++;
    }
    i64 pos = 0;
    for (size_t k = 0; k < uniq.size(); k++) {
        if (pos + (i64)uniq[k].size() + 1 > names_cap) return h->fail(WFS_E_CAPACITY, "names buffer too small");
        memcpy(names + pos, uniq[k].c_str(), uniq[k].size() + 1); pos += (i64)uniq[k].size() + 1;
        ms[k] = tot[k]; n_launches[k] = cnt[k];
    }
    *n_kernels = (int32_t)uniq.size();
    return WFS_OK;
} WFS_CATCH(h)

}  // extern "C"
