// Two kinds of facts that the kernels and the host must agree on, each written once:
//
//  * the dynamic-LDS layout of every kernel that has one: a struct of byte offsets plus `total`, filled by one function of exactly the
//    parameters the sizes depend on.  The kernel takes its pointers from the layout, its launch passes layout.total, and wfs_create
//    grants a cap that the largest total is checked against.  Offsets are plain integers: a pointer that went through an integer cast
//    loses its LDS address space.  Every total is what the launch sites reserved before the layouts existed; where that was more than
//    the kernel carves, the excess is a member `slack` -- unused, kept so that no workgroup's LDS allocation moves.
//  * the sample window of a tile and the meaning of a row slot (tile_window, row_slot, row_span): the rule of the device kernels, of the
//    debug offsets a run uploads and of the offsets the copy functions hand out.
//
// No HIP types: tests/host/layout_main.cpp compiles this header with the host compiler.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define WFS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define WFS_HD inline
#endif

typedef long long i64;        // (as wfs_device.h has them)
typedef int i32;
typedef unsigned int u32;

// ---- the sizes the layouts are made of ---------------------------------------------------------------------------------------------
#define WFS_MAX_CH 1024          // channels that fit the LDS histograms of the bucketing kernels
#define WFS_DT 10                // sample_duration [ns] of the specialised kernels; wfs_create rejects anything else for them
constexpr int TILE_TLEN = 22;        // samples of a photon's pulse template: a live sample sees TILE_TLEN start bins
#define WFS_MAX_DT 16            // any digitiser geometry (k_pulse_generic): sample_duration and template length it accepts
#define WFS_MAX_TLEN 256
constexpr int SPE_BINS = 2000, SPE_ROW_LEN = SPE_BINS + 1;
#define TAP_W2_LEN (22 * WFS_DT + 2)   // tap_block: taps by time difference, the zero tap behind them
#define TAP_LIST_LEN 64                // entries of a wave's list (unsigned short): one per lane
#define SPARSE_MAX_PHOTONS 32      // tiles with a handful of photons (S1-like) go to the sorted-list kernel
#define SPARSE_MAX_BINS 64
#define SPARSE_PPT 16              // photons per thread held in registers: tile photons <= TPB * SPARSE_PPT
constexpr int SPARSE_TPB = 64;         // the one form of k_pulse_sparse: the class limits fit it
constexpr int SPARSE_TREP = 260;       // doubles of one template copy of k_pulse_sparse (rows padded to 24, 4 bank pairs of offset)
#define PW_U 2                     // pad photons behind a wave's list (wave_tile_pulse reads PW_U per trip)
#define WAVE_TZ_LEN (WFS_DT * (22 + 2))    // templates[r][k] with a zero tap in front of and behind every row
constexpr int WAVE_PHOTON_BYTES = 16;      // sizeof(WavePhoton), asserted beside the struct
#define RES_SHORT_LEN 768          // resident rows up to this length: 4 waves x 3 KB of LDS per workgroup, eight workgroups per CU
constexpr int RES_MAX_LEN = 7168;      // longest region of a wave of k_row_pulse (the long form)
#define WFS_TILE_CHUNK 256          // samples of a tile gathered per pass (<= 256: one per thread); the H table holds WFS_TILE_CHUNK + 21 start bins
#define AP_STAGE 128               // afterpulse candidates a block parks in LDS (48 bytes each; a block of 2048 photons has ~60)
constexpr int AP_CAND_BYTES = 48;          // sizeof(ApCand), asserted beside the struct
constexpr int AP_STAGE_BYTES = AP_STAGE * AP_CAND_BYTES;
#define BRIGHT_LDS_MAX (128 * 1024)        // most bytes of H table + ballots of k_s2_bright, whatever the device grants
#define BRIGHT_SPE_BYTES ((SPE_ROW_LEN + 1) * 8)       // the channel's SPE row beside them
constexpr int BRIGHT_STATIC_RESERVE = 2048;            // what wfs_create leaves for the static arrays of k_s2_bright
#ifndef GEN_LOG
#define GEN_LOG 11
#endif
#define GEN_BLOCK (1 << GEN_LOG)   // photons per block of the generator
#define GEN_WIN 512                // emitter offsets staged in LDS per block
#define TILE_ORDER_MAX 4096        // photons of a range that a workgroup orders in LDS (k_tile_order_big)

// the dynamic-LDS caps wfs_create asks for (hipFuncAttributeMaxDynamicSharedMemorySize), in bytes
constexpr int LDS_CAP_PULSE = 100 * 1024, LDS_CAP_SPARSE = 100 * 1024, LDS_CAP_GENERIC = 128 * 1024, LDS_CAP_TILE = 100 * 1024;
constexpr int LDS_CAP_ROW = 128 * 1024, LDS_CAP_FILL = 100 * 1024, LDS_CAP_ORDER = 100 * 1024;

constexpr int lds_round16(int bytes) { return (bytes + 15) / 16 * 16; }

// ---- tap_block: [TAP_W2_LEN doubles][waves][TAP_LIST_LEN] unsigned short; the lists follow W2 directly (tap_block finds them there)
constexpr int TAP_LISTS_OFF = TAP_W2_LEN * 8;
constexpr int tap_lds_bytes(int waves) { return TAP_LISTS_OFF + waves * TAP_LIST_LEN * 2; }

// ---- k_pulse<TPB, ..> (dense tiles, 10 ns / 22 taps)
struct PulseLds {
    int H;          // double[TPB + 21][dt], align 16 (read as double2): merged gain per (start bin, ns remainder)
    int red;        // double[TPB / 64][8], align 8
    int wsum;       // u32[16], align 4
    int W2;         // tap_block's tables for TPB / 64 waves, align 8
    int slack;      // unused: the lists of the waves a 128-thread workgroup does not have, and 16 bytes
    int total;
};
constexpr PulseLds pulse_lds(int tpb)
{
    PulseLds o{};
    o.H = 0;
    o.red = o.H + (tpb + TILE_TLEN - 1) * WFS_DT * 8;
    o.wsum = o.red + 8 * (tpb / 64) * 8;
    o.W2 = o.wsum + 16 * 4;
    o.slack = o.W2 + tap_lds_bytes(tpb / 64);
    o.total = lds_round16(o.slack + (tap_lds_bytes(256 / 64) - tap_lds_bytes(tpb / 64)) + 16);
    return o;
}

// ---- k_pulse_sparse<SPARSE_TPB, ..>: NP photons (multiple of 8), W start bins (multiple of 8), 10 ns
struct SparseLds {
    int cg;         // double[NP], align 8: merged gain of the sorted photons
    int red;        // double[TPB / 64][8], align 8
    int ctoff;      // i32[NP], align 4
    int boff;       // u16[dt W + 4], align 2: exclusive offsets per ns
    int wsum;       // u32[8], align 4
    int cnt;        // align 8: first u32[dt W / 2] packed u16 pairs (photons per ns), later double[SPARSE_TREP] (a template copy): the larger
    int slack;      // unused: 24 bytes
    int total;
};
constexpr SparseLds sparse_lds(int NP, int W, int tpb)
{
    SparseLds o{};
    o.cg = 0;
    o.red = o.cg + NP * 8;
    o.ctoff = o.red + 8 * (tpb / 64) * 8;
    o.boff = o.ctoff + NP * 4;
    o.wsum = o.boff + ((WFS_DT * W + 2 + 3) & ~3) * 2;
    o.cnt = o.wsum + 8 * 4;
    o.slack = o.cnt + (WFS_DT * W * 2 > SPARSE_TREP * 8 ? WFS_DT * W * 2 : SPARSE_TREP * 8);
    o.total = lds_round16(o.slack + 24);
    return o;
}

// ---- k_pulse_generic<256, ..>: any dt <= WFS_MAX_DT, tlen <= WFS_MAX_TLEN; split: two H tables (order-independent merge)
struct GenericLds {
    int H;          // double[256 + tlen - 1][dt], align 8
    int Hlo;        // the same again, align 8 (split only; no bytes otherwise)
    int T;          // double[dt][tlen] templates, align 8
    int red;        // double[4][8], align 8
    int slack;      // unused: 64 bytes
    int total;
};
constexpr GenericLds generic_lds(int dt, int tlen, bool split)
{
    GenericLds o{};
    o.H = 0;
    o.Hlo = o.H + (256 + tlen - 1) * dt * 8;
    o.T = o.Hlo + (split ? (256 + tlen - 1) * dt * 8 : 0);
    o.red = o.T + dt * tlen * 8;
    o.slack = o.red + 4 * 8 * 8;
    o.total = lds_round16(o.slack + 64);
    return o;
}
// two tables where they fit the cap, one otherwise; a geometry whose single table does not fit is refused by the run
constexpr bool generic_lds_split(int dt, int tlen) { return generic_lds(dt, tlen, true).total <= LDS_CAP_GENERIC; }

// ---- k_s2_tile<AP, FMA>
struct TileLds {
    int H;          // double[WFS_TILE_CHUNK + 21][dt], align 16; before the chunks: the channel's SPE row, then the truth partial sums
    int wsum;       // u32[16], align 4
    int W2;         // tap_block's tables for 4 waves, align 8 (the exact form; no bytes in the fused form, which gathers densely)
    int slack;      // unused: 64 bytes in the exact form, 16 in the fused form
    int ap;         // ApCand[AP_STAGE], align 16 (AP forms; no bytes otherwise)
    int total;
};
constexpr TileLds tile_lds(bool fma, bool ap)
{
    TileLds o{};
    o.H = 0;
    o.wsum = o.H + (WFS_TILE_CHUNK + TILE_TLEN - 1) * WFS_DT * 8;
    o.W2 = o.wsum + 16 * 4;
    o.slack = o.W2 + (fma ? 0 : tap_lds_bytes(4));
    o.ap = lds_round16(o.slack + (fma ? 16 : 64));
    o.total = o.ap + (ap ? AP_STAGE_BYTES : 0);
    return o;
}

// ---- k_s2_tile_gen<AP>: the afterpulse stage alone
struct TileGenLds { int ap /* ApCand[AP_STAGE], align 16 */, total; };
constexpr TileGenLds tile_gen_lds(bool ap) { return TileGenLds{0, ap ? AP_STAGE_BYTES : 0}; }

// ---- k_s2_bright<AP, ..>: bright_lds bytes (multiple of 16) of H table and ballots
struct BrightLds {
    int H;          // double[rows][dt] then u64 ballots, align 16: bright_lds bytes for both (bright_fits)
    int spe;        // double[SPE_ROW_LEN + 1], align 8: the channel's SPE row
    int ap;         // ApCand[AP_STAGE], align 16 (AP forms)
    int total;
};
constexpr BrightLds bright_lds_layout(int bright_lds, bool ap)
{
    BrightLds o{};
    o.H = 0;
    o.spe = o.H + bright_lds;
    o.ap = o.spe + BRIGHT_SPE_BYTES;
    o.total = o.ap + (ap ? AP_STAGE_BYTES : 0);
    return o;
}
// bytes a bright tile may take for H table and ballots on a device that grants `granted` bytes to a workgroup: what is left beside the
// SPE row, the afterpulse stage and the kernel's static arrays; the start bins that fit them (21 zero rows on either side)
constexpr int bright_lds_of_grant(int granted)
{
    const int left = granted - bright_lds_layout(0, true).total - BRIGHT_STATIC_RESERVE;
    return (left < 0 ? 0 : (left > BRIGHT_LDS_MAX ? BRIGHT_LDS_MAX : left)) / 16 * 16;
}
constexpr int bright_bins_of_lds(int bright_lds) { return bright_lds / (WFS_DT * 8) - 2 * (TILE_TLEN - 1) > 0 ? bright_lds / (WFS_DT * 8) - 2 * (TILE_TLEN - 1) : 0; }

// ---- k_row_pulse: region samples (multiple of 256) for each of the 4 waves
struct RowLds {
    int sTz;        // double[WAVE_TZ_LEN], align 8
    int cmax;       // double[16], align 8
    int ph;         // WavePhoton[4][64 + PW_U], align 16
    int acc;        // i32[4][region], align 16 (zeroed as int4)
    int total;
};
constexpr RowLds row_pulse_lds(int region)
{
    RowLds o{};
    o.sTz = 0;
    o.cmax = o.sTz + WAVE_TZ_LEN * 8;
    o.ph = o.cmax + 16 * 8;
    o.acc = o.ph + 4 * (64 + PW_U) * WAVE_PHOTON_BYTES;
    o.total = o.acc + 4 * region * 4;
    return o;
}

// ---- k_tile_order_big: a range of n photons is sorted as np2 = the next power of two (>= 128); launched for the largest range
struct OrderLds { int key /* u64[np2] */, rec /* PhotonRec[np2] */, gain /* double[np2] */, total; };      // align 8 each
constexpr OrderLds order_lds(int np2) { return OrderLds{0, np2 * 8, np2 * 16, np2 * 24}; }

// ---- k_photon_count: the alias cells of one channel row, a histogram over the channels
struct CountLds { int A /* uint2[2^lg], align 8 */, hist /* i32[nch], align 4 */, total; };
constexpr CountLds count_lds(int nch, int lg) { return CountLds{0, 8 << lg, (8 << lg) + nch * 4}; }

// ---- k_map_rows: one pattern
struct MapRowsLds { int p /* double[nch], align 8 */, total; };
constexpr MapRowsLds map_rows_lds(int nch) { return MapRowsLds{0, nch * 8}; }

// ---- k_photon_fill
struct GenFillLds { int wtime, T, hist, cur, hmin, hmax, hoff, chmap, pidx, stage, ap, total; };
constexpr GenFillLds gen_fill_lds(int nch, int lg, bool with_ap)
{
    const int nch1 = nch + 1 + ((nch + 1) & 1);              // even: keeps what follows 8-byte aligned
    GenFillLds o{};
    o.wtime = GEN_WIN * 4;                                    // win i32[GEN_WIN] at 0: first photon of the block's emitters, relative to the block
    o.T = o.wtime + GEN_WIN * 4;                              // wtime i32[GEN_WIN]: emitter times relative to the set's origin
    o.hist = o.T + (8 << lg);                                 // T: uint2[2^lg] alias cells of the channel row; hist i32[nch1]: photons per channel, then their prefix sums
    o.cur = o.hist + nch1 * 4;                                // i32[nch]: rank counters
    o.hmin = o.cur + nch * 4;                                 // i32[nch], i32[nch]: earliest / latest photon of the block per channel
    o.hmax = o.hmin + nch * 4;
    o.hoff = o.hmax + nch * 4;                                // i32[nch]: slot of bucket position 0 of every channel, relative to the set's first photon
    o.chmap = o.hoff + nch * 4;                               // u16[GEN_BLOCK]: channel of every bucket position
    o.pidx = o.chmap + GEN_BLOCK * 2;                         // u16[GEN_BLOCK]: block-relative photon index of every bucket position
    o.stage = (o.pidx + GEN_BLOCK * 2 + 7) & ~7;              // PhotonRec[GEN_BLOCK]: the block's photons in bucket order
    o.ap = o.stage + GEN_BLOCK * 8;                           // afterpulse staging
    o.total = ((o.ap + (with_ap ? AP_STAGE * AP_CAND_BYTES : 0) + 7) & ~7) + 16;
    return o;
}

// the largest total of every kernel with a raised cap fits it (k_s2_bright: its cap IS its total at the device's grant)
static_assert(pulse_lds(256).total <= LDS_CAP_PULSE && pulse_lds(128).total <= LDS_CAP_PULSE, "dense pulse kernel");
static_assert(SPARSE_MAX_PHOTONS <= SPARSE_TPB * SPARSE_PPT, "the photons of a sparse tile fit the registers of the 64-thread form");
static_assert(SPARSE_MAX_PHOTONS % 8 == 0 && SPARSE_MAX_BINS % 8 == 0 && sparse_lds(SPARSE_MAX_PHOTONS, SPARSE_MAX_BINS, SPARSE_TPB).total <= LDS_CAP_SPARSE,
              "the largest sparse tile fits the cap");
static_assert(generic_lds(1, 1, true).total <= LDS_CAP_GENERIC, "some geometry fits");
static_assert(tile_lds(false, true).total <= LDS_CAP_TILE && tile_lds(true, true).total <= LDS_CAP_TILE, "tile kernel");
static_assert(row_pulse_lds(RES_MAX_LEN).total <= LDS_CAP_ROW, "the longest region of k_row_pulse fits the cap");
static_assert(order_lds(TILE_ORDER_MAX).total <= LDS_CAP_ORDER, "k_tile_order_big");
static_assert(WFS_MAX_CH <= 1 << 10 && gen_fill_lds(WFS_MAX_CH, 10, true).total <= LDS_CAP_FILL, "k_photon_fill at the most channels");

// ---- window rules ------------------------------------------------------------------------------------------------------------------
WFS_HD i64 floordiv(i64 a, i64 b) { i64 q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// The samples of a tile (pulse.py:118-127): photons between t0 + tmin and t0 + tmax [ns] start in the bins bin0 .. bin0 + nb - 1, the
// pulse is stored from `left` to `right`, L samples.  D: anything with dt, store_before, samples_before, store_after, samples_after.
struct TileWindow { i64 left, right, bin0, nb, L; };
template <class D>
WFS_HD TileWindow tile_window(const D &d, i64 t0, i32 tmin, i32 tmax)
{
    TileWindow w;
    w.bin0 = floordiv(t0 + tmin, (i64)d.dt);
    const i64 bin1 = floordiv(t0 + tmax, (i64)d.dt);
    w.nb = bin1 - w.bin0 + 1;
    w.left = w.bin0 - d.store_before - d.samples_before;
    w.right = bin1 + d.store_after + d.samples_after;
    w.L = w.right - w.left + 1;
    return w;
}

// A row slot.  Slot idx of the row arrays is slot idx % row_slots of window g = idx / row_slots: the TPC channels, then the HE rows (of
// the top channels from he_first on), and last -- when the switch is on -- the window's sum row, which has no accumulator row of a
// channel behind it (acc_ch -1) and is finished like an HE row.  D: anything with row_slots, n_tpc, he_first, sum_channel.
template <class D>
WFS_HD bool row_slot_is_sum(const D &d, i32 slot) { return d.sum_channel >= 0 && slot == d.row_slots - 1; }
struct RowSlot { i64 g; i32 slot, channel, acc_ch; bool he, sum; };
template <class D>
WFS_HD RowSlot row_slot(const D &d, i64 idx)
{
    RowSlot r;
    r.g = idx / d.row_slots; r.slot = (i32)(idx - r.g * d.row_slots);
    r.sum = row_slot_is_sum(d, r.slot);
    if (r.sum) { r.he = true; r.acc_ch = -1; r.channel = d.sum_channel; return r; }
    r.he = r.slot >= d.n_tpc; r.acc_ch = r.he ? r.slot - d.n_tpc : r.slot; r.channel = r.he ? d.he_first + r.acc_ch : r.slot;
    return r;
}
// A row made of the samples lo .. hi of its window's pulses has tw more on either side (rawdata.py:258-259): its length, its first and
// last sample (relative to the window when lo and hi are)
struct RowSpan { i64 len, left, right; };
WFS_HD RowSpan row_span(i64 lo, i64 hi, i64 tw) { return RowSpan{hi - lo + 1 + 2 * tw, lo - tw, hi + tw}; }
// Full readout (wfs_set_full_readout): every row of a window, with or without a pulse of its own, has the range of the window's union
// mask -- the range row_span gives a channel whose pulses reach both grp_lo and grp_hi, the minimum left and the maximum right over
// all pulses of the window.  The window's sum row keeps the union of the bottom rows' pulses.
WFS_HD RowSpan full_row_span(i64 grp_lo, i64 grp_hi, i64 tw) { return row_span(grp_lo, grp_hi, tw); }
