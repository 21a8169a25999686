// The rules of the back end of a row, each written once for host and device: hold-off and interval slots, closing a ZLE interval, the
// records of an interval and the layout of a record, the noise index, the padded length of a finished 16-bit row, the finished sample.
// They decide the bytes of a raw_record; two encoders (ZleFast; ZleChunks, the general path of k_zle and k_row_empty) and three packers (k_rec_keys, k_pack_res,
// k_pack) must agree on them to the sample.  All of it is integer arithmetic on a few scalars.
//
// No HIP types: tests/host/rows_main.cpp compiles this header with the host compiler and tests/test_row_rules_cpu.py holds what it
// computes against the reference's own rows, ZLE tuples and records (tests/golden/zle_edges.npz).  D: anything with the fields of
// WfsDev a rule reads (baseline, he_factor).
#pragma once
#include "wfs_layout.h"      // WFS_HD, i32, i64, u32, row_span

typedef unsigned long long u64;        // (as wfs_device.h has it)

// ---- hold-off and interval slots ---------------------------------------------------------------------------------------------------
// Two hits belong to one interval when they are no more than the hold-off apart (rawdata.py:296-300, utils.py:13-58)
WFS_HD i64 zle_holdoff(i64 tw) { const i64 hold = 2 * tw + 1; return hold < 1 ? 1 : hold; }
// the smallest hold-off of the chunked bookkeeping (ZleFast: only the first hit of a 64-sample chunk can open an interval) and
// therefore of resident rows, which have no other
constexpr i32 ZLE_FAST_HOLD = 63;
// interval slots reserved for a row of len samples: two interval starts are at least hold + 1 samples apart
WFS_HD i64 zle_slots(i64 len, i64 hold) { return (len + hold) / (hold + 1); }

// ---- records of an interval and the layout of a record (strax_interface.py:391-436) ------------------------------------------------
constexpr int WFS_SPR = 110;               // samples per strax record (strax DEFAULT_RECORD_LENGTH; a compile-time constant: the divisions by it are in every row kernel)
// the header: time i64 | length i32 | dt i16, channel i16 | pulse_length i32 | record_i i16, baseline i16 (always 0); dword indices
enum RecDword : int { REC_TIME_LO = 0, REC_TIME_HI = 1, REC_LENGTH = 2, REC_DT_CHANNEL = 3, REC_PULSE_LENGTH = 4, REC_RECORD_I = 5, REC_HEADER_DWORDS = 6 };
constexpr int REC_HEADER_BYTES = 4 * REC_HEADER_DWORDS;
constexpr int REC_DWORDS = REC_HEADER_DWORDS + WFS_SPR / 2;        // two 16-bit samples per dword behind the header
constexpr int WFS_RECORD_BYTES = 4 * REC_DWORDS;
constexpr int REC_LENGTH_BYTE = 4 * REC_LENGTH, REC_DATA_BYTE = REC_HEADER_BYTES;      // what a reader of packed records needs: the length field, the first sample
static_assert(WFS_SPR % 2 == 0 && WFS_RECORD_BYTES == 244, "the record layout of include/wfsim_amd.h");

// records of an interval of plen samples; an interval whose left landed above its right (plen <= 0) has none
WFS_HD i32 records_of(i32 plen) { return plen > 0 ? (plen + WFS_SPR - 1) / WFS_SPR : 0; }
// record f of an interval: its first sample inside the interval, that sample counted from what `left` counts from, and its time
// (F: the width of the product is the caller's -- k_rec_keys, a record per lane, multiplies in 64 bits)
template <class F> WFS_HD F rec_fragment_first(F f) { return WFS_SPR * f; }
template <class F> WFS_HD i64 rec_fragment_sample(i64 left, F f) { return left + rec_fragment_first(f); }
WFS_HD i64 rec_fragment_time(i32 dt, i64 left, i32 f) { return (i64)dt * rec_fragment_sample(left, f); }
// its samples: WFS_SPR, the last record of an interval what is left.  FROM_END says how the comparison is written, `first + WFS_SPR
// <= plen` or `plen - first >= WFS_SPR` -- one condition (nothing here comes near 2^31), two spellings that the compiler does not
// take for each other: the four unrolled records of k_pack_res are a subtraction and a minimum each in the second (16 scalar
// instructions and 6 SGPRs more in the first); k_pack<1> and k_pack<2> take 4 VGPRs more in the second and k_pack<2> loses a wave.
template <bool FROM_END = false>
WFS_HD i32 rec_fragment_len(i32 plen, i32 f)
{
    const i32 first = rec_fragment_first(f), rest = plen - first;
    return (FROM_END ? first + WFS_SPR <= plen : rest >= WFS_SPR) ? WFS_SPR : rest;
}
// the header dwords of record f of an interval of plen samples that begins at absolute sample left; dt_channel: of the whole row
WFS_HD u32 rec_dt_channel(i32 dt, i32 channel) { return ((u32)(uint16_t)dt) | ((u32)(uint16_t)channel << 16); }
struct RecHeader { u32 w[REC_HEADER_DWORDS]; };
template <bool FROM_END = false>
WFS_HD RecHeader rec_header(i32 dt, u32 dt_channel, i64 left, i32 plen, i32 f)
{
    const i64 time = rec_fragment_time(dt, left, f);
    RecHeader h;
    h.w[REC_TIME_LO] = (u32)(u64)time; h.w[REC_TIME_HI] = (u32)((u64)time >> 32);
    h.w[REC_LENGTH] = (u32)rec_fragment_len<FROM_END>(plen, f);
    h.w[REC_DT_CHANNEL] = dt_channel;
    h.w[REC_PULSE_LENGTH] = (u32)plen;
    h.w[REC_RECORD_I] = (u32)(uint16_t)f;                  // baseline = 0
    return h;
}

// ---- sort keys: the bits in use --------------------------------------------------------------------------------------------------------
// Bits needed for values below v, the smallest b with v <= 2^b: 0 for v <= 1, k for 2^(k-1) < v <= 2^k, 64 above 2^63.  A radix sort
// over keys below v ends at this bit; every "how many key bits are in use" of the engine is this function (the record sort, the seed
// sort of the lone-hit passes, the keys of the overlay).
WFS_HD int bits_below(u64 v) { if (v < 2) return 0; int b = 1; while (b < 64 && ((v - 1) >> b) != 0) b++; return b; }
// The record key of k_rec_keys: (first sample of the record - key origin) << REC_KEY_SHIFT | channel, channels below 2^REC_KEY_SHIFT.
constexpr int REC_KEY_SHIFT = 12;
// The end bit of the sort over the record keys of rows that span `span` = key_end - key_origin samples: relative samples up to span, at
// least one bit of them.  (The loop this replaces, `end = 13; while (((span << 12) >> end) != 0) end++`, gave the same for every span
// below 2^52 and lost the top bits of span << 12 from there on, which no batch reaches; here such a span sorts all 64 bits.)
WFS_HD unsigned rec_key_end_bit(u64 span) { const int b = REC_KEY_SHIFT + bits_below((span < 1 ? 1 : span) + 1); return b < 64 ? (unsigned)b : 64u; }

// ---- closing an interval ------------------------------------------------------------------------------------------------------------
// The interval of the hits rawl .. rawr of a row of len samples (rawdata.py:302-311): tw samples more on either side, clipped into the
// row, left up and right down to an even sample; the records it needs.  Relative to the row, which is shorter than 10^6 samples
// (k_group_final): 32 bits.
struct ZleWindow { i32 left, right, nrec; };
WFS_HD ZleWindow zle_window(i32 rawl, i32 rawr, i32 tw, i32 len)
{
    i32 l = rawl - tw, r = rawr + tw;
    l = l < 0 ? 0 : (l > len - 1 ? len - 1 : l); r = r < 0 ? 0 : (r > len - 1 ? len - 1 : r);
    l = (l + 1) / 2 * 2; r = r / 2 * 2;                    // ceil(l/2)*2, floor(r/2)*2 for non-negative ints
    return ZleWindow{l, r, records_of(r - l + 1)};
}

// ---- the noise index ----------------------------------------------------------------------------------------------------------------
// Sample i of a row reads noise[(ix_rand + i) mod noise_len] (rawdata.py:433-434).  The row kernels walk it as a scalar start per block
// of samples, nrun < noise_len, that steps with the block, plus a lane's offset inside the block -- a row may be any number of table
// lengths long.  PRECONDITION of noise_wrap: in < 2 * noise_len, so that one conditional subtraction is the modulo; it holds for
// nrun + step and for nrun + off with step, off <= noise_len, which is what NOISE_MIN_FAST grants the fast row kernels.
constexpr int NOISE_MIN_FAST = 512;        // shortest noise table of the fast row kernels (a block of 256 samples wraps at most once)
WFS_HD u32 noise_wrap(u32 in, u32 noise_len) { return in >= noise_len ? in - noise_len : in; }
WFS_HD u32 noise_advance(u32 nrun, u32 step, u32 noise_len) { return noise_wrap(nrun + step, noise_len); }
static_assert(256 <= NOISE_MIN_FAST && 2 * WFS_SPR <= NOISE_MIN_FAST, "the steps and offsets of k_zle, k_row_pulse and k_pack fit the shortest fast table");

// ---- finished 16-bit rows (k_row_pulse) ---------------------------------------------------------------------------------------------
// A resident row is stored in whole groups of four samples; k_pack_res reads pairs, and clamps a pair index past the row to the last
// pair that is stored
WFS_HD i32 fin_padded_len(i32 len) { return (len + 3) & ~3; }
WFS_HD i32 fin_last_pair(i32 len) { return fin_padded_len(len) - 2; }

// ---- the finished sample ------------------------------------------------------------------------------------------------------------
// NK is the noise kind of the batch (NoiseKind of wfs_noise.h; 0: none, 1: int16 table, 2: float64 table, 3, 4, 5: drawn).
// accumulated ADC (times the HE factor, rawdata.py:242-246) + noise + baseline, clamped at 0 (rawdata.py:398-458 add_noise /
// add_baseline / digitizer_saturation, fused into the read).  nz: the integer noise of kinds 1, 3, 4, 5; nzf: that of kind 2, added in
// floating point -- numba's int64 += float64 stores the TRUNCATED SUM, not the sum with the truncated noise.  noisy false (a row
// outside the table, wave-uniform): the tables' value was read from row 0 and is dropped here; the drawn kinds hand in 0.
template <int NK, class D>
WFS_HD i32 finish_value(const D &d, i32 acc, bool he, bool noisy, i32 nz, double nzf)
{
    i64 v = acc;
    if (he) v *= d.he_factor;
    if constexpr (NK == 1) v += noisy ? nz : 0;
    if constexpr (NK == 2) { const i64 w = (i64)((double)v + nzf); v = noisy ? w : v; }
    if constexpr (NK >= 3) v += nz;
    v += d.baseline;
    return v < 0 ? 0 : (i32)v;
}
WFS_HD i32 add_sat32(i32 a, i32 b)
{
#if defined(__HIPCC__)
    return __builtin_elementwise_add_sat(a, b);            // (v_add_i32 with clamp)
#else
    const i64 s = (i64)a + b; return s > 0x7fffffffLL ? 0x7fffffff : (s < -0x80000000LL ? (i32)-0x80000000LL : (i32)s);
#endif
}
// The rule of resident rows with integer noise (k_row_pulse; no HE rows there, so no factor): 32-bit arithmetic with a saturating add,
// deliberately cheaper than finish_value.  DOMAIN on which it is finish_value<NK>(d, acc, false, noisy, nz, 0): |baseline + nz| <=
// 2^16 and acc + baseline + nz <= 2^31 - 1, which every acc < 2^31 - 2^16 grants (a row of a 14-bit digitiser is some 10^5 times
// smaller); any negative acc is inside it.  Beyond it this rule stays at 2^31 - 1 where the 64-bit sum of finish_value does not fit.
template <int NK, class D>
WFS_HD i32 finish_resident(const D &d, i32 acc, bool noisy, i32 nz)
{
    static_assert(NK != 2, "float noise is added in floating point: finish_value");
    i32 add = d.baseline;
    if constexpr (NK == 1) add += noisy ? nz : 0;
    if constexpr (NK >= 3) add += nz;
    const i32 v = add_sat32(acc, add);
    return v < 0 ? 0 : v;
}
// The ZLE threshold in 32 bits: `v < zle_thr32(thr)` is `(i64)v < thr` for every finished sample 0 <= v < 2^31 - 1 whatever the
// threshold (a saturated sample of exactly 2^31 - 1 is no hit in 32 bits under a threshold beyond them).  That includes a threshold
// NO sample can reach: with zle_threshold below -2^15, thr_zle = baseline - zle_threshold - 1 lies above every finished sample a
// 16-bit record can hold, every sample of a row is a hit in either form, the row is ONE interval (zle_window: clipped into the row,
// even landing) and is stored whole -- the "no suppression" mode of full readout is this rule and nothing else.
WFS_HD i32 zle_thr32(i64 thr) { return thr > 0x7fffffffLL ? 0x7fffffff : (thr < -0x7fffffffLL ? -0x7fffffff : (i32)thr); }
