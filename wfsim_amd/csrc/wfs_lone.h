// Lone-hit rows (wfs_lone_hits): what crosses a threshold outside the rows of a run is read out in rows of its own --
// dark photons (3f) and, with wfs_set_lone_noise_hits, every sample of the noise model that crosses (3g, below).  The rule, its limits
// and the checks of the entry point; the device forms (k_lone_scan, k_lone_noise_scan, k_lone_rows, k_lone_desc) are in wfs_kernels.h.
//
// Symbols as in wfs_dark.h; start = idx - before is the first sample of a dark photon's pulse, G = tlen + 2 tw.
//   lone     a dark photon of PMT channel ch is lone when none of its pulse samples start .. start + tlen - 1 lies in a row of ch's TPC
//            slot.  Rows are those of the engine's last wfs_run at their final range (row_lo - tw .. row_hi + tw behind k_rows_widen;
//            under full readout every channel of a window has one of the window's range).  Rate 0, gain 0 and channels at or beyond
//            the rate array have no dark photons, hence no lone rows; HE slots and the sum row get none.
//   row      the lone photons of a channel in time order; a maximal chain whose consecutive starts are at most G apart is one lone row
//            of range first start - tw .. last start + tlen - 1 + tw (row_span of a channel whose pulses are exactly these), clipped so
//            that it reaches no sample of an existing row of the channel.  A chain cannot straddle an existing row: such a row holds a
//            pulse and is at least G long, so the photons on its two sides start more than G + tlen apart (lone_cannot_straddle).
//   content  D(ch, t) of wfs_dark.h over the range -- every dark photon that reaches a sample counts, the tail of one that is not lone
//            included -- finished by the one rule of wfs_rows.h (noise, baseline, clamp).  Noise kinds 3 - 5 take their value at the
//            absolute sample; table kinds 1 and 2 read index ix_rand + i, ix_rand = ((u64) w[0] noise_len) >> 32 with w the Philox call
//            at site 115, counter (low and high word of the row's first sample, ch, 115).  Then ZLE with thr_zle[ch], hold-off, even
//            landing and 110-sample fragments as for any row.
//   owner    a pass over [s0, s1) owns the rows whose first photon has start in [s0, s1).  It looks back G samples in front of s0 to
//            decide whether a photon at or after s0 begins a chain, and follows a chain beyond s1 to its end but not beyond s_limit >= s1:
//            photons that start at or after s_limit are not taken and the row ends at s_limit - 1 at the latest (an approximation: what
//            such a chain holds beyond s_limit is read out by no pass).  Records are the same however [s0, s1) is split into passes of
//            one s_limit.
// Noise-hit seeds (wfs_set_lone_noise_hits, config 'noise_lone_hits'; off by default).
//   value    v(ch, t) is the finished sample a row without a pulse would hold at absolute sample t: finish_value<NK>(d, D(ch, t), he =
//            false, noisy = ch < model channels, noise(ch, t)), D = 0 where no dark-count rate is set.  Defined for the drawn noise kinds
//            3, 4 and 5 alone: a noise table has no value at an absolute sample.
//   seed     a sample t of a PMT channel ch inside the noise model is a noise-hit seed when v(ch, t) < thr_zle[ch] -- the very comparison
//            the ZLE kernels make -- and t lies in no row of ch's TPC slot (under full readout every channel of a window has a row).
//            The seed's start is t itself, not t - before: a seed directly behind a row must start behind that row, or the clipping of
//            lone_range does not see the row.  A photon is lone when its whole pulse is clear of the rows; a seed needs only its own
//            sample to be clear (lone_seed_clear).  What made the sample cross -- noise alone, the tail of a dark pulse that is not
//            lone, both together -- does not matter.
//   rows     the seeds of a channel are its lone dark photons (the rule above, if rates are set) and its noise-hit seeds, merged by
//            start; from there on everything above applies without change: a maximal chain with consecutive starts at most G apart is
//            one row of range first start - tw .. last start + tlen - 1 + tw, clipped against the row in front, the row behind and
//            s_limit; content D finished by the one rule of wfs_rows.h; ZLE, hold-off, even landing, 110-sample fragments, ownership by
//            the first seed's start in [s0, s1) and the look-back of G samples as before.  Two seeds on the two sides of a row of
//            length len >= G start at least len + 1 > G apart (lone_seeds_cannot_straddle): a chain straddles no row.
// Consequences.  Every noise-hit seed is a hit of the row that holds it, so it lies inside exactly one stored interval of its channel.
// A dark pulse that crosses the threshold contributes its own crossing samples as seeds; these never start before the photon does, so
// the first start of a chain does not move, but they can start later, so the last start can move by up to tlen - 1 samples: a row can
// be that much longer than the same row under 3f alone -- the row of a chain is what its seeds span.  No HE rows, no sum-row entries
// and no truth, as in 3f.  A baseline excursion of a slow level that stays across the threshold makes one long chain; LONE_MAX_ROW_LEN
// applies to it.
// The windows of a run must lie more than G samples apart (lone_windows_apart), so that the one window found by bisection is the only
// one whose rows a photon's pulse or a row's margins can meet; RawData asks right_raw_extension >= (2 G + 64) dt for that.
// No HIP types: a host compiler takes this header (tests/host/lone_rules_main.cpp).
#pragma once
#include <cstdint>
#include <string>
#include "wfs_layout.h"     // WFS_HD, i32, i64, row_span
#include "wfs_rows.h"       // bits_below
#include "wfs_dark.h"

constexpr unsigned DK_SITE_LONE_IX = 115;                          // Philox site of a lone row's noise offset
constexpr int LONE_SCAN_CELLS = 256;                               // cells of a channel per workgroup of k_lone_scan, a lane each
constexpr int64_t LONE_MAX_CELLS = (int64_t)1 << 34;               // cells (channels x cells of a channel) of one pass at most
constexpr int64_t LONE_MAX_SPAN = (int64_t)1 << 40;                // samples from s0 - G to s_limit at most (the photon sort keys)
constexpr int64_t LONE_MAX_ROWS = (int64_t)1 << 24;                // lone rows of one pass at most
constexpr int LONE_MAX_ROW_LEN = 1 << 19;                          // samples of a lone row at most (a row is shorter than 2^20 samples)
constexpr int LONE_NOISE_BLOCK = 256;                              // samples of a channel per wave of k_lone_noise_scan, four per lane
constexpr int64_t LONE_MAX_BLOCKS = ((int64_t)1 << 31) - 4;        // such blocks of a channel in one pass at most (four to a workgroup, 2^31 - 1 workgroups)

// The key of a seed sorts by (channel, start, kind): channel << LONE_KEY_SHIFT | (start - a0) << 1 | kind, a0 = s0 - G the first start a
// pass lists.  kind 0: a lone dark photon, 1: a noise-hit seed.
constexpr int LONE_KIND_PHOTON = 0, LONE_KIND_NOISE = 1;
constexpr int LONE_KEY_KIND_BITS = 1, LONE_KEY_START_BITS = 40, LONE_KEY_SHIFT = LONE_KEY_START_BITS + LONE_KEY_KIND_BITS;
static_assert(LONE_MAX_SPAN <= ((int64_t)1 << LONE_KEY_START_BITS), "a start of a pass fits the start bits of its key");
static_assert(LONE_KIND_NOISE < (1 << LONE_KEY_KIND_BITS) && LONE_KIND_PHOTON < (1 << LONE_KEY_KIND_BITS), "a kind fits the kind bits");
static_assert(LONE_KEY_SHIFT + 17 <= 64, "channel numbers of up to 17 bits fit above the start (WFS_MAX_CH is far below)");
WFS_HD unsigned long long lone_key(i32 ch, i64 rel, int kind) { return ((unsigned long long)(unsigned)ch << LONE_KEY_SHIFT) | ((unsigned long long)rel << LONE_KEY_KIND_BITS) | (unsigned long long)kind; }
WFS_HD i32 lone_key_channel(unsigned long long key) { return (i32)(key >> LONE_KEY_SHIFT); }
WFS_HD i64 lone_key_rel(unsigned long long key) { return (i64)((key & (((unsigned long long)1 << LONE_KEY_SHIFT) - 1)) >> LONE_KEY_KIND_BITS); }
WFS_HD int lone_key_kind(unsigned long long key) { return (int)(key & (((unsigned long long)1 << LONE_KEY_KIND_BITS) - 1)); }
// the end bit of the sort over the seed keys of a pass with n_channels channels: start and kind, and channel bits for values up to n_channels
WFS_HD unsigned lone_key_end_bit(int n_channels) { return (unsigned)(LONE_KEY_SHIFT + bits_below((u64)n_channels + 1)); }

WFS_HD i64 lone_gap(i64 tlen, i64 tw) { return tlen + 2 * tw; }                          // G
// the cells whose photons can start in [a, b): idx = start + before lies in cell idx >> 6
WFS_HD i64 lone_first_cell(i64 a, i64 before) { return (a + before) >> DK_CELL_SHIFT; }
WFS_HD i64 lone_last_cell(i64 b, i64 before) { return (b - 1 + before) >> DK_CELL_SHIFT; }
// a pulse start .. start + tlen - 1 against a row of final range [rl, rr]
WFS_HD bool lone_pulse_meets(i64 start, i64 tlen, i64 rl, i64 rr) { return start <= rr && start + tlen - 1 >= rl; }
// the range of a chain first .. last (starts), clipped by the nearest row in front (ends at prev_r, I64 min: none), the nearest row
// behind (begins at next_l, I64 max: none) and s_limit
struct LoneRange { i64 left, right; };
WFS_HD LoneRange lone_range(i64 first, i64 last, i64 tlen, i64 tw, i64 prev_r, i64 next_l, i64 s_limit)
{
    const RowSpan sp = row_span(first, last + tlen - 1, tw);
    i64 l = sp.left, r = sp.right;
    if (prev_r >= l) l = prev_r + 1;
    if (next_l <= r) r = next_l - 1;
    if (r > s_limit - 1) r = s_limit - 1;
    return LoneRange{l, r};
}
// a noise-hit seed at sample t against a row of final range [rl, rr] (has: the channel has one in the window): the test is on the sample
WFS_HD bool lone_seed_clear(i64 t, bool has, i64 rl, i64 rr) { return !(has && t >= rl && t <= rr); }
// Two seeds on the two sides of a row of row_len >= G samples start at least row_len + 1 > G apart: never one chain.
WFS_HD bool lone_seeds_cannot_straddle(i64 row_len, i64 tlen, i64 tw) { return row_len + 1 > lone_gap(tlen, tw); }
// the blocks of k_lone_noise_scan over the samples a0 .. s_limit - 1
WFS_HD i64 lone_noise_blocks(i64 a0, i64 s_limit) { return s_limit > a0 ? (s_limit - a0 + LONE_NOISE_BLOCK - 1) / LONE_NOISE_BLOCK : 0; }
// noise offset of a lone row from word 0 of its call at site 115; 0 without a table
WFS_HD i64 lone_ix_rand(u32 w0, i64 noise_len) { return noise_len > 0 ? (i64)(((unsigned long long)w0 * (unsigned long long)noise_len) >> 32) : 0; }
// A row with a pulse is at least G long, so two lone photons on its two sides start at least len + tlen > G apart: never one chain.
WFS_HD bool lone_cannot_straddle(i64 row_len, i64 tlen, i64 tw) { return row_len >= lone_gap(tlen, tw); }
// Two windows whose rows end at a_hi and begin at b_lo are far enough apart for the single look-up: a pulse (tlen samples) or a row's
// margin (tw samples on either side of a pulse, G in all) cannot reach from one into the other.
WFS_HD bool lone_windows_apart(i64 a_hi, i64 b_lo, i64 tlen, i64 tw) { return b_lo - a_hi > lone_gap(tlen, tw); }

// The bound RawData puts on right_raw_extension (rext, ns): a new window begins where a cluster's first time lies more than rext behind
// the end of the last pulse, (a_hi - tw) dt for rows that end at a_hi.  A pulse begins `before` + samples_to_store_before samples
// ahead of its first photon, a row tw ahead of that, and the window's left may go one sample further down to an even one, so the next
// window's rows begin at b_lo >= a_hi + rext / dt - (2 tw + before + store_before + 2).  With rext >= (2 G + 64) dt = (2 tlen + 4 tw +
// 64) dt that is b_lo - a_hi >= G + tlen + (64 - before - store_before - 2), more than G + tlen - 1 while before + store_before + 2 < 64
// (checked beside this bound, dark_counts.lone_hits_from): lone_windows_apart holds, a lone row (a chain between two windows,
// margins included) meets the rows of at most one window at either end, and a photon that starts within G samples behind a window
// ends in front of the next window's rows.  The 64 is a cell.
inline int64_t lone_min_rext(int64_t dt, int64_t tlen, int64_t tw) { return (2 * lone_gap(tlen, tw) + DK_CELL) * dt; }

// the arguments of wfs_lone_hits: empty string, or what is wrong with them (code: 0 ok, 1 invalid, 2 capacity)
inline int lone_check(int64_t s0, int64_t s1, int64_t s_limit, int n_channels, int64_t tlen, int64_t tw, int64_t before, std::string &err)
{
    const std::string f = "wfs_lone_hits: ";
    const int64_t big = (int64_t)1 << 48;
    if (s1 < s0) { err = f + "s1 < s0"; return 1; }
    if (s_limit < s1) { err = f + "s_limit < s1"; return 1; }
    if (s0 < -big || s_limit > big) { err = f + "range beyond 2^48 in magnitude"; return 1; }
    const int64_t a = s0 - lone_gap(tlen, tw);
    if (s_limit - a >= LONE_MAX_SPAN) { err = f + "lone hits: a pass of more than 2^40 samples, split it"; return 2; }
    if (s1 == s0) return 0;
    const int64_t cells = lone_last_cell(s_limit, before) - lone_first_cell(a, before) + 1;
    if (cells * (int64_t)n_channels > LONE_MAX_CELLS) { err = f + "lone hits: a pass of more than 2^34 cells (channels x 64-sample cells), split it"; return 2; }
    return 0;
}
// ... and what the noise-hit scan of the same pass adds to them (same codes)
inline int lone_noise_check(int64_t s0, int64_t s_limit, int64_t tlen, int64_t tw, std::string &err)
{
    if (lone_noise_blocks(s0 - lone_gap(tlen, tw), s_limit) > LONE_MAX_BLOCKS) { err = "wfs_lone_hits: lone hits: a pass of more than 2^31 blocks of 256 samples per channel (noise hits), split it"; return 2; }
    return 0;
}
