// PMT dark counts (wfs_set_dark_counts): the definition, the host state and the check of the setter as a pure function from
// the rates to the thresholds or a message.  The device forms (dark_sample, dark_block) are in wfs_kernels.h.
//
// A dark photon is one single-PE photon on a PMT channel; it becomes a one-photon pulse by the rules every pulse follows and is added
// to the channel's rows as one more pulse.  dt: sample duration, tlen: template length, before: samples in front of the pulse centre
// (samples_before), L = DK_CELL = 64 samples in a cell, m: cell index of a channel's absolute sample axis (cell m holds the samples
// 64 m .. 64 m + 63; m may be negative, shifts are arithmetic).
//   count   w = philox4x32_10(counter (low 32 bits of m, high 32 bits of m, ch, 112), key = seed)
//           n(ch, m) = sum_{k = 1 .. 4} [w[0] < T[ch][k]],  T[ch][k] = floor(2^32 P(N >= k)),  N ~ Poisson(mu_ch),
//           mu_ch = rate_ch L dt 1e-9; the tail sums are the series sum_{i >= k}, not 1 - sum_{i < k} (no cancellation at small mu).
//           mu_ch <= 1/8 (the setter rejects more): the mass above 4 is then below 2.6e-7 and is folded into 4.
//   photon  j < n: the call at site 113 + (j >> 1) with the same first three counter words, words a = 2 (j & 1) and a + 1 of it:
//           t_ns = m L dt + (((u64) w[a] (L dt)) >> 32);  gain = photon_gain(spe_row_of(ch), gains[ch], code) with the single-PE code
//           (((u64) w[a + 1] SPE_BINS) >> 32) + 1 -- the first index of gain_code, never a double PE: a thermionic electron is one electron.
//   pulse   idx = t_ns div dt, r = t_ns mod dt (floor both): samples idx - before + k, k < tlen, value adc_of(gain templates[r tlen + k]).
//   row     D(ch, t) = the integer sum of these values over every dark photon of the channel that reaches sample t (cells
//           (t + before - tlen + 1) >> 6 .. (t + before) >> 6), every photon rounded on its own, like a pulse of its own.
//   where   acc' = acc + D(pmt channel of the slot, row_abs + i) in front of everything finish_value / finish_resident do: an HE slot
//           gets its top channel's D times int(he_factor) as a pulse of that channel would, noise, baseline and clamp follow unchanged.
//           A channel with rate 0 or gain 0 gets nothing, nor does one at or beyond the given count.
// The sum row (wfs_set_sum_signal) carries NO dark counts: k_sum_signal adds unfinished rows, and a per-sample sum over the bottom
// array is a kernel of its own.  Windows, their left / right, row ranges, ix_rand, truth, the order of the Pulse calls and the record
// order do not move.  Outside the rows of a run a dark photon is read out by a pass of wfs_lone_hits alone (wfs_lone.h).
// No HIP types: a host compiler takes this header.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

constexpr int DK_CELL_SHIFT = 6, DK_CELL = 1 << DK_CELL_SHIFT;      // samples in a cell
constexpr int DK_MAX = 4;                                          // photons of a cell at most
constexpr double DK_MU_MAX = 0.125;                                // largest mean count of a cell the setter takes
constexpr unsigned DK_SITE_COUNT = 112, DK_SITE_PHOTON = 113;      // Philox sites: the count; photons 0, 1 (113) and 2, 3 (114); 115: wfs_lone.h

struct DarkState {
    int channels = 0;                         // 0: off
    std::vector<uint32_t> thr;                // [channels][DK_MAX]: floor(2^32 P(N >= k)), k = 1 .. 4
    bool set() const { return channels > 0; }
};

// floor(2^32 P(N >= k)), k = 1 .. 4, N ~ Poisson(mu), 0 <= mu <= DK_MU_MAX: each tail is its own series from the smallest term up
inline void dark_thresholds(double mu, uint32_t out[DK_MAX])
{
    for (int k = 1; k <= DK_MAX; k++) {
        double term[48];
        double t = std::exp(-mu);
        for (int i = 1; i <= k; i++) t *= mu / i;               // e^-mu mu^k / k!
        int n = 0;
        for (int i = k; n < 48 && t > 0; i++) { term[n++] = t; t *= mu / (i + 1); }
        double tail = 0;
        while (n > 0) tail += term[--n];
        out[k - 1] = (uint32_t)std::floor(tail * 4294967296.0);     // (tail <= 1 - e^(-1/8) < 0.12)
    }
}

// rates [Hz] of n_channels <= max_channels PMTs -> thr [n_channels][DK_MAX], or false and a message
inline bool dark_check(int n_channels, int max_channels, const double *rate_hz, int dt, std::vector<uint32_t> &thr, std::string &err)
{
    const std::string f = "wfs_set_dark_counts: ";
    if (n_channels < 0 || n_channels > max_channels) { err = f + "n_channels outside 0 .. n_tpc"; return false; }
    if (n_channels > 0 && !rate_hz) { err = f + "null rate_hz"; return false; }
    thr.assign((size_t)n_channels * DK_MAX, 0u);
    for (int c = 0; c < n_channels; c++) {
        const double r = rate_hz[c];
        if (!(r >= 0.0) || !std::isfinite(r)) { err = f + "rate_hz of channel " + std::to_string(c) + " is negative or not finite"; return false; }
        const double mu = r * (double)DK_CELL * (double)dt * 1e-9;
        if (mu > DK_MU_MAX) { err = f + "rate_hz of channel " + std::to_string(c) + ": more than 1/8 dark photons per cell of 64 samples"; return false; }
        dark_thresholds(mu, thr.data() + (size_t)c * DK_MAX);
    }
    return true;
}
