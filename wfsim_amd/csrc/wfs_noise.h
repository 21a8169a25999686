// What a handle knows about the noise model, nested by lifetime: the model (wfs_set_noise_model), inside it the colour that was set on
// its shapes (wfs_set_noise_colour), inside that the slow levels that were set on the colour's rows (wfs_set_noise_slow).  A level is
// reset by assignment of a value-initialised struct, which takes everything nested in it along, and the transitions at the end are
// the only code that writes any of it.  With the state: the layouts of the two device buffers, one description each for the packer
// and for the device view, and the checks of the three setters as pure functions from the arguments to the packed words or a message.
// No HIP types: tests/host/noise_state_main.cpp compiles this header with the host compiler.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

typedef long long i64;        // (as wfs_device.h has them)
typedef int i32;
typedef unsigned int u32;

// The row kernels take the kind of noise as a template parameter (no branch between their loads).  Colour: the model with FIR taps
// and common streams; Slow: the same with slow levels (a model without a colour gets unit taps).
enum NoiseKind : int { NOISE_NONE = 0, NOISE_TABLE_I16 = 1, NOISE_TABLE_F64 = 2, NOISE_MODEL = 3, NOISE_COLOUR = 4, NOISE_SLOW = 5 };
constexpr int NOISE_KINDS = 6;

// The FIR taps of the coloured model on the device: one row of NC_TAP_STRIDE int32 (Q16) per stream, tap k at [NC_TAP_PAD + k], zeros in
// front and behind -- a lane that holds a quad of whites multiplies all four words by the taps their distance asks for, and the
// distances that fall outside 0 .. L - 1 (at most NC_TAP_PAD to either side) meet a zero instead of a branch.
constexpr int NC_MAX_TAPS = 16;
constexpr int NC_TAP_PAD = 6;
constexpr int NC_TAP_STRIDE = NC_MAX_TAPS + 2 * NC_TAP_PAD;
constexpr int NC_MAX_GROUPS = 1024, NC_MAX_MIX = 65536, NC_UNIT = 65536;       // (Q16: NC_UNIT is 1.0)
// The slow levels (wfs_set_noise_slow): at most NS_MAX_LEVELS, knots 2^shift samples apart with NS_MIN_SHIFT <= shift <= NS_MAX_SHIFT.
// A block of 256 samples touches at most 255 / 2^NS_MIN_SHIFT + 3 = 18 knots of a level, which lie in at most NS_QUADS aligned quads.
constexpr int NS_MAX_LEVELS = 8, NS_MIN_SHIFT = 4, NS_MAX_SHIFT = 30, NS_QUADS = 6;
constexpr int NM_MAX_VALUES = 4096;

struct NoiseCell { u32 x, y; };       // one cell of a Walker table, {thr, alias}: what the device reads as a uint2

// ---- the state ------------------------------------------------------------------------------------------------------------------
struct NoiseSlowState { i32 levels = 0; };                                  // 0: none
struct NoiseColourState {
    i32 n_taps = 0, groups = 0;                   // n_taps 0: white (and then no groups)
    std::vector<i64> tapsum;                      // sum |taps_q| per row, channels then common streams: the bound of the slow levels starts from it
    NoiseSlowState slow;                          // set on the rows of this colour (or on the channels of a white model)
};
struct NoiseModelState {
    i32 channels = 0, k = 0, shift = 0, vmin = 0, values = 0;       // channels 0: no model; k cells per channel, all of one size
    std::vector<NoiseCell> cells;                 // [channels][k], the channels' alone (on the device the common streams' follow)
    NoiseColourState colour;                      // set on the shapes of this model
    bool set() const { return channels > 0; }
    bool coloured() const { return set() && colour.n_taps > 0; }
    i32 levels() const { return set() ? colour.slow.levels : 0; }
    i32 rows() const { return channels + colour.groups; }      // streams: the channels, then the common ones
};

// ---- the device buffers, in int32 words --------------------------------------------------------------------------------------------
// colour buffer: taps [channels + groups][NC_TAP_STRIDE] | group [channels] | mix [channels]
struct NoiseColourLayout {
    size_t taps, group, mix, size;
    NoiseColourLayout(i32 channels, i32 groups)
        : taps(0), group((size_t)(channels + groups) * NC_TAP_STRIDE), mix(group + (size_t)channels), size(mix + (size_t)channels) {}
    size_t tap(i32 row, i32 k) const { return taps + (size_t)row * NC_TAP_STRIDE + NC_TAP_PAD + (size_t)k; }
};
// slow buffer: shift [NS_MAX_LEVELS] | amplitudes [rows][NS_MAX_LEVELS] | for a model without a colour, unit taps [channels][NC_TAP_STRIDE]
// that stand in for the colour buffer's (a white model has no groups: rows = channels)
struct NoiseSlowLayout {
    size_t shifts, amps, unit_taps, size;
    NoiseSlowLayout(i32 channels, i32 groups, bool colour)
        : shifts(0), amps(NS_MAX_LEVELS), unit_taps(amps + (size_t)(channels + (colour ? groups : 0)) * NS_MAX_LEVELS),
          size(unit_taps + (colour ? 0 : (size_t)channels * NC_TAP_STRIDE)) {}
    size_t amp(i32 row, i32 j) const { return amps + (size_t)row * NS_MAX_LEVELS + (size_t)j; }
    size_t unit_tap(i32 channel) const { return unit_taps + (size_t)channel * NC_TAP_STRIDE + NC_TAP_PAD; }
};

// ---- the checks: arguments in, packed words out, or false and a message --------------------------------------------------------------
// Rows of a probability mass function ("<what> ... <unit> N" in the messages): every entry non-negative, every row sums to 1;
// cum takes the cumulative rows, [n_rows][n_values], from which the engine builds the alias cells.
inline bool noise_pmf_rows(const std::string &what, const char *unit, i32 n_rows, i32 n_values, const double *pmf, std::vector<double> &cum, std::string &err)
{
    cum.resize((size_t)n_rows * (size_t)n_values);
    for (i32 r = 0; r < n_rows; r++) {
        const double *row = pmf + (size_t)r * n_values;
        double acc = 0;
        for (i32 v = 0; v < n_values; v++) {
            if (!(row[v] >= 0.0)) { err = what + " has a negative (or NaN) entry in " + unit + " " + std::to_string(r); return false; }
            acc += row[v]; cum[(size_t)r * n_values + v] = acc;
        }
        if (!(fabs(acc - 1.0) <= 1e-9)) { err = what + " of " + unit + " " + std::to_string(r) + " does not sum to 1"; return false; }
    }
    return true;
}
inline i64 noise_vmax(i32 vmin, i32 values) { const i64 lo = std::llabs((long long)vmin), hi = std::llabs((long long)vmin + values - 1); return lo > hi ? lo : hi; }
// what keeps every int32 sum of the kernels exact: (sum of |Q16 weights| of a row) * max |value| stays below 2^29
inline bool noise_sum_fits(i64 weight_sum, i64 vmax) { return weight_sum * vmax < ((i64)1 << 29); }

inline bool noise_model_check(i32 n_channels, i32 max_channels, i32 n_values, i32 vmin, const double *pmf, std::vector<double> &cum, std::string &err)
{
    const std::string f = "wfs_set_noise_model: ";
    if (n_channels < 0 || n_channels > max_channels) { err = f + "n_channels outside 0 .. n_rows of the digitiser array"; return false; }
    if (n_values < 1 || n_values > NM_MAX_VALUES) { err = f + "n_values outside 1 .. 4096"; return false; }
    if (vmin < -32768 || (i64)vmin + n_values - 1 > 32767) { err = f + "vmin .. vmin + n_values - 1 leaves the int16 range"; return false; }
    if (!pmf) { err = f + "null pmf"; return false; }
    return noise_pmf_rows(f + "pmf", "channel", n_channels, n_values, pmf, cum, err);
}

// buf: the colour buffer (NoiseColourLayout of the model's channels and n_groups); tapsum: per row; common_cum: the cumulative rows of
// the common streams
inline bool noise_colour_pack(const NoiseModelState &m, i32 n_taps, const i32 *taps_q, i32 n_groups, const i32 *group, const i32 *mix_q, const double *common_pmf,
                              std::vector<i32> &buf, std::vector<i64> &tapsum, std::vector<double> &common_cum, std::string &err)
{
    const std::string f = "wfs_set_noise_colour: ";
    if (n_taps < 1 || n_taps > NC_MAX_TAPS) { err = f + "n_taps outside 1 .. 16"; return false; }
    if (n_groups < 0 || n_groups > NC_MAX_GROUPS) { err = f + "n_groups outside 0 .. 1024"; return false; }
    if (!taps_q) { err = f + "null taps_q"; return false; }
    if (n_groups > 0 && (!group || !mix_q || !common_pmf)) { err = f + "null group, mix_q or common_pmf with n_groups > 0"; return false; }
    const i32 C = m.channels, R = C + n_groups;
    const i64 vmax = noise_vmax(m.vmin, m.values);
    const NoiseColourLayout at(C, n_groups);
    buf.assign(at.size, 0); tapsum.assign((size_t)R, 0);
    for (i32 r = 0; r < R; r++) {
        i64 sum = 0;
        for (i32 k = 0; k < n_taps; k++) { const i32 v = taps_q[(size_t)r * n_taps + k]; sum += std::llabs((long long)v); buf[at.tap(r, k)] = v; }
        tapsum[(size_t)r] = sum;
        if (!noise_sum_fits(sum, vmax)) { err = f + "taps_q of row " + std::to_string(r) + ": sum |taps| * max |value| reaches 2^29"; return false; }
    }
    for (i32 c = 0; c < C; c++) {
        const i32 g = n_groups > 0 ? group[c] : -1, x = n_groups > 0 ? mix_q[c] : 0;
        buf[at.group + (size_t)c] = g; buf[at.mix + (size_t)c] = x;
        if (g < -1 || g >= n_groups) { err = f + "group of channel " + std::to_string(c) + " outside -1 .. n_groups - 1"; return false; }
        if (x < -NC_MAX_MIX || x > NC_MAX_MIX) { err = f + "mix_q of channel " + std::to_string(c) + " beyond 65536 in magnitude"; return false; }
    }
    return noise_pmf_rows(f + "common_pmf", "group", n_groups, m.values, common_pmf, common_cum, err);
}

// buf: the slow buffer (NoiseSlowLayout of the model as it stands); the shifts of the levels that are not there repeat the last one
inline bool noise_slow_pack(const NoiseModelState &m, i32 n_levels, const i32 *shifts, const i32 *slow_q, std::vector<i32> &buf, std::string &err)
{
    const std::string f = "wfs_set_noise_slow: ";
    if (n_levels < 1 || n_levels > NS_MAX_LEVELS) { err = f + "n_levels outside 0 .. 8"; return false; }
    if (!shifts || !slow_q) { err = f + "null shifts or slow_q"; return false; }
    for (i32 j = 0; j < n_levels; j++) {
        if (shifts[j] < NS_MIN_SHIFT || shifts[j] > NS_MAX_SHIFT) { err = f + "shifts[" + std::to_string(j) + "] outside 4 .. 30"; return false; }
        if (j > 0 && shifts[j] <= shifts[j - 1]) { err = f + "shifts not strictly ascending at level " + std::to_string(j); return false; }
    }
    const bool colour = m.coloured();
    const i32 C = m.channels, R = C + (colour ? m.colour.groups : 0);
    const i64 vmax = noise_vmax(m.vmin, m.values);
    const NoiseSlowLayout at(C, m.colour.groups, colour);
    buf.assign(at.size, 0);
    for (i32 j = 0; j < NS_MAX_LEVELS; j++) buf[at.shifts + (size_t)j] = shifts[j < n_levels ? j : n_levels - 1];
    for (i32 r = 0; r < R; r++) {
        i64 sum = colour ? m.colour.tapsum[(size_t)r] : NC_UNIT;     // (without a colour F = 65536 w)
        for (i32 j = 0; j < n_levels; j++) { const i32 v = slow_q[(size_t)r * n_levels + j]; sum += std::llabs((long long)v); buf[at.amp(r, j)] = v; }
        if (!noise_sum_fits(sum, vmax)) { err = f + "slow_q of row " + std::to_string(r) + ": (sum |taps| + sum |slow|) * max |value| reaches 2^29"; return false; }
    }
    if (!colour) for (i32 c = 0; c < C; c++) buf[at.unit_tap(c)] = NC_UNIT;
    return true;
}

// ---- the transitions: nothing else writes the state ----------------------------------------------------------------------------------
// Each returns the device buffers that no longer describe anything and are to be dropped (the handle keeps the three buffers next to
// the state): the cells, the colour buffer, the slow buffer.
enum NoiseBuf : unsigned { NOISE_BUF_NONE = 0, NOISE_BUF_CELLS = 1, NOISE_BUF_COLOUR = 2, NOISE_BUF_SLOW = 4 };
struct NoiseTransitions {
    NoiseModelState &m;
    // a model of these shapes is on the device; a colour and slow levels belong to the shapes of the model they were set on
    unsigned model_set(i32 channels, i32 k, i32 shift, i32 vmin, i32 values, std::vector<NoiseCell> &&cells) const
    {
        m = NoiseModelState{};
        m.channels = channels; m.k = k; m.shift = shift; m.vmin = vmin; m.values = values; m.cells = std::move(cells);
        return NOISE_BUF_COLOUR | NOISE_BUF_SLOW;
    }
    unsigned model_cleared() const { m = NoiseModelState{}; return NOISE_BUF_CELLS | NOISE_BUF_COLOUR | NOISE_BUF_SLOW; }
    // the slow levels belong to the rows of the colour they were set on
    unsigned colour_set(i32 n_taps, i32 groups, std::vector<i64> &&tapsum) const
    {
        m.colour = NoiseColourState{};
        m.colour.n_taps = n_taps; m.colour.groups = groups; m.colour.tapsum = std::move(tapsum);
        return NOISE_BUF_SLOW;
    }
    unsigned colour_cleared() const { m.colour = NoiseColourState{}; return NOISE_BUF_COLOUR | NOISE_BUF_SLOW; }
    unsigned slow_set(i32 levels) const { m.colour.slow = NoiseSlowState{}; m.colour.slow.levels = levels; return NOISE_BUF_NONE; }
    unsigned slow_cleared() const { m.colour.slow = NoiseSlowState{}; return NOISE_BUF_SLOW; }
};
