// Drives the noise-model state of a handle (wfsim_amd/csrc/wfs_noise.h) on the host: the transitions are the only writers of the
// state, a level is reset by assignment of a value-initialised struct, the two device buffers have one layout description each, and
// the setters' checks are pure functions from the arguments to the packed words or a message.
// Prints one line "<case> ok|FAILED" per case and exits 0 when every case holds (tests/test_noise_state_cpu.py).
#include "wfs_noise.h"

#include <cstdio>
#include <tuple>

// Every member of the three structs, once.  The structured bindings name as many members as the structs have, so a member added to
// wfs_noise.h stops this file from compiling until it is listed here -- and then every "back at its initial value" check covers it.
static auto members(const NoiseSlowState &s)
{
    const auto &[levels] = s;
    return std::tie(levels);
}
static auto members(const NoiseColourState &c)
{
    const auto &[n_taps, groups, tapsum, slow] = c;
    return std::tuple_cat(std::tie(n_taps, groups, tapsum), members(slow));
}
static bool same_cells(const std::vector<NoiseCell> &a, const std::vector<NoiseCell> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (a[i].x != b[i].x || a[i].y != b[i].y) return false;
    return true;
}
static bool same(const NoiseColourState &a, const NoiseColourState &b) { return members(a) == members(b); }
static bool same(const NoiseModelState &a, const NoiseModelState &b)
{
    const auto &[channels, k, shift, vmin, values, cells, colour] = a;
    const auto &[channels_b, k_b, shift_b, vmin_b, values_b, cells_b, colour_b] = b;
    return std::tie(channels, k, shift, vmin, values) == std::tie(channels_b, k_b, shift_b, vmin_b, values_b) && same_cells(cells, cells_b) && same(colour, colour_b);
}
template <class T> static bool initial(const T &a) { return same(a, T{}); }

static int failures = 0;
static void report(const char *name, bool ok)
{
    printf("%s %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) failures++;
}

static const unsigned CELLS = NOISE_BUF_CELLS, COLOUR = NOISE_BUF_COLOUR, SLOW = NOISE_BUF_SLOW;

// a model of 3 channels and 9 values from -4, a colour of 3 taps with two groups, two slow levels: nothing at its initial value
static std::vector<NoiseCell> some_cells(i32 channels, i32 k) { return std::vector<NoiseCell>((size_t)channels * k, NoiseCell{7u, 1u}); }
static void set_model(const NoiseTransitions &t) { t.model_set(3, 16, 28, -4, 9, some_cells(3, 16)); }
static void set_colour(const NoiseTransitions &t) { t.colour_set(3, 2, std::vector<i64>{10, 20, 30, 40, 50}); }
static void set_all(const NoiseTransitions &t) { set_model(t); set_colour(t); t.slow_set(2); }

// the message of a refused call ("" when it passed)
static std::string model_msg(i32 n_channels, i32 max_channels, i32 n_values, i32 vmin, const double *pmf)
{
    std::vector<double> cum; std::string err;
    return noise_model_check(n_channels, max_channels, n_values, vmin, pmf, cum, err) ? "" : err;
}
static std::string colour_msg(const NoiseModelState &m, i32 n_taps, const i32 *taps, i32 n_groups, const i32 *group, const i32 *mix, const double *pmf)
{
    std::vector<i32> buf; std::vector<i64> tapsum; std::vector<double> cum; std::string err;
    return noise_colour_pack(m, n_taps, taps, n_groups, group, mix, pmf, buf, tapsum, cum, err) ? "" : err;
}
static std::string slow_msg(const NoiseModelState &m, i32 n_levels, const i32 *shifts, const i32 *slow)
{
    std::vector<i32> buf; std::string err;
    return noise_slow_pack(m, n_levels, shifts, slow, buf, err) ? "" : err;
}
// a model of 2 channels with values vmin .. vmin + values - 1 (the shapes of the edge cases of tests/test_noise_colour_cpu.py / test_noise_slow_cpu.py)
static NoiseModelState edge_model(i32 values, i32 vmin)
{
    NoiseModelState m; const NoiseTransitions t{m};
    t.model_set(2, 32, 27, vmin, values, some_cells(2, 32));
    return m;
}

int main()
{
    {
        NoiseModelState m;
        report("fresh", initial(m) && !m.set() && !m.coloured() && m.levels() == 0 && m.rows() == 0);
        NoiseModelState f; const NoiseTransitions t{f};
        set_all(t);
        const auto &[channels, k, shift, vmin, values, cells, colour] = f;
        const auto &[n_taps, groups, tapsum, slow] = colour;
        const auto &[levels] = slow;
        report("fill_sets_every_member", channels && k && shift && vmin && values && !cells.empty() && n_taps && groups && !tapsum.empty() && levels
                                          && f.set() && f.coloured() && f.levels() == 2 && f.rows() == 5);
    }
    {   // model_set: the shapes and the cells, a white model without levels; asks for the colour and slow buffers to go
        NoiseModelState m; const NoiseTransitions t{m};
        const unsigned dropped = t.model_set(3, 16, 28, -4, 9, some_cells(3, 16));
        NoiseModelState want; want.channels = 3; want.k = 16; want.shift = 28; want.vmin = -4; want.values = 9; want.cells = some_cells(3, 16);
        report("model_set", dropped == (COLOUR | SLOW) && same(m, want) && m.set() && !m.coloured() && m.levels() == 0 && m.rows() == 3);
    }
    {
        NoiseModelState m; const NoiseTransitions t{m};
        set_all(t);
        const unsigned dropped = t.model_cleared();
        report("model_cleared", dropped == (CELLS | COLOUR | SLOW) && initial(m));
    }
    {   // a colour and slow levels belong to the shapes of the model they were set on
        NoiseModelState m; const NoiseTransitions t{m};
        set_all(t);
        const unsigned dropped = t.model_set(2, 8, 29, -2, 5, some_cells(2, 8));
        report("model_set_drops_colour_and_levels", dropped == (COLOUR | SLOW) && initial(m.colour) && m.channels == 2 && m.k == 8 && m.shift == 29
                                                     && m.vmin == -2 && m.values == 5 && m.cells.size() == 16 && m.rows() == 2);
    }
    {   // colour_set: taps, groups, tapsum; the model stays; the levels of the rows before are gone
        NoiseModelState m; const NoiseTransitions t{m};
        set_model(t);
        const NoiseModelState before = m;
        unsigned dropped = t.colour_set(3, 2, std::vector<i64>{10, 20, 30, 40, 50});
        NoiseModelState want = before; want.colour.n_taps = 3; want.colour.groups = 2; want.colour.tapsum = {10, 20, 30, 40, 50};
        bool ok = dropped == SLOW && same(m, want) && m.coloured() && m.rows() == 5;
        t.slow_set(2);
        dropped = t.colour_set(16, 0, std::vector<i64>{1, 2, 3});
        want.colour = NoiseColourState{}; want.colour.n_taps = 16; want.colour.tapsum = {1, 2, 3};
        ok = ok && dropped == SLOW && same(m, want) && m.levels() == 0 && m.rows() == 3;
        report("colour_set_drops_levels", ok);
    }
    {
        NoiseModelState m; const NoiseTransitions t{m};
        set_model(t);
        const NoiseModelState before = m;
        set_colour(t); t.slow_set(2);
        const unsigned dropped = t.colour_cleared();
        report("colour_cleared_drops_levels", dropped == (COLOUR | SLOW) && same(m, before) && !m.coloured() && m.levels() == 0);
    }
    {   // slow levels on a colour and on a white model; cleared, everything else stays
        bool ok = true;
        for (int coloured = 0; coloured < 2; coloured++) {
            NoiseModelState m; const NoiseTransitions t{m};
            set_model(t);
            if (coloured) set_colour(t);
            const NoiseModelState before = m;
            unsigned dropped = t.slow_set(2);
            NoiseModelState want = before; want.colour.slow.levels = 2;
            ok = ok && dropped == NOISE_BUF_NONE && same(m, want) && m.levels() == 2 && m.coloured() == (coloured != 0);
            dropped = t.slow_set(5);
            ok = ok && dropped == NOISE_BUF_NONE && m.levels() == 5;
            dropped = t.slow_cleared();
            ok = ok && dropped == SLOW && same(m, before);
        }
        report("slow_set_and_cleared", ok);
    }
    {   // colour buffer with groups: taps [C + G][stride] | group [C] | mix [C]
        const NoiseColourLayout at(3, 2);
        report("layout_colour_with_groups", at.taps == 0 && at.group == 5 * (size_t)NC_TAP_STRIDE && at.mix == at.group + 3 && at.size == at.group + 6
                                             && at.tap(0, 0) == (size_t)NC_TAP_PAD && at.tap(4, 15) == 4 * (size_t)NC_TAP_STRIDE + NC_TAP_PAD + 15 && at.tap(4, 15) + NC_TAP_PAD < at.group
                                             && NC_TAP_STRIDE == NC_MAX_TAPS + 2 * NC_TAP_PAD);
        const NoiseSlowLayout sl(3, 2, true);
        report("layout_slow_on_colour", sl.shifts == 0 && sl.amps == (size_t)NS_MAX_LEVELS && sl.amp(4, 7) == (size_t)NS_MAX_LEVELS * 6 - 1 && sl.unit_taps == (size_t)NS_MAX_LEVELS * 6
                                         && sl.size == sl.unit_taps);
    }
    {
        const NoiseColourLayout at(3, 0);
        report("layout_colour_without_groups", at.taps == 0 && at.group == 3 * (size_t)NC_TAP_STRIDE && at.mix == at.group + 3 && at.size == at.group + 6);
    }
    {   // levels without a colour: the unit taps behind the amplitudes, 1.0 at NC_TAP_PAD of every channel's row and zeros around it
        const NoiseSlowLayout sl(3, 0, false);
        bool ok = sl.amps == (size_t)NS_MAX_LEVELS && sl.unit_taps == (size_t)NS_MAX_LEVELS * 4 && sl.size == sl.unit_taps + 3 * (size_t)NC_TAP_STRIDE
                  && sl.unit_tap(2) == sl.unit_taps + 2 * (size_t)NC_TAP_STRIDE + NC_TAP_PAD;
        NoiseModelState m; const NoiseTransitions t{m};
        set_model(t);
        const i32 shifts[2] = {4, 6}, slow[6] = {1, -2, 3, -4, 5, -6};
        std::vector<i32> buf; std::string err;
        ok = ok && noise_slow_pack(m, 2, shifts, slow, buf, err) && buf.size() == sl.size;
        for (i32 j = 0; ok && j < NS_MAX_LEVELS; j++) ok = buf[sl.shifts + j] == (j == 0 ? 4 : 6);      // (the levels that are not there repeat the last shift)
        for (i32 r = 0; ok && r < 3; r++) for (i32 j = 0; j < NS_MAX_LEVELS; j++) ok = ok && buf[sl.amp(r, j)] == (j < 2 ? slow[2 * r + j] : 0);
        for (i32 c = 0; ok && c < 3; c++) for (i32 u = 0; u < NC_TAP_STRIDE; u++) ok = ok && buf[sl.unit_taps + (size_t)c * NC_TAP_STRIDE + u] == (u == NC_TAP_PAD ? 65536 : 0);
        report("layout_levels_without_colour", ok);
    }
    {   // what the packers write: taps at their pads, groups and gains behind; tapsum per row; the amplitudes of every stream
        NoiseModelState m; const NoiseTransitions t{m};
        set_model(t);
        const i32 taps[15] = {1, 2, 3, -4, 5, 6, 7, 8, -9, 10, 11, 12, 13, 14, -15}, group[3] = {0, -1, 1}, mix[3] = {100, 0, -65536};
        const double pmf[18] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0, 0, 0, 0.5};
        std::vector<i32> buf; std::vector<i64> tapsum; std::vector<double> cum; std::string err;
        bool ok = noise_colour_pack(m, 3, taps, 2, group, mix, pmf, buf, tapsum, cum, err);
        const NoiseColourLayout at(3, 2);
        ok = ok && buf.size() == at.size && tapsum == std::vector<i64>{6, 15, 24, 33, 42} && cum.size() == 18 && cum[3] == 0 && cum[4] == 1 && cum[9] == 0.5 && cum[17] == 1;
        for (i32 r = 0; ok && r < 5; r++) for (i32 u = 0; u < NC_TAP_STRIDE; u++) {
            const i32 k = u - NC_TAP_PAD;
            ok = ok && buf[at.taps + (size_t)r * NC_TAP_STRIDE + u] == (k >= 0 && k < 3 ? taps[3 * r + k] : 0);
        }
        for (i32 c = 0; ok && c < 3; c++) ok = buf[at.group + c] == group[c] && buf[at.mix + c] == mix[c];
        // without groups the channels have group -1 and gain 0, whatever the pointers
        ok = ok && noise_colour_pack(m, 3, taps, 0, nullptr, nullptr, nullptr, buf, tapsum, cum, err) && buf.size() == NoiseColourLayout(3, 0).size && tapsum.size() == 3 && cum.empty();
        for (i32 c = 0; ok && c < 3; c++) ok = buf[NoiseColourLayout(3, 0).group + c] == -1 && buf[NoiseColourLayout(3, 0).mix + c] == 0;
        // slow levels on the colour: one amplitude row per stream, no unit taps
        set_colour(t);
        const i32 shifts[2] = {4, 6}, slow[10] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
        std::vector<i32> sb;
        const NoiseSlowLayout sl(3, 2, true);
        ok = ok && noise_slow_pack(m, 2, shifts, slow, sb, err) && sb.size() == sl.size && sb[sl.amp(4, 1)] == 10 && sb[sl.amp(4, 2)] == 0 && sb[sl.amp(0, 0)] == 1;
        report("packers_fill_the_layouts", ok);
    }
    {
        const double good[4] = {0.25, 0.75, 1.0, 0.0}, neg[4] = {0.5, 0.5, 1.5, -0.5}, nan_[4] = {0.5, 0.5, std::nan(""), 1.0}, off[4] = {0.5, 0.5, 0.5, 0.4};
        bool ok = model_msg(2, 494, 2, -1, good) == ""
            && model_msg(-1, 494, 2, -1, good) == "wfs_set_noise_model: n_channels outside 0 .. n_rows of the digitiser array"
            && model_msg(495, 494, 2, -1, good) == "wfs_set_noise_model: n_channels outside 0 .. n_rows of the digitiser array"
            && model_msg(2, 494, 0, -1, good) == "wfs_set_noise_model: n_values outside 1 .. 4096"
            && model_msg(2, 494, 4097, -1, good) == "wfs_set_noise_model: n_values outside 1 .. 4096"
            && model_msg(2, 494, 2, -32769, good) == "wfs_set_noise_model: vmin .. vmin + n_values - 1 leaves the int16 range"
            && model_msg(2, 494, 2, 32767, good) == "wfs_set_noise_model: vmin .. vmin + n_values - 1 leaves the int16 range"
            && model_msg(2, 494, 2, 32766, good) == ""
            && model_msg(2, 494, 2, -1, nullptr) == "wfs_set_noise_model: null pmf"
            && model_msg(2, 494, 2, -1, neg) == "wfs_set_noise_model: pmf has a negative (or NaN) entry in channel 1"
            && model_msg(2, 494, 2, -1, nan_) == "wfs_set_noise_model: pmf has a negative (or NaN) entry in channel 1"
            && model_msg(2, 494, 2, -1, off) == "wfs_set_noise_model: pmf of channel 1 does not sum to 1";
        std::vector<double> cum; std::string err;
        ok = ok && noise_model_check(2, 494, 2, -1, good, cum, err) && cum == std::vector<double>{0.25, 1.0, 1.0, 1.0};
        report("model_refusals", ok);
    }
    {
        NoiseModelState m; const NoiseTransitions t{m};
        set_model(t);                                   // 3 channels, 9 values
        const i32 taps[5] = {1, 1, 1, 1, 1}, g_ok[3] = {0, -1, 1}, g_hi[3] = {0, 2, 1}, g_lo[3] = {0, -2, 1}, x_ok[3] = {65536, 0, -65536}, x_hi[3] = {0, 65537, 0}, x_lo[3] = {0, 0, -65537};
        std::vector<i32> many((size_t)3 * 17, 1);
        double pmf[18] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0, 0, 0, 0.5}, bad[18], off[18];
        for (int i = 0; i < 18; i++) { bad[i] = pmf[i]; off[i] = pmf[i]; }
        bad[10] = -0.1; off[17] = 0.4;
        const bool ok = colour_msg(m, 1, taps, 2, g_ok, x_ok, pmf) == ""
            && colour_msg(m, 0, taps, 2, g_ok, x_ok, pmf) == "wfs_set_noise_colour: n_taps outside 1 .. 16"
            && colour_msg(m, 17, many.data(), 0, nullptr, nullptr, nullptr) == "wfs_set_noise_colour: n_taps outside 1 .. 16"
            && colour_msg(m, 1, taps, -1, g_ok, x_ok, pmf) == "wfs_set_noise_colour: n_groups outside 0 .. 1024"
            && colour_msg(m, 1, taps, 1025, g_ok, x_ok, pmf) == "wfs_set_noise_colour: n_groups outside 0 .. 1024"
            && colour_msg(m, 1, nullptr, 2, g_ok, x_ok, pmf) == "wfs_set_noise_colour: null taps_q"
            && colour_msg(m, 1, taps, 2, nullptr, x_ok, pmf) == "wfs_set_noise_colour: null group, mix_q or common_pmf with n_groups > 0"
            && colour_msg(m, 1, taps, 2, g_ok, nullptr, pmf) == "wfs_set_noise_colour: null group, mix_q or common_pmf with n_groups > 0"
            && colour_msg(m, 1, taps, 2, g_ok, x_ok, nullptr) == "wfs_set_noise_colour: null group, mix_q or common_pmf with n_groups > 0"
            && colour_msg(m, 1, taps, 2, g_hi, x_ok, pmf) == "wfs_set_noise_colour: group of channel 1 outside -1 .. n_groups - 1"
            && colour_msg(m, 1, taps, 2, g_lo, x_ok, pmf) == "wfs_set_noise_colour: group of channel 1 outside -1 .. n_groups - 1"
            && colour_msg(m, 1, taps, 2, g_ok, x_hi, pmf) == "wfs_set_noise_colour: mix_q of channel 1 beyond 65536 in magnitude"
            && colour_msg(m, 1, taps, 2, g_ok, x_lo, pmf) == "wfs_set_noise_colour: mix_q of channel 2 beyond 65536 in magnitude"
            && colour_msg(m, 1, taps, 2, g_ok, x_ok, bad) == "wfs_set_noise_colour: common_pmf has a negative (or NaN) entry in group 1"
            && colour_msg(m, 1, taps, 2, g_ok, x_ok, off) == "wfs_set_noise_colour: common_pmf of group 1 does not sum to 1";
        report("colour_refusals", ok);
    }
    {
        NoiseModelState m; const NoiseTransitions t{m};
        set_model(t);
        const i32 slow[6] = {1, 1, 1, 1, 1, 1}, up[2] = {4, 6}, low[2] = {3, 6}, high[2] = {4, 31}, down[2] = {6, 4}, flat[2] = {6, 6}, nine[9] = {4, 5, 6, 7, 8, 9, 10, 11, 12};
        std::vector<i32> wide((size_t)3 * 9, 1);
        const bool ok = slow_msg(m, 2, up, slow) == "" && slow_msg(m, 1, high + 0, slow) == ""
            && slow_msg(m, 9, nine, wide.data()) == "wfs_set_noise_slow: n_levels outside 0 .. 8"
            && slow_msg(m, -1, up, slow) == "wfs_set_noise_slow: n_levels outside 0 .. 8"
            && slow_msg(m, 2, nullptr, slow) == "wfs_set_noise_slow: null shifts or slow_q"
            && slow_msg(m, 2, up, nullptr) == "wfs_set_noise_slow: null shifts or slow_q"
            && slow_msg(m, 2, low, slow) == "wfs_set_noise_slow: shifts[0] outside 4 .. 30"
            && slow_msg(m, 2, high, slow) == "wfs_set_noise_slow: shifts[1] outside 4 .. 30"
            && slow_msg(m, 2, down, slow) == "wfs_set_noise_slow: shifts not strictly ascending at level 1"
            && slow_msg(m, 2, flat, slow) == "wfs_set_noise_slow: shifts not strictly ascending at level 1";
        report("slow_refusals", ok);
    }
    {   // sum |taps| * max |value| < 2^29, at its edge (the values of tests/test_noise_colour_cpu.py test_overflow_bound_at_its_edge)
        const NoiseModelState one = edge_model(3, -1);             // values -1 .. 1: the bound is on sum |taps_q| itself
        std::vector<i32> row(16, 1 << 25); row[3] = -row[3];       // sum = 2^29
        std::vector<i32> edge(row); edge[7] -= 1;                  // 2^29 - 1
        std::vector<i32> pass(edge), fail(edge);
        pass.insert(pass.end(), edge.begin(), edge.end()); fail.insert(fail.end(), row.begin(), row.end());
        bool ok = noise_vmax(-1, 3) == 1 && noise_vmax(-12, 25) == 12 && noise_vmax(-4, 2) == 4 && noise_vmax(5, 3) == 7
                  && noise_sum_fits(((i64)1 << 29) - 1, 1) && !noise_sum_fits((i64)1 << 29, 1);
        ok = ok && colour_msg(one, 16, pass.data(), 0, nullptr, nullptr, nullptr) == ""
                && colour_msg(one, 16, fail.data(), 0, nullptr, nullptr, nullptr) == "wfs_set_noise_colour: taps_q of row 1: sum |taps| * max |value| reaches 2^29";
        const NoiseModelState twelve = edge_model(25, -12);        // max |value| = 12: the same figure bounds the product
        const i32 at = ((1 << 29) - 1) / 12, in[2] = {at, -at}, out[2] = {at, -at - 1};
        ok = ok && colour_msg(twelve, 1, in, 0, nullptr, nullptr, nullptr) == ""
                && colour_msg(twelve, 1, out, 0, nullptr, nullptr, nullptr) == "wfs_set_noise_colour: taps_q of row 1: sum |taps| * max |value| reaches 2^29";
        report("colour_bound_at_its_edge", ok);
    }
    {   // (sum |taps| + sum |slow|) * max |value| < 2^29, at its edge (the values of tests/test_noise_slow_cpu.py test_overflow_bound_at_its_edge)
        NoiseModelState one = edge_model(3, -1);
        NoiseTransitions{one}.colour_set(16, 0, std::vector<i64>{(i64)1 << 28, (i64)1 << 28});      // taps 16 x 2^24 per row
        std::vector<i32> full(8, 1 << 25); full[2] = -full[2];     // sum |slow| = 2^28: together 2^29
        std::vector<i32> edge(full); edge[5] -= 1;                 // 2^29 - 1
        std::vector<i32> pass(edge), fail(edge);
        pass.insert(pass.end(), edge.begin(), edge.end()); fail.insert(fail.end(), full.begin(), full.end());
        const i32 sh[8] = {4, 5, 6, 7, 8, 9, 10, 11}, four[1] = {4};
        bool ok = slow_msg(one, 8, sh, pass.data()) == ""
                  && slow_msg(one, 8, sh, fail.data()) == "wfs_set_noise_slow: slow_q of row 1: (sum |taps| + sum |slow|) * max |value| reaches 2^29";
        // without a colour the taps count as one unit tap: 65536
        const NoiseModelState white = edge_model(3, -1);
        const i32 at = (1 << 29) - 1 - 65536, in[2] = {at, -at}, out[2] = {at, -at - 1};
        ok = ok && slow_msg(white, 1, four, in) == ""
                && slow_msg(white, 1, four, out) == "wfs_set_noise_slow: slow_q of row 1: (sum |taps| + sum |slow|) * max |value| reaches 2^29";
        const NoiseModelState twelve = edge_model(25, -12);
        const i32 at12 = ((1 << 29) - 1) / 12 - 65536, in12[2] = {at12, -at12}, out12[2] = {at12 + 1, -at12};
        ok = ok && slow_msg(twelve, 1, four, in12) == ""
                && slow_msg(twelve, 1, four, out12) == "wfs_set_noise_slow: slow_q of row 0: (sum |taps| + sum |slow|) * max |value| reaches 2^29";
        report("slow_bound_at_its_edge", ok);
    }
    return failures ? 1 : 0;
}
