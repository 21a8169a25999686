// The host-only pieces of wfsim_amd/csrc/wfs_lone.h, compiled with the host compiler and run on its own (tests/test_lone_hits_cpu.py):
// the cells of a range, the clipped range of a chain, ix_rand, the check of wfs_lone_hits' arguments and the bound on
// right_raw_extension.  One line per case: its name and `ok`, or what went wrong.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "wfs_lone.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (!bad++) std::printf(" failed:"); std::printf(" [%s]", #c); } } while (0)
#define CASE(name) for (int bad = 0, once = (std::printf("%s", name), 1); once; once = 0, std::printf(bad ? "\n" : " ok\n"), failures += bad)

int main()
{
    const i64 tlen = 22, tw = 50, before = 2, G = lone_gap(tlen, tw);
    const i64 NONE_L = -0x7fffffffffffffffLL - 1, NONE_R = 0x7fffffffffffffffLL;
    CASE("gap") { CHECK(G == 122); CHECK(lone_gap(1, 0) == 1); }
    CASE("cells") {
        // starts a .. b - 1 have idx = start + before in the cells (a + before) >> 6 .. (b - 1 + before) >> 6, negative starts included
        CHECK(lone_first_cell(0, before) == 0 && lone_last_cell(62, before) == 0 && lone_last_cell(63, before) == 1);
        CHECK(lone_first_cell(-2, before) == 0 && lone_first_cell(-3, before) == -1 && lone_first_cell(-66, before) == -1 && lone_first_cell(-67, before) == -2);
        CHECK(lone_last_cell(-2, before) == -1 && lone_last_cell(-1, before) == 0);
        CHECK(lone_first_cell(((i64)1 << 47) + 5, before) == (((i64)1 << 47) + 7) >> 6);
    }
    CASE("pulse_meets") {
        CHECK(!lone_pulse_meets(100 - tlen, tlen, 100, 300));     // last pulse sample row_lo - 1: lone
        CHECK(lone_pulse_meets(101 - tlen, tlen, 100, 300));      // last pulse sample row_lo: not lone
        CHECK(lone_pulse_meets(300, tlen, 100, 300));             // first sample row_hi: not lone
        CHECK(!lone_pulse_meets(301, tlen, 100, 300));            // first sample row_hi + 1: lone
    }
    CASE("range") {
        LoneRange r = lone_range(1000, 1000, tlen, tw, NONE_L, NONE_R, 5000);
        CHECK(r.left == 950 && r.right == 1000 + tlen - 1 + tw);
        r = lone_range(1000, 1100, tlen, tw, NONE_L, NONE_R, 5000);
        CHECK(r.left == 950 && r.right == 1100 + tlen - 1 + tw && r.right - r.left + 1 == row_span(1000, 1100 + tlen - 1, tw).len);
        r = lone_range(1000, 1000, tlen, tw, 999, NONE_R, 5000);          // a row ends right in front of the pulse
        CHECK(r.left == 1000);
        r = lone_range(1000, 1000, tlen, tw, 949, NONE_R, 5000);          // ... just outside the margin
        CHECK(r.left == 950);
        r = lone_range(1000, 1000, tlen, tw, 950, NONE_R, 5000);
        CHECK(r.left == 951);
        r = lone_range(1000, 1000, tlen, tw, NONE_L, 1000 + tlen, 5000);  // a row begins right behind the pulse
        CHECK(r.right == 1000 + tlen - 1);
        r = lone_range(1000, 1000, tlen, tw, NONE_L, 1000 + tlen + tw, 5000);
        CHECK(r.right == 1000 + tlen - 1 + tw);
        r = lone_range(1000, 1000, tlen, tw, NONE_L, NONE_R, 1010);       // s_limit cuts the row, never in front of its first photon
        CHECK(r.right == 1009 && r.right >= 1000);
    }
    CASE("straddle") {
        // the shortest row with a pulse is G long: the photons on its two sides start at least G + tlen apart
        CHECK(lone_cannot_straddle(G, tlen, tw) && !lone_cannot_straddle(G - 1, tlen, tw));
        const i64 rl = 500, rr = rl + G - 1, before_row = rl - tlen, behind_row = rr + 1;
        CHECK(!lone_pulse_meets(before_row, tlen, rl, rr) && !lone_pulse_meets(behind_row, tlen, rl, rr) && behind_row - before_row == G + tlen);
    }
    CASE("ix_rand") {
        CHECK(lone_ix_rand(0u, 3000) == 0 && lone_ix_rand(0xffffffffu, 3000) == 2999 && lone_ix_rand(0x80000000u, 3000) == 1500);
        CHECK(lone_ix_rand(12345u, 0) == 0 && lone_ix_rand(0xffffffffu, (i64)1 << 31) == ((i64)1 << 31) - 1);
    }
    CASE("check") {
        std::string e;
        CHECK(lone_check(0, 0, 0, 494, tlen, tw, before, e) == 0 && lone_check(-5, 7, 7, 494, tlen, tw, before, e) == 0);
        CHECK(lone_check(5, 4, 9, 494, tlen, tw, before, e) == 1 && e.find("s1 < s0") != std::string::npos);
        CHECK(lone_check(0, 9, 8, 494, tlen, tw, before, e) == 1 && e.find("s_limit < s1") != std::string::npos);
        CHECK(lone_check(-((i64)1 << 48) - 1, 0, 0, 494, tlen, tw, before, e) == 1 && lone_check(0, 1, ((i64)1 << 48) + 1, 494, tlen, tw, before, e) == 1);
        CHECK(lone_check(0, (i64)1 << 40, (i64)1 << 40, 1, tlen, tw, before, e) == 2 && e.find("lone hits") != std::string::npos);
        // 494 channels: 2^34 cells are 2^34 / 494 cells of a channel, 64 samples each
        const i64 fits = (LONE_MAX_CELLS / 494 - 4) * 64;
        CHECK(lone_check(0, fits, fits, 494, tlen, tw, before, e) == 0);
        CHECK(lone_check(0, fits + 1024, fits + 1024, 494, tlen, tw, before, e) == 2 && e.find("lone hits") != std::string::npos);
    }
    CASE("rext") {
        CHECK(lone_min_rext(10, tlen, tw) == (2 * 122 + 64) * 10);
        // two windows whose rows lie rext / dt - G - 2 samples apart are apart for the single look-up once rext reaches the bound
        const i64 rext = lone_min_rext(10, tlen, tw) / 10, a_hi = 1000, b_lo = a_hi + rext - G - 2;
        CHECK(lone_windows_apart(a_hi, b_lo, tlen, tw) && !lone_windows_apart(a_hi, a_hi + G, tlen, tw) && lone_windows_apart(a_hi, a_hi + G + 1, tlen, tw));
    }
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
