// The host-only pieces that the noise-hit seeds add to wfsim_amd/csrc/wfs_lone.h, compiled with the host compiler and run
// on its own (tests/test_lone_noise_cpu.py): the key of a seed, the test of a seed's sample against a row, the straddle argument, the
// blocks of the scan and their check.  One line per case: its name and `ok`, or what went wrong.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "wfs_lone.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (!bad++) std::printf(" failed:"); std::printf(" [%s]", #c); } } while (0)
#define CASE(name) for (int bad = 0, once = (std::printf("%s", name), 1); once; once = 0, std::printf(bad ? "\n" : " ok\n"), failures += bad)

int main()
{
    const i64 tlen = 22, tw = 50, G = lone_gap(tlen, tw);
    const i64 NONE_L = -0x7fffffffffffffffLL - 1, NONE_R = 0x7fffffffffffffffLL;
    CASE("key") {
        const unsigned long long k = lone_key(493, LONE_MAX_SPAN - 1, LONE_KIND_NOISE);
        CHECK(lone_key_channel(k) == 493 && lone_key_rel(k) == LONE_MAX_SPAN - 1 && lone_key_kind(k) == LONE_KIND_NOISE);
        CHECK(lone_key_channel(lone_key(0, 0, LONE_KIND_PHOTON)) == 0 && lone_key(0, 0, LONE_KIND_PHOTON) == 0ull);
        CHECK(lone_key_channel(lone_key(65535, 7, 1)) == 65535 && lone_key_rel(lone_key(65535, 7, 1)) == 7);
        // by (channel, start, kind): a photon sorts in front of a noise hit of the same start, both in front of the next start
        CHECK(lone_key(3, 100, LONE_KIND_PHOTON) < lone_key(3, 100, LONE_KIND_NOISE) && lone_key(3, 100, LONE_KIND_NOISE) < lone_key(3, 101, LONE_KIND_PHOTON));
        CHECK(lone_key(3, LONE_MAX_SPAN - 1, LONE_KIND_NOISE) < lone_key(4, 0, LONE_KIND_PHOTON));
        CHECK(LONE_KEY_SHIFT == 41 && LONE_KEY_START_BITS == 40);
    }
    CASE("seed_clear") {
        CHECK(lone_seed_clear(99, true, 100, 300) && !lone_seed_clear(100, true, 100, 300));      // row_lo - 1, row_lo
        CHECK(!lone_seed_clear(300, true, 100, 300) && lone_seed_clear(301, true, 100, 300));     // row_hi, row_hi + 1
        CHECK(lone_seed_clear(200, false, 100, 300));                                             // the channel has no row in the window
        // a photon there is not lone (its pulse reaches the row), a seed is clear: the test is on the sample
        CHECK(lone_pulse_meets(99, tlen, 100, 300) && lone_seed_clear(99, true, 100, 300));
    }
    CASE("seed_range") {
        // a seed directly behind a row starts behind it: the row in front clips the range at the seed
        LoneRange r = lone_range(301, 301, tlen, tw, 300, NONE_R, 5000);
        CHECK(r.left == 301 && r.right == 301 + tlen - 1 + tw);
        r = lone_range(99, 99, tlen, tw, NONE_L, 100, 5000);                                      // ... directly in front of one: a row of one sample at the least
        CHECK(r.left == 99 - tw && r.right == 99);
        r = lone_range(99, 99, tlen, tw, NONE_L, NONE_R, 100);                                    // s_limit right behind the seed
        CHECK(r.right == 99);
    }
    CASE("straddle") {
        CHECK(lone_seeds_cannot_straddle(G, tlen, tw) && lone_seeds_cannot_straddle(G + 7, tlen, tw) && !lone_seeds_cannot_straddle(G - 1, tlen, tw));
        const i64 rl = 500, rr = rl + G - 1;
        CHECK(lone_seed_clear(rl - 1, true, rl, rr) && lone_seed_clear(rr + 1, true, rl, rr) && (rr + 1) - (rl - 1) == G + 1);
    }
    CASE("blocks") {
        CHECK(lone_noise_blocks(0, 0) == 0 && lone_noise_blocks(5, 3) == 0 && lone_noise_blocks(0, 1) == 1 && lone_noise_blocks(0, 256) == 1 && lone_noise_blocks(0, 257) == 2);
        CHECK(lone_noise_blocks(-300, -44) == 1 && lone_noise_blocks(-300, -43) == 2 && lone_noise_blocks(-((i64)1 << 40), 0) == (i64)1 << 32);
    }
    CASE("check") {
        std::string e;
        CHECK(lone_noise_check(0, 1000, tlen, tw, e) == 0 && lone_noise_check(-((i64)1 << 38), 0, tlen, tw, e) == 0);
        const i64 fits = LONE_MAX_BLOCKS * LONE_NOISE_BLOCK - G;
        CHECK(lone_noise_check(0, fits, tlen, tw, e) == 0);
        CHECK(lone_noise_check(0, fits + 1, tlen, tw, e) == 2 && e.find("lone hits") != std::string::npos && e.find("noise hits") != std::string::npos);
    }
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
