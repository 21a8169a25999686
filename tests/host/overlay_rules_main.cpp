// wfsim_amd/csrc/wfs_overlay.h alone, compiled with the host compiler and run on its own (tests/test_overlay_cpu.py): the header of a
// record, the validity predicates, key packing at epoch-scale times, when pulses merge, and the sample rule.  One line per case: its
// name and `ok`, or what went wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "wfs_overlay.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (!bad++) std::printf(" failed:"); std::printf(" [%s]", #c); } } while (0)
#define CASE(name) for (int bad = 0, once = (std::printf("%s", name), 1); once; once = 0, std::printf(bad ? "\n" : " ok\n"), failures += bad)

static OvHeader rec(i64 s0, i32 plen, i32 f, i32 ch = 3, i32 dt = 10)
{
    u32 w[REC_HEADER_DWORDS];
    const RecHeader h = rec_header(dt, rec_dt_channel(dt, ch), s0, plen, f);
    std::memcpy(w, h.w, sizeof w);
    return ov_header(w);
}

int main()
{
    const i64 EPOCH = 1700000000000000000LL, E = EPOCH / 10;       // ns, samples of 10 ns
    CASE("header") {
        const OvHeader q = rec(E + 7, 331, 3, 800);
        CHECK(q.time == (E + 7 + 330) * 10 && q.length == 1 && q.dt == 10 && q.channel == 800 && q.pulse_length == 331 && q.record_i == 3);
        CHECK(ov_fragment_sample(q) == E + 337 && ov_pulse_sample(q) == E + 7 && ov_pulse_last(q) == E + 337);
        CHECK(rec(5, 110, 0).length == 110 && rec(5, 111, 0).length == 110 && rec(5, 111, 1).length == 1 && rec(5, 109, 0).length == 109);
    }
    CASE("record") {
        OvHeader q = rec(E, 250, 2);
        CHECK(ov_record_check(q, 10, 801) == OV_OK && q.length == 30);
        CHECK(ov_record_check(q, 2, 801) == OV_BAD_DT);
        q.time += 3; CHECK(ov_record_check(q, 10, 801) == OV_BAD_TIME); q.time -= 3;
        q.length = 0; CHECK(ov_record_check(q, 10, 801) == OV_BAD_LENGTH);
        q.length = 111; CHECK(ov_record_check(q, 10, 801) == OV_BAD_LENGTH);
        q.length = 31; CHECK(ov_record_check(q, 10, 801) == OV_BAD_FRAGMENT_LENGTH); q.length = 30;
        CHECK(ov_record_check(q, 10, 3) == OV_BAD_CHANNEL && ov_record_check(q, 10, 4) == OV_OK);
        q.channel = -1; CHECK(ov_record_check(q, 10, 801) == OV_BAD_CHANNEL); q.channel = 3;
        q.record_i = 3; CHECK(ov_record_check(q, 10, 801) == OV_BAD_FRAGMENT);
        q.record_i = -1; CHECK(ov_record_check(q, 10, 801) == OV_BAD_FRAGMENT); q.record_i = 2;
        q.pulse_length = 0; CHECK(ov_record_check(q, 10, 801) == OV_BAD_FRAGMENT);
    }
    CASE("pairs") {
        const OvHeader a0 = rec(E, 250, 0), a1 = rec(E, 250, 1), a2 = rec(E, 250, 2);
        CHECK(ov_pair_check(false, a0, a0) == OV_OK && ov_pair_check(true, a0, a1) == OV_OK && ov_pair_check(true, a1, a2) == OV_OK && ov_last_check(a2) == OV_OK);
        CHECK(ov_last_check(a1) == OV_BAD_INCOMPLETE && ov_pair_check(false, a1, a1) == OV_BAD_INCOMPLETE);
        CHECK(ov_pair_check(true, a0, a2) != OV_OK);                                  // the middle fragment is missing
        CHECK(ov_pair_check(true, a2, rec(E + 250, 5, 0)) == OV_OK);                   // touching: valid
        CHECK(ov_pair_check(true, a2, rec(E + 249, 5, 0)) == OV_BAD_OVERLAP);          // one shared sample
        CHECK(ov_pair_check(true, a0, rec(E + 50, 5, 0)) == OV_BAD_OVERLAP);           // a pulse inside another
        CHECK(ov_pair_check(true, a1, rec(E + 400, 5, 0)) == OV_BAD_INCOMPLETE);       // the pulse in front lacks its last fragment
        CHECK(ov_pair_check(true, a0, a0) == OV_BAD_OVERLAP);                          // the same record twice
        CHECK(ov_pair_check(true, rec(E + 50, 5, 0), a1) != OV_OK);                    // another pulse between two fragments
        CHECK(ov_pair_check(true, a0, rec(E, 251, 1)) != OV_OK);                       // two pulse lengths in one pulse
        OvHeader late = a1; late.time += 10;
        CHECK(ov_pair_check(true, a0, late) != OV_OK);                                 // fragments 111 samples apart
    }
    CASE("keys") {
        // a pass of 2^40 samples at the epoch on 801 row slots: keys are relative to smin, so the epoch takes no bits
        const i64 smin = E, smax = E + ((i64)1 << 40) - 1;
        OvBits b; b.sbits = ov_bits_of((u64)smax - (u64)smin + 1ull); b.chbits = ov_bits_of(800);
        CHECK(b.sbits == 41 && b.chbits == 10 && ov_bits_fit(b));
        const i64 rel = smax - smin;
        const u64 ka = ov_record_key(b, 0, 800, rel), kb = ov_record_key(b, 1, 0, 0);
        CHECK(ka < kb && ov_key_rel(b, ka) == rel && ov_key_channel(b, ka) == 800 && (ka >> (b.sbits + b.chbits)) == 0 && (kb >> (b.sbits + b.chbits)) == 1);
        CHECK(ov_record_key(b, 0, 5, rel) < ov_record_key(b, 0, 6, 0) && ov_record_key(b, 1, 5, 7) < ov_record_key(b, 1, 5, 8));
        const u64 pa = ov_pulse_key(b, 0, 800, rel), pb = ov_pulse_key(b, 1, 800, rel);
        CHECK(pa + 1 == pb && ov_key_rel(b, pa >> 1) == rel && ov_key_channel(b, pb >> 1) == 800);
        CHECK(ov_pulse_key(b, 1, 7, 99) < ov_pulse_key(b, 0, 7, 100) && ov_pulse_key(b, 1, 7, rel) < ov_pulse_key(b, 0, 8, 0));
        const u64 o = ov_output_key(b, 800, rel);
        CHECK(ov_output_rel(b, o) == rel && ov_output_channel(b, o) == 800 && ov_output_key(b, 800, 5) < ov_output_key(b, 0, 6) && ov_output_key(b, 3, 5) < ov_output_key(b, 4, 5));
        CHECK(smin + ov_output_rel(b, o) == smax && (smin + ov_output_rel(b, o)) * 10 == smax * 10);
        OvBits wide; wide.sbits = 54; wide.chbits = 10;
        CHECK(!ov_bits_fit(wide)); wide.sbits = 53; CHECK(ov_bits_fit(wide));
        CHECK(ov_bits_of(0) == 1 && ov_bits_of(1) == 1 && ov_bits_of(2) == 2 && ov_bits_of(1023) == 10 && ov_bits_of(1024) == 11 && ov_bits_of(~0ull) == 64);
    }
    CASE("merge") {
        OvBits b; b.sbits = 20; b.chbits = 10;
        // a pulse on channel 7 that ends at 149; the next begins at 149 (shared), at 150 (touching), on channel 8 at 0
        const u64 run = ov_end_key(b, 7, 149);
        CHECK(!ov_begins_merged(run, ov_pulse_key(b, 1, 7, 149)) && !ov_begins_merged(run, ov_pulse_key(b, 0, 7, 100)));
        CHECK(ov_begins_merged(run, ov_pulse_key(b, 1, 7, 150)) && ov_begins_merged(run, ov_pulse_key(b, 0, 7, 150)));
        CHECK(ov_begins_merged(run, ov_pulse_key(b, 0, 8, 0)));
        CHECK(ov_end_key(b, 7, (1 << 20) - 1) < ov_end_key(b, 8, 0));                 // a later channel outranks every end
    }
    CASE("sample") {
        const i32 bl = 16000;
        CHECK(ov_sample(false, true, 0, 15990, bl, 15000) == 15990 && ov_sample(false, true, 0, -5, bl, 15000) == -5);       // B alone: as recorded
        CHECK(ov_sample(true, false, 15900, 0, bl, 15000) == 14900 && ov_sample(true, false, 15900, 0, bl, bl) == 15900);
        CHECK(ov_sample(true, true, 15900, 14990, bl, 15000) == 14890);                // the recorded baseline is in b already
        CHECK(ov_sample(true, true, 100, 50, bl, bl) == 0 && ov_sample(true, false, 100, 0, bl, 50) == 0);
        CHECK(ov_sample(true, true, 32000, 30000, bl, bl) == 32767 && ov_sample(true, false, 32000, 0, bl, 32000) == 32767);
        CHECK(ov_sample(true, true, 16001, 32766, bl, bl) == 32767 && ov_sample(true, true, 16000, 32767, bl, bl) == 32767 && ov_sample(true, true, 16000, 0, bl, bl) == 0);
        CHECK(ov_sample(true, true, 32767, 32767, 0, 0) == 32767 && ov_sample(true, true, -32768, -32768, 32767, 0) == 0);
    }
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
