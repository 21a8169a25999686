// Drives wfsim_amd/csrc/wfs_rows.h on the host (tests/test_row_rules_cpu.py).
//
//   rows_main                      the rules that need no rows: one line "<case> ok|FAILED ..." for geometry, noise_index, finish, padded_len,
//                                  key_bits (bits_below and the three rules written through it: the end bits of the record sort and of the
//                                  lone seed sort, the key fields of the overlay -- each against the loop it replaced, written out here)
//   rows_main noise <file>         noise_index once more, on the rows of a file of lines "<noise_len> <row length>"
//   rows_main rows <file>          a family of designed rows, one per line: length, trigger window, absolute first sample, channel, dt, and
//                                  the positions of its hits.  The hits are grouped one after the other with zle_holdoff, every interval is
//                                  closed with zle_window, the slots are counted with zle_slots and the header of every record is made by
//                                  rec_header.  Prints, per row r, "row r <slots> <intervals>", per interval "itv r k <left> <right> <records>"
//                                  and per record "rec r k f" and its six header dwords; then "intervals ok" and "records ok" when what it
//                                  printed is consistent with itself.  The comparison with the reference's tuples and records is the test's.
// Exits 0 when every case holds.
#include "wfs_rows.h"
#include "wfs_lone.h"        // lone_key_end_bit
#include "wfs_overlay.h"     // ov_bits_of

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

static int failures = 0;
static void report(const char *name, bool ok, const std::string &what = "")
{
    printf("%s %s%s%s\n", name, ok ? "ok" : "FAILED", what.empty() ? "" : " ", what.c_str());
    if (!ok) failures++;
}

// ---- geometry ---------------------------------------------------------------------------------------------------------------------------
static bool geometry()
{
    static_assert(WFS_SPR == 110, "the literals below are those of 110 samples per record");
    // the two spellings of the fragment length are one rule, also behind the last record (k_pack_res looks at four whatever the interval has)
    for (i32 plen = 1; plen <= 2000; plen++)
        for (i32 f = 0; f <= records_of(plen) + 3; f++) {
            const i32 first = WFS_SPR * f, want = plen - first < WFS_SPR ? plen - first : WFS_SPR;
            if (rec_fragment_len<false>(plen, f) != want || rec_fragment_len<true>(plen, f) != want || rec_fragment_first(f) != first) return false;
        }
    return WFS_RECORD_BYTES == 244 && REC_DWORDS == 61 && REC_HEADER_DWORDS == 6 && REC_HEADER_BYTES == 24 && REC_LENGTH_BYTE == 8 && REC_DATA_BYTE == 24
           && REC_TIME_LO == 0 && REC_TIME_HI == 1 && REC_LENGTH == 2 && REC_DT_CHANNEL == 3 && REC_PULSE_LENGTH == 4 && REC_RECORD_I == 5
           && records_of(-1) == 0 && records_of(0) == 0 && records_of(1) == 1 && records_of(110) == 1 && records_of(111) == 2 && records_of(881) == 9
           && rec_fragment_len(111, 0) == 110 && rec_fragment_len(111, 1) == 1 && rec_fragment_len(220, 1) == 110
           && rec_fragment_time(10, 1000, 2) == 12200 && rec_fragment_sample(-7, 1) == 103
           && zle_holdoff(0) == 1 && zle_holdoff(-3) == 1 && zle_holdoff(31) == 63 && zle_holdoff(50) == 101 && ZLE_FAST_HOLD == 63
           && zle_slots(1, 1) == 1 && zle_slots(2, 1) == 1 && zle_slots(3, 1) == 2 && zle_slots(64, 63) == 1 && zle_slots(65, 63) == 2;
}

// ---- noise_index --------------------------------------------------------------------------------------------------------------------------
// a row of `len` samples that starts at table index ix, walked in blocks of `step` as the row kernels do: against (ix + i) % noise_len
static bool noise_walk(u32 N, u32 step, u32 ix, u32 len, const std::vector<u32> &mod, std::string &what)
{
    u32 nrun = ix;
    for (u32 b = 0; b < len; b += step) {
        for (u32 off = 0; off < step && b + off < len; off++) {
            const u32 got = noise_wrap(nrun + off, N);
            if (got != mod[ix + b + off]) {
                std::ostringstream o; o << "noise_len " << N << " step " << step << " ix " << ix << " sample " << b + off << ": " << got << " for " << mod[ix + b + off];
                what = o.str(); return false;
            }
        }
        nrun = noise_advance(nrun, step, N);
    }
    return true;
}
static bool noise_rows(u32 N, const std::vector<u32> &lens, std::string &what)
{
    u32 longest = 0;
    for (u32 l : lens) longest = l > longest ? l : longest;
    std::vector<u32> mod((size_t)N + longest + 1);
    for (size_t j = 0; j < mod.size(); j++) mod[j] = (u32)(j % N);
    for (u32 step : {64u, 256u, (u32)WFS_SPR})
        for (u32 len : lens)
            for (u32 ix = 0; ix < N; ix++)
                if (!noise_walk(N, step, ix, len, mod, what)) return false;
    return true;
}
static bool noise_index(std::string &what)
{
    // a row of three table lengths and a bit holds the rows of one and of two: the walk has no memory but nrun
    for (u32 N : {512u, 513u, 700u, 4096u, 12288u})
        if (!noise_rows(N, {3 * N + 5}, what)) return false;
    return noise_rows(512, {1, 63, 64, 65, 109, 110, 111, 255, 256, 257, 512, 513, 1024, 1025}, what);
}

// ---- finish -----------------------------------------------------------------------------------------------------------------------------
struct Dev { i32 baseline, he_factor; };
static bool finish(std::string &what)
{
    const Dev d{16000, 20};
    bool ok = true;
    auto want = [&](const char *name, i32 got, i32 exp) {
        if (got != exp) { std::ostringstream o; o << name << ": " << got << " for " << exp; what = o.str(); ok = false; }
    };
    // no noise: ADC (times the HE factor) + baseline, clamped at 0
    want("k0", finish_value<0>(d, -100, false, false, 0, 0), 15900);
    want("k0 he", finish_value<0>(d, -100, true, false, 0, 0), 14000);
    want("k0 he at 0", finish_value<0>(d, -800, true, false, 0, 0), 0);
    want("k0 he clamp", finish_value<0>(d, -801, true, false, 0, 0), 0);
    want("k0 clamp", finish_value<0>(d, -16001, false, false, 0, 0), 0);
    want("k0 one above", finish_value<0>(d, -15999, false, false, 0, 0), 1);
    want("k0 he 64 bits", finish_value<0>(d, -2000000000, true, false, 0, 0), 0);                     // (the product does not fit 32 bits)
    // int16 table: the noise is not multiplied; a row outside the table drops the value that was read
    want("k1", finish_value<1>(d, -100, false, true, -7, 0), 15893);
    want("k1 he", finish_value<1>(d, -100, true, true, -7, 0), 13993);
    want("k1 outside", finish_value<1>(d, -100, false, false, -7, 0), 15900);
    want("k1 clamp", finish_value<1>(d, 0, false, true, -16001, 0), 0);
    // float table: the truncated SUM, not the sum with the truncated noise
    want("k2 up", finish_value<2>(d, -100, false, true, 0, 0.5), 15901);                              // -99.5 -> -99 (truncated noise: -100)
    want("k2 down", finish_value<2>(d, 100, false, true, 0, -0.5), 16099);                            //  99.5 ->  99 (truncated noise: 100)
    want("k2 same sign", finish_value<2>(d, -100, false, true, 0, -0.5), 15900);                      // -100.5 -> -100
    want("k2 he", finish_value<2>(d, -5, true, true, 0, 0.5), 15901);                                 // -100 + 0.5
    want("k2 outside", finish_value<2>(d, -100, false, false, 0, 0.5), 15900);
    want("k2 clamp", finish_value<2>(d, 0, false, true, 0, -16000.5), 0);                             // -16000.5 -> -16000 -> 0
    // drawn noise: always added (a row outside the model hands in 0)
    want("k3", finish_value<3>(d, -100, false, true, 9, 0), 15909);
    want("k3 he", finish_value<3>(d, -100, true, true, 9, 0), 14009);
    want("k3 clamp", finish_value<3>(d, -16000, false, true, -1, 0), 0);

    // the resident rule on its domain: |baseline + nz| <= 2^16, acc + baseline + nz <= 2^31 - 1
    const i64 top = 0x7fffffffLL, two16 = 65536;
    const i64 accs[] = {-(top + 1), -top, -(top + 1 - two16) - 1, -(top + 1 - two16), -two16 - 1, -two16, -two16 + 1, -16001, -16000, -15999, -1, 0, 1,
                        two16 - 1, two16, top - two16 - 1, top - two16, top - two16 + 1, top + 1 - two16};
    const i64 adds[] = {-two16, -two16 + 1, -32768, -1, 0, 1, 32767, two16 - 1, two16};
    for (i64 acc : accs)
        for (i64 add : adds) {
            if (acc + add > top) continue;                      // outside the domain
            for (i32 nz : {-32768, -1, 0, 1, 32767}) {           // every split of `add` into baseline and noise
                const Dev e{(i32)(add - nz), 1};
                if (finish_resident<1>(e, (i32)acc, true, nz) != finish_value<1>(e, (i32)acc, false, true, nz, 0)
                    || finish_resident<3>(e, (i32)acc, true, nz) != finish_value<3>(e, (i32)acc, false, true, nz, 0)) {
                    std::ostringstream o; o << "resident: acc " << acc << " baseline " << e.baseline << " noise " << nz; what = o.str(); ok = false;
                }
            }
            const Dev e{(i32)add, 1};
            if (finish_resident<0>(e, (i32)acc, false, 0) != finish_value<0>(e, (i32)acc, false, false, 0, 0)
                || finish_resident<1>(e, (i32)acc, false, 77) != finish_value<1>(e, (i32)acc, false, false, 77, 0)) {
                std::ostringstream o; o << "resident, no noise: acc " << acc << " baseline " << add; what = o.str(); ok = false;
            }
        }
    // beyond the domain the rule saturates
    want("resident saturates", finish_resident<0>(Dev{65536, 1}, 0x7fffffff, false, 0), 0x7fffffff);

    // the hit decision in 32 bits: every finished sample below 2^31 - 1, thresholds inside and beyond 32 bits
    const i64 thrs[] = {-(1LL << 40), -(top + 1) - 1, -(top + 1), -top, -1, 0, 1, 15984, top - 1, top, top + 1, top + 2, 1LL << 40};
    const i32 vals[] = {0, 1, 15983, 15984, 15985, 0x7ffffffd, 0x7ffffffe};
    for (i64 thr : thrs)
        for (i32 v : vals)
            if ((v < zle_thr32(thr)) != ((i64)v < thr)) { std::ostringstream o; o << "thr32: sample " << v << " threshold " << thr; what = o.str(); ok = false; }
    for (i64 thr : thrs)
        if (thr <= top && (0x7fffffff < zle_thr32(thr)) != (top < thr)) { what = "thr32: sample 2^31 - 1"; ok = false; }
    return ok;
}

// ---- padded_len -------------------------------------------------------------------------------------------------------------------------
static bool padded_len()
{
    bool ok = true;
    auto check = [&](i32 len) {
        const i32 p = fin_padded_len(len);
        ok = ok && p % 4 == 0 && p >= len && p - len < 4 && fin_last_pair(len) == p - 2 && fin_last_pair(len) % 2 == 0 && fin_last_pair(len) + 1 < p;
    };
    for (i32 len = 1; len <= 16; len++) check(len);
    for (i32 base : {768, 7168})
        for (i32 m = 0; m < 4; m++) { check(base - 4 + m); check(base + m); }
    return ok && fin_padded_len(1) == 4 && fin_padded_len(4) == 4 && fin_padded_len(5) == 8 && fin_padded_len(768) == 768 && fin_padded_len(769) == 772
           && fin_padded_len(7167) == 7168 && fin_last_pair(1) == 2 && fin_last_pair(7168) == 7166;
}

// ---- key_bits ---------------------------------------------------------------------------------------------------------------------------
// the loops the engine and wfs_overlay.h held before bits_below, literally
static unsigned old_record_end_bit(u64 span) { unsigned end_bit = 13; while (end_bit < 64 && ((span << 12) >> end_bit) != 0) end_bit++; return end_bit; }
static unsigned old_seed_end_bit(u64 n_ch) { unsigned end_bit = 41; while (end_bit < 64 && (n_ch >> (end_bit - 41)) != 0) end_bit++; return end_bit; }
static int old_ov_bits_of(u64 v) { int b = 1; while (b < 64 && (v >> b) != 0) b++; return b; }
static bool key_bits(std::string &what)
{
    bool ok = true;
    auto want = [&](const char *name, u64 arg, long long got, long long exp) {
        if (got != exp) { std::ostringstream o; o << name << "(" << arg << "): " << got << " for " << exp; what = o.str(); ok = false; }
    };
    // bits needed for values below v: the smallest b with v <= 2^b
    want("bits_below", 0, bits_below(0), 0); want("bits_below", 1, bits_below(1), 0); want("bits_below", 2, bits_below(2), 1);
    for (int k = 1; k <= 51; k++) {
        const u64 p = (u64)1 << k;
        want("bits_below 2^k - 1", p - 1, bits_below(p - 1), k == 1 ? 0 : (k == 2 ? 2 : k));      // 1: no bit; 3: two bits; above, 2^(k-1) < 2^k - 1
        want("bits_below 2^k", p, bits_below(p), k);
        want("bits_below 2^k + 1", p + 1, bits_below(p + 1), k + 1);
    }
    want("bits_below 2^63", (u64)1 << 63, bits_below((u64)1 << 63), 63);
    want("bits_below 2^63 + 1", ((u64)1 << 63) + 1, bits_below(((u64)1 << 63) + 1), 64);
    want("bits_below 2^64 - 1", ~0ull, bits_below(~0ull), 64);
    // the record key: span << 12 | channel
    static_assert(REC_KEY_SHIFT == 12, "the literal of the old loop");
    for (u64 span : {(u64)1, (u64)2, (u64)4095, (u64)4096, (u64)1 << 31, ((u64)1 << 51) - 1})
        want("rec_key_end_bit", span, rec_key_end_bit(span), old_record_end_bit(span));
    want("rec_key_end_bit", 0, rec_key_end_bit(0), 13);                          // (the engine hands in at least 1)
    want("rec_key_end_bit", 1, rec_key_end_bit(1), 13);
    want("rec_key_end_bit", 4096, rec_key_end_bit(4096), 25);
    want("rec_key_end_bit 2^52", (u64)1 << 52, rec_key_end_bit((u64)1 << 52), 64);      // where the old loop began to lose bits: every bit is sorted
    // the lone seed key: channel << 41 | start << 1 | kind
    static_assert(LONE_KEY_SHIFT == 41, "the literal of the old loop");
    for (int n_ch : {1, 2, 493, 494, 512, 4095})
        want("lone_key_end_bit", (u64)n_ch, lone_key_end_bit(n_ch), old_seed_end_bit((u64)n_ch));
    want("lone_key_end_bit", 494, lone_key_end_bit(494), 50);
    want("lone_key_end_bit", 0, lone_key_end_bit(0), 41);
    // the overlay's key fields, at its three uses: the samples of a pass, n_rows - 1, the 800 of the key case of overlay_rules_main.cpp
    for (u64 span : {(u64)1, (u64)2, (u64)1000, (u64)1 << 40, ((u64)1 << 40) + 1, ((u64)1 << 53) - 1})
        want("ov_bits_of span + 1", span, ov_bits_of(span + 1), old_ov_bits_of(span + 1));
    for (u64 n_rows : {(u64)1, (u64)2, (u64)3, (u64)494, (u64)513, (u64)801, (u64)1025})
        want("ov_bits_of n_rows - 1", n_rows, ov_bits_of(n_rows - 1 > 1 ? n_rows - 1 : 1), old_ov_bits_of(n_rows - 1 > 1 ? n_rows - 1 : 1));
    want("ov_bits_of", 800, ov_bits_of(800), old_ov_bits_of(800));
    for (u64 v : {(u64)0, (u64)1, (u64)2, (u64)1023, (u64)1024, ~0ull}) want("ov_bits_of", v, ov_bits_of(v), old_ov_bits_of(v));
    return ok;
}

// ---- rows -------------------------------------------------------------------------------------------------------------------------------
static int rows(const char *path)
{
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string line, what_i, what_r;
    bool ok_i = true, ok_r = true;
    long r = 0;
    for (; std::getline(in, line); r++) {
        std::istringstream ls(line);
        long long len, tw, abs0, channel, dt;
        if (!(ls >> len >> tw >> abs0 >> channel >> dt)) { fprintf(stderr, "line %ld: %s\n", r, line.c_str()); return 2; }
        std::vector<i32> hits; long long hpos;
        while (ls >> hpos) hits.push_back((i32)hpos);
        const i64 hold = zle_holdoff(tw);
        // the hits one after the other: a hit more than the hold-off behind the last one opens an interval (utils.py:13-58)
        struct Raw { i32 first, last; };
        std::vector<Raw> raw;
        for (i32 p : hits) {
            if (raw.empty() || p - raw.back().last > hold) raw.push_back(Raw{p, p});
            else raw.back().last = p;
        }
        const i64 slots = zle_slots(len, hold);
        printf("row %ld %lld %zu\n", r, slots, raw.size());
        if ((i64)raw.size() > slots) { ok_i = false; what_i = "row " + std::to_string(r) + " needs more than its slots"; }
        const u32 dtc = rec_dt_channel((i32)dt, (i32)channel);
        for (size_t k = 0; k < raw.size(); k++) {
            const ZleWindow w = zle_window(raw[k].first, raw[k].last, (i32)tw, (i32)len);
            printf("itv %ld %zu %d %d %d\n", r, k, w.left, w.right, w.nrec);
            const i32 plen = w.right - w.left + 1;
            if (w.nrec != records_of(plen) || w.left < 0 || w.right > len - 1 || w.left % 2 || w.right % 2) { ok_i = false; what_i = "row " + std::to_string(r) + " interval " + std::to_string(k); }
            i32 covered = 0;
            for (i32 f = 0; f < w.nrec; f++) {
                const RecHeader h = rec_header((i32)dt, dtc, abs0 + w.left, plen, f);
                printf("rec %ld %zu %d %u %u %u %u %u %u\n", r, k, f, h.w[0], h.w[1], h.w[2], h.w[3], h.w[4], h.w[5]);
                const i32 length = rec_fragment_len(plen, f);
                if (length < 1 || length > WFS_SPR || (f + 1 < w.nrec && length != WFS_SPR) || (i32)h.w[REC_LENGTH] != length) { ok_r = false; what_r = "row " + std::to_string(r) + " record length"; }
                covered += length;
            }
            if (covered != (plen > 0 ? plen : 0)) { ok_r = false; what_r = "row " + std::to_string(r) + ": the records do not cover the interval"; }
        }
    }
    report("intervals", ok_i, what_i);
    report("records", ok_r, what_r);
    return failures ? 1 : 0;
}

static int noise_file(const char *path)
{
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string what; bool ok = true;
    unsigned N, len;
    while (ok && (in >> N >> len)) ok = noise_rows(N, {len}, what);
    report("noise_index", ok, what);
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "rows")) return rows(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "noise")) return noise_file(argv[2]);
    if (argc != 1) { fprintf(stderr, "usage: rows_main [rows <file> | noise <file>]\n"); return 2; }
    std::string what;
    report("geometry", geometry());
    { const bool ok = noise_index(what); report("noise_index", ok, what); }
    what.clear();
    { const bool ok = finish(what); report("finish", ok, what); }
    report("padded_len", padded_len());
    what.clear();
    { const bool ok = key_bits(what); report("key_bits", ok, what); }
    return failures ? 1 : 0;
}
