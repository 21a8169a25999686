// Drives wfsim_amd/csrc/wfs_layout.h on the host: the dynamic-LDS layout of every kernel that has one (regions ascending, disjoint, aligned,
// inside the total; the totals the byte counts the launch sites reserved before the layouts existed, held here as literals; the largest
// total under the cap wfs_create grants) and the window rules (tile_window, row_slot, row_span) on values worked out by hand.
// Prints one line "<case> ok|FAILED" per case and exits 0 when every case holds (tests/test_layout_cpu.py).
#include "wfs_layout.h"

#include <cstdio>
#include <vector>

static int failures = 0;
static void report(const char *name, bool ok)
{
    printf("%s %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) failures++;
}

// one region of a layout as the kernel uses it: where it starts, the bytes the kernel touches there, the alignment its accesses need
struct Region { int off, bytes, align; };
// ascending, disjoint, aligned, inside the total; the total a multiple of `total_align`
static bool regions_hold(const std::vector<Region> &r, int total, int total_align = 16)
{
    int end = 0;
    for (const Region &q : r) {
        if (q.off < end || q.bytes < 0 || q.off % q.align != 0) return false;
        end = q.off + q.bytes;
    }
    return end <= total && total % total_align == 0;
}
static int tap_bytes(int waves) { return (22 * 10 + 2) * 8 + waves * 64 * 2; }      // W2 and the waves' lists (tap_block)
static const int AP_BYTES = 128 * 48;                                                 // AP_STAGE candidates of 48 bytes

// ---- regions --------------------------------------------------------------------------------------------------------------------------
static bool dense_regions(int tpb)
{
    const PulseLds o = pulse_lds(tpb);
    return regions_hold({{o.H, (tpb + 21) * 10 * 8, 16}, {o.red, tpb / 64 * 8 * 8, 8}, {o.wsum, 16 * 4, 4}, {o.W2, tap_bytes(tpb / 64), 8}, {o.slack, 0, 1}}, o.total)
           && TAP_LISTS_OFF == 222 * 8 && TAP_LISTS_OFF % 2 == 0;
}
static bool sparse_regions(int NP, int W)
{
    const SparseLds o = sparse_lds(NP, W, SPARSE_TPB);
    const int cnt_bytes = 10 * W / 2 * 4, trep_bytes = 260 * 8;      // the two uses of the last region
    return regions_hold({{o.cg, NP * 8, 8}, {o.red, 8 * 8, 8}, {o.ctoff, NP * 4, 4}, {o.boff, (10 * W + 2) * 2, 2}, {o.wsum, 8 * 4, 4},
                         {o.cnt, cnt_bytes > trep_bytes ? cnt_bytes : trep_bytes, 8}, {o.slack, 0, 1}}, o.total);
}
static bool generic_regions(int dt, int tlen, bool split)
{
    const GenericLds o = generic_lds(dt, tlen, split);
    const int h = (256 + tlen - 1) * dt * 8;
    return regions_hold({{o.H, h, 8}, {o.Hlo, split ? h : 0, 8}, {o.T, dt * tlen * 8, 8}, {o.red, 4 * 8 * 8, 8}, {o.slack, 0, 1}}, o.total);
}
static bool tile_regions(bool fma, bool ap)
{
    const TileLds o = tile_lds(fma, ap);
    // (the H table also stages the channel's SPE row: 2001 doubles, moved 16 bytes at a time)
    return regions_hold({{o.H, 277 * 10 * 8, 16}, {o.wsum, 16 * 4, 4}, {o.W2, fma ? 0 : tap_bytes(4), 8}, {o.slack, 0, 1}, {o.ap, ap ? AP_BYTES : 0, 16}}, o.total)
           && 277 * 10 >= 2002;
}
static bool bright_regions(int bright_lds, bool ap)
{
    const BrightLds o = bright_lds_layout(bright_lds, ap);
    return regions_hold({{o.H, bright_lds, 16}, {o.spe, 2001 * 8, 8}, {o.ap, ap ? AP_BYTES : 0, 16}}, o.total);
}
static bool row_regions(int region)
{
    const RowLds o = row_pulse_lds(region);
    return regions_hold({{o.sTz, 240 * 8, 8}, {o.cmax, 16 * 8, 8}, {o.ph, 4 * 66 * 16, 16}, {o.acc, 4 * region * 4, 16}}, o.total)
           && row_pulse_lds(0).acc == o.acc;      // (the kernel takes the offsets from the layout of an empty region)
}
static bool fill_regions(int nch, int lg, bool ap)
{
    const GenFillLds o = gen_fill_lds(nch, lg, ap);
    const int nch1 = nch + 1 + ((nch + 1) & 1);
    // (its total is a multiple of 8: what the launch reserved before, kept to the byte)
    return regions_hold({{0, 512 * 4, 4}, {o.wtime, 512 * 4, 4}, {o.T, 8 << lg, 8}, {o.hist, nch1 * 4, 4}, {o.cur, nch * 4, 4}, {o.hmin, nch * 4, 4}, {o.hmax, nch * 4, 4},
                         {o.hoff, nch * 4, 4}, {o.chmap, 2048 * 2, 2}, {o.pidx, 2048 * 2, 2}, {o.stage, 2048 * 8, 8}, {o.ap, ap ? AP_BYTES : 0, 8}}, o.total, 8);
}

// ---- what the launch sites reserved before the layouts existed, written as they wrote it ---------------------------------------------
static int parent_generic(int dt, int tlen, bool &split)
{
    const int h_bytes = (256 + tlen - 1) * dt * 8, rest = dt * tlen * 8 + 4 * 8 * 8 + 64;
    split = (2 * h_bytes + rest + 15) / 16 * 16 <= 128 * 1024;
    return ((split ? 2 : 1) * h_bytes + rest + 15) / 16 * 16;
}

struct Geom { int dt, store_before, samples_before, store_after, samples_after; };          // stand-ins for the device view
struct Rows { int row_slots, n_tpc, he_first, sum_channel; };

int main()
{
    {
        bool ok = dense_regions(128) && dense_regions(256);
        for (int NP = 8; NP <= 32; NP += 8) for (int W = 8; W <= 64; W += 8) ok = ok && sparse_regions(NP, W);
        for (int dt = 1; dt <= WFS_MAX_DT; dt++) for (int tlen = 1; tlen <= WFS_MAX_TLEN; tlen++) ok = ok && generic_regions(dt, tlen, false) && generic_regions(dt, tlen, true);
        for (int v = 0; v < 4; v++) ok = ok && tile_regions(v & 1, v & 2);
        for (int b : {0, 16, BRIGHT_LDS_MAX}) ok = ok && bright_regions(b, false) && bright_regions(b, true);
        for (int region : {RES_SHORT_LEN, 256, 7168}) ok = ok && row_regions(region);
        for (int np2 = 128; np2 <= TILE_ORDER_MAX; np2 *= 2) { const OrderLds o = order_lds(np2); ok = ok && regions_hold({{o.key, np2 * 8, 8}, {o.rec, np2 * 8, 8}, {o.gain, np2 * 8, 8}}, o.total); }
        ok = ok && regions_hold({{tile_gen_lds(true).ap, AP_BYTES, 16}}, tile_gen_lds(true).total) && tile_gen_lds(false).total == 0;
        // the three whose totals the launch never rounded: multiples of their element size (kept to the byte, like every other total)
        for (int nch : {1, 2, 253, 494, 1024}) {
            int lg = 1; while ((1 << lg) < nch) lg++;
            const CountLds c = count_lds(nch, lg);
            ok = ok && regions_hold({{c.A, 8 << lg, 8}, {c.hist, nch * 4, 4}}, c.total, 4) && regions_hold({{map_rows_lds(nch).p, nch * 8, 8}}, map_rows_lds(nch).total, 8);
            ok = ok && fill_regions(nch, lg, false) && fill_regions(nch, lg, true);
        }
        report("regions", ok);
    }
    {
        bool ok = pulse_lds(256).total == 24784 && pulse_lds(128).total == 14416;
        ok = ok && pulse_lds(128).total - pulse_lds(128).slack == 2 * 64 * 2 + 16 && pulse_lds(256).total - pulse_lds(256).slack == 16;      // the named slack
        static const int sparse[4][8] = {{2464, 2624, 2784, 2944, 3104, 3264, 3424, 3584},         // NP 8 .. 32 down, W 8 .. 64 across
                                         {2560, 2720, 2880, 3040, 3200, 3360, 3520, 3680},
                                         {2656, 2816, 2976, 3136, 3296, 3456, 3616, 3776},
                                         {2752, 2912, 3072, 3232, 3392, 3552, 3712, 3872}};
        for (int i = 0; i < 4; i++) for (int j = 0; j < 8; j++) ok = ok && sparse_lds(8 * (i + 1), 8 * (j + 1), SPARSE_TPB).total == sparse[i][j];
        ok = ok && tile_lds(true, false).total == 22240 && tile_lds(false, false).total == 24576 && tile_lds(true, true).total == 22240 + 6144 && tile_lds(false, true).total == 24576 + 6144;
        ok = ok && tile_lds(true, true).ap == 22240 && tile_lds(false, true).ap == 24576;
        ok = ok && bright_lds_layout(0, false).total == 16016 && bright_lds_layout(0, true).total == 22160 && bright_lds_layout(16, false).total == 16032
             && bright_lds_layout(16, true).total == 22176 && bright_lds_layout(131072, false).total == 147088 && bright_lds_layout(131072, true).total == 153232;
        ok = ok && row_pulse_lds(768).total == 18560 && row_pulse_lds(256).total == 10368 && row_pulse_lds(7168).total == 120960;
        ok = ok && order_lds(TILE_ORDER_MAX).total == 98304 && count_lds(494, 9).total == 6072 && map_rows_lds(494).total == 3952;
        ok = ok && tile_gen_lds(true).total == 6144 && tile_gen_lds(false).total == 0;
        ok = ok && gen_fill_lds(494, 9, false).total == 42672 && gen_fill_lds(494, 9, true).total == 48816 && gen_fill_lds(1024, 10, true).total == 63512;
        report("totals_as_before", ok);
    }
    {
        // spot values, then every geometry against the expression the launch site had
        bool ok = generic_lds(10, 22, true).total == 46400 && generic_lds(1, 1, true).total == 4432 && generic_lds(16, 256, false).total == 98496
                  && generic_lds(16, 100, true).total == 104000 && generic_lds(16, 128, true).total == 114752 && generic_lds(13, 200, true).total == 115760;
        ok = ok && generic_lds_split(16, 128) && !generic_lds_split(16, 256);
        for (int dt = 1; dt <= WFS_MAX_DT; dt++)
            for (int tlen = 1; tlen <= WFS_MAX_TLEN; tlen++) {
                bool split; const int total = parent_generic(dt, tlen, split);
                ok = ok && generic_lds_split(dt, tlen) == split && generic_lds(dt, tlen, split).total == total;
            }
        report("generic_totals_as_before", ok);
    }
    {
        bool ok = LDS_CAP_PULSE == 100 * 1024 && LDS_CAP_SPARSE == 100 * 1024 && LDS_CAP_GENERIC == 128 * 1024 && LDS_CAP_TILE == 100 * 1024 && LDS_CAP_ROW == 128 * 1024
                  && LDS_CAP_FILL == 100 * 1024 && LDS_CAP_ORDER == 100 * 1024;      // the values granted stay what they were
        ok = ok && pulse_lds(256).total <= LDS_CAP_PULSE && pulse_lds(128).total <= LDS_CAP_PULSE;
        ok = ok && sparse_lds(SPARSE_MAX_PHOTONS, SPARSE_MAX_BINS, SPARSE_TPB).total <= LDS_CAP_SPARSE && SPARSE_MAX_PHOTONS <= SPARSE_TPB * SPARSE_PPT;
        for (int dt = 1; dt <= WFS_MAX_DT; dt++)        // every geometry the engine accepts runs with one table or two, under the cap
            for (int tlen = 1; tlen <= WFS_MAX_TLEN; tlen++) ok = ok && generic_lds(dt, tlen, generic_lds_split(dt, tlen)).total <= LDS_CAP_GENERIC;
        ok = ok && tile_lds(false, true).total <= LDS_CAP_TILE && tile_lds(true, true).total <= LDS_CAP_TILE;
        ok = ok && row_pulse_lds(RES_MAX_LEN).total <= LDS_CAP_ROW && RES_MAX_LEN == 7168 && row_pulse_lds(RES_SHORT_LEN).total <= 64 * 1024;      // (the short form keeps the default cap)
        ok = ok && order_lds(TILE_ORDER_MAX).total <= LDS_CAP_ORDER && gen_fill_lds(WFS_MAX_CH, 10, true).total <= LDS_CAP_FILL;
        ok = ok && count_lds(WFS_MAX_CH, 10).total <= 64 * 1024 && map_rows_lds(WFS_MAX_CH).total <= 64 * 1024 && tile_gen_lds(true).total <= 64 * 1024;
        report("caps", ok);
    }
    {
        // the bright kernel's grant: H bytes, start bins and the cap wfs_create sets, for a device of 64 KB and of 160 KB per workgroup
        bool ok = bright_lds_of_grant(65536) == 41328 && bright_bins_of_lds(41328) == 474 && bright_lds_layout(41328, true).total == 63488;
        ok = ok && bright_lds_of_grant(163840) == 131072 && bright_bins_of_lds(131072) == 1596 && bright_lds_layout(131072, true).total == 153232;
        ok = ok && bright_lds_of_grant(1000) == 0 && bright_bins_of_lds(0) == 0 && bright_bins_of_lds(16) == 0;
        ok = ok && bright_lds_layout(bright_lds_of_grant(163840), true).total + BRIGHT_STATIC_RESERVE <= 163840;
        report("bright_grant", ok);
    }
    {
        // pulse.py:118-127 with dt 10, 5 + 2 samples in front, 3 + 20 behind
        const Geom d{10, 5, 2, 3, 20};
        const TileWindow a = tile_window(d, -95, -10, 4);        // -105 .. -91 ns: bins -11 (floor of -10.5) and -10 (floor of -9.1)
        bool ok = a.bin0 == -11 && a.nb == 2 && a.left == -18 && a.right == 13 && a.L == 32;
        const TileWindow b = tile_window(d, 1000, 37, 37);       // one photon time: bin 103
        ok = ok && b.bin0 == 103 && b.nb == 1 && b.left == 96 && b.right == 126 && b.L == 31;
        const TileWindow c = tile_window(d, 0, 19, 20);          // 19 and 20 ns: either side of a multiple of dt
        ok = ok && c.bin0 == 1 && c.nb == 2 && c.left == -6 && c.right == 25 && c.L == 32;
        const TileWindow e = tile_window(d, -100, 0, 9);         // -100 ns exactly: bin -10, no step down
        ok = ok && e.bin0 == -10 && e.nb == 1 && e.left == -17 && e.right == 13 && e.L == 31;
        ok = ok && floordiv(-105, 10) == -11 && floordiv(-100, 10) == -10 && floordiv(105, 10) == 10 && floordiv(-1, 10) == -1;
        report("tile_window", ok);
    }
    {
        const Rows off{747, 494, 500, -1}, on{748, 494, 500, 800};      // 494 TPC channels, 253 HE rows from channel 500 on, the sum row last
        const RowSlot a = row_slot(off, 3 * 747 + 10);
        bool ok = a.g == 3 && a.slot == 10 && a.channel == 10 && a.acc_ch == 10 && !a.he && !a.sum;
        const RowSlot b = row_slot(off, 2 * 747 + 494 + 7);
        ok = ok && b.g == 2 && b.slot == 501 && b.channel == 507 && b.acc_ch == 7 && b.he && !b.sum;
        const RowSlot c = row_slot(on, 1 * 748 + 747);
        ok = ok && c.g == 1 && c.slot == 747 && c.channel == 800 && c.acc_ch == -1 && c.he && c.sum;
        const RowSlot e = row_slot(off, 746);                           // the last slot with the switch off: the last HE row
        ok = ok && e.g == 0 && e.slot == 746 && e.channel == 752 && e.acc_ch == 252 && e.he && !e.sum;
        const RowSlot f = row_slot(on, 746);                            // the same slot with the switch on: still the HE row
        ok = ok && f.channel == 752 && f.acc_ch == 252 && f.he && !f.sum && row_slot_is_sum(on, 747) && !row_slot_is_sum(off, 746);
        report("row_slot", ok);
    }
    {
        const RowSpan a = row_span(100, 149, 0), b = row_span(100, 149, 50), c = row_span(-30, -30, 50);
        report("row_span", a.len == 50 && a.left == 100 && a.right == 149 && b.len == 150 && b.left == 50 && b.right == 199 && c.len == 101 && c.left == -80 && c.right == 20);
    }
    return failures ? 1 : 0;
}
