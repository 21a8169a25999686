// Drives the kernel families of wfsim_amd/csrc/wfs_family.h on the host: plain function templates that return their own template
// arguments encoded in an int play the kernels.  Prints one line "<case> ok|FAILED ..." per case and exits 0 when every case holds
// (tests/test_family_cpu.py).
#include "wfs_family.h"

#include <cstdio>
#include <set>
#include <string>
#include <vector>

template <int NK, bool FMA, bool SEG, bool DK> int k4() { return ((NK * 2 + FMA) * 2 + SEG) * 2 + DK; }
template <bool A, bool B, bool C> int k3() { return (A * 2 + B) * 2 + C; }
template <bool A, bool B> int k2() { return A * 2 + B; }
template <bool A> int k1() { return A; }
template <int TPB, bool RES> int kmapped() { return TPB * 2 + RES; }
int kplain() { return 7; }

static const auto K4 = family<6, 2, 2, 2>("k4", [](int, int, int seg, int) { return seg ? 4096 : 0; },
                                          [](auto nk, auto fma, auto seg, auto dk) { return &k4<nk(), fma() != 0, seg() != 0, dk() != 0>; });
static const auto K3 = family<2, 2, 2>("k3", 0, [](auto a, auto b, auto c) { return &k3<a() != 0, b() != 0, c() != 0>; });
static const auto K2 = family<2, 2>("k2", 1000, [](auto a, auto b) { return &k2<a() != 0, b() != 0>; });
static const auto K1 = family<2>("k1", 0, [](auto a) { return &k1<a() != 0>; });
// a mapped axis: index 0 / 1 -> 128 / 256 threads
static const auto KM = family<2, 2>("kmapped", 2000, [](auto big, auto res) { return &kmapped<big() ? 256 : 128, res() != 0>; });

static int failures = 0;
static void report(const char *name, bool ok, const std::string &detail = "")
{
    printf("%s %s %s\n", name, ok ? "ok" : "FAILED", detail.c_str());
    if (!ok) failures++;
}

// every member of a family through its untyped view: as many as the product of the axes, none null, all distinct
static bool distinct(const FamilyBase &f, int product)
{
    std::set<const void *> seen;
    for (int m = 0; m < f.size(); m++) seen.insert(f.address(m));
    return f.size() == product && (int)seen.size() == product && !seen.count(nullptr) && !f.address(-1) && !f.address(product);
}

int main()
{
    {   // every index tuple picks the member made from exactly those constants
        bool ok = true;
        for (int nk = 0; nk < 6; nk++) for (int f = 0; f < 2; f++) for (int s = 0; s < 2; s++) for (int d = 0; d < 2; d++) {
            auto fn = K4.pick(nk, f, s, d);
            ok = ok && fn && fn() == ((nk * 2 + f) * 2 + s) * 2 + d && K4(nk, f, s, d).fn == fn && fn == K4.table[(std::size_t)K4.flat(nk, f, s, d)];
        }
        report("pick_6222", ok);
        ok = true;
        for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) for (int c = 0; c < 2; c++) { auto fn = K3.pick(a, b, c); ok = ok && fn && fn() == (a * 2 + b) * 2 + c; }
        report("pick_222", ok);
        ok = true;
        for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) { auto fn = K2.pick(a, b); ok = ok && fn && fn() == a * 2 + b; }
        report("pick_22", ok);
        // (bool indices, as the engine passes its switches)
        report("pick_2", K1.pick(0) && K1.pick(1) && K1.pick(false)() == 0 && K1.pick(true)() == 1);
        ok = true;
        for (int big = 0; big < 2; big++) for (int r = 0; r < 2; r++) { auto fn = KM.pick(big, r); ok = ok && fn && fn() == (big ? 256 : 128) * 2 + r; }
        report("pick_mapped", ok);
    }
    report("size_is_product", K4.SIZE == 48 && K3.SIZE == 8 && K2.SIZE == 4 && K1.SIZE == 2 && KM.SIZE == 4
                              && K4.table.size() == 48 && K3.table.size() == 8 && K2.table.size() == 4 && K1.table.size() == 2 && KM.table.size() == 4);
    report("members_distinct", distinct(K4, 48) && distinct(K3, 8) && distinct(K2, 4) && distinct(K1, 2) && distinct(KM, 4));
    {   // -1 or N on any axis: null, whatever the other indices are
        bool ok = true;
        for (int bad : {-1, 6}) ok = ok && !K4.pick(bad, 0, 0, 0) && !K4.pick(bad, 1, 1, 1) && !K4(bad, 0, 0, 0).fn;
        for (int bad : {-1, 2}) {
            ok = ok && !K4.pick(0, bad, 0, 0) && !K4.pick(5, 1, bad, 1) && !K4.pick(5, 1, 1, bad);
            ok = ok && !K3.pick(bad, 0, 0) && !K3.pick(1, bad, 1) && !K3.pick(1, 1, bad);
            ok = ok && !K2.pick(bad, 1) && !K2.pick(1, bad) && !KM.pick(bad, 0) && !KM.pick(0, bad) && !K1.pick(bad);
        }
        ok = ok && !K4.pick(1 << 30, 0, 0, 0) && !K2.pick(0, 1 << 30) && K4.flat(6, 0, 0, 0) == -1 && K4.flat(5, 1, 1, 1) == 47;
        report("outside_is_null", ok);
    }
    {   // the name goes with every picked member, a null one included (the launch function names the family it refuses)
        const bool names = std::string(K4.name) == "k4" && std::string(K4(0, 0, 0, 0).name) == "k4" && std::string(K4(9, 0, 0, 0).name) == "k4"
                           && std::string(KM(1, 1).name) == "kmapped" && std::string(kernel(&kplain, "kplain").name) == "kplain" && kernel(&kplain, "kplain").fn() == 7;
        bool caps = true;
        for (int m = 0; m < 48; m++) caps = caps && K4.lds_cap(m) == (((m >> 1) & 1) ? 4096 : 0);      // (the third axis alone decides)
        for (int m = 0; m < 4; m++) caps = caps && K2.lds_cap(m) == 1000 && KM.lds_cap(m) == 2000;
        for (int m = 0; m < 8; m++) caps = caps && K3.lds_cap(m) == 0;
        caps = caps && K2.lds_cap(-1) == 0 && K2.lds_cap(4) == 0;
        report("name_and_cap", names && caps);
    }
    {   // the families with a cap, in the order of declaration; those without one are not listed
        std::vector<std::string> listed;
        FamilyBase::each([&](const FamilyBase &f) { listed.push_back(f.name); });
        std::string all;
        for (const std::string &s : listed) all += s + ",";
        report("capped_are_listed", listed == std::vector<std::string>{"k4", "k2", "kmapped"}, all);
    }
    return failures ? 1 : 0;
}
