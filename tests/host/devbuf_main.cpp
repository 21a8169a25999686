// Drives DevBuf and DevArr (wfsim_amd/csrc/wfs_devbuf.h) on the host: a counting malloc / free pair plays the device allocator.
// Prints one line "<case> ok|FAILED ..." per case and exits 0 when every case holds (tests/test_devbuf_cpu.py).
#include "wfs_devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

static_assert(!std::is_copy_constructible<DevBuf>::value, "a DevBuf has one owner");
static_assert(!std::is_copy_assignable<DevBuf>::value, "a DevBuf has one owner");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value, "a vector of them moves");

// a typed array has one owner too, and is no DevBuf: what takes a DevBuf and a size in bytes (the engine's helper for sort_tmp and the
// record arenas, ensure_bytes here) does not take it
struct Wide { char c[64]; };
static_assert(!std::is_copy_constructible<DevArr<int>>::value && !std::is_copy_assignable<DevArr<Wide>>::value, "a DevArr has one owner");
static_assert(std::is_nothrow_move_constructible<DevArr<int>>::value && std::is_nothrow_move_assignable<DevArr<Wide>>::value, "a vector of them moves");
inline int ensure_bytes(DevBuf &b, size_t bytes) { return b.ensure(bytes); }
template <class B, class = void> struct takes_bytes : std::false_type {};
template <class B> struct takes_bytes<B, std::void_t<decltype(ensure_bytes(std::declval<B &>(), (size_t)1))>> : std::true_type {};
static_assert(takes_bytes<DevBuf>::value && !takes_bytes<DevArr<char>>::value && !takes_bytes<DevArr<double>>::value, "a byte count for an element count does not compile");
static_assert(!std::is_convertible<DevArr<int> &, DevBuf &>::value && sizeof(DevArr<double>) == sizeof(DevBuf), "a DevArr owns a DevBuf and nothing else");

static long n_alloc = 0, n_free = 0, n_bad_free = 0;
static size_t last_bytes = 0;
static bool fail_next = false;
static std::set<void *> blocks;        // what is allocated now: a free of anything else is a double free

static int wfs_dev_alloc(void **p, size_t bytes)
{
    if (fail_next) { fail_next = false; return 2; }
    *p = malloc(bytes);
    if (!*p) return 2;
    blocks.insert(*p); n_alloc++; last_bytes = bytes;
    return 0;
}

static void wfs_dev_free(void *p)
{
    n_free++;
    if (blocks.erase(p) != 1) { n_bad_free++; return; }
    free(p);
}

static long live() { return (long)wfs_dev_live_buffers.load(); }
static long live_bytes() { return (long)wfs_dev_live_bytes.load(); }
// the header's counters agree with the allocator's own, and nothing was freed that was not allocated
static bool balanced() { return n_bad_free == 0 && live() == (long)blocks.size() && n_alloc - n_free == live(); }

static int failures = 0;
static void report(const char *name, bool ok)
{
    ok = ok && balanced();
    printf("%s %s live=%ld bytes=%ld allocs=%ld frees=%ld\n", name, ok ? "ok" : "FAILED", live(), live_bytes(), n_alloc, n_free);
    if (!ok) failures++;
}

struct Several { DevBuf a, b, c; std::vector<DevBuf> v; DevBuf pair[2]; };
struct SeveralTyped { DevArr<char> a; DevArr<double> b; DevArr<Wide> c; std::vector<DevArr<short>> v; DevArr<int> pair[2]; DevBuf bytes; };

// ensure(count) of a DevArr<T> allocates what DevBuf::ensure(count * sizeof(T)) does, block for block: nothing, a first block, none for
// a smaller count, none at the capacity, a grown one
template <class T> static bool arr_matches_buf()
{
    bool ok = true;
    for (size_t count : {(size_t)0, (size_t)1, (size_t)7, (size_t)1000, (size_t)100003}) {
        DevArr<T> a; DevBuf b;
        const long a0 = n_alloc;
        ok = ok && a.p() == nullptr && a.grows(count) && a.ensure(count) == 0 && last_bytes == a.buf().cap && b.ensure(count * sizeof(T)) == 0 && last_bytes == b.cap;
        ok = ok && a.buf().cap == b.cap && (void *)a.p() == a.buf().p && a.p() && n_alloc == a0 + 2 && !a.grows(count);
        const size_t fits = a.buf().cap / sizeof(T);
        ok = ok && a.ensure(count / 2) == 0 && a.ensure(fits) == 0 && n_alloc == a0 + 2 && a.grows(fits + 1) == b.grows((fits + 1) * sizeof(T));
        ok = ok && a.ensure(fits + 1) == 0 && b.ensure((fits + 1) * sizeof(T)) == 0 && a.buf().cap == b.cap && n_alloc == a0 + 4;
        ok = ok && live_bytes() == (long)(a.buf().cap + b.cap);
    }
    return ok && live() == 0;
}

int main()
{
    {   // ensure grows a buffer, and changes nothing when the capacity suffices
        DevBuf b;
        bool ok = b.p == nullptr && b.cap == 0 && live() == 0;
        ok = ok && b.ensure(1000) == 0 && b.p && b.cap >= 1000 && live() == 1 && live_bytes() == (long)b.cap;
        void *p0 = b.p; const size_t c0 = b.cap; const long a0 = n_alloc;
        ok = ok && b.ensure(1000) == 0 && b.ensure(10) == 0 && b.ensure(0) == 0 && b.ensure(c0) == 0;
        ok = ok && b.p == p0 && b.cap == c0 && n_alloc == a0 && n_free == 0;
        ok = ok && b.as<int>() == (int *)p0;
        ok = ok && b.ensure(c0 + 1) == 0 && b.cap >= c0 + 1 && n_alloc == a0 + 1 && live() == 1 && live_bytes() == (long)b.cap;
        report("ensure_grows", ok);
    }
    report("scope_end_frees", live() == 0 && live_bytes() == 0);
    {   // capacity: bytes + bytes / 8 + 256, and 16 for nothing
        bool ok = true;
        for (size_t bytes : {(size_t)1, (size_t)7, (size_t)16, (size_t)1000, (size_t)4096, (size_t)1000003}) {
            DevBuf b;
            ok = ok && b.ensure(bytes) == 0 && b.cap == bytes + bytes / 8 + 256 && last_bytes == b.cap;
        }
        DevBuf z;
        ok = ok && z.ensure(0) == 0 && z.p && z.cap == 16 + 16 / 8 + 256 && last_bytes == z.cap;
        report("capacity_rule", ok);
    }
    {   // a growing ensure frees the old block exactly once
        DevBuf b;
        const long f0 = n_free, a0 = n_alloc;
        bool ok = b.ensure(100) == 0 && n_free == f0;
        void *p0 = b.p;
        ok = ok && b.ensure(5000) == 0 && n_free == f0 + 1 && n_alloc == a0 + 2 && blocks.count(p0) == 0 && blocks.count(b.p) == 1 && live() == 1;
        report("grow_frees_old_once", ok);
    }
    {   // an allocator that fails leaves the buffer empty and the counters right
        DevBuf b;
        bool ok = b.ensure(100) == 0;
        fail_next = true;
        ok = ok && b.ensure(100000) == 2 && b.p == nullptr && b.cap == 0 && live() == 0 && live_bytes() == 0;
        ok = ok && b.ensure(50) == 0 && live() == 1;
        report("failed_alloc_leaves_empty", ok);
    }
    {   // move construction and move assignment: the source is empty, nothing is freed twice
        const long f0 = n_free;
        DevBuf a;
        bool ok = a.ensure(300) == 0;
        void *pa = a.p; const size_t ca = a.cap;
        DevBuf b(std::move(a));
        ok = ok && a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == ca && n_free == f0 && live() == 1;
        DevBuf c;
        ok = ok && c.ensure(40) == 0 && live() == 2;
        void *pc = c.p;
        c = std::move(b);        // c's own block goes, b's moves in
        ok = ok && b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == ca && n_free == f0 + 1 && blocks.count(pc) == 0 && live() == 1;
        DevBuf &same = c;
        c = std::move(same);     // onto itself: nothing happens
        ok = ok && c.p == pa && c.cap == ca && n_free == f0 + 1 && live() == 1;
        a = std::move(b);        // empty onto empty
        ok = ok && a.p == nullptr && n_free == f0 + 1;
        ok = ok && a.ensure(8) == 0 && live() == 2;        // a moved-from buffer is usable again
        report("move", ok);
    }
    report("move_scope_end", live() == 0 && live_bytes() == 0);
    {   // reset() twice is harmless
        DevBuf b;
        const long f0 = n_free;
        bool ok = b.ensure(64) == 0;
        b.reset();
        ok = ok && b.p == nullptr && b.cap == 0 && n_free == f0 + 1 && live() == 0;
        b.reset();
        ok = ok && b.p == nullptr && b.cap == 0 && n_free == f0 + 1 && live() == 0;
        DevBuf never;
        never.reset();
        ok = ok && n_free == f0 + 1;
        report("reset_twice", ok);
    }
    {   // a vector that is resized, reallocated and cleared
        std::vector<DevBuf> v;
        v.resize(3);
        bool ok = true;
        for (auto &b : v) ok = ok && b.ensure(100) == 0;
        void *p1 = v[1].p;
        v.reserve(v.capacity() * 4 + 7);          // the elements move to new storage
        ok = ok && v[1].p == p1 && live() == 3 && n_free == n_alloc - 3;
        v.resize(40);
        for (auto &b : v) ok = ok && b.ensure(100) == 0;
        ok = ok && live() == 40;
        v.resize(5);
        ok = ok && live() == 5;
        v.erase(v.begin());                        // move assignment down the vector
        ok = ok && live() == 4;
        v.clear();
        ok = ok && live() == 0 && live_bytes() == 0;
        v.resize(2);
        ok = ok && v[0].ensure(1) == 0 && live() == 1;
        report("vector", ok);
    }
    report("vector_scope_end", live() == 0 && live_bytes() == 0);
    {   // a struct of several buffers
        auto s = new Several();
        bool ok = s->a.ensure(10) == 0 && s->c.ensure(20000) == 0 && s->pair[1].ensure(0) == 0;
        s->v.resize(4);
        ok = ok && s->v[2].ensure(77) == 0 && live() == 4;
        Several t(std::move(*s));
        delete s;
        ok = ok && live() == 4 && t.a.p && !t.b.p && t.c.p && t.v.size() == 4 && t.pair[1].p;
        report("struct", ok);
    }
    report("struct_scope_end", live() == 0 && live_bytes() == 0 && blocks.empty());
    report("arr_sizes", arr_matches_buf<char>() && arr_matches_buf<short>() && arr_matches_buf<int>() && arr_matches_buf<double>() && arr_matches_buf<Wide>());
    {   // counts of 0 and 1, a grow that frees the old block once, a failed allocation, reset
        DevArr<double> a;
        const long f0 = n_free, a0 = n_alloc;
        bool ok = a.ensure(0) == 0 && a.buf().cap == 16 + 16 / 8 + 256 && live() == 1;
        ok = ok && a.ensure(1) == 0 && n_alloc == a0 + 1;                  // (one double fits the block of nothing)
        double *p0 = a.p();
        ok = ok && a.ensure(1000) == 0 && a.buf().cap == 8000 + 8000 / 8 + 256 && n_free == f0 + 1 && n_alloc == a0 + 2 && blocks.count(p0) == 0 && blocks.count(a.p()) == 1 && live() == 1;
        fail_next = true;
        ok = ok && a.ensure(100000) == 2 && a.p() == nullptr && a.buf().cap == 0 && live() == 0 && live_bytes() == 0;
        ok = ok && a.ensure(3) == 0 && live() == 1;
        a.reset(); a.reset();
        ok = ok && a.p() == nullptr && live() == 0;
        report("arr_grow", ok);
    }
    {   // moves: the source is empty, nothing is freed twice; arrays of different T in one struct and in a vector
        const long f0 = n_free;
        DevArr<int> a;
        bool ok = a.ensure(75) == 0;
        int *pa = a.p(); const size_t ca = a.buf().cap;
        DevArr<int> b(std::move(a));
        ok = ok && a.p() == nullptr && a.buf().cap == 0 && b.p() == pa && b.buf().cap == ca && n_free == f0 && live() == 1;
        DevArr<int> c;
        ok = ok && c.ensure(10) == 0 && live() == 2;
        c = std::move(b);
        ok = ok && b.p() == nullptr && c.p() == pa && n_free == f0 + 1 && live() == 1 && a.ensure(2) == 0 && live() == 2;
        std::vector<DevArr<Wide>> v(3);
        for (auto &w : v) ok = ok && w.ensure(5) == 0;
        Wide *p1 = v[1].p();
        v.reserve(v.capacity() * 4 + 7);
        ok = ok && v[1].p() == p1 && live() == 5;
        v.erase(v.begin());
        ok = ok && live() == 4;
        auto s = new SeveralTyped();
        ok = ok && s->a.ensure(10) == 0 && s->c.ensure(300) == 0 && s->pair[1].ensure(0) == 0 && s->bytes.ensure(99) == 0;
        s->v.resize(4);
        ok = ok && s->v[2].ensure(77) == 0 && live() == 9;
        // (the address of the block's DevBuf tells buffers of different T apart: the engine's pack_uses)
        ok = ok && (const void *)&s->a.buf() != (const void *)&s->b.buf() && &s->bytes != &s->c.buf();
        SeveralTyped t(std::move(*s));
        delete s;
        ok = ok && live() == 9 && t.a.p() && !t.b.p() && t.c.p() && t.v.size() == 4 && t.v[2].p() && t.pair[1].p() && t.bytes.p;
        report("arr_move", ok);
    }
    report("arr_scope_end", live() == 0 && live_bytes() == 0 && blocks.empty());
    return failures ? 1 : 0;
}
