// wfs_family.h -- a kernel family: the instantiations of one kernel template over its axes, tabulated once.
//
// Every instantiation of one kernel template has the same function type, so a family is an array of plain function pointers indexed
// row-major by run-time axis values.  It is declared by a generic lambda that names the axes in order and is called once per member
// with a constant per axis (a std::integral_constant<int, i>: i() is the index as a constant expression):
//
//     const auto K_S2_TILE = family<2, 2>("k_s2_tile", LDS_CAP_TILE, [](auto ap, auto fma) { return &k_s2_tile<ap() != 0, fma() != 0>; });
//     K_S2_TILE(ap_on, cfg.fma)        // the member: function pointer and name
//
// An axis whose template values are not 0 .. N-1 maps the index to the value inside the lambda.  The family also carries what else
// is said once per kernel: the name its launches are timed and checked under, and the cap of its dynamic LDS (0: none; a function of
// the member's indices where only some members have one).  A family with a cap enters the list that FamilyBase::each walks, in the
// order of declaration, so that whoever raises the caps cannot miss one.
// A member index outside its axis is a programming error: it picks a null pointer, never an element past the table.
// No HIP type occurs here: the host compiler builds this header alone (tests/host/family_main.cpp).
#pragma once
#include <array>
#include <cstddef>
#include <type_traits>
#include <utility>

// a kernel that can be launched: the function and the name it is timed and checked under (fn null: no such member of the family `name`)
template <class Fn> struct Kernel { Fn fn; const char *name; };
template <class Fn> constexpr Kernel<Fn> kernel(Fn fn, const char *name) { return Kernel<Fn>{fn, name}; }

// what does not depend on the function type: name, members as untyped addresses with their caps, and the list of the families with a cap
struct FamilyBase {
    const char *name;
    FamilyBase(const char *name_) : name(name_) {}
    FamilyBase(const FamilyBase &) = delete;
    FamilyBase &operator=(const FamilyBase &) = delete;
    virtual ~FamilyBase() = default;
    virtual int size() const = 0;
    virtual const void *address(int member) const = 0;      // (a kernel's address as the runtime's attribute calls take it)
    virtual int lds_cap(int member) const = 0;              // bytes of dynamic LDS the member may ask for; 0: the default limit
    // f(family) for every family that declared a cap, in the order of declaration
    template <class F> static void each(F &&f) { for (const FamilyBase *p = head(); p; p = p->next) f(*p); }
protected:
    void enlist() { const FamilyBase **q = &head(); while (*q) q = &(*q)->next; *q = this; }
private:
    mutable const FamilyBase *next = nullptr;      // (mutable: a later family appends itself behind a const one)
    static const FamilyBase *&head() { static const FamilyBase *first = nullptr; return first; }
};

template <class Fn, int... N> struct Family final : FamilyBase {
    static_assert(sizeof...(N) >= 1 && ((N >= 1) && ...), "a family has at least one axis, an axis at least one value");
    static constexpr int AXES = (int)sizeof...(N), SIZE = (N * ...);
    std::array<Fn, (std::size_t)SIZE> table;
    std::array<int, (std::size_t)SIZE> caps;

    // row-major position of an index tuple, -1 when an index lies outside its axis
    template <class... I> static constexpr int flat(I... idx)
    {
        static_assert(sizeof...(I) == sizeof...(N), "one index per axis");
        const int n[] = {N...}, i[] = {(int)idx...};
        int at = 0;
        for (int a = 0; a < AXES; a++) { if (i[a] < 0 || i[a] >= n[a]) return -1; at = at * n[a] + i[a]; }
        return at;
    }
    template <class... I> Fn pick(I... idx) const { const int at = flat(idx...); return at < 0 ? nullptr : table[(std::size_t)at]; }
    template <class... I> Kernel<Fn> operator()(I... idx) const { return Kernel<Fn>{pick(idx...), name}; }

    int size() const override { return SIZE; }
    const void *address(int m) const override { return m < 0 || m >= SIZE ? nullptr : reinterpret_cast<const void *>(table[(std::size_t)m]); }
    int lds_cap(int m) const override { return m < 0 || m >= SIZE ? 0 : caps[(std::size_t)m]; }

    template <class Cap, class Make> Family(const char *name_, Cap cap, Make make) : FamilyBase(name_), table(members(make, std::make_integer_sequence<int, SIZE>{})), caps(caps_of(cap, std::make_integer_sequence<int, SIZE>{}))
    {
        for (int c : caps) if (c != 0) { enlist(); break; }
    }
private:
    // index of member M on axis A (row-major: the last axis runs fastest)
    template <int M, int A> static constexpr int index_of()
    {
        const int n[] = {N...};
        int m = M;
        for (int a = AXES - 1; a > A; a--) m /= n[a];
        return m % n[A];
    }
    template <int M, class Make, int... A> static Fn member(Make &make, std::integer_sequence<int, A...>) { return make(std::integral_constant<int, index_of<M, A>()>{}...); }
    template <class Make, int... M> static std::array<Fn, (std::size_t)SIZE> members(Make &make, std::integer_sequence<int, M...>)
    {
        return {{member<M>(make, std::make_integer_sequence<int, AXES>{})...}};
    }
    template <int M, class Cap, int... A> static int cap_of(Cap &cap, std::integer_sequence<int, A...>)
    {
        if constexpr (std::is_convertible<Cap, int>::value) return (int)cap;
        else return (int)cap(index_of<M, A>()...);
    }
    template <class Cap, int... M> static std::array<int, (std::size_t)SIZE> caps_of(Cap &cap, std::integer_sequence<int, M...>)
    {
        return {{cap_of<M>(cap, std::make_integer_sequence<int, AXES>{})...}};
    }
};

// The function type of a family is what its lambda returns for the first member; every other member must convert to it.
template <int... N, class Cap, class Make> auto family(const char *name, Cap cap, Make make)
{
    using Fn = decltype(make(std::integral_constant<int, 0 * N>{}...));
    static_assert(std::is_pointer<Fn>::value && std::is_function<std::remove_pointer_t<Fn>>::value, "the lambda returns the address of a function");
    return Family<Fn, N...>(name, cap, make);
}
