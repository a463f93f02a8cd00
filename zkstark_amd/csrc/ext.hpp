// ext.hpp -- arithmetic in E = GF(P)[u] / (u^2 - 5), the quadratic extension the challenges of an `ext_log = 1` proof live in
// (DESIGN.md 7j), shared by host and device code.
//
// 5 = GEN_W generates GF(P)^*, so it is a non-residue (5^((P-1)/2) = -1) and u^2 - 5 is irreducible.  An element is
// (c0, c1) = c0 + c1 u with both components canonical residues:
//   (a0 + a1 u)(b0 + b1 u) = (a0 b0 + 5 a1 b1) + (a0 b1 + a1 b0) u.
//
// Conventions follow field.hpp: bulk data is canonical, constants are Montgomery.  A constant of E that multiplies data is an
// ExtConst: its two components in Montgomery form and 5 c1 beside them, so that a product by it is four base multiplications and
// two additions -- no multiplication by 5 on the device, and fewer instructions than the three multiplications of Karatsuba, whose
// five extra additions and subtractions each cost a carry select in this field (counts in DESIGN.md 7j).
#pragma once
#include "field.hpp"

namespace zk {

constexpr uint32_t EXT_NONRESIDUE = GEN_W;   // u^2

struct Ext { uint32_t c0, c1; };                 // canonical
struct ExtConst { uint32_t c0, c1, c1w; };      // Montgomery: c0, c1, 5 c1

ZK_HD Ext ext_add(Ext a, Ext b) { return Ext{add(a.c0, b.c0), add(a.c1, b.c1)}; }
ZK_HD Ext ext_sub(Ext a, Ext b) { return Ext{sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
// a * s for a base-field s in Montgomery form
ZK_HD Ext ext_scale(Ext a, uint32_t s_mont) { return Ext{mont_mul(a.c0, s_mont), mont_mul(a.c1, s_mont)}; }
// a * k: canonical in, canonical out
ZK_HD Ext ext_mul_const(Ext a, const ExtConst& k) {
    return Ext{add(mont_mul(a.c0, k.c0), mont_mul(a.c1, k.c1w)), add(mont_mul(a.c0, k.c1), mont_mul(a.c1, k.c0))};
}

// Host-side helpers.  Plain residues in and out; the product is the device's.
inline ExtConst ext_const(Ext b) { return ExtConst{to_mont(b.c0), to_mont(b.c1), to_mont(mulmod(b.c1 % P, EXT_NONRESIDUE))}; }
inline Ext ext_reduce(uint32_t r0, uint32_t r1) { return Ext{r0 % P, r1 % P}; }
inline Ext ext_mul(Ext a, Ext b) { return ext_mul_const(a, ext_const(b)); }
inline bool ext_is_zero(Ext a) { return (a.c0 | a.c1) == 0; }
inline bool ext_eq(Ext a, Ext b) { return a.c0 == b.c0 && a.c1 == b.c1; }
// 1 / a = (a0 - a1 u) / (a0^2 - 5 a1^2); the norm of a non-zero element is non-zero because 5 is a non-residue.  a != 0.
inline Ext ext_inv(Ext a) {
    const uint32_t norm = sub(mulmod(a.c0, a.c0), mulmod(EXT_NONRESIDUE, mulmod(a.c1, a.c1)));
    const uint32_t ni = invmod(norm);
    return Ext{mulmod(a.c0, ni), mulmod(neg(a.c1), ni)};
}
inline Ext ext_pow(Ext a, uint64_t e) {
    Ext r{1u, 0u}, b = a;
    while (e) {
        if (e & 1) r = ext_mul(r, b);
        b = ext_mul(b, b);
        e >>= 1;
    }
    return r;
}

}  // namespace zk
