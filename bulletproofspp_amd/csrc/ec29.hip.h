// ec29.hip.h — the mixed addition of ec.hip.h over fq29 (9 x 29-bit limbs, fq29.hip.h), for the sized accumulation (msm.hip section 3').
// Same formula (madd-2008-s), same completeness (infinity on either side, P = Q, P = -Q) and the same invariants in fq29's
// magnitudes:   affine x 1, y <= 2 (after the sign fold)      XYZZ  X <= 5, Y <= 3, ZZ = ZZZ = 1 (tight)
// Infinity: affine (0, 0); XYZZ with every limb of ZZ exactly zero.  Every line's magnitude is derived, and asserted at its worst case, in
// benchmarks/fe29_model.py (xyzz_madd).  What differs from fq26: fq29_sqr takes magnitude <= 2, so Pd (7) and R (5) take a
// weak pass before they are squared.  Pd's is the one its zero test makes anyway; R's is the one new pass of an addition.
#pragma once
#include "ec.hip.h"
#include "fq29.hip.h"

namespace bppp {

struct aff29 { fq29 x, y; };
struct xyzz29 { fq29 X, Y, ZZ, ZZZ; };

BPPP_DI bool aff29_is_inf(const aff29 &p) { return fq29_all_zero(p.x) && fq29_all_zero(p.y); }   // canonical inputs
BPPP_DI bool xyzz29_is_inf(const xyzz29 &p) { return fq29_all_zero(p.ZZ); }
BPPP_DI xyzz29 xyzz29_inf() { xyzz29 r; r.X = fq29_zero(); r.Y = fq29_zero(); r.ZZ = fq29_zero(); r.ZZZ = fq29_zero(); return r; }
BPPP_DI xyzz29 xyzz29_from_aff(const aff29 &p) {
  xyzz29 r; r.X = p.x; r.Y = p.y;
  r.ZZ = fq29_zero(); r.ZZ.n[0] = aff29_is_inf(p) ? 0u : 1u; r.ZZZ = r.ZZ;
  return r;
}
// the sign of the digit folded into the point (aff_cneg): y of magnitude 1 in, <= 2 out
BPPP_DI aff29 aff29_cneg(const aff29 &p, bool neg) {
  aff29 r; r.x = p.x;
  const fq29 ny = fq29_neg<1>(p.y);
  const bool inf = aff29_is_inf(p);
#pragma unroll
  for (int i = 0; i < 9; i++) r.y.n[i] = (neg && !inf) ? ny.n[i] : p.y.n[i];
  return r;
}
BPPP_DI aff29 aff29_load(const uint32_t *p) {            // ABI format: canonical x ++ y, 8 x u32 each
  aff29 r; r.x = fq29_from_fe(fe_load(p)); r.y = fq29_from_fe(fe_load(p + 8)); return r;
}

// doubling of an affine point into XYZZ, y magnitude <= 2.  Only the P = Q branch of the mixed addition comes here (one entry in ~2^256 for
// independent points), so it goes through the 10 x 26 form: xyzz_dbl_aff of ec.hip.h on the repacked point, the result normalised and cut
// back into 29-bit limbs: canonical, so tight.
BPPP_DI fq29 fq29_from_fq26(const fq &a) { return fq29_from_fe(fq_to_fe(a)); }
BPPP_DI xyzz29 xyzz29_dbl_aff(const aff29 &p) {
  aff q; q.x = fq29_to_fq26(p.x); q.y = fq29_to_fq26(p.y);     // limbs below 2^26: magnitude 1
  const xyzz d = xyzz_dbl_aff(q);                               // infinity (all limbs zero) for y = 0
  xyzz29 r; r.X = fq29_from_fq26(d.X); r.Y = fq29_from_fq26(d.Y); r.ZZ = fq29_from_fq26(d.ZZ); r.ZZZ = fq29_from_fq26(d.ZZZ);
  return r;
}

// acc += q (q affine, y magnitude <= 2): madd-2008-s, complete
BPPP_DI void xyzz29_madd(xyzz29 &acc, const aff29 &q) {
  if (aff29_is_inf(q)) return;
  if (xyzz29_is_inf(acc)) { acc = xyzz29_from_aff(q); return; }
  const fq29 U2 = fq29_mul(q.x, acc.ZZ), S2 = fq29_mul(q.y, acc.ZZZ);        // 1 * 1, 2 * 1
  const fq29 Pd = fq29_weak_pass(fq29_sub<5>(U2, acc.X));                    // 1 + 6 = 7 -> 1
  const fq29 R = fq29_weak_pass(fq29_sub<3>(S2, acc.Y));                     // 1 + 4 = 5 -> 1
  if (fq29_weak_is_zero(Pd)) {                                               // same x: P = Q or P = -Q
    if (fq29_weak_is_zero(R)) acc = xyzz29_dbl_aff(q); else acc = xyzz29_inf();
    return;
  }
  const fq29 PP = fq29_sqr(Pd), PPP = fq29_mul(Pd, PP), Q = fq29_mul(acc.X, PP);               // Q: 5 * 1
  const fq29 X3 = fq29_sub<3>(fq29_sqr(R), fq29_add(PPP, fq29_mul_int(Q, 2)));                 // 1 + 4 = 5
  const fq29 Y3 = fq29_sub<1>(fq29_mul(R, fq29_sub<5>(Q, X3)), fq29_mul(acc.Y, PPP));          // 1 * 7, 3 * 1;  1 + 2 = 3
  acc.ZZ = fq29_mul(acc.ZZ, PP); acc.ZZZ = fq29_mul(acc.ZZZ, PPP);
  acc.X = X3; acc.Y = Y3;
}

// ---- the exception-free addition of k_acc_points_sized29_fast (msm.hip section 3').  It tests nothing: on a finite accumulator and a finite
// q != +-acc it gives the group element xyzz29_madd gives.  On any other input every limb stays inside the same bounds, because the magnitude
// contracts of fq29 depend on limb bounds and not on values, and ZZ3 = ZZ * Pd^2 is 0 (mod p) from the first step with Pd = 0 (mod p) to the end
// of the item (Fq has no zero divisors, so it is 0 for no other reason): the caller tests ZZ once per item and redoes a flagged item with xyzz29_madd.
// An input point at infinity must not come here (it would leave ZZ != 0); aff29_load_finite tells the caller.
// Y3 = R (Q - X3) - Y PPP is ONE reduced sum of two products (fq29_mul_add2): Q - X3 (1 + 6 = 7) takes a weak pass, then 1 * 1 + 4 * 1 = 5; Y3
// comes out tight.  Every line's magnitude is asserted at its worst case in benchmarks/fe29_model.py (xyzz_madd_fast).
// Limb 8 of PP, PPP and of the new ZZ, ZZZ is made opaque (fq29_opaque8).  Each is `c & 0xFFFFFF` of a product's tail, which the compiler sees
// as a 24-bit value; where such a limb meets another limb 8 it knows to be 24 bits wide (x >> 8 of a loaded point, or another product's, also
// through the loop's phi) it takes the product a8 * b8 of column 16 for a 24-bit multiplication, drops the masks as that form ignores the upper
// bits, and then selects the full 32 x 32 v_mad_u64_u32 for it: the multiplicand is the unmasked carry.  Seen in the gfx950 assembly (hipcc -O3)
// of ZZ * PP and ZZZ * PPP of this function (wrong ZZ and ZZZ from the second trip of the item loop on; on the first ZZ.n[8] is 0) and of
// x1 * PP in xyzz29_from_two.  Limbs read from memory, weak-passed limbs (25 bits) and sums do not match, which is why the host and the one-call
// test kernel are right.  xyzz29_madd has the same products in its source and its generated code is right in every kernel that holds it: checked
// in assembly with benchmarks/isa_carry_operands.py, which finds such a multiplicand (DESIGN.md 0.2 names the products and what was scanned).
BPPP_DI void fq29_opaque8(fq29 &a) { asm volatile("" : "+v"(a.n[8])); }
BPPP_DI void xyzz29_madd_fast(xyzz29 &acc, const aff29 &q) {
  const fq29 U2 = fq29_mul(q.x, acc.ZZ), S2 = fq29_mul(q.y, acc.ZZZ);        // 1 * 1, 2 * 1
  const fq29 Pd = fq29_weak_pass(fq29_sub<5>(U2, acc.X));                    // 1 + 6 = 7 -> 1
  const fq29 R = fq29_weak_pass(fq29_sub<3>(S2, acc.Y));                     // 1 + 4 = 5 -> 1
  fq29 PP = fq29_sqr(Pd); fq29_opaque8(PP);
  fq29 PPP = fq29_mul(Pd, PP); fq29_opaque8(PPP);
  const fq29 Q = fq29_mul(acc.X, PP);                                        // 5 * 1
  const fq29 X3 = fq29_sub<3>(fq29_sqr(R), fq29_add(PPP, fq29_mul_int(Q, 2)));                 // 1 + 4 = 5
  const fq29 Y3 = fq29_mul_add2(R, fq29_weak_pass(fq29_sub<5>(Q, X3)), fq29_neg<3>(acc.Y), PPP);   // 1 * 1 + 4 * 1 = 5 -> 1
  acc.ZZ = fq29_mul(acc.ZZ, PP); acc.ZZZ = fq29_mul(acc.ZZZ, PPP);
  fq29_opaque8(acc.ZZ); fq29_opaque8(acc.ZZZ);                               // they meet q.x and the next PP, PPP
  acc.X = X3; acc.Y = Y3;
}
// p + q for two finite affine points of different x (y magnitude <= 2): mmadd-2008-s, 4 M + 2 S, the start of an item of two or more finite
// entries.  x1 = x2 gives ZZ = 0 (mod p), the same flag.  PP and PPP are opaque in limb 8 before they meet x1, y1 and, as ZZ and ZZZ, the next point.
BPPP_DI xyzz29 xyzz29_from_two(const aff29 &p, const aff29 &q) {
  const fq29 Pd = fq29_weak_pass(fq29_sub<1>(q.x, p.x));                     // 1 + 2 = 3 -> 1
  const fq29 R = fq29_weak_pass(fq29_sub<2>(q.y, p.y));                      // 2 + 3 = 5 -> 1
  xyzz29 r;
  r.ZZ = fq29_sqr(Pd); fq29_opaque8(r.ZZ);
  r.ZZZ = fq29_mul(Pd, r.ZZ); fq29_opaque8(r.ZZZ);
  const fq29 Q = fq29_mul(p.x, r.ZZ);
  r.X = fq29_sub<3>(fq29_sqr(R), fq29_add(r.ZZZ, fq29_mul_int(Q, 2)));                         // 1 + 4 = 5
  r.Y = fq29_mul_add2(R, fq29_weak_pass(fq29_sub<5>(Q, r.X)), fq29_neg<2>(p.y), r.ZZZ);        // 1 * 1 + 3 * 1 = 4 -> 1
  return r;
}
// a gathered point with its sign folded in, and whether it is finite: the 16 ABI words are tested with one OR chain before the limb conversion
BPPP_DI aff29 aff29_load_finite(const uint32_t *p, bool neg, bool &finite) {
  const fe x = fe_load(p), y = fe_load(p + 8);
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= x.v[i] | y.v[i];
  finite = o != 0;
  aff29 r; r.x = fq29_from_fe(x);
  const fq29 py = fq29_from_fe(y), ny = fq29_neg<1>(py);
#pragma unroll
  for (int i = 0; i < 9; i++) r.y.n[i] = neg ? ny.n[i] : py.n[i];
  return r;
}

// the accumulator in the stored layout of ec.hip.h (40 words of fq26 limbs): every limb below 2^26, so X, Y, ZZ and ZZZ have magnitude 1,
// within what every reader of `buckets` and `pieces` accepts (X <= 5, Y <= 3, ZZ = ZZZ = 1); infinity stays ZZ all zero
BPPP_DI xyzz xyzz29_to_xyzz(const xyzz29 &a) {
  xyzz r; r.X = fq29_to_fq26(a.X); r.Y = fq29_to_fq26(a.Y); r.ZZ = fq29_to_fq26(a.ZZ); r.ZZZ = fq29_to_fq26(a.ZZZ);
  return r;
}

}  // namespace bppp
