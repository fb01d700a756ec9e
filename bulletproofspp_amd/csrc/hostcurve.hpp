// hostcurve.hpp — the host's window combine of an MSM on lazily reduced 5 x 52-bit limbs.
//
// The combine is one dependency chain on one core after the stream has drained: ~256 doublings, one addition per window sum and
// one inversion.  hostmath.hpp's U256 routines keep every value canonical (a compare and a conditional subtraction after every
// add, sub and mul); here a value is five 64-bit limbs of radix 2^52 whose limbs may exceed 52 bits, products are summed in
// 128-bit columns, add / negate / small multiples are limb-wise without carries, and the only full reduction is the one before a
// zero test or the output.  The layout is the one of csrc/fq26.hip.h with limbs paired (52 = 2 x 26), so a device value converts
// with five shifts and its magnitude carries over unchanged.
//
// Magnitude rule (the device's, fq26.hip.h): a value has magnitude m when n[i] <= 2 m (2^52 - 1) for i < 4 and
// n[4] <= 2 m (2^48 - 1).  Every routine states what it takes and what it returns:
//   f52_mul, f52_sqr      take <= 8 (both operands), return 1
//   f52_add               adds magnitudes;  f52_mul_int(a, k) multiplies the magnitude by k
//   f52_neg(a, m)         takes <= m, returns m + 1
//   f52_weak              takes any limbs < 2^59, returns 1
//   f52_normalize         takes <= 16, returns the canonical value (< p, magnitude 1)
//   f52_is_zero           takes <= 16
// No intermediate exceeds 2^128: a column holds at most five products of two limbs < 2^56 (magnitude 8), < 2^115.
//
// hostmath.hpp's generic mmul / mpow path shares nothing with this file and is the reference of tests/native/hostcurve_check.cpp.
#pragma once
#include "hostmath.hpp"

namespace bppp_host {

struct F52 { uint64_t n[5]; };

static const uint64_t F52_M52 = 0xFFFFFFFFFFFFFULL, F52_M48 = 0x0FFFFFFFFFFFFULL;
static const uint64_t F52_P0 = 0xFFFFEFFFFFC2FULL;          // p = 2^256 - 0x1000003D1: limbs P0, M52, M52, M52, M48
static const uint64_t F52_R = 0x1000003D1ULL;               // 2^256 mod p;  2^260 mod p = 16 R
static const int HC_XYZZ_WORDS = 40;                       // a device point: X, Y, ZZ, ZZZ of 10 x 26-bit limbs each

inline F52 f52_zero() { return F52{{0, 0, 0, 0, 0}}; }
inline F52 f52_one() { return F52{{1, 0, 0, 0, 0}}; }

// canonical U256 -> magnitude 1 (any 256-bit value is accepted; it is not reduced)
inline F52 f52_from_u256(const U256 &a) {
  F52 r;
  r.n[0] = a.w[0] & F52_M52;
  r.n[1] = ((a.w[0] >> 52) | (a.w[1] << 12)) & F52_M52;
  r.n[2] = ((a.w[1] >> 40) | (a.w[2] << 24)) & F52_M52;
  r.n[3] = ((a.w[2] >> 28) | (a.w[3] << 36)) & F52_M52;
  r.n[4] = a.w[3] >> 16;
  return r;
}

// carries and the part above 2^256 folded once: any limbs < 2^59 -> magnitude 1 (not canonical)
inline void f52_weak(F52 &r) {
  uint64_t t0 = r.n[0], t1 = r.n[1], t2 = r.n[2], t3 = r.n[3], t4 = r.n[4];
  const uint64_t x = t4 >> 48; t4 &= F52_M48;
  t0 += x * F52_R;                                           // x < 2^11: no overflow
  t1 += t0 >> 52; t0 &= F52_M52;
  t2 += t1 >> 52; t1 &= F52_M52;
  t3 += t2 >> 52; t2 &= F52_M52;
  t4 += t3 >> 52; t3 &= F52_M52;                             // t4 <= 2^48 + 2^7
  r.n[0] = t0; r.n[1] = t1; r.n[2] = t2; r.n[3] = t3; r.n[4] = t4;
}

// magnitude <= 16 -> the canonical representative
inline void f52_normalize(F52 &r) {
  uint64_t t0 = r.n[0], t1 = r.n[1], t2 = r.n[2], t3 = r.n[3], t4 = r.n[4];
  uint64_t x = t4 >> 48; t4 &= F52_M48;
  t0 += x * F52_R;
  t1 += t0 >> 52; t0 &= F52_M52;
  t2 += t1 >> 52; t1 &= F52_M52; uint64_t m = t1;
  t3 += t2 >> 52; t2 &= F52_M52; m &= t2;
  t4 += t3 >> 52; t3 &= F52_M52; m &= t3;
  // the value is now < 2^256 + 2^(208 + 8): at most one more subtraction of p, when bit 256 is set or the value is >= p
  x = (t4 >> 48) | ((t4 == F52_M48) & (m == F52_M52) & (t0 >= F52_P0));
  t0 += x * F52_R;                                           // adding R and dropping bit 256 subtracts p
  t1 += t0 >> 52; t0 &= F52_M52;
  t2 += t1 >> 52; t1 &= F52_M52;
  t3 += t2 >> 52; t2 &= F52_M52;
  t4 += t3 >> 52; t3 &= F52_M52;
  t4 &= F52_M48;
  r.n[0] = t0; r.n[1] = t1; r.n[2] = t2; r.n[3] = t3; r.n[4] = t4;
}
inline bool f52_is_zero(F52 a) {                              // a = 0 (mod p); magnitude <= 16
  f52_normalize(a);
  return (a.n[0] | a.n[1] | a.n[2] | a.n[3] | a.n[4]) == 0;
}
inline U256 f52_to_u256(F52 a) {                              // magnitude <= 16 -> canonical 4 x u64
  f52_normalize(a);
  U256 o;
  o.w[0] = a.n[0] | (a.n[1] << 52);
  o.w[1] = (a.n[1] >> 12) | (a.n[2] << 40);
  o.w[2] = (a.n[2] >> 24) | (a.n[3] << 28);
  o.w[3] = (a.n[3] >> 36) | (a.n[4] << 16);
  return o;
}

// a device value (10 x 26-bit limbs, csrc/fq26.hip.h) with its limbs paired: device magnitude m -> magnitude m.
// Arbitrary 32-bit limbs give limbs < 2^58, which f52_weak takes.
inline F52 f52_from_limbs26(const uint32_t *q) {
  F52 r;
  for (int i = 0; i < 5; i++) r.n[i] = (uint64_t)q[2 * i] + ((uint64_t)q[2 * i + 1] << 26);
  return r;
}

inline F52 f52_add(const F52 &a, const F52 &b) {                // magnitudes add
  F52 r; for (int i = 0; i < 5; i++) r.n[i] = a.n[i] + b.n[i];
  return r;
}
inline F52 f52_mul_int(const F52 &a, uint64_t k) {             // magnitude x k
  F52 r; for (int i = 0; i < 5; i++) r.n[i] = a.n[i] * k;
  return r;
}
inline F52 f52_neg(const F52 &a, uint64_t m) {                 // -a for a of magnitude <= m: 2 (m + 1) p - a, magnitude m + 1
  F52 r;
  r.n[0] = F52_P0 * 2 * (m + 1) - a.n[0];
  r.n[1] = F52_M52 * 2 * (m + 1) - a.n[1];
  r.n[2] = F52_M52 * 2 * (m + 1) - a.n[2];
  r.n[3] = F52_M52 * 2 * (m + 1) - a.n[3];
  r.n[4] = F52_M48 * 2 * (m + 1) - a.n[4];
  return r;
}

// nine 128-bit columns (each < 2^115) -> magnitude 1.  The upper four are carried into 52-bit limbs first, so that their fold
// (2^260 = 16 R) fits a column; the carry out of 2^256 folds once more with R and lands in n[0], n[1].
inline F52 f52_reduce9(u128 c0, u128 c1, u128 c2, u128 c3, u128 c4, u128 c5, u128 c6, u128 c7, u128 c8) {
  const uint64_t R16 = F52_R << 4;
  u128 t = c5;
  const uint64_t h0 = (uint64_t)t & F52_M52; t >>= 52; t += c6;
  const uint64_t h1 = (uint64_t)t & F52_M52; t >>= 52; t += c7;
  const uint64_t h2 = (uint64_t)t & F52_M52; t >>= 52; t += c8;
  const uint64_t h3 = (uint64_t)t & F52_M52; t >>= 52;
  const uint64_t h4 = (uint64_t)t;                          // < 2^63
  F52 r;
  t = c0 + (u128)h0 * R16;
  r.n[0] = (uint64_t)t & F52_M52; t >>= 52; t += c1 + (u128)h1 * R16;
  r.n[1] = (uint64_t)t & F52_M52; t >>= 52; t += c2 + (u128)h2 * R16;
  r.n[2] = (uint64_t)t & F52_M52; t >>= 52; t += c3 + (u128)h3 * R16;
  r.n[3] = (uint64_t)t & F52_M52; t >>= 52; t += c4 + (u128)h4 * R16;
  r.n[4] = (uint64_t)t & F52_M48; t >>= 48;                  // t < 2^68
  t = t * F52_R + r.n[0];                                    // < 2^102
  r.n[0] = (uint64_t)t & F52_M52; t >>= 52;
  r.n[1] += (uint64_t)t;                                    // < 2^52 + 2^50
  return r;
}
inline F52 f52_mul(const F52 &a, const F52 &b) {                // magnitudes <= 8 -> 1
  const uint64_t a0 = a.n[0], a1 = a.n[1], a2 = a.n[2], a3 = a.n[3], a4 = a.n[4];
  const uint64_t b0 = b.n[0], b1 = b.n[1], b2 = b.n[2], b3 = b.n[3], b4 = b.n[4];
  return f52_reduce9((u128)a0 * b0,
                    (u128)a0 * b1 + (u128)a1 * b0,
                    (u128)a0 * b2 + (u128)a1 * b1 + (u128)a2 * b0,
                    (u128)a0 * b3 + (u128)a1 * b2 + (u128)a2 * b1 + (u128)a3 * b0,
                    (u128)a0 * b4 + (u128)a1 * b3 + (u128)a2 * b2 + (u128)a3 * b1 + (u128)a4 * b0,
                    (u128)a1 * b4 + (u128)a2 * b3 + (u128)a3 * b2 + (u128)a4 * b1,
                    (u128)a2 * b4 + (u128)a3 * b3 + (u128)a4 * b2,
                    (u128)a3 * b4 + (u128)a4 * b3,
                    (u128)a4 * b4);
}
inline F52 f52_sqr(const F52 &a) {                             // magnitude <= 8 -> 1
  const uint64_t a0 = a.n[0], a1 = a.n[1], a2 = a.n[2], a3 = a.n[3], a4 = a.n[4];
  const uint64_t d0 = a0 * 2, d1 = a1 * 2, d2 = a2 * 2, d3 = a3 * 2;     // < 2^57
  return f52_reduce9((u128)a0 * a0,
                    (u128)d0 * a1,
                    (u128)d0 * a2 + (u128)a1 * a1,
                    (u128)d0 * a3 + (u128)d1 * a2,
                    (u128)d0 * a4 + (u128)d1 * a3 + (u128)a2 * a2,
                    (u128)d1 * a4 + (u128)d2 * a3,
                    (u128)d2 * a4 + (u128)a3 * a3,
                    (u128)d3 * a4,
                    (u128)a4 * a4);
}
inline F52 f52_sqrn(F52 a, int k) { for (int i = 0; i < k; i++) a = f52_sqr(a); return a; }

// a^(p - 2) by a fixed addition chain, 255 squarings and 15 multiplications; 0 -> 0.  Magnitude <= 8 -> 1.
// p - 2 in binary: 223 ones, a zero, 22 ones, then 0000101101; x_k below is a^(2^k - 1).
inline F52 f52_inv(const F52 &a) {
  const F52 x2 = f52_mul(f52_sqr(a), a);
  const F52 x3 = f52_mul(f52_sqr(x2), a);
  const F52 x6 = f52_mul(f52_sqrn(x3, 3), x3);
  const F52 x9 = f52_mul(f52_sqrn(x6, 3), x3);
  const F52 x11 = f52_mul(f52_sqrn(x9, 2), x2);
  const F52 x22 = f52_mul(f52_sqrn(x11, 11), x11);
  const F52 x44 = f52_mul(f52_sqrn(x22, 22), x22);
  const F52 x88 = f52_mul(f52_sqrn(x44, 44), x44);
  const F52 x176 = f52_mul(f52_sqrn(x88, 88), x88);
  const F52 x220 = f52_mul(f52_sqrn(x176, 44), x44);
  const F52 x223 = f52_mul(f52_sqrn(x220, 3), x3);
  F52 t = f52_mul(f52_sqrn(x223, 23), x22);
  t = f52_mul(f52_sqrn(t, 5), a);
  t = f52_mul(f52_sqrn(t, 3), x2);
  return f52_mul(f52_sqrn(t, 2), a);
}

// ---- curve y^2 = x^3 + 7 on that field
// Jacobian accumulator; infinity is the flag (X, Y, Z are then unspecified).  Magnitudes: X <= 6, Y <= 4, Z <= 2 after fj_dbl,
// all 1 after fj_add_xyzz; both routines take X, Y, Z <= 8.
struct FJac { F52 X, Y, Z; bool inf; };
// a device window sum: x = X / ZZ, y = Y / ZZZ with ZZ^3 = ZZZ^2; ZZ = 0 (mod p) is infinity
struct FXyzz { F52 X, Y, ZZ, ZZZ; bool inf; };
inline FJac fj_inf() { return FJac{f52_one(), f52_one(), f52_zero(), true}; }

// 40 words of the device (any 32-bit limbs; the reduce kernels state X <= 5, Y <= 3, ZZ = ZZZ = 1) -> magnitude 1 each
inline FXyzz fx_from_device(const uint32_t *q) {
  FXyzz p;
  p.X = f52_from_limbs26(q); p.Y = f52_from_limbs26(q + 10); p.ZZ = f52_from_limbs26(q + 20); p.ZZZ = f52_from_limbs26(q + 30);
  f52_weak(p.X); f52_weak(p.Y); f52_weak(p.ZZ); f52_weak(p.ZZZ);
  p.inf = f52_is_zero(p.ZZ);
  return p;
}

// 2 P for a = 0 (dbl-2009-l shape): 3 M + 4 S, no modular add or sub.  With L = 3 X^2 and T = 2 Y^2:
//   X3 = L^2 - 4 X T,  Y3 = L (6 X T - L^2) - 2 T^2,  Z3 = 2 Y Z.
// The curve has odd order, so Y = 0 does not occur on it (Z3 would be 0 with the flag clear).
inline FJac fj_dbl(const FJac &p) {
  if (p.inf) return p;
  FJac r; r.inf = false;
  r.Z = f52_mul_int(f52_mul(p.Y, p.Z), 2);                    // 2
  const F52 L = f52_mul_int(f52_sqr(p.X), 3);                  // 3
  const F52 LL = f52_sqr(L);                                  // 1
  const F52 T = f52_mul_int(f52_sqr(p.Y), 2);                  // 2
  const F52 TT2 = f52_mul_int(f52_sqr(T), 2);                  // 2: 8 Y^4
  const F52 XT = f52_mul(T, p.X);                             // 1: 2 X Y^2
  r.X = f52_add(f52_neg(f52_mul_int(XT, 4), 4), LL);           // 5 + 1 = 6
  const F52 u = f52_add(f52_mul_int(XT, 6), f52_neg(LL, 1));    // 6 + 2 = 8
  r.Y = f52_add(f52_mul(L, u), f52_neg(TT2, 2));               // 1 + 3 = 4
  return r;
}

// P + Q for a Jacobian P and a device XYZZ Q, complete (either side infinity, P = Q, P = -Q): 13 M + 3 S.
// On the common denominators Z1^2 ZZ and Z1^3 ZZZ:  U1 = X1 ZZ, U2 = X2 Z1^2, S1 = Y1 ZZZ, S2 = Y2 Z1^3, H = U2 - U1, R = S2 - S1,
//   X' = R^2 - H^3 - 2 U1 H^2,  Y' = R (U1 H^2 - X') - S1 H^3   over the denominators (Z1^2 ZZ H^2, Z1^3 ZZZ H^3).
// Q has no Z with Z^2 = ZZ to hand, so the result is scaled by it: (ZZ X', ZZZ Y', Z1 ZZ H) is Jacobian, since
//   ZZ X' / (Z1 ZZ H)^2 = X' / (Z1^2 ZZ H^2)  and  ZZZ Y' / (Z1 ZZ H)^3 = Y' / (Z1^3 ZZZ H^3)  by ZZ^3 = ZZZ^2.
inline FJac fj_add_xyzz(const FJac &p, const FXyzz &q) {
  if (q.inf) return p;
  if (p.inf) return FJac{f52_mul(q.X, q.ZZ), f52_mul(q.Y, q.ZZZ), q.ZZ, false};     // (X ZZ, Y ZZZ, ZZ)
  const F52 z1z1 = f52_sqr(p.Z), z1c = f52_mul(z1z1, p.Z);
  const F52 u1 = f52_mul(p.X, q.ZZ), u2 = f52_mul(q.X, z1z1);
  const F52 s1 = f52_mul(p.Y, q.ZZZ), s2 = f52_mul(q.Y, z1c);
  const F52 h = f52_add(u2, f52_neg(u1, 1)), r = f52_add(s2, f52_neg(s1, 1));          // 3, 3
  if (f52_is_zero(h)) return f52_is_zero(r) ? fj_dbl(p) : fj_inf();
  const F52 hh = f52_sqr(h), hhh = f52_mul(h, hh), v = f52_mul(u1, hh);
  const F52 x = f52_add(f52_add(f52_sqr(r), f52_neg(hhh, 1)), f52_neg(f52_mul_int(v, 2), 2));     // 1 + 2 + 3 = 6
  const F52 y = f52_add(f52_mul(r, f52_add(v, f52_neg(x, 6))), f52_neg(f52_mul(s1, hhh), 1));     // (1 + 7 = 8) -> 1 + 2 = 3
  return FJac{f52_mul(x, q.ZZ), f52_mul(y, q.ZZZ), f52_mul(f52_mul(p.Z, q.ZZ), h), false};
}

// Jacobian -> canonical affine (x, y), infinity -> (0, 0)
inline void fj_to_affine(const FJac &p, uint64_t out_xy[8]) {
  if (p.inf || f52_is_zero(p.Z)) { memset(out_xy, 0, 64); return; }
  const F52 zi = f52_inv(p.Z), zi2 = f52_sqr(zi);
  f52_to_u256(f52_mul(p.X, zi2)).store(out_xy);
  f52_to_u256(f52_mul(p.Y, f52_mul(zi2, zi))).store(out_xy + 4);
}

// The Horner combine of one MSM's window sums, highest window first:  result = sum_w 2^(off_w) V_w,  off_w = the widths below w.
//   ws     W window values as the device leaves them: HC_XYZZ_WORDS words each, or two points (W1, W2) each when marg
//   width  window w is c bits wide for w < acnt and c - 1 bits above (balanced widths); pass acnt = W when all are c wide
//   marg   V_w = 2^a W1 + W2 (the marginal reduction): the window's doublings are split around W1
// out_xy is the canonical affine point, (0, 0) for infinity.
inline void window_combine_host(const uint32_t *ws, int W, int c, int acnt, bool marg, int a, uint64_t out_xy[8]) {
  FJac r = fj_inf();
  for (int w = W - 1; w >= 0; w--) {
    const int cw = w < acnt ? c : c - 1;
    if (marg) {
      const uint32_t *q = ws + (size_t)w * 2 * HC_XYZZ_WORDS;
      for (int k = 0; k < cw - a; k++) r = fj_dbl(r);
      r = fj_add_xyzz(r, fx_from_device(q));
      for (int k = 0; k < a; k++) r = fj_dbl(r);
      r = fj_add_xyzz(r, fx_from_device(q + HC_XYZZ_WORDS));
    } else {
      for (int k = 0; k < cw; k++) r = fj_dbl(r);
      r = fj_add_xyzz(r, fx_from_device(ws + (size_t)w * HC_XYZZ_WORDS));
    }
  }
  fj_to_affine(r, out_xy);
}

}  // namespace bppp_host
