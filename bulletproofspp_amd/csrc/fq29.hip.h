// fq29.hip.h — the coordinate field Fq (p = 2^256 - 2^32 - 977) in 9 x 29-bit limbs with lazy reduction: 81 partial products per
// multiplication instead of fq26's 100, for the one kernel that is bound by their issue rate (k_acc_points_sized29, msm.hip section 3').
// Limb i holds bits 29 i .. 29 i + 28; limb 8 holds 24 bits.  The same two pinned carry chains as fq_mul (fq26.hip.h): H = columns 8 .. 16,
// L = columns 0 .. 7 with the fold of H's limbs, 2^261 = R1 * 2^29 + R0 (mod p) held in scalar registers: 81 + 15 products for the fold + 4 in
// the tail, 17 carry cuts.  A squaring has 45 products.
//
// The price is headroom, 3 spare bits per limb instead of 6.  Bound discipline (modelled bit-exactly and in upper bounds, with an assertion on
// every 64-bit accumulator and every 32-bit limb, in benchmarks/fe29_model.py; tests/test_fe29_model.py):
//   a value has magnitude m when limb[i] <= m * (2^29 + 2^8) for i < 8 and limb[8] <= m * (2^24 + 2^8); a u32 limb holds magnitude 7 at most.
//   tight = magnitude 1.  The 2^8 is slack: a weak pass leaves limb 8 <= 2^24 + 7, a product leaves limb 3 <= 2^29.
//   mul(a, b)   mag(a) * mag(b) <= 7, tight out.  Column 7 has 8 full products: 8 * 7 * 2^58 = 0.875 * 2^64; the rest covers the carry-in
//               (< 2^36), the two fold terms (< 2^45) and the slack.  mag 1 * 8 and 2 * 4 reach 2^64: forbidden.
//   sqr(a)      mag(a) <= 2 (the doubled limbs make column 7 8 * m^2 * 2^58), tight out.
//   mul_add2(a, b, c, d) = a b + c d under one fold and one tail: mag(a) * mag(b) + mag(c) * mag(d) <= 7, tight out (column 7: 16 products).
//   add         adds magnitudes;  sub<K>(a, b): mag(b) <= K, result mag(a) + K + 1;  neg<K>: K + 1;  mul_int(a, k): k * mag(a).
//   weak_pass   any magnitude <= 7 in, tight out, value < 2^256 + 2^236.
// Only the sized accumulation uses this type: points come in as canonical 8 x 32 words and sums leave as fq26 limbs (fq29_to_fq26).
#pragma once
#include "fq26.hip.h"

namespace bppp {

struct fq29 { uint32_t n[9]; };

static constexpr uint32_t FQ29_M29 = 0x1FFFFFFFu, FQ29_M24 = 0xFFFFFFu;
static constexpr uint32_t FQ29_R0 = 0x7A20u, FQ29_R1 = 0x100u;   // 2^261 = R1 * 2^29 + R0 (mod p)

BPPP_DI uint32_t fq29_plimb(int i) { return i == 0 ? 0x1FFFFC2Fu : i == 1 ? 0x1FFFFFF7u : i == 8 ? FQ29_M24 : FQ29_M29; }

BPPP_DI fq29 fq29_zero() { fq29 r; for (int i = 0; i < 9; i++) r.n[i] = 0; return r; }
BPPP_DI bool fq29_all_zero(const fq29 &a) {      // exact all-limbs-zero test (the infinity marker)
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) o |= a.n[i];
  return o == 0;
}

// ---- multiplication
// the tail shared by mul and sqr: limb 8 and everything above 2^256 folded back (2^256 = 8 * 2^29 + 0x3D1)
BPPP_DI void fq29_mul_tail(fq29 &r, uint64_t c, uint32_t t8, uint64_t u8, uint32_t u7) {
  c += (uint64_t)t8 + u8 * FQ29_R0 + (uint64_t)u7 * FQ29_R1;
  r.n[8] = (uint32_t)c & FQ29_M24;
  const uint64_t top = (c >> 24) + ((u8 * FQ29_R1) << 5);   // units of 2^256
  c = (uint64_t)r.n[0] + top * 0x3D1u; r.n[0] = (uint32_t)c & FQ29_M29; c >>= 29;
  c += (uint64_t)r.n[1] + (top << 3); r.n[1] = (uint32_t)c & FQ29_M29; c >>= 29;
  c += r.n[2]; r.n[2] = (uint32_t)c & FQ29_M29; c >>= 29;
  r.n[3] += (uint32_t)c;
}
BPPP_DI fq29 fq29_mul(const fq29 &a, const fq29 &b) {
  const uint32_t R0 = fq_sreg(FQ29_R0), R1 = fq_sreg(FQ29_R1);
  uint64_t d = 0;
#pragma unroll
  for (int i = 0; i <= 8; i++) d = fq_madc(a.n[i], b.n[8 - i], d);
  const uint32_t t8 = (uint32_t)d & FQ29_M29; d >>= 29;
  uint32_t u[8];
#pragma unroll
  for (int k = 9; k <= 16; k++) {
#pragma unroll
    for (int i = k - 8; i <= 8; i++) d = fq_madc(a.n[i], b.n[k - i], d);
    u[k - 9] = (uint32_t)d & FQ29_M29; d >>= 29;
  }
  const uint64_t u8 = d;                           // leftover carry, < 2^36
  fq29 r;
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
#pragma unroll
    for (int i = 0; i <= k; i++) c = fq_madc(a.n[i], b.n[k - i], c);
    c = fq_madc(u[k], R0, c);
    if (k) c = fq_madc(u[k - 1], R1, c);
    r.n[k] = (uint32_t)c & FQ29_M29; c >>= 29;
  }
  fq29_mul_tail(r, c, t8, u8, u[7]);
  return r;
}

// a b + c d under one reduction: both products' terms go into each column of the same two chains, so the pair pays one fold and one tail
// (19 products and 17 carry cuts less than two multiplications).  mag(a) * mag(b) + mag(c) * mag(d) <= 7, tight out: column 7 holds 16
// products that together stay below what mul's 8 reach at 1 * 7 (fe29_model.py, mul_add2).
BPPP_DI fq29 fq29_mul_add2(const fq29 &a, const fq29 &b, const fq29 &c, const fq29 &e) {
  const uint32_t R0 = fq_sreg(FQ29_R0), R1 = fq_sreg(FQ29_R1);
  uint64_t d = 0;
#pragma unroll
  for (int i = 0; i <= 8; i++) { d = fq_madc(a.n[i], b.n[8 - i], d); d = fq_madc(c.n[i], e.n[8 - i], d); }
  const uint32_t t8 = (uint32_t)d & FQ29_M29; d >>= 29;
  uint32_t u[8];
#pragma unroll
  for (int k = 9; k <= 16; k++) {
#pragma unroll
    for (int i = k - 8; i <= 8; i++) { d = fq_madc(a.n[i], b.n[k - i], d); d = fq_madc(c.n[i], e.n[k - i], d); }
    u[k - 9] = (uint32_t)d & FQ29_M29; d >>= 29;
  }
  const uint64_t u8 = d;                           // leftover carry, < 2^36
  fq29 r;
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
#pragma unroll
    for (int i = 0; i <= k; i++) { s = fq_madc(a.n[i], b.n[k - i], s); s = fq_madc(c.n[i], e.n[k - i], s); }
    s = fq_madc(u[k], R0, s);
    if (k) s = fq_madc(u[k - 1], R1, s);
    r.n[k] = (uint32_t)s & FQ29_M29; s >>= 29;
  }
  fq29_mul_tail(r, s, t8, u8, u[7]);
  return r;
}

// squaring: 45 products (off-diagonal terms use the doubled limb), the same two chains
#define FQ29_SQCHAIN(acc, k)                                                                            \
  _Pragma("unroll") for (int i = ((k) > 8 ? (k)-8 : 0); 2 * i < (k); i++) acc = fq_madc(a2[i], a.n[(k)-i], acc); \
  if (((k)&1) == 0) acc = fq_madc(a.n[(k) / 2], a.n[(k) / 2], acc);

BPPP_DI fq29 fq29_sqr(const fq29 &a) {
  const uint32_t R0 = fq_sreg(FQ29_R0), R1 = fq_sreg(FQ29_R1);
  uint32_t a2[9];
#pragma unroll
  for (int i = 0; i < 9; i++) a2[i] = a.n[i] << 1;      // < 2^31 + 2^10 for magnitude <= 2
  uint64_t d = 0;
  FQ29_SQCHAIN(d, 8)
  const uint32_t t8 = (uint32_t)d & FQ29_M29; d >>= 29;
  uint32_t u[8];
#pragma unroll
  for (int k = 9; k <= 16; k++) {
    FQ29_SQCHAIN(d, k)
    u[k - 9] = (uint32_t)d & FQ29_M29; d >>= 29;
  }
  const uint64_t u8 = d;
  fq29 r;
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    FQ29_SQCHAIN(c, k)
    c = fq_madc(u[k], R0, c);
    if (k) c = fq_madc(u[k - 1], R1, c);
    r.n[k] = (uint32_t)c & FQ29_M29; c >>= 29;
  }
  fq29_mul_tail(r, c, t8, u8, u[7]);
  return r;
}

// ---- carry-free linear operations
BPPP_DI fq29 fq29_add(const fq29 &a, const fq29 &b) {
  fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.n[i] = a.n[i] + b.n[i];
  return r;
}
// -a for a of magnitude <= K; result magnitude K + 1
template <int K> BPPP_DI fq29 fq29_neg(const fq29 &a) {
  fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.n[i] = (uint32_t)(K + 1) * fq29_plimb(i) - a.n[i];
  return r;
}
// a - b for b of magnitude <= K; result magnitude mag(a) + K + 1
template <int K> BPPP_DI fq29 fq29_sub(const fq29 &a, const fq29 &b) {
  fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.n[i] = a.n[i] + ((uint32_t)(K + 1) * fq29_plimb(i) - b.n[i]);
  return r;
}
BPPP_DI fq29 fq29_mul_int(const fq29 &a, uint32_t k) {
  fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.n[i] = a.n[i] * k;
  return r;
}

// ---- normalisation
// one folding pass, any magnitude <= 7: limbs 0 .. 7 < 2^29, limb 8 <= 2^24 + 7 (tight), value < 2^256 + 2^236
BPPP_DI fq29 fq29_weak_pass(const fq29 &a) {
  fq29 t = a;
  const uint32_t x = t.n[8] >> 24; t.n[8] &= FQ29_M24;
  t.n[0] += x * 0x3D1u; t.n[1] += x << 3;
#pragma unroll
  for (int i = 0; i < 8; i++) { t.n[i + 1] += t.n[i] >> 29; t.n[i] &= FQ29_M29; }
  return t;
}
// on the output of a weak pass: the value is below 2 p with limbs 0 .. 7 below 2^29, so 0 (mod p) is all zero or exactly the limbs of p
BPPP_DI bool fq29_weak_is_zero(const fq29 &t) {
  uint32_t z0 = 0, z1 = FQ29_M29;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    z0 |= t.n[i];
    z1 &= t.n[i] ^ (fq29_plimb(i) ^ FQ29_M29);
  }
  return (z0 == 0) | (z1 == FQ29_M29);
}
// true iff a = 0 (mod p); any magnitude <= 7
BPPP_DI bool fq29_normalizes_to_zero(const fq29 &a) { return fq29_weak_is_zero(fq29_weak_pass(a)); }

// ---- conversions
// canonical 8 x 32-bit words (the ABI format) -> tight limbs
BPPP_DI fq29 fq29_from_fe(const fe &a) {
  fq29 r;
  r.n[0] = a.v[0] & FQ29_M29;
  r.n[1] = ((a.v[0] >> 29) | (a.v[1] << 3)) & FQ29_M29;
  r.n[2] = ((a.v[1] >> 26) | (a.v[2] << 6)) & FQ29_M29;
  r.n[3] = ((a.v[2] >> 23) | (a.v[3] << 9)) & FQ29_M29;
  r.n[4] = ((a.v[3] >> 20) | (a.v[4] << 12)) & FQ29_M29;
  r.n[5] = ((a.v[4] >> 17) | (a.v[5] << 15)) & FQ29_M29;
  r.n[6] = ((a.v[5] >> 14) | (a.v[6] << 18)) & FQ29_M29;
  r.n[7] = ((a.v[6] >> 11) | (a.v[7] << 21)) & FQ29_M29;
  r.n[8] = a.v[7] >> 8;
  return r;
}
// any magnitude <= 7 -> fq26 limbs of the same residue, each below 2^26 (magnitude 1 of fq26.hip.h): a weak pass, then the same bits cut
// into 10 x 26.  All-zero limbs stay all zero and no other value becomes all zero (the infinity marker of a stored XYZZ point).
BPPP_DI fq fq29_to_fq26(const fq29 &a) {
  const fq29 t = fq29_weak_pass(a);
  fq r;
  r.n[0] = t.n[0] & FQ_M26;
  r.n[1] = ((t.n[0] >> 26) | (t.n[1] << 3)) & FQ_M26;
  r.n[2] = ((t.n[1] >> 23) | (t.n[2] << 6)) & FQ_M26;
  r.n[3] = ((t.n[2] >> 20) | (t.n[3] << 9)) & FQ_M26;
  r.n[4] = ((t.n[3] >> 17) | (t.n[4] << 12)) & FQ_M26;
  r.n[5] = ((t.n[4] >> 14) | (t.n[5] << 15)) & FQ_M26;
  r.n[6] = ((t.n[5] >> 11) | (t.n[6] << 18)) & FQ_M26;
  r.n[7] = ((t.n[6] >> 8) | (t.n[7] << 21)) & FQ_M26;
  r.n[8] = ((t.n[7] >> 5) | (t.n[8] << 24)) & FQ_M26;
  r.n[9] = t.n[8] >> 2;
  return r;
}

// ---- raw limbs in memory (test hooks)
BPPP_DI void fq29_store9(uint32_t *p, const fq29 &a) {
#pragma unroll
  for (int i = 0; i < 9; i++) p[i] = a.n[i];
}
BPPP_DI fq29 fq29_load9(const uint32_t *p) {
  fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.n[i] = p[i];
  return r;
}

}  // namespace bppp
