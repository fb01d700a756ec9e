// ec_quad.hip.h — one XYZZ point operation shared by the four lanes of a quad (lanes 4k .. 4k+3).
//
// A dependent chain of point additions runs at one wavefront's instruction rate whatever the lane count, so where chain depth and
// not issue rate sets the time (the tails of the bucket reduction: a few hundred wavefronts on 1024 SIMDs) the 12M + 2S of an
// add-2008-s can be spread over a quad: the multiplications fall into four stages of at most four independent products, every lane
// computes one product per stage (the SAME fq_mul call on operands picked by lane & 3, so the wavefront runs one instruction stream),
// and quad_perm DPP moves (10 per value, no LDS) broadcast what the next stage needs.  Every lane of the quad ends with the whole
// result, limb for limb equal to xyzz_add / xyzz_dbl (ec.hip.h): the squares are fq_mul(x, x), whose column sums are the same
// integers as fq_sqr's, and every other product keeps the scalar routine's operand order and fq_sub bounds.
//
// The multiplier is a template argument: fq_mul by default, fq_mul_lone (fq26.hip.h: no stall slots when nothing else runs on the SIMD) for
// k_reduce_tail_quad, whose wavefronts have a SIMD each.  A lane has ONE product per stage, so the pair forms have nothing to pair here.
//
// Rules for callers:
//  - all four lanes of a quad are active at every call (DPP reads across the quad): a quad with nothing to add adds infinity; never
//    branch around a call on anything that is not uniform within the quad;
//  - the lane's position in its quad is threadIdx.x & 3, so the workgroup's lanes are laid out in whole quads (blockDim.x % 4 == 0);
//  - the complete-law branch (same x: doubling or infinity) is uniform within a quad, since every lane sees the same Pd and R; it may
//    diverge between the quads of a wavefront, which DPP within a quad does not mind.
#pragma once
#include "ec.hip.h"

namespace bppp {

BPPP_DI uint32_t quad_lane() { return threadIdx.x & 3u; }
// value of lane K of this lane's quad (quad_perm [K, K, K, K]).  Each moved limb is pinned in a VGPR (the empty asm): left free, the
// compiler folds the move into its consumer as a DPP operand, and a subtraction of two broadcasts of one register (Y3 = bcast<0>(m)
// - bcast<1>(m)) came out as the same lane twice.
template <int K> BPPP_DI fq fq_quad_bcast(const fq &a) {
  fq r;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    r.n[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a.n[i], K * 0x55, 0xF, 0xF, false);
    asm("" : "+v"(r.n[i]));
  }
  return r;
}
// a_s for s = lane & 3 (three selects per limb)
BPPP_DI fq fq_sel4(uint32_t s, const fq &a0, const fq &a1, const fq &a2, const fq &a3) {
  fq r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.n[i] = (s & 2u) ? ((s & 1u) ? a3.n[i] : a2.n[i]) : ((s & 1u) ? a1.n[i] : a0.n[i]);
  return r;
}
BPPP_DI xyzz xyzz_sel(bool c, const xyzz &a, const xyzz &b) {     // c ? a : b, limb by limb (no branch)
  xyzz r;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    r.X.n[i] = c ? a.X.n[i] : b.X.n[i]; r.Y.n[i] = c ? a.Y.n[i] : b.Y.n[i];
    r.ZZ.n[i] = c ? a.ZZ.n[i] : b.ZZ.n[i]; r.ZZZ.n[i] = c ? a.ZZZ.n[i] : b.ZZZ.n[i];
  }
  return r;
}
BPPP_DI xyzz xyzz_or_inf(bool keep, const xyzz &p) { return xyzz_sel(keep, p, xyzz_inf()); }

// LONE: the multiplier is fq_mul_lone (fq26.hip.h) — for kernels whose wavefronts have a SIMD to themselves; same limbs either way
template <bool LONE> BPPP_DI fq fq_mul_q(const fq &a, const fq &b) { return LONE ? fq_mul_lone(a, b) : fq_mul(a, b); }

// dbl-2008-s-1 (a = 0) on a quad, three stages:  V = U^2, XX = X^2  |  W = U V, S = X V, ZZ3 = V ZZ, M^2  |  M (S - X3), W Y, ZZZ3 = W ZZZ
template <bool LONE = false> BPPP_DI void xyzz_dbl_quad(xyzz &p) {
  const uint32_t s = quad_lane();
  const bool inf = xyzz_is_inf(p) || fq_normalizes_to_zero(p.Y);
  const fq U = fq_mul_int(p.Y, 2);                                 // <= 6
  const fq a1 = fq_sel4(s, U, p.X, U, p.X);
  const fq m1 = fq_mul_q<LONE>(a1, a1);
  const fq V = fq_quad_bcast<0>(m1), M = fq_mul_int(fq_quad_bcast<1>(m1), 3);
  const fq m2 = fq_mul_q<LONE>(fq_sel4(s, U, p.X, V, M), fq_sel4(s, V, V, p.ZZ, M));
  const fq W = fq_quad_bcast<0>(m2), S = fq_quad_bcast<1>(m2), ZZ3 = fq_quad_bcast<2>(m2);
  const fq X3 = fq_sub<2>(fq_quad_bcast<3>(m2), fq_mul_int(S, 2));                  // 4
  const fq m3 = fq_mul_q<LONE>(fq_sel4(s, M, W, W, W), fq_sel4(s, fq_sub<4>(S, X3), p.Y, p.ZZZ, p.ZZZ));
  xyzz r;
  r.X = X3;
  r.Y = fq_sub<1>(fq_quad_bcast<0>(m3), fq_quad_bcast<1>(m3));                       // 3
  r.ZZ = ZZ3; r.ZZZ = fq_quad_bcast<2>(m3);
  p = xyzz_sel(inf, xyzz_inf(), r);
}

// acc += q (both XYZZ) on a quad: add-2008-s, complete.  Stages (lane 0 / 1 / 2 / 3):
//   1. U1 = X1 ZZ2, U2 = X2 ZZ1, S1 = Y1 ZZZ2, S2 = Y2 ZZZ1          -> Pd = U2 - U1, R = S2 - S1, complete-law test
//   2. PP = Pd^2, RR = R^2, Z12 = ZZ1 ZZ2, Z123 = ZZZ1 ZZZ2          (Z12 and Z123 stay in lanes 2 and 3)
//   3. PPP = Pd PP, Q = U1 PP, ZZ3 = Z12 PP, -                       -> X3
//   4. R (Q - X3), S1 PPP, -, ZZZ3 = Z123 PPP                        -> Y3
template <bool LONE = false> BPPP_DI void xyzz_add_quad(xyzz &acc, const xyzz &q) {
  const uint32_t s = quad_lane();
  const bool ia = xyzz_is_inf(acc), iq = xyzz_is_inf(q);
  const fq m1 = fq_mul_q<LONE>(fq_sel4(s, acc.X, q.X, acc.Y, q.Y), fq_sel4(s, q.ZZ, acc.ZZ, q.ZZZ, acc.ZZZ));
  const fq U1 = fq_quad_bcast<0>(m1), S1 = fq_quad_bcast<2>(m1);
  const fq Pd = fq_sub<1>(fq_quad_bcast<1>(m1), U1), R = fq_sub<1>(fq_quad_bcast<3>(m1), S1);     // 3, 3
  if (!ia && !iq && fq_normalizes_to_zero(Pd)) {                  // same x: uniform within the quad
    if (fq_normalizes_to_zero(R)) xyzz_dbl_quad<LONE>(acc); else acc = xyzz_inf();
    return;
  }
  const fq m2 = fq_mul_q<LONE>(fq_sel4(s, Pd, R, acc.ZZ, acc.ZZZ), fq_sel4(s, Pd, R, q.ZZ, q.ZZZ));
  const fq PP = fq_quad_bcast<0>(m2), RR = fq_quad_bcast<1>(m2);
  const fq m3 = fq_mul_q<LONE>(fq_sel4(s, Pd, U1, m2, m2), PP);
  const fq PPP = fq_quad_bcast<0>(m3), Q = fq_quad_bcast<1>(m3);
  xyzz r;
  r.ZZ = fq_quad_bcast<2>(m3);
  r.X = fq_sub<3>(RR, fq_add(PPP, fq_mul_int(Q, 2)));                                 // 5
  const fq m4 = fq_mul_q<LONE>(fq_sel4(s, R, S1, m2, m2), s == 0 ? fq_sub<5>(Q, r.X) : PPP);
  r.Y = fq_sub<1>(fq_quad_bcast<0>(m4), fq_quad_bcast<1>(m4));                       // 3
  r.ZZZ = fq_quad_bcast<3>(m4);
  acc = xyzz_sel(iq, acc, xyzz_sel(ia, q, r));
}

}  // namespace bppp
