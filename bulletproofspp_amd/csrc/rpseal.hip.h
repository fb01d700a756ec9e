// rpseal.hip.h — a P for ONE scalar a and a point P of its own per lane: the walk of a view-key scan (csrc/rpseal.hip), where every output on
// the chain is multiplied by the same view secret.  In a header because the test library (csrc/testhooks.hip) runs the walk alone.
//
// The scalar is the same for the whole grid, so it is recoded once on the host (scan_recode) and travels as a kernel argument: every digit
// test below is a scalar branch, uniform across every wavefront, and a lane needs no other lane — one lane per point, no cross-lane traffic,
// where the quad walk (csrc/rpexcess.hip.h) spends four lanes and a vector branch per bit on a scalar of its own per instance.
//
// Form: the GLV joint walk.  a mod n = a1 + a2 lambda with |a1|, |a2| < 2^129 (decompose_eis, csrc/hosteis.hpp — the split csrc/glv.hip makes
// on the device) and lambda (x, y) = (beta x, y), so  a P = |a1| T1 + |a2| T2  with T1 = sign (a1) P and T2 = sign (a2) (beta x, y): both affine,
// one field product and two negations.  The two magnitudes are walked MSB-first side by side, one doubling per bit of the longer one and one
// addition of T1, T2 or T3 = T1 + T2 per bit pair that is not (0, 0): about 128 doublings and 96 additions (64 of them mixed) against the
// binary walk's 256 and 128.  T3 stays in XYZZ: making it affine costs an inversion a lane, more than the 4 products a general addition adds
// to each of its ~32 uses.
//
// Every operation is the complete XYZZ law of csrc/ec.hip.h: P at infinity, a = 0 (no bit set: the accumulator stays at infinity) and an
// accumulator that meets a table point or its negative are ordinary input.  For a point of prime order the last two cannot happen — the
// accumulator and the table point differ by a pair of halves too short to be a non-zero vector of the GLV lattice
// (tests/test_seal_scan_host.py states the argument, replays the walk on discrete logs and counts the classes) — but nothing here rests on that.
#pragma once
#include "ec.hip.h"
#include "hosteis.hpp"

namespace bppp {

// the recoded scalar: digit i (two bits: bit i of |a1|, then bit i of |a2|) is bits 2 (i & 15) .. of d[i >> 4]; nbits digits, walked from
// nbits - 1 down; neg: bit 0 a1 < 0, bit 1 a2 < 0.  144 digits hold every split (the halves stay below 2^129).
static constexpr uint32_t SCAN_DIGIT_WORDS = 9;
struct ScanWalk { uint32_t d[SCAN_DIGIT_WORDS]; uint32_t nbits, neg; };

// a (any 256-bit integer, reduced mod n here) -> its walk; false if a half does not fit (it cannot: see above)
inline bool scan_recode(const uint64_t scalar[4], ScanWalk &W) {
  using namespace bppp_host;
  U256 x = U256::load(scalar), t;
  if (!sub_raw(t, x, FR().m)) x = t;                     // a < 2^256 < 2 n: one subtraction reduces
  const bppp_eis::Eis e = bppp_eis::decompose_eis(x);
  memset(&W, 0, sizeof W);
  const int bits = std::max(e.a.bits(), e.b.bits());
  if (bits > (int)(16 * SCAN_DIGIT_WORDS)) return false;
  W.nbits = (uint32_t)bits;
  W.neg = (e.a.neg ? 1u : 0u) | (e.b.neg ? 2u : 0u);
  for (int i = 0; i < bits; i++) {
    const uint32_t dg = (uint32_t)((e.a.m[i >> 6] >> (i & 63)) & 1) | ((uint32_t)((e.b.m[i >> 6] >> (i & 63)) & 1) << 1);
    W.d[i >> 4] |= dg << (2 * (i & 15));
  }
  return true;
}

// beta, the cube root of unity in Fq that goes with lambda (csrc/glv.hip holds the same words)
BPPP_DI fq scan_beta() {
  const fe b = {{0x719501EEu, 0xC1396C28u, 0x12F58995u, 0x9CF04975u, 0xAC3434E9u, 0x6E64479Eu, 0x657C0710u, 0x7AE96A2Bu}};
  return fq_from_fe(b);
}

// The lane's table lives in LDS, not in registers: T1 and T2 as affine fq limbs and T3 as XYZZ, 80 words a lane, word-major so that the 64
// lanes of a wavefront read 64 consecutive words (no bank conflict) and every lane reads only the column it wrote (no barrier).  Only the
// accumulator stays live across the loop; an operand is read where its addition is.  A workgroup is ONE wavefront: tab is [SCAN_TAB_WORDS][64].
static constexpr uint32_t SCAN_TAB_WORDS = 80, SCAN_T1 = 0, SCAN_T2 = 20, SCAN_T3 = 40;
typedef uint32_t ScanTab[64];
BPPP_DI void scan_tab_put(ScanTab *tab, uint32_t lane, uint32_t o, const fq &a) {
#pragma unroll
  for (int i = 0; i < 10; i++) tab[o + i][lane] = a.n[i];
}
BPPP_DI fq scan_tab_get(const ScanTab *tab, uint32_t lane, uint32_t o) {
  fq r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.n[i] = tab[o + i][lane];
  return r;
}
BPPP_DI aff scan_tab_aff(const ScanTab *tab, uint32_t lane, uint32_t o) { aff r; r.x = scan_tab_get(tab, lane, o); r.y = scan_tab_get(tab, lane, o + 10); return r; }

// W.a P, one lane (lane: its column of tab, threadIdx.x of a 64-thread workgroup).  W is uniform (a kernel argument): the loop bound and
// every digit are scalar values.
BPPP_DI xyzz scan_mul_lane(const ScanWalk &W, const aff &P, ScanTab *tab, uint32_t lane) {
  {
    aff T1 = aff_cneg(P, (W.neg & 1u) != 0), T2 = P;
    T1.y = fq_normalize(T1.y);
    if (!aff_is_inf(P)) T2.x = fq_normalize(fq_mul(P.x, scan_beta()));
    T2 = aff_cneg(T2, (W.neg & 2u) != 0);
    T2.y = fq_normalize(T2.y);
    xyzz T3 = xyzz_from_aff(T1);
    xyzz_madd(T3, T2);
    scan_tab_put(tab, lane, SCAN_T1, T1.x); scan_tab_put(tab, lane, SCAN_T1 + 10, T1.y);
    scan_tab_put(tab, lane, SCAN_T2, T2.x); scan_tab_put(tab, lane, SCAN_T2 + 10, T2.y);
    scan_tab_put(tab, lane, SCAN_T3, T3.X); scan_tab_put(tab, lane, SCAN_T3 + 10, T3.Y);
    scan_tab_put(tab, lane, SCAN_T3 + 20, T3.ZZ); scan_tab_put(tab, lane, SCAN_T3 + 30, T3.ZZZ);
  }
  xyzz acc = xyzz_inf();
#pragma unroll 1
  for (int i = (int)W.nbits - 1; i >= 0; i--) {
    acc = xyzz_dbl(acc);
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_DIGIT_WORDS; k++) if ((uint32_t)(i >> 4) == k) word = W.d[k];
    const uint32_t dg = (word >> (2 * (i & 15))) & 3u;
    if (dg == 3u) {
      xyzz T3;
      T3.X = scan_tab_get(tab, lane, SCAN_T3); T3.Y = scan_tab_get(tab, lane, SCAN_T3 + 10);
      T3.ZZ = scan_tab_get(tab, lane, SCAN_T3 + 20); T3.ZZZ = scan_tab_get(tab, lane, SCAN_T3 + 30);
      xyzz_add(acc, T3);
    } else if (dg) {
      xyzz_madd(acc, scan_tab_aff(tab, lane, dg == 1u ? SCAN_T1 : SCAN_T2));
    }
  }
  return acc;
}

// XYZZ -> affine in a launch of its own, so that the walk's registers are the walk's alone (infinity: all zeros)
BPPP_DI void scan_affine_lane(const uint32_t *acc, uint32_t *out) { aff_store(out, xyzz_to_aff(xyzz_load(acc))); }

}  // namespace bppp
