// rpexpart.hip.h — b P + c Q for two points of their own per instance, one quad (four lanes) per instance: the joint walk of
// k_rp_expart_mulcheck (csrc/rpexpart.hip).  In a header because the test library (csrc/testhooks.hip) runs the walk alone, on scalars and
// points a test chooses.
//
// Shamir's trick on XYZZ: the table holds P, Q and P + Q — P and Q as the affine points they came as (ZZ = ZZZ = 1 is not kept: 40 limbs fewer
// alive through the loop), P + Q in XYZZ; MSB first over the 256 positions of both scalars, one xyzz_dbl_quad and then one xyzz_add_quad of the
// entry the two bits choose (csrc/ec_quad.hip.h) — 256 doublings and about 192 additions for random scalars, where two walks of
// csrc/rpexcess.hip.h and their sum are 512 doublings and about 257 additions.  The entry is picked limb by limb, without a branch; the only
// branch is "either bit set", and both scalars are the same in the four lanes of a quad, so it is uniform within the quad.  Both laws are
// complete: P = Q (P + Q is a doubling), P = -Q (P + Q is infinity), P or Q infinity, zero scalars and an accumulator that meets an entry or
// its negative on the way are ordinary input; b and c are walked as the 256-bit integers they are, reduced or not.  Under that header's
// rules: the caller brings whole quads, every lane of a quad holds the same b, P, c and Q.  Every lane returns the whole result.
#pragma once
#include "ec_quad.hip.h"

namespace bppp {

BPPP_DI xyzz excess_mul2_quad(const fe &b, const aff &P, const fe &c, const aff &Q) {
  xyzz PQ = xyzz_from_aff(P);
  xyzz_add_quad(PQ, xyzz_from_aff(Q));
  xyzz acc = xyzz_inf();
#pragma unroll 1
  for (int i = 255; i >= 0; i--) {
    xyzz_dbl_quad(acc);
    uint32_t lb = 0, lc = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) if ((i >> 5) == k) { lb = b.v[k]; lc = c.v[k]; }
    const bool bb = (lb >> (i & 31)) & 1u, bc = (lc >> (i & 31)) & 1u;
    if (bb || bc) {
      aff one;                                           // P or Q, whichever the single set bit names
#pragma unroll
      for (int k = 0; k < 10; k++) { one.x.n[k] = bb ? P.x.n[k] : Q.x.n[k]; one.y.n[k] = bb ? P.y.n[k] : Q.y.n[k]; }
      xyzz_add_quad(acc, xyzz_sel(bb && bc, PQ, xyzz_from_aff(one)));
    }
  }
  return acc;
}

}  // namespace bppp
