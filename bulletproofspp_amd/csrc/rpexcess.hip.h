// rpexcess.hip.h — c X for a point X of its own per instance, one quad (four lanes) per instance: the walk of k_rp_excess_mulcheck
// (csrc/rpexcess.hip).  In a header because the test library (csrc/testhooks.hip) runs the walk alone, on scalars a test chooses.
//
// MSB-first binary double-and-add over all 256 bits of c on XYZZ, from the affine X: 256 xyzz_dbl_quad and one xyzz_add_quad per set bit
// (csrc/ec_quad.hip.h).  Both are the complete law, so c = 0, X = infinity and an accumulator that meets X or -X on the way are ordinary
// input; c is walked as the 256-bit integer it is, reduced or not.  Under that header's rules: the caller brings whole quads, every lane of
// a quad holds the same c and X, and the only branch is on a bit of c — uniform within the quad.  Every lane returns the whole result.
#pragma once
#include "ec_quad.hip.h"

namespace bppp {

BPPP_DI xyzz excess_mul_quad(const fe &c, const aff &X) {
  const xyzz Xp = xyzz_from_aff(X);
  xyzz acc = xyzz_inf();
#pragma unroll 1
  for (int i = 255; i >= 0; i--) {
    xyzz_dbl_quad(acc);
    uint32_t limb = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) if ((i >> 5) == k) limb = c.v[k];
    if ((limb >> (i & 31)) & 1u) xyzz_add_quad(acc, Xp);
  }
  return acc;
}

}  // namespace bppp
