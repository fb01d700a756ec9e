// rplift.hip.h — one encoded field element and one encoded point of the reference's files on the device: Binary (Prime p) get and
// fromXWithSign (src/Encoding.hs:76-80, :97-103).  The verifier's decoders (csrc/rpdecode.hip.h) and the excess signatures
// (csrc/rpexcess.hip) lift their points here.  No kernels.
#pragma once
#include "ec.hip.h"

namespace bppp {

// Binary (Prime p) get (Encoding.hs:76-80): limb i = big-endian 64-bit word at bytes 8i..8i+7, least-significant limb first;
// toP reduces (one conditional subtraction: the value is < 2^256 < 2m)
template <int MOD> BPPP_DI fe load_field_be(const uint8_t *p) {
  fe v;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint8_t *q = p + 8 * i;
    v.v[2 * i + 1] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    v.v[2 * i] = ((uint32_t)q[4] << 24) | ((uint32_t)q[5] << 16) | ((uint32_t)q[6] << 8) | q[7];
  }
  fe t;
  uint32_t br = raw_sub(t, v, modulus<MOD>());
#pragma unroll
  for (int i = 0; i < 8; i++) v.v[i] = br ? v.v[i] : t.v[i];
  return v;
}

// the same 32 bytes as the 256-bit integer they hold, not reduced
BPPP_DI fe load_field_be_raw(const uint8_t *p) {
  fe v;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint8_t *q = p + 8 * i;
    v.v[2 * i + 1] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    v.v[2 * i] = ((uint32_t)q[4] << 24) | ((uint32_t)q[5] << 16) | ((uint32_t)q[6] << 8) | q[7];
  }
  return v;
}

// pointX and fromXWithSign (Encoding.hs:97-103) of a reduced x: the root of x^3 + 7 whose (y > p - y) equals the sign bit; ok = false
// (and an unspecified point) when the x has no curve point.  Shared with the excess signatures' R (csrc/rpexcess.hip).
BPPP_DI aff rp_lift_x(const fe &xe, bool want_big, bool &ok) {
  const fq x = fq_from_fe(xe);
  fq seven = fq_zero(); seven.n[0] = 7;
  const fq rhs = fq_add(fq_mul(fq_sqr(x), x), seven);         // magnitude 2
  fq y = fq_sqrt_candidate(rhs);
  ok = fq_normalizes_to_zero(fq_sub<2>(fq_sqr(y), rhs));
  y = fq_normalize(y);
  const fe ye = fq_to_fe(y), yn = fe_neg<0>(ye);
  fe d;
  const bool y_big = raw_sub(d, yn, ye) != 0;                  // -y < y
  aff r; r.x = x; r.y = (y_big != want_big) ? fq_from_fe(yn) : y;
  return r;
}

}  // namespace bppp
