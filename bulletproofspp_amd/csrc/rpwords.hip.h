// rpwords.hip.h — device helpers on the 8-word images of plain integers, scalars and points that the witness kernels
// (csrc/rpwitness.hip.h) and the commit / open kernels (csrc/rpcommit.hip) share: two's-complement comparison and reduction of an
// amount, the canonical test of a claimed scalar, and the byte and sign-bit rules of the reference's files.  No kernels here.
#pragma once
#include "fe.hip.h"

namespace bppp {

// ---- 256-bit integers in two's complement (csrc/rpsetup.hpp: s_neg, s_lt, s_mod_n)
BPPP_DI bool wi_neg(const fe &a) { return (a.v[7] >> 31) != 0; }
BPPP_DI bool wi_ult(const fe &a, const fe &b) { fe t; return raw_sub(t, a, b) != 0; }
BPPP_DI bool wi_slt(const fe &a, const fe &b) { return wi_neg(a) != wi_neg(b) ? wi_neg(a) : wi_ult(a, b); }
BPPP_DI fe wi_umod_n(const fe &a) { fe t; return raw_sub(t, a, fr_modulus()) ? a : t; }
BPPP_DI fe wi_smod_n(const fe &a) {
  if (!wi_neg(a)) return wi_umod_n(a);
  fe m;
  raw_sub(m, fe_zero(), a);
  return fe_neg<1>(wi_umod_n(m));
}
BPPP_DI bool wi_canonical(const fe &a) { return wi_ult(a, fr_modulus()); }
// Binary (Prime p) put (Encoding.hs:81-86) as put_field (csrc/rpprove_host.hpp) writes it: the four 64-bit limbs least significant first,
// each big-endian; byte o (< 32) from 8 little-endian 32-bit words
BPPP_DI uint8_t enc_be_byte(const uint32_t *w, uint32_t o) {
  const uint32_t j = 8 * (o >> 3) + 7 - (o & 7);       // index of the byte in the little-endian image
  return (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
}
// the sign bit of encodeCommitments (Encoding.hs:130-134): y > p - y
BPPP_DI uint32_t enc_sign(const uint32_t *pt) {
  const fe y = fe_load(pt + 8);
  if (fe_is_zero(y)) return 0;
  fe ny;
  raw_sub(ny, fp_modulus(), y);
  return wi_ult(ny, y) ? 1u : 0u;
}

}  // namespace bppp
