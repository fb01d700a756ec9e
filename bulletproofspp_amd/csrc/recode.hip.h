// recode.hip.h — the signed-digit format every MSM here reads its scalars in (csrc/msm.hip's bucket route, csrc/comb.hip's fixed-base comb).
//
// A scalar s is folded as reduceScalar does (Commitment.hs:276-279): s > n - s takes n - s and the negated point.  Adding the bias
// K = sum_w 2^(cw-1) 2^(off_w) to the folded value turns every signed window digit into an unsigned cw-bit field f of the 9-limb sum
// sp: the digit is f - 2^(cw-1), and the windows are peeled off from the bottom (recode_next).
//
// The top window may be left unbiased (make_recode_k's top_unbiased).  The folded value is v <= (n - 1) / 2 < 2^255, and the biases below the
// top window, which starts at bit off, sum to less than 2^off: what is left for the top window is d = (v + K) >> off <= 2^(255 - off), never
// negative.  With the bias a top window of cw = 255 - off + 1 bits overflows in the one case d = 2^(cw-1) and needs a further window for
// the carry; without it d itself is the digit, fits the cw bits, and its largest magnitude 2^(cw-1) is that of the digit -2^(cw-1) of any
// other window.  The windows then cover 256 bits or more and v + K < 2^255 + 2^off <= 2^256: after the last recode_next sp is zero, sp[8]
// included.
#pragma once
#include <string.h>
#include "fe.hip.h"

namespace bppp {

struct RecodeK { uint32_t k[9]; };

// K = sum_{w<W} 2^(cw-1) 2^(off_w) as 9 x 32-bit limbs: the first `acnt` windows are c bits wide, the others c - 1 (balanced widths; acnt < 0: all c);
// top_unbiased: the sum stops before window W - 1, whose field is then the (non-negative) digit itself
inline RecodeK make_recode_k(int c, int W, int acnt = -1, bool top_unbiased = false) {
  RecodeK K; memset(&K, 0, sizeof K);
  if (acnt < 0) acnt = W;
  int off = 0;
  for (int w = 0; w < W - (top_unbiased ? 1 : 0); w++) {
    const int cw = w < acnt ? c : c - 1, bit = off + cw - 1;
    if (bit < 288) K.k[bit >> 5] |= 1u << (bit & 31);
    off += cw;
  }
  return K;
}

// sp = v + K for the folded scalar v (s or n - s, also returned); true: v = n - s, the point is negated
BPPP_DI bool recode_fold(const fe &s, const RecodeK &K, uint32_t (&sp)[9], fe &v) {
  fe t, tmp;
  raw_sub(t, fr_modulus(), s);                                  // n - s
  const bool neg = raw_sub(tmp, t, s) != 0;                     // t < s  <=>  s > n - s   (reduceScalar, Commitment.hs:279)
  uint64_t cy = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) { v.v[q] = neg ? t.v[q] : s.v[q]; cy += (uint64_t)v.v[q] + K.k[q]; sp[q] = (uint32_t)cy; cy >>= 32; }
  sp[8] = (uint32_t)cy + K.k[8];
  return neg;
}
BPPP_DI bool recode_fold(const fe &s, const RecodeK &K, uint32_t (&sp)[9]) { fe v; return recode_fold(s, K, sp, v); }

// the next window: the low cw bits of sp (the digit plus 2^(cw-1)); sp moves on by cw bits
BPPP_DI uint32_t recode_next(uint32_t (&sp)[9], int cw) {
  const uint32_t f = sp[0] & ((1u << cw) - 1u);
#pragma unroll
  for (int q = 0; q < 8; q++) sp[q] = (sp[q] >> cw) | (sp[q + 1] << (32 - cw));
  sp[8] >>= cw;
  return f;
}

}  // namespace bppp
