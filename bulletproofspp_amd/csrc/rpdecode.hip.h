// rpdecode.hip.h — the verifier's first stage: the untrusted bytes of the commitments and proof files -> points and scalars
// (decodeProof' / decodeCommitments, src/RangeProof.hs:68-85, src/Encoding.hs:92-128).
//   k_rp_decode_points   one lane per encoded point: Binary (Prime p) x, toP, pointX, fromXWithSign
//   k_rp_decode_scalars  the final witness scalars of the proof file, toP
//   rp_decode_launch     both, queued on a stream: what rp_verify_prepare (csrc/rp.hip) runs per upload slice
// The kernels and their launcher live in a header because the test library (csrc/testhooks.hip) runs this stage alone.
#pragma once
#include "ec.hip.h"
#include "rp_internal.hpp"
#include "rplift.hip.h"

namespace bppp {

// Point t of a proof IN TRANSCRIPT ORDER (newest first, the order shaOracle's final call sees, src/ZKP.hs:98):
//   t < 2k            the argument's responses, last round first  = bpComs of the proof file (RangeProof.hs:60-66)
//   2k <= t < 2k + 4  blCom, rCom, dmCom, mCom  (Binary: blCom, dCom) = rpComs of the proof file
//   else              the input commitments                         = the commitments file
// Output: responses to resp[b][t], the rest to init[b][...] in the order blCom : rCom : dmCom : mCom : nComs.
__global__ void __launch_bounds__(64) k_rp_decode_points(RpDims D, uint32_t batch, const uint8_t *__restrict__ coms, const uint8_t *__restrict__ proofs,
                                                         uint32_t *__restrict__ init_pts, uint32_t *__restrict__ resp_pts, uint32_t *__restrict__ bad,
                                                         uint32_t *__restrict__ any_bad) {   // bad[b] per proof of this launch, *any_bad for the call
  const uint32_t npts = rp_npts(D);
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (uint64_t)batch * npts) return;
  const uint32_t b = (uint32_t)(g / npts), t = (uint32_t)(g % npts);
  const uint8_t *signs, *xs;
  uint32_t idx;
  const uint32_t nproof_pts = D.nrp + 2 * D.k;
  if (t < 2 * D.k + D.nrp) {
    const uint8_t *pf = proofs + (size_t)b * D.proof_bytes + (size_t)(D.fn + D.fl) * 32;
    signs = pf; xs = pf + (nproof_pts + 7) / 8;
    idx = t < 2 * D.k ? D.nrp + t : t - 2 * D.k;
  } else {
    const uint8_t *cf = coms + (size_t)b * D.coms_bytes;
    signs = cf; xs = cf + (D.nr + 7) / 8;
    idx = t - 2 * D.k - D.nrp;
  }
  const bool want_big = (signs[idx >> 3] >> (idx & 7)) & 1;
  bool ok;
  aff r = rp_lift_x(load_field_be<0>(xs + (size_t)idx * 32), want_big, ok);
  if (!ok) { r = aff_inf(); atomicOr(bad + b, 1u); atomicOr(any_bad, 1u); }
  uint32_t *out = t < 2 * D.k ? resp_pts + ((size_t)b * 2 * D.k + t) * 16
                              : init_pts + ((size_t)b * (D.nrp + D.nr) + (t - 2 * D.k)) * 16;
  aff_store(out, r);
}

// final witness scalars: norm part then linear part (encodeProof', RangeProof.hs:60-66)
__global__ void __launch_bounds__(64) k_rp_decode_scalars(RpDims D, uint32_t batch, const uint8_t *__restrict__ proofs, uint32_t *__restrict__ wit_norm,
                                                          uint32_t *__restrict__ wit_lin) {
  const uint32_t ns = D.fn + D.fl;
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (uint64_t)batch * ns) return;
  const uint32_t b = (uint32_t)(g / ns), i = (uint32_t)(g % ns);
  const fe v = load_field_be<1>(proofs + (size_t)b * D.proof_bytes + (size_t)i * 32);
  if (i < D.fn) fe_store(wit_norm + ((size_t)b * D.fn + i) * 8, v);
  else fe_store(wit_lin + ((size_t)b * D.fl + (i - D.fn)) * 8, v);
}

// decodeProof' of `nb` proofs whose files are in HBM at dc / dp: the two kernels queued on `stream`.  init_pts [nb][nrp + nr][16],
// resp_pts [nb][2k][16], wit_norm [nb][fn][8], wit_lin [nb][fl][8]; bad [nb] and any_bad[0] are OR-ed into (the caller zeroes them).
// A launch error stays in the runtime's last-error slot for the caller's next check.
inline void rp_decode_launch(const RpDims &D, size_t nb, const uint8_t *dc, const uint8_t *dp, uint32_t *init_pts, uint32_t *resp_pts, uint32_t *wit_norm,
                             uint32_t *wit_lin, uint32_t *bad, uint32_t *any_bad, hipStream_t stream) {
  const uint64_t np = (uint64_t)nb * rp_npts(D), ns = (uint64_t)nb * (D.fn + D.fl);
  k_rp_decode_points<<<dim3((unsigned)((np + 63) / 64)), dim3(64), 0, stream>>>(D, (uint32_t)nb, dc, dp, init_pts, resp_pts, bad, any_bad);
  if (ns) k_rp_decode_scalars<<<dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, stream>>>(D, (uint32_t)nb, dp, wit_norm, wit_lin);
}

}  // namespace bppp
