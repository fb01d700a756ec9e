// rpeach.hip — every range proof of a batch decided on its own (bppp_rp_verify_each{,_device}), and the bounded-cost culprit search
// behind BPPP_RP_OPT_CULPRITS = 1.
//
// Proof b is valid iff E_b = MSM(T_b) is the identity, T_b being exactly the term list verifyWith builds for that proof alone
// (src/Bulletproof.hs:362-368, :375-377; verifyM of one proof).  No random weights: the verdict is exact.  T_b splits in two:
//   row[b]  the scalars on the handle's basis [g | H | G] (1 + llen + nlen terms)   -> fixed-base MSM, one instance per proof:
//           comb_msm over rp->comb when the handle has its comb table, else the windowed table of rp->commit_basis
//   tail[b] the scalars on the proof's own points [init commitments | responses] (ninit + 2k terms) -> msm_batch_dev, distinct points
// and k_each_finish adds the two parts and writes the status word and E_b.  Only those cross to the host.
//
// Pipeline per call: rp_verify_prepare (decode, hashing, public scalars; its rho is not used), then for every chunk of proofs
// each_rows_assemble (csrc/nlbatch.hip: factors, g scalar and tail with rho = 1, the H / G columns), the two MSMs and k_each_finish.
// Chunks bound the memory: rows of at most EACH_ROWS_BYTES (a binary 64 x 64 handle has 4099-term rows, 131 KB per proof).
#include <string.h>
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "ec.hip.h"
#include "comb.hpp"
#include "rp_internal.hpp"

namespace bppp {

// rows of one chunk at most this many bytes, in whole 64s of proofs (64by64: 774-term rows, 5376 proofs; binary 64 x 64: 4099-term rows, 960)
static constexpr size_t EACH_ROWS_BYTES = (size_t)128 << 20;
static constexpr size_t EACH_MIN_INST = 8;       // the MSMs' instances per launch at least (zero rows pad a smaller last chunk)

static size_t each_chunk(const bppp_rp *rp) {
  if (rp->each_chunk) return rp->each_chunk;
  const size_t T = 1 + rp->st.llen + rp->st.nlen;
  const size_t c = EACH_ROWS_BYTES / (T * 32);
  return std::max<size_t>(64, c / 64 * 64);
}

__global__ void __launch_bounds__(64) k_each_ones(uint32_t n, uint32_t *__restrict__ ones) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe o = fe_zero(); o.v[0] = 1;
  fe_store(ones + (size_t)i * 8, o);
}

// E_b = fixed[b] + own[b]; status[b] = MALFORMED (a point did not decode; E_b written as zeros), VALID (E_b is infinity) or INVALID
__global__ void __launch_bounds__(64) k_each_finish(uint32_t n, const uint32_t *__restrict__ fixed, const uint32_t *__restrict__ own,
                                                    const uint32_t *__restrict__ bad, uint32_t *__restrict__ status, uint32_t *__restrict__ xy) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  xyzz acc = xyzz_from_aff(aff_load(fixed + (size_t)b * 16));
  xyzz_madd(acc, aff_load(own + (size_t)b * 16));
  aff e = xyzz_to_aff(acc);
  const bool malformed = bad[b] != 0;
  if (malformed) e = aff_inf();
  status[b] = malformed ? BPPP_RP_MALFORMED : aff_is_inf(e) ? BPPP_RP_VALID : BPPP_RP_INVALID;
  aff_store(xy + (size_t)b * 16, e);
}

int rp_each_pass(bppp_rp *rp, const RpVerifyArrays &A, uint32_t *proof_status, uint64_t *proof_xy) {
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  const bppp_rps::Setup &S = rp->st;
  const RpDims &D = rp->D;
  const size_t B = A.batch, nlen = S.nlen, llen = S.llen, k = S.rounds, ninit = D.nrp + D.nr, per = ninit + 2 * k, T = 1 + llen + nlen;
  const size_t C = std::min(each_chunk(rp), B), Cp = std::max(C, EACH_MIN_INST);
  if (!rp->comb && !rp->commit_basis) { int rc = bppp_basis_create_device(ctx, rp->d_basis, T, 0, 4096, &rp->commit_basis); if (rc) return rc; }
  const size_t cbytes = rp->comb ? comb_rows_scratch_bytes(Cp) : 0;
  // workspace: ones | row scratch | rows | tail | points | fixed part | own part | comb scratch | status [B] | E [B]
  uint32_t *ones = nullptr, *scratch = nullptr, *rows = nullptr, *tail = nullptr, *pts = nullptr, *fixed = nullptr, *own = nullptr, *cscratch = nullptr,
           *status = nullptr, *xy = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->ework : nullptr, rp->ework_bytes);
    ones = cv.take<uint32_t>(Cp * 8); scratch = (uint32_t *)cv.take<uint8_t>(each_rows_scratch(S.flavour, Cp, llen, k, D.fn));
    rows = cv.take<uint32_t>(Cp * T * 8); tail = cv.take<uint32_t>(Cp * per * 8); pts = cv.take<uint32_t>(Cp * per * 16);
    fixed = cv.take<uint32_t>(Cp * 16); own = cv.take<uint32_t>(Cp * 16); cscratch = (uint32_t *)cv.take<uint8_t>(cbytes + 16);
    status = cv.take<uint32_t>(B); xy = cv.take<uint32_t>(B * 16);
    if (!pass && cv.off > rp->ework_bytes) {
      BPPP_HIP(ctx, hipStreamSynchronize(st));
      if (rp->ework) BPPP_HIP(ctx, hipFree(rp->ework));
      rp->ework = nullptr; rp->ework_bytes = 0;
      BPPP_HIP(ctx, hipMalloc(&rp->ework, cv.off));
      rp->ework_bytes = cv.off;
    }
  }
  k_each_ones<<<dim3((unsigned)((Cp + 63) / 64)), dim3(64), 0, st>>>((uint32_t)Cp, ones);
  for (size_t o = 0; o < B; o += C) {
    const size_t n = std::min(C, B - o), np = std::max(n, EACH_MIN_INST);
    if (np > n) {                                   // padding instances: zero scalars, infinity points
      BPPP_HIP(ctx, hipMemsetAsync(rows + n * T * 8, 0, (np - n) * T * 32, st));
      BPPP_HIP(ctx, hipMemsetAsync(tail + n * per * 8, 0, (np - n) * per * 32, st));
      BPPP_HIP(ctx, hipMemsetAsync(pts + n * per * 16, 0, (np - n) * per * 64, st));
    }
    int rc = each_rows_assemble(ctx, S.flavour, n, nlen, llen, k, D.fn, D.fl, ninit, ones, A.q + o * 8, A.sp + o * 8, A.pub_norm + o * nlen * 8,
                                A.pub_lin_c + o * llen * 8, A.pub_lin_x + o * llen * 8, A.es + o * k * 8, A.wit_norm + o * D.fn * 8, A.wit_lin + o * D.fl * 8,
                                A.init_sc + o * ninit * 8, A.init_pts + o * ninit * 16, A.resp_pts + o * 2 * k * 16, scratch, rows, tail, pts);
    if (rc) return rc;
    if (rp->comb) {
      rc = comb_msm(rp->comb, rows, np, fixed, st, COMB_ROWS_DENSE, T, cscratch, cbytes);
      if (rc) return fail(ctx, rc, "rp_verify_each: the fixed-base MSM failed");
    } else if ((rc = basis_msm_dev(rp->commit_basis, rows, T, np, fixed))) return rc;
    if ((rc = msm_batch_dev(ctx, tail, pts, per, np, 0, 0, own))) return rc;
    k_each_finish<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st>>>((uint32_t)n, fixed, own, A.bad + o, status + o, xy + o * 16);
    BPPP_HIP(ctx, hipGetLastError());
  }
  BPPP_HIP(ctx, hipMemcpyAsync(proof_status, status, B * 4, hipMemcpyDeviceToHost, st));
  if (proof_xy) BPPP_HIP(ctx, hipMemcpyAsync(proof_xy, xy, B * 64, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  rp->n_each++;
  return BPPP_OK;
}

}  // namespace bppp

using namespace bppp;

extern "C" {

// the per-proof verifier behind every bppp_rp_verify_each* entry point: files and public amounts (NULL: the handle's own) on the host
// (`host`) or in HBM; nothing of the call is in flight once it returns
static int rp_verify_each_impl(bppp_rp *rp, size_t batch, const void *coms, const void *proofs, const void *pub, bool host, uint32_t *proof_status,
                               uint64_t *proof_xy, const void *bindings = nullptr) {
  if (!rp || !proof_status) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  rp->n_combined = rp->n_each = 0;
  if (!batch) return BPPP_OK;
  if (host && (!coms || !proofs)) return fail(ctx, BPPP_ERR_ARG, "rp_verify_each: null input");
  if (!coms || !proofs || batch >= (1u << 22)) return fail(ctx, BPPP_ERR_ARG, "rp_verify_each: bad arguments");
  const uint8_t seed[32] = {0};                    // the prepared weights rho are not used
  RpVerifyArrays A;
  RpBindGuard guard{rp};
  int rc = rp_bind_begin(rp, bindings, !host, batch, "rp_verify_each_bound");
  if (!rc) rc = rp_verify_start(rp, batch, 0, coms, proofs, pub, host, seed, A);
  if (!rc) rc = rp_each_pass(rp, A, proof_status, proof_xy);
  if (rc || host) ctx_drain(ctx);
  return rc;
}

int bppp_rp_verify_each(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint8_t *proof_files, uint32_t *proof_status, uint64_t *proof_xy) {
  return rp_verify_each_impl(rp, batch, coms_files, proof_files, nullptr, true, proof_status, proof_xy);
}
int bppp_rp_verify_each_pub(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint8_t *proof_files, const uint64_t *public_amounts, uint32_t *proof_status,
                            uint64_t *proof_xy) {
  return rp_verify_each_impl(rp, batch, coms_files, proof_files, public_amounts, true, proof_status, proof_xy);
}
int bppp_rp_verify_each_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_proof_files, uint32_t *proof_status, uint64_t *proof_xy) {
  return rp_verify_each_impl(rp, batch, d_coms_files, d_proof_files, nullptr, false, proof_status, proof_xy);
}
int bppp_rp_verify_each_pub_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_proof_files, const void *d_public_amounts,
                                   uint32_t *proof_status, uint64_t *proof_xy) {
  return rp_verify_each_impl(rp, batch, d_coms_files, d_proof_files, d_public_amounts, false, proof_status, proof_xy);
}
int bppp_rp_verify_each_bound(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint8_t *proof_files, const uint64_t *public_amounts, const uint8_t *bindings,
                              uint32_t *proof_status, uint64_t *proof_xy) {
  return rp_verify_each_impl(rp, batch, coms_files, proof_files, public_amounts, true, proof_status, proof_xy, bindings);
}
int bppp_rp_verify_each_bound_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_proof_files, const void *d_public_amounts,
                                     const void *d_bindings, uint32_t *proof_status, uint64_t *proof_xy) {
  return rp_verify_each_impl(rp, batch, d_coms_files, d_proof_files, d_public_amounts, false, proof_status, proof_xy, d_bindings);
}

}  // extern "C"
