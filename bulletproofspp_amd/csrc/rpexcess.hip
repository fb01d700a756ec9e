// rpexcess.hip — excess signatures: bppp_rp_excess_sign*, bppp_rp_excess_verify_each*, bppp_rp_excess_verify_batch* (include/bppp.h).
// The balance check for a checker who is NOT told the blinding sum: the excess of sum t over its public claim,
//   X_t = S_t - a_t g - ty_t H0 = e_t B        (B: H1 of a typed handle, h0 of a binary one),
// is a public key, and the builder proves knowledge of e_t by a Schnorr signature (R, s) over a 32-byte message:
//   c_t = decode (SHA-256 (Dc || R || X_t || msg_t)) mod n,    s_t B - c_t X_t = R_t.
// The verifier takes the pool and the CSR job of the tally and shares its sum stage (csrc/rptally.hip through rp_internal.hpp).
// Kernels (one lane per sum unless said otherwise):
//   k_rp_excess_nonce      signer: the verdict on e_t and k_t = decode (SHA-256 (Dn || put (e) || msg || aux)) mod n; the scalar rows of R = k B, X = e B
//   k_rp_excess_respond    signer: c_t, s_t = k_t + c_t e_t and the 65 bytes of the signature
//   k_rp_excess_sigs       verifier: s canonical, the sign byte in range, R lifted by the decoder the pool uses (csrc/rplift.hip.h)
//   k_rp_excess_key        verifier: X_t = S_t - claim_t by one mixed addition, and ZZ ZZZ for the batch inversion
//   k_rp_excess_challenge  verifier: the verdict that needs no equation, and c_t over the canonical affine X_t
//   k_rp_excess_mulcheck   verifier: one QUAD per sum: c_t X_t by the walk of csrc/rpexcess.hip.h, then s_t B - c_t X_t against R_t, cross-multiplied
//   k_rp_excess_weights    batch: rho_t, the product column - rho_t s_t and the two MSM terms of the sum
// Every kernel is bounds-checked on its own index, reads the 65-byte signature rows bytewise and writes with ordinary vector stores.
// The domains, the three-block hash and the challenge are in csrc/rpexcess_shared.hip.h: the stated keys (csrc/rpexkeys.hip) hash the same
// messages and run k_rp_excess_sigs, k_rp_excess_mulcheck and k_rp_excess_weights through the launches at the end of the kernels here.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ec.hip.h"
#include "rp_internal.hpp"
#include "rphostcall.hpp"
#include "rpprove_host.hpp"
#include "rpwords.hip.h"
#include "rplift.hip.h"
#include "rpexcess.hip.h"
#include "rpexcess_shared.hip.h"
#include "sha256.hip.h"

namespace bppp {

// ---- signer.  in_sc [2n][3][8]: row t the scalars of R_t = k_t B, row n + t those of X_t = e_t B, on base `slot` (typed 2: H1, binary 1: h0); a
// refused sum gets zero scalars, so its two points are the infinity encoding
__global__ void __launch_bounds__(64) k_rp_excess_nonce(uint32_t n, uint32_t slot, ExDomain dn, const uint32_t *__restrict__ blinds, const uint8_t *__restrict__ msgs,
                                                        const uint8_t *__restrict__ aux, uint32_t *__restrict__ nonce, uint32_t *__restrict__ in_sc,
                                                        uint32_t *__restrict__ status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t *ew = blinds + (size_t)t * 8;
  const uint8_t *msg = msgs + (size_t)t * EX_MSG;
  const fe e = fe_load(ew);
  uint32_t st = !wi_canonical(e) ? (uint32_t)BPPP_RP_EXCESS_NOT_CANONICAL : fe_is_zero(e) ? (uint32_t)BPPP_RP_EXCESS_ZERO : (uint32_t)BPPP_RP_EXCESS_OK;
  fe k = fe_zero();
  if (st == BPPP_RP_EXCESS_OK) {
    k = ex_hash3(32 + 32 + EX_MSG + 32, [&](uint32_t b) -> uint32_t {
      if (b < 32) return ex_dom_byte(dn, b);
      if (b < 64) return enc_be_byte(ew, b - 32);
      if (b < 96) return msg[b - 64];
      return aux[b - 96];
    });
    if (fe_is_zero(k)) st = BPPP_RP_EXCESS_NONCE;
  }
  const bool ok = st == BPPP_RP_EXCESS_OK;
  for (uint32_t b = 0; b < 3; b++) {
    fe_store(in_sc + ((size_t)t * 3 + b) * 8, (ok && b == slot) ? k : fe_zero());
    fe_store(in_sc + ((size_t)(n + t) * 3 + b) * 8, (ok && b == slot) ? e : fe_zero());
  }
  fe_store(nonce + (size_t)t * 8, k);
  status[t] = st;
}
// pts [2n][16]: R then X, as in_sc; sigs [n][65]: put (R.x), the sign byte of R, put (s); zero bytes for a refused sum
__global__ void __launch_bounds__(64) k_rp_excess_respond(uint32_t n, ExDomain dc, const uint32_t *__restrict__ blinds, const uint32_t *__restrict__ nonce,
                                                          const uint32_t *__restrict__ pts, const uint8_t *__restrict__ msgs, const uint32_t *__restrict__ status,
                                                          uint8_t *__restrict__ sigs) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint8_t *sig = sigs + (size_t)t * EX_SIG;
  if (status[t] != BPPP_RP_EXCESS_OK) { for (uint32_t o = 0; o < EX_SIG; o++) sig[o] = 0; return; }
  const uint32_t *R = pts + (size_t)t * 16, *X = pts + (size_t)(n + t) * 16;
  const fe c = ex_challenge(dc, [&](uint32_t o) -> uint32_t { return ex_pt_byte(R, o); }, X, msgs + (size_t)t * EX_MSG);
  const fe s = fe_add<1>(fe_load(nonce + (size_t)t * 8), fe_mul<1>(c, fe_load(blinds + (size_t)t * 8)));
  uint32_t sw[8];
  fe_store(sw, s);
  for (uint32_t o = 0; o < 33; o++) sig[o] = (uint8_t)ex_pt_byte(R, o);
  for (uint32_t o = 0; o < 32; o++) sig[33 + o] = enc_be_byte(sw, o);
}

// ---- verifier.  bits[t]: 1 = s >= n, 2 = the sign byte is not 0 or 1 or R.x has no curve point.  in_sc [n][3][8]: the scalars of P_t = s_t B
// (zero for an s that is no scalar); R [n][16]: the lifted point, the infinity encoding where there is none
__global__ void __launch_bounds__(64) k_rp_excess_sigs(uint32_t n, uint32_t slot, const uint8_t *__restrict__ sigs, uint32_t *__restrict__ in_sc, uint32_t *__restrict__ R,
                                                       uint32_t *__restrict__ bits) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint8_t *sig = sigs + (size_t)t * EX_SIG;
  const fe s = load_field_be_raw(sig + 33);
  const bool bad_s = !wi_canonical(s);
  const uint32_t sign = sig[32];
  bool ok;
  aff r = rp_lift_x(load_field_be<0>(sig), sign == 1, ok);
  const bool bad_r = sign > 1 || !ok;
  if (bad_r) r = aff_inf();
  for (uint32_t b = 0; b < 3; b++) fe_store(in_sc + ((size_t)t * 3 + b) * 8, (!bad_s && b == slot) ? s : fe_zero());
  aff_store(R + (size_t)t * 16, r);
  bits[t] = (bad_s ? 1u : 0u) | (bad_r ? 2u : 0u);
}
// sums[t] (XYZZ) becomes X_t = S_t - rec[t] in place; zz[t] = ZZ ZZZ of it, zero for infinity and for a malformed sum
__global__ void __launch_bounds__(256) k_rp_excess_key(uint32_t n, uint32_t *__restrict__ sums, const uint32_t *__restrict__ rec, const uint32_t *__restrict__ malformed,
                                                       uint32_t *__restrict__ zz) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  xyzz S = xyzz_load(sums + (size_t)t * XYZZ_WORDS);
  xyzz_madd(S, aff_cneg(aff_load(rec + (size_t)t * 16), true));
  xyzz_store(sums + (size_t)t * XYZZ_WORDS, S);
  fe_store(zz + (size_t)t * 8, (malformed[t] || xyzz_is_inf(S)) ? fe_zero() : fq_to_fe(fq_mul(S.ZZ, S.ZZZ)));
}
// the first verdict that applies, in the header's order; EX_EVAL and the challenge where the equation has to decide.  X [n][16]: the canonical
// affine excess, all zeros for infinity (and for a malformed sum, whose verdict is taken before it is looked at)
__global__ void __launch_bounds__(64) k_rp_excess_challenge(uint32_t n, ExDomain dc, const uint8_t *__restrict__ sigs, const uint32_t *__restrict__ X,
                                                            const uint8_t *__restrict__ msgs, const uint32_t *__restrict__ malformed, const uint32_t *__restrict__ flag,
                                                            const uint32_t *__restrict__ bits, uint32_t *__restrict__ c, uint32_t *__restrict__ pre) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t *x = X + (size_t)t * 16;
  uint32_t any = 0;
  for (int k = 0; k < 16; k++) any |= x[k];
  const uint32_t st = malformed[t]                 ? (uint32_t)BPPP_RP_OPEN_MALFORMED
                      : (flag[t] || (bits[t] & 1u)) ? (uint32_t)BPPP_RP_OPEN_NOT_CANONICAL
                      : (bits[t] & 2u)              ? (uint32_t)BPPP_RP_EXCESS_BAD_R
                      : !any                        ? (uint32_t)BPPP_RP_EXCESS_NO_KEY
                                                    : EX_EVAL;
  fe ch = fe_zero();
  if (st == EX_EVAL) {
    const uint8_t *sig = sigs + (size_t)t * EX_SIG;
    ch = ex_challenge(dc, [&](uint32_t o) -> uint32_t { return sig[o]; }, x, msgs + (size_t)t * EX_MSG);
  }
  fe_store(c + (size_t)t * 8, ch);
  pre[t] = st;
}

// ---- the hot path: lanes 4q .. 4q + 3 of the launch are sum q.  c_t X_t by the quad walk, then  c_t X_t - P_t  against  - R_t  (the
// equation s B - c X = R with both sides negated, so that the negations fall on affine points), cross-multiplied as k_rp_tally_compare
// does: no inversion.  A quad past n and a quad whose verdict is taken leave as a whole; every branch below is on values all four lanes
// hold alike.  Lane 0 of the quad stores the verdict.
__global__ void __launch_bounds__(64) k_rp_excess_mulcheck(uint32_t n, const uint32_t *__restrict__ c, const uint32_t *__restrict__ X, const uint32_t *__restrict__ P,
                                                           const uint32_t *__restrict__ R, const uint32_t *__restrict__ pre, uint32_t *__restrict__ status) {
  const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (t >= n) return;
  const uint32_t st = pre[t];
  if (st != EX_EVAL) { if (quad_lane() == 0) status[t] = st; return; }
  xyzz acc = excess_mul_quad(fe_load(c + (size_t)t * 8), aff_load(X + (size_t)t * 16));
  xyzz_add_quad(acc, xyzz_from_aff(aff_cneg(aff_load(P + (size_t)t * 16), true)));
  const aff nr = aff_cneg(aff_load(R + (size_t)t * 16), true);       // R is a curve point here: never infinity
  const bool eq = !xyzz_is_inf(acc) && fq_normalizes_to_zero(fq_sub<5>(fq_mul(nr.x, acc.ZZ), acc.X)) && fq_normalizes_to_zero(fq_sub<3>(fq_mul(nr.y, acc.ZZZ), acc.Y));
  if (quad_lane() == 0) status[t] = eq ? (uint32_t)BPPP_RP_OPEN_OK : (uint32_t)BPPP_RP_OPEN_MISMATCH;
}

// ---- the batch: rho_t = decode (SHA-256 (seed || le64 (j0 + t) || sig_t || put (X_t.x) || sign (X_t) || msg_t)) mod n, 1 for 0: 170 bytes.
// prods [n][3][8]: - rho_t s_t in column 0 (rpp_negated_column_sums negates the sum back); terms 2t and 2t + 1 of the MSM:  n - rho_t c_t  on
// X_t and  n - rho_t  on R_t.  A sum whose verdict is already taken puts in zero scalars and the infinity encoding and raises any[0].
__global__ void __launch_bounds__(64) k_rp_excess_weights(uint32_t n, uint32_t slot, uint64_t j0, const uint8_t *__restrict__ seed, const uint8_t *__restrict__ sigs,
                                                          const uint32_t *__restrict__ X, const uint8_t *__restrict__ msgs, const uint32_t *__restrict__ pre,
                                                          const uint32_t *__restrict__ c, const uint32_t *__restrict__ in_sc, const uint32_t *__restrict__ R,
                                                          uint32_t *__restrict__ prods, uint32_t *__restrict__ sc, uint32_t *__restrict__ pt, uint32_t *__restrict__ any) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const bool part = pre[t] == EX_EVAL;
  fe rs = fe_zero(), rc = fe_zero(), r1 = fe_zero();
  if (part) {
    const uint8_t *sig = sigs + (size_t)t * EX_SIG, *msg = msgs + (size_t)t * EX_MSG;
    const uint32_t *x = X + (size_t)t * 16;
    const uint64_t j = j0 + t;
    fe rho = ex_hash3(32 + 8 + EX_SIG + 33 + EX_MSG, [&](uint32_t k) -> uint32_t {
      if (k < 32) return seed[k];
      if (k < 40) return (uint32_t)(j >> (8 * (k - 32)));
      if (k < 105) return sig[k - 40];
      if (k < 138) return ex_pt_byte(x, k - 105);
      return msg[k - 138];
    });
    if (fe_is_zero(rho)) rho = fe_one();
    rs = fe_neg<1>(fe_mul<1>(rho, fe_load(in_sc + ((size_t)t * 3 + slot) * 8)));
    rc = fe_neg<1>(fe_mul<1>(rho, fe_load(c + (size_t)t * 8)));
    r1 = fe_neg<1>(rho);
  } else any[0] = 1u;                                   // every lane that stores here stores the same word
  fe_store(prods + (size_t)t * 24, rs); fe_store(prods + (size_t)t * 24 + 8, fe_zero()); fe_store(prods + (size_t)t * 24 + 16, fe_zero());
  fe_store(sc + (size_t)t * 16, rc); fe_store(sc + (size_t)t * 16 + 8, r1);
  for (int k = 0; k < 16; k++) {
    pt[(size_t)t * 32 + k] = part ? X[(size_t)t * 16 + k] : 0u;
    pt[(size_t)t * 32 + 16 + k] = part ? R[(size_t)t * 16 + k] : 0u;
  }
}

}  // namespace bppp

namespace bppp {
namespace excess {

// the launches the stated keys share (csrc/rpexkeys.hip, declared in csrc/rpexcess_shared.hip.h): the grids of verify_stage and of the two passes below
int sigs_launch(bppp_ctx *ctx, size_t n, uint32_t slot, const uint8_t *sigs, uint32_t *in_sc, uint32_t *R, uint32_t *bits) {
  k_rp_excess_sigs<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>((uint32_t)n, slot, sigs, in_sc, R, bits);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}
int mulcheck_launch(bppp_ctx *ctx, size_t n, const uint32_t *c, const uint32_t *X, const uint32_t *P, const uint32_t *R, const uint32_t *pre, uint32_t *status) {
  k_rp_excess_mulcheck<<<dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, ctx->stream>>>((uint32_t)n, c, X, P, R, pre, status);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}
int batch_assemble(bppp_rp *rp, size_t n, uint64_t j0, const uint8_t *seed, const uint8_t *sigs, const uint32_t *X, const uint8_t *msgs, const uint32_t *pre, const uint32_t *c,
                   const uint32_t *sp, const uint32_t *R, uint32_t *prods, uint32_t *red, uint32_t *sc3, uint32_t *msm_sc, uint32_t *msm_pt, uint32_t *any) {
  bppp_ctx *ctx = rp->ctx;
  k_rp_excess_weights<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>((uint32_t)n, blind_slot(rp), j0, seed, sigs, X, msgs, pre, c, sp, R, prods, msm_sc, msm_pt, any);
  BPPP_HIP(ctx, hipGetLastError());
  return rpp_negated_column_sums(rp, n, prods, red, sc3);                                 // sum rho s: the scalar of B
}
int batch_chunk(bppp_rp *rp, size_t n, uint64_t j0, const uint8_t *seed, const uint8_t *sigs, const uint32_t *X, const uint8_t *msgs, const uint32_t *pre, const uint32_t *c,
                const uint32_t *sp, const uint32_t *R, uint32_t *prods, uint32_t *red, uint32_t *sc3, uint32_t *msm_sc, uint32_t *msm_pt, uint32_t *any, BatchParts &parts) {
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  const uint32_t slot = blind_slot(rp);
  int rc;
  if ((rc = batch_assemble(rp, n, j0, seed, sigs, X, msgs, pre, c, sp, R, prods, red, sc3, msm_sc, msm_pt, any))) return rc;
  BPPP_HIP(ctx, hipMemcpyAsync(msm_sc + 2 * n * 8, sc3, 32, hipMemcpyDeviceToDevice, st));
  BPPP_HIP(ctx, hipMemcpyAsync(msm_pt + 2 * n * 16, rp->d_basis + 16 * slot, 64, hipMemcpyDeviceToDevice, st));   // [g | H0 | H1 ...]: the registered basis starts with them
  return parts.msm(ctx, msm_sc, msm_pt, 2 * n + 1);
}

}  // namespace excess
}  // namespace bppp

using namespace bppp;
using namespace bppp::tally;
using namespace bppp::excess;

namespace {

const char *sign_status_text(uint32_t s) {
  return s == BPPP_RP_EXCESS_NOT_CANONICAL ? "the blinding sum is not canonical (>= n)"
         : s == BPPP_RP_EXCESS_ZERO        ? "the blinding sum is zero: the excess is the point at infinity (the plain tally with a zero blinding serves this case)"
                                           : "the nonce is zero";
}

int sign_device(bppp_rp *rp, size_t nsums, const void *d_blinds, const void *d_msgs, const uint8_t aux[32], void *d_sigs, uint64_t *excess_xy, uint32_t *sign_status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  if (!d_blinds || !d_msgs || !aux || !d_sigs) return fail(ctx, BPPP_ERR_ARG, "rp_excess_sign: null input");
  if (nsums > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, "rp_excess_sign: nsums must be below 2^31");
  hipSetDevice(ctx->device);
  int rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const size_t C = std::min(nsums, rpp_flat_chunk(rp));         // sums per pass over the workspace
  uint32_t *in_sc = nullptr, *pts = nullptr, *nonce = nullptr, *status = nullptr;
  uint8_t *d_aux = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    in_sc = cv.take<uint32_t>(2 * C * 24); pts = cv.take<uint32_t>(2 * C * 16); nonce = cv.take<uint32_t>(C * 8); status = cv.take<uint32_t>(C);
    d_aux = cv.take<uint8_t>(32);
    if (!pass && (rc = rpp_ensure_pwork(rp, cv.off))) return rc;
  }
  hipStream_t st = ctx->stream;
  const ExDomain dn = nonce_domain(rp), dc = challenge_domain(rp);
  const uint32_t slot = blind_slot(rp);
  std::vector<uint32_t> h_status(nsums);
  std::vector<uint32_t> h_pts;
  BPPP_HIP(ctx, hipMemcpyAsync(d_aux, aux, 32, hipMemcpyHostToDevice, st));
  for (size_t o = 0; o < nsums; o += C) {
    const size_t n = std::min(C, nsums - o);
    const uint32_t *bl = (const uint32_t *)d_blinds + o * 8;
    const uint8_t *msgs = (const uint8_t *)d_msgs + o * EX_MSG;
    const dim3 grid((unsigned)((n + 63) / 64));
    k_rp_excess_nonce<<<grid, dim3(64), 0, st>>>((uint32_t)n, slot, dn, bl, msgs, d_aux, nonce, in_sc, status);
    BPPP_HIP(ctx, hipGetLastError());
    if ((rc = rpp_commit_inputs(rp, in_sc, 2 * n, pts))) return rc;
    k_rp_excess_respond<<<grid, dim3(64), 0, st>>>((uint32_t)n, dc, bl, nonce, pts, msgs, status, (uint8_t *)d_sigs + o * EX_SIG);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(h_status.data() + o, status, n * 4, hipMemcpyDeviceToHost, st));
    if (excess_xy) BPPP_HIP(ctx, hipMemcpyAsync(excess_xy + o * 8, pts + n * 16, n * 64, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return rpp_report_refusals(ctx, "rp_excess_sign", "sum", h_status.data(), nsums, sign_status, sign_status_text);
}

// the verifier's own arrays of one pass, carved behind the tally's (Work::extra)
struct ExWork { uint32_t *sp, *P, *R, *bits, *pre, *c, *zero, *any; };
size_t ex_carve(uint8_t *base, size_t ns, ExWork &X) {
  Carver cv(base, 0);
  X.sp = cv.take<uint32_t>(ns * 24); X.P = cv.take<uint32_t>(ns * 16); X.R = cv.take<uint32_t>(ns * 16); X.bits = cv.take<uint32_t>(ns);
  X.pre = cv.take<uint32_t>(ns); X.c = cv.take<uint32_t>(ns * 8); X.zero = cv.take<uint32_t>(ns * 8); X.any = cv.take<uint32_t>(4);
  return cv.off;
}

struct ExJob { Job J; const uint8_t *msgs, *sigs; };

// the argument checks of both verifiers; the CSR verdict is read back before anything gathers (tally_checks)
int verify_checks(ExJob &E, bppp_rp *rp, const char *who, size_t rows, const void *coms, size_t nsums, const void *start, const void *entries, size_t nnz, const void *amt,
                  const void *ty, const void *msgs, const void *sigs, bool null_args) {
  Job &J = E.J;
  fill(J, rp, who, rows, coms, nsums, start, entries, nnz, amt, ty, nullptr);
  E.msgs = (const uint8_t *)msgs; E.sigs = (const uint8_t *)sigs;
  int rc = tally_checks(J, null_args || (rows && !coms) || !msgs || !sigs, false); if (rc) return rc;
  if (rp->st.kind != 1 && (J.amt == nullptr) != (J.ty == nullptr))
    return fail(rp->ctx, BPPP_ERR_ARG, std::string(who) + ": claim_amounts and claim_types must be given together or both be NULL");
  if (rp->st.kind == 1 && !J.amt) J.ty = nullptr;
  J.zero_claims = !J.amt;
  return BPPP_OK;
}

// sums [t0, t0 + ns) up to the verdict that needs no equation: W.xy the affine excess, X.R, X.c, X.pre (and X.sp, the scalars of s B)
int verify_stage(const ExJob &E, const Work &W, const ExWork &X, size_t t0, size_t ns, const Levels &L, const ExDomain &dc) {
  const Job &J = E.J;
  bppp_rp *rp = J.rp;
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  int rc;
  if ((rc = sum_launches(J, W, t0, ns, L))) return rc;
  BPPP_HIP(ctx, hipMemsetAsync(X.zero, 0, ns * 32, st));
  const uint32_t *amt = J.zero_claims ? X.zero : J.amt + t0 * 8, *ty = J.zero_claims ? X.zero : J.ty ? J.ty + t0 * 8 : nullptr;
  if ((rc = rpp_claim_scalars(rp, ns, amt, ty, X.zero, W.in_sc, W.flag, W.any + 1)) || (rc = rpp_commit_inputs(rp, W.in_sc, ns, W.rec))) return rc;
  if ((rc = sigs_launch(ctx, ns, blind_slot(rp), E.sigs + t0 * EX_SIG, X.sp, X.R, X.bits))) return rc;
  k_rp_excess_key<<<dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st>>>((uint32_t)ns, W.sums, W.rec, W.malformed, W.zz);
  BPPP_HIP(ctx, hipGetLastError());
  if ((rc = batch_inverse_run(ctx, W.zz, ns, 0, W.zinv)) || (rc = affine_launch(ctx, ns, W.sums, W.zinv, W.xy))) return rc;
  k_rp_excess_challenge<<<dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, st>>>((uint32_t)ns, dc, E.sigs + t0 * EX_SIG, W.xy, E.msgs + t0 * EX_MSG, W.malformed, W.flag, X.bits, X.c, X.pre);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

// every sum decided on its own: status [nsums] and, when not NULL, excess_xy [nsums][8], both on the host.  The job has passed verify_checks.
int verify_each_pass(const ExJob &E, uint32_t *status, uint64_t *excess_xy) {
  const Job &J = E.J;
  bppp_rp *rp = J.rp;
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  int rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const Plan P = make_plan(J);
  Work W;
  ExWork X;
  if ((rc = carve(J, P.ns_max, true, P.ni, P.np, false, 0, W, ex_carve(nullptr, P.ns_max, X))) || (rc = decode_pool(J, W))) return rc;
  ex_carve(W.extra, P.ns_max, X);
  const ExDomain dc = challenge_domain(rp);
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (rp->opt.timing) for (auto &e : ev) BPPP_HIP(ctx, hipEventCreate(&e));
  for (size_t c = 0; c + 1 < P.cb.size(); c++) {
    const size_t t0 = P.cb[c], ns = P.cb[c + 1] - t0;
    if ((rc = verify_stage(E, W, X, t0, ns, P.plans[c], dc)) || (rc = rpp_commit_inputs(rp, X.sp, ns, X.P))) break;
    if (ev[0]) hipEventRecord(ev[0], st);
    rc = mulcheck_launch(ctx, ns, X.c, W.xy, X.P, X.R, X.pre, W.status);
    if (ev[0]) hipEventRecord(ev[1], st);
    if (rc) break;
    hipError_t e = hipMemcpyAsync(status + t0, W.status, ns * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && excess_xy) e = hipMemcpyAsync(excess_xy + t0 * 8, W.xy, ns * 64, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { rc = fail(ctx, BPPP_ERR_HIP, std::string("rp_excess_verify_each: ") + hipGetErrorString(e)); break; }
    if (ev[0]) {
      float ms = 0;
      hipEventElapsedTime(&ms, ev[0], ev[1]);
      fprintf(stderr, "[rp excess] k_rp_excess_mulcheck     %8zu sums %9.3f ms\n", ns, ms);
    }
  }
  for (auto &e : ev) if (e) hipEventDestroy(e);
  return rc;
}

int verify_each_device(bppp_rp *rp, size_t rows, const void *d_coms, size_t nsums, const void *d_start, const void *d_entries, size_t nnz, const void *d_amt, const void *d_ty,
                       const void *d_msgs, const void *d_sigs, uint32_t *status, uint64_t *excess_xy) {
  if (!rp) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  ExJob E;
  int rc = verify_checks(E, rp, "rp_excess_verify_each", rows, d_coms, nsums, d_start, d_entries, nnz, d_amt, d_ty, d_msgs, d_sigs, !status);
  return rc ? rc : verify_each_pass(E, status, excess_xy);
}

int verify_batch_device(bppp_rp *rp, size_t rows, const void *d_coms, size_t nsums, const void *d_start, const void *d_entries, size_t nnz, const void *d_amt, const void *d_ty,
                        const void *d_msgs, const void *d_sigs, uint64_t index_offset, const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  if (!nsums) { if (combined_xy) memset(combined_xy, 0, 64); *accept = 1; return BPPP_OK; }
  ExJob E;
  int rc = verify_checks(E, rp, "rp_excess_verify_batch", rows, d_coms, nsums, d_start, d_entries, nnz, d_amt, d_ty, d_msgs, d_sigs, !seed); if (rc) return rc;
  const Job &J = E.J;
  if (combined_xy) memset(combined_xy, 0, 64);
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  hipStream_t st = ctx->stream;
  const Plan P = make_plan(J);
  Work W;
  ExWork X;
  if ((rc = carve(J, P.ns_max, true, P.ni, P.np, true, 2 * P.ns_max, W, ex_carve(nullptr, P.ns_max, X))) || (rc = decode_pool(J, W))) return rc;
  ex_carve(W.extra, P.ns_max, X);
  const ExDomain dc = challenge_domain(rp);
  BPPP_HIP(ctx, hipMemcpyAsync(W.seed, seed, 32, hipMemcpyHostToDevice, st));
  BPPP_HIP(ctx, hipMemsetAsync(X.any, 0, 16, st));
  BatchParts parts;                             // one combined point per pass
  for (size_t c = 0; c + 1 < P.cb.size(); c++) {
    const size_t t0 = P.cb[c], ns = P.cb[c + 1] - t0;
    if ((rc = verify_stage(E, W, X, t0, ns, P.plans[c], dc))) return rc;
    if ((rc = batch_chunk(rp, ns, index_offset + t0, W.seed, E.sigs + t0 * EX_SIG, W.xy, E.msgs + t0 * EX_MSG, X.pre, X.c, X.sp, X.R, W.prods, W.red, W.sc3, W.msm_sc, W.msm_pt, X.any,
                          parts))) return rc;
  }
  uint32_t any = 0;
  BPPP_HIP(ctx, hipMemcpy(&any, X.any, 4, hipMemcpyDeviceToHost));
  if ((rc = parts.finish(ctx, any != 0, combined_xy, accept))) return rc;
  if (!status) return BPPP_OK;
  if (*accept) { memset(status, 0, nsums * 4); return BPPP_OK; }
  return verify_each_pass(E, status, nullptr);  // one exact pass, whatever the number of bad sums
}

// ---- host variants: upload, the _device variant, download
// the tally's arrays without a third claim, and the messages and signatures of the sums
struct HostJob : HostCsr {
  DevBuf msgs, sigs;
  int up(bppp_rp *rp, size_t rows, const void *h_coms, size_t nsums, const uint32_t *sum_start, const uint32_t *ent, size_t nnz, const uint64_t *ca, const uint64_t *cty,
         const uint8_t *m, const uint8_t *s) {
    if (!rpp_sizes_ok(rp, rows, nsums, nnz)) return BPPP_OK;
    int rc = HostCsr::up(rp, rows, h_coms, rp->D.coms_bytes, nsums, sum_start, ent, nnz, ca, cty, nullptr, nsums * 32);
    if (!rc) rc = msgs.up(rp->ctx, m, nsums * EX_MSG);
    if (!rc) rc = sigs.up(rp->ctx, s, nsums * EX_SIG);
    return rc;
  }
};

}  // namespace

extern "C" {

int bppp_rp_excess_sign_device(bppp_rp *rp, size_t nsums, const void *d_claim_blinds, const void *d_msgs, const uint8_t aux[32], void *d_sigs, uint64_t *excess_xy,
                               uint32_t *sign_status) {
  return sign_device(rp, nsums, d_claim_blinds, d_msgs, aux, d_sigs, excess_xy, sign_status);
}

int bppp_rp_excess_sign(bppp_rp *rp, size_t nsums, const uint64_t *claim_blinds, const uint8_t *msgs, const uint8_t aux[32], uint8_t *sigs, uint64_t *excess_xy,
                        uint32_t *sign_status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  DevBuf bl, m, s;
  if (nsums <= RPP_LIM31) {
    hipSetDevice(ctx->device);
    int rc = bl.up(ctx, claim_blinds, nsums * 32);
    if (!rc) rc = m.up(ctx, msgs, nsums * EX_MSG);
    if (!rc) rc = s.out(ctx, sigs, nsums * EX_SIG);
    if (rc) return rc;
  }
  int rc = sign_device(rp, nsums, bl.p, m.p, aux, s.p, excess_xy, sign_status);
  return rpp_download_refused(ctx, rc, "rp_excess_sign: sum ", sigs, s.p, nsums * EX_SIG);
}

int bppp_rp_excess_verify_each_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                                      const void *d_claim_amounts, const void *d_claim_types, const void *d_msgs, const void *d_sigs, uint32_t *status,
                                      uint64_t *excess_xy) {
  return verify_each_device(rp, rows, d_coms_files, nsums, d_sum_start, d_entries, nnz, d_claim_amounts, d_claim_types, d_msgs, d_sigs, status, excess_xy);
}

int bppp_rp_excess_verify_each(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                               const uint64_t *claim_amounts, const uint64_t *claim_types, const uint8_t *msgs, const uint8_t *sigs, uint32_t *status,
                               uint64_t *excess_xy) {
  if (!rp) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  HostJob H;
  int rc = H.up(rp, rows, coms_files, nsums, sum_start, entries, nnz, claim_amounts, claim_types, msgs, sigs);
  if (rc) return rc;
  return verify_each_device(rp, rows, H.coms.p, nsums, H.start.p, H.entries.p, nnz, H.a.p, H.ty.p, H.msgs.p, H.sigs.p, status, excess_xy);
}

int bppp_rp_excess_verify_batch_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                                       const void *d_claim_amounts, const void *d_claim_types, const void *d_msgs, const void *d_sigs, uint64_t index_offset,
                                       const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy) {
  return verify_batch_device(rp, rows, d_coms_files, nsums, d_sum_start, d_entries, nnz, d_claim_amounts, d_claim_types, d_msgs, d_sigs, index_offset, seed, accept, status,
                             combined_xy);
}

int bppp_rp_excess_verify_batch(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                                const uint64_t *claim_amounts, const uint64_t *claim_types, const uint8_t *msgs, const uint8_t *sigs, const uint8_t seed[32], int *accept,
                                uint32_t *status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  HostJob H;
  if (nsums) {
    int rc = H.up(rp, rows, coms_files, nsums, sum_start, entries, nnz, claim_amounts, claim_types, msgs, sigs);
    if (rc) return rc;
  }
  return verify_batch_device(rp, rows, H.coms.p, nsums, H.start.p, H.entries.p, nnz, H.a.p, H.ty.p, H.msgs.p, H.sigs.p, 0, seed, accept, status, combined_xy);
}

}  // extern "C"
