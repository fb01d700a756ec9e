// rpblock.hip — a block in ONE call and ONE MSM: the range proofs of its new outputs, the kernel signatures against their stated keys and the
// sums after cut-through (bppp_rp_verify_block*, include/bppp.h).  combined = V + K + S, the combined points of bppp_rp_verify_bound_device,
// bppp_rp_excess_verify_keys_batch_device and bppp_rp_excess_sums_batch_device under the part seeds SHA-256 ("bppp block" || seed || p), over
//   [ union basis g | H | G (1 + llen + nlen) | nproofs x (ninit + 2k) per-proof terms | nnz entry terms | nkeys x (X_k, R_k) ]
// Every part is the counterpart's own assembly writing into this call's buffer:
//   proofs      rp_verify_prepare, then nl_/ip_verify_batch_assemble with gather_shared = false (as csrc/rpmixed.hip runs a group)
//   signatures  key_stage (k_rp_excess_sigs, k_rp_exkeys_challenge: the ONE lift of every key, written behind the pool) and excess::batch_assemble
//               (k_rp_excess_weights) straight onto the key terms
//   sums        tally::batch_weights and tally::batch_terms over the caller's own CSR; the keys are not merged into it
// and what is new is the glue:
//   k_rp_block_pool_rows  pool rows [0, nproofs) copied from the points the proofs' decoder already lifted; only rows [nproofs, rows) are decoded
//   k_rp_block_key_terms  the sums' share  - rho^S_t(k)  added onto the scalar of X_k, so that a key is one term and not two
//   k_rp_block_shared     the scalars of the union basis: the proofs' shared scalars in stream order, the sums' three negated column sums on
//                         g, H0, H1 and the signatures' sum rho s on B
// All three are one lane per item, bounds-checked on their own index, gather form without atomics, and write with ordinary vector stores.
// A rejected block names its culprits by the counterparts' own exact passes (rp_find_culprits, verify_keys_each_pass, tally::each_pass).
// bppp_rp_verify_block_agg* is the same call with the half-aggregate of the signatures (csrc/rpexagg.hip) in their place:  K' = rho_A (s_agg B -
// sum z_k (c_k X_k + R_k))  stands for K.  The hash tree, s_agg and rho_A come first; key_stage then runs over the R rows widened to signatures with
// s = 0, k_rp_exagg_weights writes the key terms where k_rp_excess_weights does, and rho_A s_agg is the signatures' scalar on B.  The keys of a
// rejected block get the aggregate's own verdict (exagg::verify_run).
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ec.hip.h"
#include "rp_internal.hpp"
#include "rphostcall.hpp"
#include "rpprove_host.hpp"
#include "rpexcess_shared.hip.h"
#include "rpexagg.hip.h"

namespace bppp {

// lane i: commitment i % nr of proven row i / nr, as k_rp_decode_points left it among the row's init points (the infinity encoding for an x
// without a curve point, which is what rp_decode_coms writes)
__global__ void __launch_bounds__(256) k_rp_block_pool_rows(uint32_t n, uint32_t nr, uint32_t nrp, const uint32_t *__restrict__ init_pts, uint32_t *__restrict__ pool) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 *src = (const uint4 *)(init_pts + ((size_t)(i / nr) * (nrp + nr) + nrp + i % nr) * 16);
  uint4 *dst = (uint4 *)(pool + (size_t)i * 16);
  for (int q = 0; q < 4; q++) dst[q] = src[q];
}

// lane k: key k.  k_rp_excess_weights has written terms 2k (n - rho^K c on X_k) and 2k + 1 (n - rho^K on R_k), or zeros and the infinity
// encoding for a signature whose verdict is already taken.  The sum of key k is the last t < nsums with key_start[t] <= k (validated: at most 32
// steps); its weight is subtracted from the scalar of X_k, and a key whose signature takes no part puts its point back for the sums' share.  A
// key without a point contributes nothing and raises reject[0].  rho_s NULL (nsums == 0): the keys belong to no sum.
__global__ void __launch_bounds__(256) k_rp_block_key_terms(uint32_t nkeys, uint32_t nsums, const uint32_t *__restrict__ key_start, const uint32_t *__restrict__ rho_s,
                                                            const uint32_t *__restrict__ pre, const uint32_t *__restrict__ X, uint32_t *__restrict__ sc,
                                                            uint32_t *__restrict__ pt, uint32_t *__restrict__ reject) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  const uint32_t st = pre[k];
  if (st == BPPP_RP_EXCESS_BAD_KEY) { reject[0] = 1u; return; }      // every lane that stores here stores the same word
  if (!rho_s || !nsums) return;
  uint32_t lo = 0, hi = nsums - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (key_start[mid] <= k) lo = mid; else hi = mid - 1;
  }
  fe_store(sc + (size_t)k * 16, fe_sub<1>(fe_load(sc + (size_t)k * 16), fe_load(rho_s + (size_t)lo * 8)));
  if (st != EX_EVAL) {
    const uint4 *src = (const uint4 *)(X + (size_t)k * 16);
    uint4 *dst = (uint4 *)(pt + (size_t)k * 32);
    for (int q = 0; q < 4; q++) dst[q] = src[q];
  }
}

// lane i: position i of the union basis in stream order (g -> 0, H_j -> 1 + j, G_j -> 1 + llen + j).  shared: the proofs' scalars [G | H | g]
// (csrc/nlbatch.hip's order), sums3: the sums' [3][8] on positions 0, 1, 2 (g, H0, H1; the third is zero on a binary handle), sig1: the
// signatures' sum rho s on position `slot`; each may be NULL.
__global__ void __launch_bounds__(256) k_rp_block_shared(uint32_t ulen, uint32_t llen, uint32_t nlen, const uint32_t *__restrict__ shared, const uint32_t *__restrict__ sums3,
                                                         const uint32_t *__restrict__ sig1, uint32_t slot, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ulen) return;
  fe acc = fe_zero();
  if (shared) {
    const uint32_t idx = i == 0 ? nlen + llen : i - 1 < llen ? nlen + (i - 1) : i - 1 - llen;
    acc = fe_load(shared + (size_t)idx * 8);
  }
  if (sums3 && i < 3) acc = fe_add<1>(acc, fe_load(sums3 + (size_t)i * 8));
  if (sig1 && i == slot) acc = fe_add<1>(acc, fe_load(sig1));
  fe_store(out + (size_t)i * 8, acc);
}

}  // namespace bppp

using namespace bppp;
using namespace bppp::tally;
using namespace bppp::excess;
using namespace bppp::exkeys;
using namespace bppp::exagg;

namespace {

const char *WHO = "rp_verify_block";

// seed_p = SHA-256 ("bppp block" || seed || byte p)
void part_seed(const uint8_t seed[32], uint8_t p, uint8_t out[32]) {
  Sha256 h;
  h.update("bppp block", 10);
  h.update(seed, 32);
  h.update(&p, 1);
  uint32_t w[8];
  h.finish(w);
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)(w[i >> 2] >> (24 - 8 * (i & 3)));
}

// what can be judged before anything is read or uploaded: the sizes and the one-pass contract
int block_sizes(bppp_rp *rp, const bppp_rp_block &b) {
  bppp_ctx *ctx = rp->ctx;
  const std::string w = WHO;
  const size_t nr = rp->D.nr;
  if (b.nproofs > b.rows) return fail(ctx, BPPP_ERR_ARG, w + ": nproofs = " + std::to_string(b.nproofs) + " is above rows = " + std::to_string(b.rows));
  if (b.nproofs >= ((size_t)1 << 22)) return fail(ctx, BPPP_ERR_ARG, w + ": 2^22 proofs or more");
  if (!nr || b.rows > RPP_LIM31 / nr || b.nkeys > RPP_LIM31 || b.rows * nr + b.nkeys > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, w + ": rows * nranges + nkeys must be below 2^31");
  if (b.nnz > RPP_LIM31 || b.nnz + b.nkeys > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, w + ": nnz + nkeys must be below 2^31");
  if (b.nsums > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, w + ": nnz and nsums must be below 2^31");
  const size_t E = std::max<size_t>(1, rp->tally_chunk), C = std::max<size_t>(1, rpp_flat_chunk(rp) / 4);
  if (b.nsums && (b.nnz + b.nkeys > E || b.nsums > E))
    return fail(ctx, BPPP_ERR_ARG, w + ": the block does not fit one pass: nnz + nkeys = " + std::to_string(b.nnz + b.nkeys) + " and nsums = " + std::to_string(b.nsums) +
                                       " against the tally chunk of " + std::to_string(E) + "; shard it (the offsets place the shards)");
  if (b.nkeys > C)
    return fail(ctx, BPPP_ERR_ARG, w + ": the block does not fit one pass: nkeys = " + std::to_string(b.nkeys) + " against the key pass of " + std::to_string(C) +
                                       " (a quarter of the flat chunk); shard it (the offsets place the shards)");
  return BPPP_OK;
}

struct BlockWork {
  uint32_t *sc, *pts, *shared, *flags, *reject;
  KeyWork K;
  Work T;
  AggWork A;                                      // bppp_rp_verify_block_agg alone
};

int block_carve(bppp_rp *rp, const bppp_rp_block &b, size_t Tn, bool zero_claims, bool with_agg, BlockWork &W) {
  bppp_ctx *ctx = rp->ctx;
  const size_t nr = rp->D.nr, total = b.rows * nr, ulen = 1 + rp->st.llen + rp->st.nlen, nk = b.nkeys, ns = b.nsums;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? ctx->mix : nullptr, ctx->mix_bytes);
    W.sc = cv.take<uint32_t>((Tn + 32) * 8); W.pts = cv.take<uint32_t>(Tn * 16); W.shared = cv.take<uint32_t>(ulen * 8); W.flags = cv.take<uint32_t>(4);
    W.reject = cv.take<uint32_t>(4);
    KeyWork &K = W.K;
    K = KeyWork{};
    K.sp = cv.take<uint32_t>(nk * 24); K.R = cv.take<uint32_t>(nk * 16); K.bits = cv.take<uint32_t>(nk); K.pre = cv.take<uint32_t>(nk); K.c = cv.take<uint32_t>(nk * 8);
    K.any = cv.take<uint32_t>(4); K.prods = cv.take<uint32_t>(nk * 24); K.red = cv.take<uint32_t>((size_t)RPP_REDUCE_BLOCKS * 24); K.sc3 = cv.take<uint32_t>(24);
    K.seed = cv.take<uint8_t>(32);
    Work &T = W.T;
    T = Work{};
    T.pool = cv.take<uint32_t>((total + nk) * 16 + 16); T.bad = cv.take<uint32_t>(std::max<size_t>(1, b.rows)); T.any = cv.take<uint32_t>(4);
    T.in_sc = cv.take<uint32_t>(ns * 24); T.flag = cv.take<uint32_t>(ns); T.zero = cv.take<uint32_t>(zero_claims ? ns * 8 : 0);
    T.rho = cv.take<uint32_t>(ns * 8); T.prods = cv.take<uint32_t>(ns * 24); T.red = cv.take<uint32_t>((size_t)RPP_REDUCE_BLOCKS * 24); T.sc3 = cv.take<uint32_t>(24);
    T.seed = cv.take<uint8_t>(32);
    K.X = T.pool + total * 16;                    // the lifted keys: the tail of the pool, slot rows * nranges + k
    W.A = AggWork{};
    if (with_agg) agg_carve(cv, nk, nk, W.A);
    if (!pass && cv.off > ctx->mix_bytes) {
      BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (ctx->mix) BPPP_HIP(ctx, hipFree(ctx->mix));
      ctx->mix = nullptr; ctx->mix_bytes = 0;
      BPPP_HIP(ctx, hipMalloc(&ctx->mix, cv.off + cv.off / 8));
      ctx->mix_bytes = cv.off + cv.off / 8;
    }
  }
  return BPPP_OK;
}

// every pointer of the block in HBM.  Checks first (no output is written before they have passed), then the one MSM, then the statuses.
// with_agg: bppp_rp_verify_block_agg — the half-aggregate agg [33 nkeys + 32] (csrc/rpexagg.hip) stands where blk->sigs stands otherwise; without
// it the call is bppp_rp_verify_block, launch for launch.
int block_device(bppp_rp *rp, const bppp_rp_block *blk, const uint8_t *agg, bool with_agg, const uint8_t seed[32], int *accept, const bppp_rp_block_status *status,
                 uint64_t *combined_xy) {
  if (!rp || !blk || !accept) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  const bppp_rp_block &b = *blk;
  uint32_t *proof_status = status ? status->proof_status : nullptr, *key_status = status ? status->key_status : nullptr, *sum_status = status ? status->sum_status : nullptr;
  const size_t np = b.nproofs, nk = b.nkeys, ns = b.nsums;
  if (!np && !nk && !ns) {                               // nothing to check: accepted, and nothing else is looked at
    rp->blk_msms = rp->blk_terms = rp->blk_key_lifts = rp->blk_coms = 0;
    rp->n_combined = rp->n_each = 0;
    if (combined_xy) memset(combined_xy, 0, 64);
    *accept = 1;
    return BPPP_OK;
  }
  int rc;
  if (with_agg && (b.sigs || b.key_offset)) return fail(ctx, BPPP_ERR_ARG, "rp_verify_block_agg: blk->sigs must be NULL and blk->key_offset 0: the aggregate stands for the signatures of the whole job");
  if ((rc = block_sizes(rp, b))) return rc;
  if (!seed || (np && (!b.coms_files || !b.proof_files))) return fail(ctx, BPPP_ERR_ARG, std::string(WHO) + ": null input");
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  SumsJob S;
  KeyJob KJ{};
  if (ns && (rc = sums_checks(S, rp, WHO, b.rows, b.coms_files, ns, b.sum_start, b.entries, b.nnz, b.claim_amounts, b.claim_types, b.claim_offsets, nk, b.key_start, b.keys, false)))
    return rc;
  if (nk && (rc = key_checks(KJ, rp, WHO, nk, b.keys, b.msgs, with_agg ? (const void *)agg : b.sigs, false))) return rc;
  RpBindGuard guard{rp};
  if (np && (rc = rp_bind_begin(rp, b.bindings, true, np, WHO))) return rc;
  // ---- the checks have passed: from here on the call writes its outputs and the handle's counters
  rp->blk_msms = rp->blk_terms = rp->blk_key_lifts = rp->blk_coms = 0;
  rp->n_combined = rp->n_each = 0;
  *accept = 0;
  if (combined_xy) memset(combined_xy, 0, 64);
  uint8_t seeds[3][32];
  for (int p = 0; p < 3; p++) part_seed(seed, (uint8_t)p, seeds[p]);
  const bppp_rps::Setup &St = rp->st;
  const RpDims &D = rp->D;
  const size_t nlen = St.nlen, llen = St.llen, k = St.rounds, nr = D.nr, ninit = D.nrp + D.nr, per = ninit + 2 * k, ulen = 1 + llen + nlen;
  const size_t nnz = ns ? b.nnz : 0;
  const size_t proof_off = ulen, entry_off = proof_off + np * per, key_off = entry_off + nnz, Tn = key_off + 2 * nk;
  BlockWork W;
  if ((rc = block_carve(rp, b, Tn, ns && S.J.zero_claims, with_agg && nk, W))) return rc;
  LapTimer timer(rp->opt.timing, "[rp_verify_block]");
  auto lap = [&](const char *what) { if (rp->opt.timing) { hipStreamSynchronize(st); timer.lap(what); } };
  BPPP_HIP(ctx, hipMemsetAsync(W.flags, 0, 16, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.reject, 0, 16, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.K.any, 0, 16, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.T.any, 0, 16, st));
  // ---- proofs: the single-setup pipeline up to the MSM, its per-proof terms at their place and its shared scalars aside
  RpVerifyArrays A{};
  if (np) {
    if ((rc = rp_verify_prepare(rp, np, b.proof_offset, RpFiles{b.coms_files, b.proof_files}, seeds[0], A))) return rc;
    if ((rc = ensure_scratch(ctx, St.flavour ? ip_verify_batch_scratch(np, nlen, llen, k, D.fn) : nl_verify_batch_scratch(np, nlen, llen, k)))) return rc;
    auto assemble = St.flavour ? ip_verify_batch_assemble : nl_verify_batch_assemble;
    if ((rc = assemble(ctx, np, nlen, llen, k, D.fn, D.fl, ninit, rp->d_g(), rp->d_G(), rp->d_H(), A.rho, A.q, A.sp, A.pub_norm, A.pub_lin_c, A.pub_lin_x, A.es, A.wit_norm,
                       A.wit_lin, A.init_sc, A.init_pts, A.resp_pts, false, W.shared, W.sc + proof_off * 8, W.pts + proof_off * 16, false, W.flags)))
      return rc;
    rp->blk_coms += np * nr;
    lap("proofs: prepare + assemble");
  }
  // ---- sums over the caller's own CSR: the proven rows of the pool from the proofs' decoder, the others decoded here
  if (ns) {
    const uint32_t n_copy = (uint32_t)(np * nr);
    if (n_copy) k_rp_block_pool_rows<<<dim3((n_copy + 255) / 256), dim3(256), 0, st>>>(n_copy, (uint32_t)nr, D.nrp, A.init_pts, W.T.pool);
    BPPP_HIP(ctx, hipGetLastError());
    Job Jd = S.J;                                       // rows [nproofs, rows) alone
    Jd.rows = b.rows - np; Jd.coms = S.J.coms + np * (size_t)D.coms_bytes;
    Work Wd = W.T;
    Wd.pool = W.T.pool + np * nr * 16;
    if ((rc = decode_pool(Jd, Wd))) return rc;
    rp->blk_coms += (b.rows - np) * nr;
    BPPP_HIP(ctx, hipMemcpyAsync(W.T.seed, seeds[2], 32, hipMemcpyHostToDevice, st));
    if ((rc = batch_weights(S.J, W.T, 0, ns, b.sum_offset)) || (rc = batch_terms(S.J, W.T, 0, ns, 0, nnz, W.sc + entry_off * 8, W.pts + entry_off * 16))) return rc;
    lap("sums: pool + weights + terms");
  }
  // ---- signatures: every key lifted once, behind the pool; the sums' share folded onto the key's own term
  if (nk) {
    const ExDomain dc = challenge_domain(rp);
    BPPP_HIP(ctx, hipMemcpyAsync(W.K.seed, seeds[1], 32, hipMemcpyHostToDevice, st));
    if (with_agg) {                                     // the tree over the whole job, s_agg and rho_A; the R rows as signatures with s = 0 for the stage
      KJ.sigs = W.A.sigx;
      if ((rc = expand_launch(ctx, nk, agg, W.A.sigx)) || (rc = commit_tree(rp, nk, KJ.keys, KJ.msgs, agg, AGG_ROW, W.A)) || (rc = sagg_launch(ctx, agg + nk * AGG_ROW, W.A)) ||
          (rc = rho_launch(ctx, W.K.seed, nk, agg + nk * AGG_ROW, W.A)))
        return rc;
    }
    if ((rc = key_stage(KJ, W.K, 0, nk, dc))) return rc;
    rp->blk_key_lifts += nk;
    if (with_agg) rc = weights_launch(rp, nk, 0, nk, W.A.root, W.A.rho, W.K.X, W.K.pre, W.K.c, W.K.sp, W.K.R, nullptr, W.sc + key_off * 8, W.pts + key_off * 16, W.K.any);
    else rc = batch_assemble(rp, nk, b.key_offset, W.K.seed, KJ.sigs, W.K.X, KJ.msgs, W.K.pre, W.K.c, W.K.sp, W.K.R, W.K.prods, W.K.red, W.K.sc3, W.sc + key_off * 8,
                             W.pts + key_off * 16, W.K.any);
    if (rc) return rc;
    k_rp_block_key_terms<<<dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st>>>((uint32_t)nk, (uint32_t)ns, ns ? S.key_start : nullptr, ns ? W.T.rho : nullptr, W.K.pre, W.K.X,
                                                                                 W.sc + key_off * 8, W.pts + key_off * 16, W.reject);
    BPPP_HIP(ctx, hipGetLastError());
    lap("signatures: stage + terms");
  }
  // ---- the union basis and its scalars, then the one MSM
  k_rp_block_shared<<<dim3((unsigned)((ulen + 255) / 256)), dim3(256), 0, st>>>((uint32_t)ulen, (uint32_t)llen, (uint32_t)nlen, np ? W.shared : nullptr, ns ? W.T.sc3 : nullptr,
                                                                              !nk ? nullptr : with_agg ? W.A.rho + 8 : W.K.sc3, blind_slot(rp), W.sc);
  BPPP_HIP(ctx, hipGetLastError());
  BPPP_HIP(ctx, hipMemcpyAsync(W.pts, rp->d_basis, ulen * 64, hipMemcpyDeviceToDevice, st));
  uint64_t out_xy[8];
  rp->blk_msms = 1; rp->blk_terms = Tn;
  if ((rc = msm_run(ctx, W.sc, W.pts, Tn, 1, 1, 0, out_xy))) return rc;
  lap("the MSM");
  // (msm_run returned with the stream drained) what the point cannot show
  uint32_t hflags = 0, reject = 0, kany = 0, tany[2] = {0, 0};
  BPPP_HIP(ctx, hipMemcpy(&hflags, W.flags, 4, hipMemcpyDeviceToHost));
  BPPP_HIP(ctx, hipMemcpy(&reject, W.reject, 4, hipMemcpyDeviceToHost));
  BPPP_HIP(ctx, hipMemcpy(&kany, W.K.any, 4, hipMemcpyDeviceToHost));
  BPPP_HIP(ctx, hipMemcpy(tany, W.T.any, 8, hipMemcpyDeviceToHost));
  uint32_t bad_s = 0;                                   // s_agg >= n
  if (with_agg && nk) BPPP_HIP(ctx, hipMemcpy(&bad_s, W.A.flag, 4, hipMemcpyDeviceToHost));
  if (np && St.flavour && (rc = ip_verify_batch_flags(ctx, hflags))) return rc;
  const bool bad = (np && rp->hflag[0] != 0) || reject || kany || tany[0] || tany[1] || bad_s;
  if (combined_xy) memcpy(combined_xy, out_xy, 64);
  *accept = (rp_point_is_inf(out_xy) && !bad) ? 1 : 0;
  if (*accept) {
    if (proof_status) memset(proof_status, 0, np * 4);
    if (key_status) memset(key_status, 0, nk * 4);
    if (sum_status) memset(sum_status, 0, ns * 4);
    return BPPP_OK;
  }
  // ---- rejected: the point does not say which part failed, so every array asked for is computed, each by its counterpart's exact pass.  The
  // proofs first: the arrays of rp_verify_prepare lie in the handle's verifier workspace, which the other two passes leave alone.
  if (proof_status && np) {
    BPPP_HIP(ctx, hipMemcpy(proof_status, A.bad, np * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < np; i++) proof_status[i] = proof_status[i] ? BPPP_RP_MALFORMED : BPPP_RP_VALID;
    if ((rc = rp_find_culprits(rp, A, false, proof_status))) return rc;
  }
  if (key_status && nk) {
    int part = 0;                                       // the aggregate's own verdict: one equation for all open keys
    if ((rc = with_agg ? verify_run(rp, nk, KJ.keys, KJ.msgs, agg, &part, key_status, nullptr) : verify_keys_each_pass(KJ, key_status))) return rc;
  }
  if (sum_status && ns) {
    const Ext E = sums_ext(S);
    if ((rc = each_pass(S.J, sum_status, nullptr, &E))) return rc;
  }
  return BPPP_OK;
}

int block_host(bppp_rp *rp, const bppp_rp_block *blk, const uint8_t *agg, bool with_agg, const uint8_t seed[32], int *accept, const bppp_rp_block_status *status,
               uint64_t *combined_xy);

}  // namespace

extern "C" {

int bppp_rp_verify_block_device(bppp_rp *rp, const bppp_rp_block *blk, const uint8_t seed[32], int *accept, const bppp_rp_block_status *status, uint64_t *combined_xy) {
  const int rc = block_device(rp, blk, nullptr, false, seed, accept, status, combined_xy);
  if (rc && rp && !ctx_closed(rp->ctx)) ctx_drain(rp->ctx);
  return rc;
}

int bppp_rp_verify_block_agg_device(bppp_rp *rp, const bppp_rp_block *blk, const void *d_agg, const uint8_t seed[32], int *accept, const bppp_rp_block_status *status,
                                    uint64_t *combined_xy) {
  const int rc = block_device(rp, blk, (const uint8_t *)d_agg, true, seed, accept, status, combined_xy);
  if (rc && rp && !ctx_closed(rp->ctx)) ctx_drain(rp->ctx);
  return rc;
}

int bppp_rp_verify_block(bppp_rp *rp, const bppp_rp_block *blk, const uint8_t seed[32], int *accept, const bppp_rp_block_status *status, uint64_t *combined_xy) {
  return block_host(rp, blk, nullptr, false, seed, accept, status, combined_xy);
}

int bppp_rp_verify_block_agg(bppp_rp *rp, const bppp_rp_block *blk, const uint8_t *agg, const uint8_t seed[32], int *accept, const bppp_rp_block_status *status,
                             uint64_t *combined_xy) {
  return block_host(rp, blk, agg, true, seed, accept, status, combined_xy);
}

}  // extern "C"

namespace {

// the host variants: every array of the struct (and the aggregate) uploaded, the _device body, the context drained
int block_host(bppp_rp *rp, const bppp_rp_block *blk, const uint8_t *agg, bool with_agg, const uint8_t seed[32], int *accept, const bppp_rp_block_status *status,
               uint64_t *combined_xy) {
  if (!rp || !blk || !accept) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  bppp_rp_block d = *blk;
  DevBuf coms, proofs, bind, start, entries, a, ty, off, kstart, keys, msgs, sigs, aggb;
  if (d.nproofs || d.nkeys || d.nsums) {
    int rc = block_sizes(rp, d);                         // before any size is multiplied
    if (rc) return rc;
    hipSetDevice(ctx->device);
    const RpDims &D = rp->D;
    const bool sums = d.nsums != 0;
    rc = coms.up(ctx, d.coms_files, d.rows * (size_t)D.coms_bytes);
    if (!rc) rc = proofs.up(ctx, d.proof_files, d.nproofs * (size_t)D.proof_bytes);
    if (!rc) rc = bind.up(ctx, d.bindings, d.nproofs * RP_BINDING_BYTES);
    if (!rc && sums) rc = start.up(ctx, d.sum_start, (d.nsums + 1) * 4);
    if (!rc && sums) rc = entries.up(ctx, d.entries, d.nnz * 4);
    if (!rc && sums) rc = a.up(ctx, d.claim_amounts, d.nsums * 32);
    if (!rc && sums) rc = ty.up(ctx, d.claim_types, d.nsums * 32);
    if (!rc && sums) rc = off.up(ctx, d.claim_offsets, d.nsums * 32);
    if (!rc && sums) rc = kstart.up(ctx, d.key_start, (d.nsums + 1) * 4);
    if (!rc) rc = keys.up(ctx, d.keys, d.nkeys * EX_KEY);
    if (!rc) rc = msgs.up(ctx, d.msgs, d.nkeys * EX_MSG);
    if (!rc && !with_agg) rc = sigs.up(ctx, d.sigs, d.nkeys * EX_SIG);
    if (!rc && with_agg) rc = aggb.up(ctx, agg, BPPP_RP_EXCESS_AGG_BYTES(d.nkeys));
    if (rc) return rc;
    d.coms_files = coms.p; d.proof_files = proofs.p; d.bindings = bind.p; d.sum_start = start.p; d.entries = entries.p; d.claim_amounts = a.p; d.claim_types = ty.p;
    d.claim_offsets = off.p; d.key_start = kstart.p; d.keys = keys.p; d.msgs = msgs.p;
    if (!with_agg) d.sigs = sigs.p;                      // with the aggregate: as the caller left it, for the _device body to judge
  }
  const int rc = block_device(rp, &d, (const uint8_t *)aggb.p, with_agg, seed, accept, status, combined_xy);
  ctx_drain(ctx);
  return rc;
}

}  // namespace
