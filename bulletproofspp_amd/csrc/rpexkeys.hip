// rpexkeys.hip — excess KEYS: the excess of a transaction stated as 33 bytes next to its signature, so that signatures are checked with no pool
// in hand and a block's sums still check after cut-through: bppp_rp_excess_keys*, bppp_rp_excess_verify_keys_each*,
// bppp_rp_excess_verify_keys_batch*, bppp_rp_excess_sums_each*, bppp_rp_excess_sums_batch* (include/bppp.h).
//   key        put (x), then the sign byte (0 or 1: y > p - y) — as a signature holds R; lifted by rp_lift_x (csrc/rplift.hip.h); every hash
//              that names the key takes the canonical 33 bytes of the LIFTED point, which is what the derived-key path (csrc/rpexcess.hip) hashes
//   signature  s B - c X = R with the challenge of csrc/rpexcess_shared.hip.h: the 65 bytes of bppp_rp_excess_sign, unchanged
//   sums       S_t - a_t g - ty_t H0 - o_t B - sum of the keys of group t = identity: the keys are lifted into a tail of the decoded pool and the
//              CSR of the job is merged with  (rows * nranges + k) | bit 31  for key k, sum by sum; from there on it is a tally
//              (tally::each_pass / tally::batch_run, csrc/rptally.hip), so a sum's keys are planned, split into pieces and summed with its entries
// Kernels (one lane per key or per sum unless said otherwise):
//   k_rp_exkeys_blinds     builder: the verdict on e_t and the scalar row of X_t = e_t B
//   k_rp_exkeys_encode     builder: the 33 bytes of X_t, zero bytes for a refused sum
//   k_rp_exkeys_challenge  verifier: the key lifted, the verdict that needs no equation, and c_t over the canonical bytes of the lifted key
//   k_rp_exsums_validate   key_start non-decreasing from 0 to nkeys, before anything reads through it: the first offending position
//   k_rp_exsums_lift       the keys into the pool's tail; a key without a point marks its sum and leaves a point that is never looked at
//   k_rp_exsums_start      merged_start[t] = sum_start[t] + key_start[t]
//   k_rp_exsums_merge      one lane per merged position: the entry or the key that stands there
//   k_rp_exsums_judge      BAD_KEY over the tally's verdict of a sum, under MALFORMED
// The signature's own kernels (k_rp_excess_sigs, k_rp_excess_mulcheck, k_rp_excess_weights) are those of csrc/rpexcess.hip, as they are.
// Every kernel is bounds-checked on its own index, takes its loop bounds from validated arrays only, reads the 33- and 65-byte rows bytewise
// and writes with ordinary vector stores.
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
#include "rpexcess_shared.hip.h"
#include "sha256.hip.h"

namespace bppp {

static constexpr uint32_t EXK_NONE = 0xFFFFFFFFu;
static constexpr uint32_t EXK_SUBTRACT = 0x80000000u;

// ---- builder.  in_sc [n][3][8]: the scalars of X_t = e_t B on base `slot`, zero for a refused sum
__global__ void __launch_bounds__(64) k_rp_exkeys_blinds(uint32_t n, uint32_t slot, const uint32_t *__restrict__ blinds, uint32_t *__restrict__ in_sc,
                                                         uint32_t *__restrict__ status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const fe e = fe_load(blinds + (size_t)t * 8);
  const uint32_t st = !wi_canonical(e) ? (uint32_t)BPPP_RP_EXCESS_NOT_CANONICAL : fe_is_zero(e) ? (uint32_t)BPPP_RP_EXCESS_ZERO : (uint32_t)BPPP_RP_EXCESS_OK;
  for (uint32_t b = 0; b < 3; b++) fe_store(in_sc + ((size_t)t * 3 + b) * 8, (st == BPPP_RP_EXCESS_OK && b == slot) ? e : fe_zero());
  status[t] = st;
}
__global__ void __launch_bounds__(64) k_rp_exkeys_encode(uint32_t n, const uint32_t *__restrict__ pts, const uint32_t *__restrict__ status, uint8_t *__restrict__ keys) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint8_t *key = keys + (size_t)t * EX_KEY;
  const bool ok = status[t] == BPPP_RP_EXCESS_OK;
  for (uint32_t o = 0; o < EX_KEY; o++) key[o] = ok ? (uint8_t)ex_pt_byte(pts + (size_t)t * 16, o) : (uint8_t)0;
}

// ---- verifier.  bits[t] as k_rp_excess_sigs leaves them.  X [n][16]: the lifted key; the first verdict that applies, in the header's order;
// EX_EVAL and the challenge where the equation has to decide
__global__ void __launch_bounds__(64) k_rp_exkeys_challenge(uint32_t n, ExDomain dc, const uint8_t *__restrict__ keys, const uint8_t *__restrict__ sigs,
                                                            const uint8_t *__restrict__ msgs, const uint32_t *__restrict__ bits, uint32_t *__restrict__ X,
                                                            uint32_t *__restrict__ c, uint32_t *__restrict__ pre) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  aff P;
  const bool key_ok = exk_lift(keys + (size_t)t * EX_KEY, P);
  uint32_t x[16];
  aff_store(x, P);
  const uint32_t st = !key_ok          ? (uint32_t)BPPP_RP_EXCESS_BAD_KEY
                      : (bits[t] & 1u) ? (uint32_t)BPPP_RP_OPEN_NOT_CANONICAL
                      : (bits[t] & 2u) ? (uint32_t)BPPP_RP_EXCESS_BAD_R
                                       : EX_EVAL;
  fe ch = fe_zero();
  if (st == EX_EVAL) {
    const uint8_t *sig = sigs + (size_t)t * EX_SIG;
    ch = ex_challenge(dc, [&](uint32_t o) -> uint32_t { return sig[o]; }, x, msgs + (size_t)t * EX_MSG);
  }
  for (int k = 0; k < 16; k++) X[(size_t)t * 16 + k] = x[k];
  fe_store(c + (size_t)t * 8, ch);
  pre[t] = st;
}

// ---- sums.  flag[0] = the lowest position whose key_start breaks "non-decreasing from 0 to nkeys"; it starts as EXK_NONE.  The bounds nsums and
// nkeys are the caller's arguments, never device data.
__global__ void __launch_bounds__(256) k_rp_exsums_validate(uint32_t nsums, uint32_t nkeys, const uint32_t *__restrict__ key_start, uint32_t *__restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= nsums; i += (uint64_t)gridDim.x * 256) {
    const uint32_t s = key_start[i];
    if ((i == 0 && s != 0) || (i == nsums && s != nkeys) || (i > 0 && s < key_start[i - 1])) atomicMin(flag, (uint32_t)i);
  }
}
// tail [nkeys][16]: the lifted keys behind the decoded pool.  A key without a point raises keybad of its sum (the last t < nsums with
// key_start[t] <= k: validated, at most 32 steps) and any[0], and leaves `filler` (a curve point) in its place: the tally's stage then still tells
// a commitment without a point (MALFORMED, which wins) from it, and the sum's verdict is taken before its point is looked at.
__global__ void __launch_bounds__(64) k_rp_exsums_lift(uint32_t nkeys, uint32_t nsums, const uint8_t *__restrict__ keys, const uint32_t *__restrict__ key_start,
                                                       const uint32_t *__restrict__ filler, uint32_t *__restrict__ tail, uint32_t *__restrict__ keybad,
                                                       uint32_t *__restrict__ any) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  aff P;
  if (exk_lift(keys + (size_t)k * EX_KEY, P)) { aff_store(tail + (size_t)k * 16, P); return; }
  for (int w = 0; w < 16; w++) tail[(size_t)k * 16 + w] = filler[w];
  uint32_t lo = 0, hi = nsums - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (key_start[mid] <= k) lo = mid; else hi = mid - 1;
  }
  keybad[lo] = 1u;                                      // every lane that stores here stores the same word
  any[0] = 1u;
}
__global__ void __launch_bounds__(256) k_rp_exsums_start(uint32_t nsums, const uint32_t *__restrict__ start, const uint32_t *__restrict__ key_start, uint32_t *__restrict__ m_start) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t <= nsums) m_start[t] = start[t] + key_start[t];
}
// merged position p lies in the last sum t < nsums with m_start[t] <= p: first the sum's entries as they are, then its keys, each subtracted from
// the point at total + k
__global__ void __launch_bounds__(256) k_rp_exsums_merge(uint32_t n, uint32_t nsums, uint32_t total, const uint32_t *__restrict__ start, const uint32_t *__restrict__ key_start,
                                                         const uint32_t *__restrict__ m_start, const uint32_t *__restrict__ entries, uint32_t *__restrict__ m_entries) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  uint32_t lo = 0, hi = nsums - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (m_start[mid] <= p) lo = mid; else hi = mid - 1;
  }
  const uint32_t o = p - m_start[lo], ne = start[lo + 1] - start[lo];
  m_entries[p] = o < ne ? entries[start[lo] + o] : ((total + key_start[lo] + (o - ne)) | EXK_SUBTRACT);
}
// after k_rp_tally_compare: a sum with a key that has no point is BAD_KEY unless it is MALFORMED, and has no point to report
__global__ void __launch_bounds__(256) k_rp_exsums_judge(uint32_t n, const uint32_t *__restrict__ keybad, uint32_t *__restrict__ status, uint32_t *__restrict__ zz) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n || !keybad[t]) return;
  if (status[t] != BPPP_RP_OPEN_MALFORMED) status[t] = BPPP_RP_EXCESS_BAD_KEY;
  if (zz) fe_store(zz + (size_t)t * 8, fe_zero());
}

}  // namespace bppp

using namespace bppp;
using namespace bppp::tally;
using namespace bppp::excess;
using namespace bppp::exkeys;

namespace {

const char *key_status_text(uint32_t s) {
  return s == BPPP_RP_EXCESS_NOT_CANONICAL ? "the blinding sum is not canonical (>= n)"
                                           : "the blinding sum is zero: the excess is the point at infinity and has no encoding";
}

// ---- the builder's keys
int keys_device(bppp_rp *rp, size_t nsums, const void *d_blinds, void *d_keys, uint32_t *key_status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  if (!d_blinds || !d_keys) return fail(ctx, BPPP_ERR_ARG, "rp_excess_keys: null input");
  if (nsums > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, "rp_excess_keys: nsums must be below 2^31");
  hipSetDevice(ctx->device);
  int rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const size_t C = keys_chunk(rp, nsums);
  uint32_t *in_sc = nullptr, *pts = nullptr, *status = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    in_sc = cv.take<uint32_t>(C * 24); pts = cv.take<uint32_t>(C * 16); status = cv.take<uint32_t>(C);
    if (!pass && (rc = rpp_ensure_pwork(rp, cv.off))) return rc;
  }
  hipStream_t st = ctx->stream;
  const uint32_t slot = blind_slot(rp);
  std::vector<uint32_t> h_status(nsums);
  for (size_t o = 0; o < nsums; o += C) {
    const size_t n = std::min(C, nsums - o);
    const dim3 grid((unsigned)((n + 63) / 64));
    k_rp_exkeys_blinds<<<grid, dim3(64), 0, st>>>((uint32_t)n, slot, (const uint32_t *)d_blinds + o * 8, in_sc, status);
    BPPP_HIP(ctx, hipGetLastError());
    if ((rc = rpp_commit_inputs(rp, in_sc, n, pts))) return rc;
    k_rp_exkeys_encode<<<grid, dim3(64), 0, st>>>((uint32_t)n, pts, status, (uint8_t *)d_keys + o * EX_KEY);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(h_status.data() + o, status, n * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return rpp_report_refusals(ctx, "rp_excess_keys", "sum", h_status.data(), nsums, key_status, key_status_text);
}

// the workspace of a pass of the signatures against stated keys (KeyWork: csrc/rpexcess_shared.hip.h)
int key_carve(bppp_rp *rp, size_t C, bool batch, KeyWork &W) {
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    W.sp = cv.take<uint32_t>(C * 24); W.P = cv.take<uint32_t>(batch ? 0 : C * 16); W.R = cv.take<uint32_t>(C * 16); W.X = cv.take<uint32_t>(C * 16);
    W.bits = cv.take<uint32_t>(C); W.pre = cv.take<uint32_t>(C); W.c = cv.take<uint32_t>(C * 8); W.status = cv.take<uint32_t>(batch ? 0 : C); W.any = cv.take<uint32_t>(4);
    W.prods = cv.take<uint32_t>(batch ? C * 24 : 0); W.red = cv.take<uint32_t>(batch ? (size_t)RPP_REDUCE_BLOCKS * 24 : 0); W.sc3 = cv.take<uint32_t>(24);
    W.msm_sc = cv.take<uint32_t>(batch ? (2 * C + 1) * 8 : 0); W.msm_pt = cv.take<uint32_t>(batch ? (2 * C + 1) * 16 : 0); W.seed = cv.take<uint8_t>(32);
    if (!pass) { int rc = rpp_ensure_pwork(rp, cv.off); if (rc) return rc; }
  }
  return BPPP_OK;
}

// what the sums against stated keys keep behind the tally's workspace (SumsJob: csrc/rpexcess_shared.hip.h)
struct SumsExtra { uint32_t *m_start, *m_entries, *keybad, *any; };
size_t sums_carve(uint8_t *base, const SumsJob &S, SumsExtra &X) {
  Carver cv(base, 0);
  X.m_start = cv.take<uint32_t>(S.J.nsums + 1); X.m_entries = cv.take<uint32_t>(S.nnz + S.nkeys); X.keybad = cv.take<uint32_t>(S.J.nsums); X.any = cv.take<uint32_t>(4);
  return cv.off;
}

}  // namespace

// ---- what the block call (csrc/rpblock.hip) shares with the entry points below, declared in csrc/rpexcess_shared.hip.h
namespace bppp {
namespace exkeys {

// ---- signatures against stated keys: no pool, no sum stage, no inversion (KeyJob, KeyWork: csrc/rpexcess_shared.hip.h)
int key_checks(KeyJob &K, bppp_rp *rp, const char *who, size_t nkeys, const void *keys, const void *msgs, const void *sigs, bool null_args) {
  bppp_ctx *ctx = rp->ctx;
  if (nkeys > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, std::string(who) + ": nkeys must be below 2^31");
  if (null_args || !keys || !msgs || !sigs) return fail(ctx, BPPP_ERR_ARG, std::string(who) + ": null input");
  K.rp = rp; K.nkeys = nkeys; K.keys = (const uint8_t *)keys; K.msgs = (const uint8_t *)msgs; K.sigs = (const uint8_t *)sigs;
  hipSetDevice(ctx->device);
  return BPPP_OK;
}
// keys [o, o + n) up to the verdict that needs no equation: W.X the lifted keys, W.R, W.c, W.pre and W.sp, the scalars of s B
int key_stage(const KeyJob &K, const KeyWork &W, size_t o, size_t n, const ExDomain &dc) {
  bppp_ctx *ctx = K.rp->ctx;
  int rc;
  if ((rc = sigs_launch(ctx, n, blind_slot(K.rp), K.sigs + o * EX_SIG, W.sp, W.R, W.bits))) return rc;
  k_rp_exkeys_challenge<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>((uint32_t)n, dc, K.keys + o * EX_KEY, K.sigs + o * EX_SIG, K.msgs + o * EX_MSG, W.bits,
                                                                                       W.X, W.c, W.pre);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

int verify_keys_each_pass(const KeyJob &K, uint32_t *status) {
  bppp_rp *rp = K.rp;
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  int rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const size_t C = keys_chunk(rp, K.nkeys);
  KeyWork W;
  if ((rc = key_carve(rp, C, false, W))) return rc;
  const ExDomain dc = challenge_domain(rp);
  for (size_t o = 0; o < K.nkeys; o += C) {
    const size_t n = std::min(C, K.nkeys - o);
    if ((rc = key_stage(K, W, o, n, dc)) || (rc = rpp_commit_inputs(rp, W.sp, n, W.P)) || (rc = mulcheck_launch(ctx, n, W.c, W.X, W.P, W.R, W.pre, W.status))) return rc;
    BPPP_HIP(ctx, hipMemcpyAsync(status + o, W.status, n * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return BPPP_OK;
}


// ---- sums against stated keys: the tally's two passes over the pool with the keys behind it and the merged CSR (SumsJob: csrc/rpexcess_shared.hip.h)
// the argument checks of both calls: the sizes before anything is read, the tally's own checks over the caller's CSR and claims, then key_start by a
// kernel whose verdict is read back before anything reads through it
int sums_checks(SumsJob &S, bppp_rp *rp, const char *who, size_t rows, const void *coms, size_t nsums, const void *start, const void *entries, size_t nnz, const void *amt,
                const void *ty, const void *off, size_t nkeys, const void *key_start, const void *keys, bool null_args) {
  bppp_ctx *ctx = rp->ctx;
  const std::string w = who;
  const size_t nr = rp->D.nr;
  if (!nr || rows > RPP_LIM31 / nr || nkeys > RPP_LIM31 || rows * nr + nkeys > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, w + ": rows * nranges + nkeys must be below 2^31");
  if (nnz > RPP_LIM31 || nnz + nkeys > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, w + ": nnz + nkeys must be below 2^31");
  Job &J = S.J;
  fill(J, rp, who, rows, coms, nsums, start, entries, nnz, amt, ty, off);
  J.bl_name = "claim_offsets";
  S.nkeys = nkeys; S.nnz = nnz; S.keys = (const uint8_t *)keys; S.key_start = (const uint32_t *)key_start;
  int rc = tally_checks(J, null_args || (rows && !coms) || !key_start || (nkeys && !keys), true); if (rc) return rc;
  uint32_t *flag = (uint32_t *)rp->pwork, h = EXK_NONE;          // tally_checks made sure of 256 bytes
  hipStream_t st = ctx->stream;
  BPPP_HIP(ctx, hipMemsetAsync(flag, 0xFF, 4, st));
  k_rp_exsums_validate<<<dim3((unsigned)std::min<size_t>((nsums + 256) / 256, 4096)), dim3(256), 0, st>>>((uint32_t)nsums, (uint32_t)nkeys, S.key_start, flag);
  BPPP_HIP(ctx, hipGetLastError());
  BPPP_HIP(ctx, hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  if (h != EXK_NONE) {                          // h <= nsums: one word of an array of nsums + 1
    uint32_t v = 0;
    BPPP_HIP(ctx, hipMemcpy(&v, S.key_start + h, 4, hipMemcpyDeviceToHost));
    return fail(ctx, BPPP_ERR_ARG, w + ": key_start[" + std::to_string(h) + "] = " + std::to_string(v) + " is not non-decreasing from 0 to nkeys = " + std::to_string(nkeys));
  }
  std::vector<uint32_t> h_kstart(nsums + 1);
  BPPP_HIP(ctx, hipMemcpy(h_kstart.data(), S.key_start, (nsums + 1) * 4, hipMemcpyDeviceToHost));
  for (size_t t = 0; t <= nsums; t++) J.h_start[t] += h_kstart[t];       // the merged sum_start, mirrored: below 2^31 by the size check
  J.nnz = nnz + nkeys;
  J.tail = nkeys;
  return BPPP_OK;
}

Ext sums_ext(const SumsJob &S) {
  SumsExtra X0;
  Ext E;
  E.extra = sums_carve(nullptr, S, X0);
  const SumsJob *Sp = &S;
  E.prepare = [Sp](Job &J, const Work &W) -> int {
    const SumsJob &S = *Sp;
    bppp_rp *rp = J.rp;
    bppp_ctx *ctx = rp->ctx;
    hipStream_t st = ctx->stream;
    SumsExtra X;
    sums_carve(W.extra, S, X);
    const size_t total = J.rows * rp->D.nr, n = S.nnz + S.nkeys, nsums = J.nsums;
    BPPP_HIP(ctx, hipMemsetAsync(X.keybad, 0, nsums * 4, st));
    BPPP_HIP(ctx, hipMemsetAsync(X.any, 0, 16, st));
    if (S.nkeys) k_rp_exsums_lift<<<dim3((unsigned)((S.nkeys + 63) / 64)), dim3(64), 0, st>>>((uint32_t)S.nkeys, (uint32_t)nsums, S.keys, S.key_start, rp->d_basis, W.pool + total * 16,
                                                                                             X.keybad, X.any);
    k_rp_exsums_start<<<dim3((unsigned)((nsums + 256) / 256)), dim3(256), 0, st>>>((uint32_t)nsums, S.J.start, S.key_start, X.m_start);
    if (n) k_rp_exsums_merge<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>((uint32_t)n, (uint32_t)nsums, (uint32_t)total, S.J.start, S.key_start, X.m_start, S.J.entries,
                                                                                    X.m_entries);
    BPPP_HIP(ctx, hipGetLastError());
    J.start = X.m_start; J.entries = X.m_entries;
    return BPPP_OK;
  };
  E.judge = [Sp](const Work &W, size_t t0, size_t ns, bool zz) -> int {
    bppp_ctx *ctx = Sp->J.rp->ctx;
    SumsExtra X;
    sums_carve(W.extra, *Sp, X);
    k_rp_exsums_judge<<<dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, ctx->stream>>>((uint32_t)ns, X.keybad + t0, W.status, zz ? W.zz : nullptr);
    BPPP_HIP(ctx, hipGetLastError());
    return BPPP_OK;
  };
  E.rejects = [Sp](const Work &W, bool &reject) -> int {
    bppp_ctx *ctx = Sp->J.rp->ctx;
    SumsExtra X;
    sums_carve(W.extra, *Sp, X);
    uint32_t any = 0;
    BPPP_HIP(ctx, hipMemcpy(&any, X.any, 4, hipMemcpyDeviceToHost));
    reject = any != 0;
    return BPPP_OK;
  };
  return E;
}

}  // namespace exkeys
}  // namespace bppp

namespace {

int verify_keys_each_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_sigs, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (!nkeys) return BPPP_OK;
  KeyJob K;
  int rc = key_checks(K, rp, "rp_excess_verify_keys_each", nkeys, d_keys, d_msgs, d_sigs, !status);
  return rc ? rc : verify_keys_each_pass(K, status);
}

int verify_keys_batch_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_sigs, uint64_t index_offset, const uint8_t seed[32], int *accept,
                             uint32_t *status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  if (!nkeys) { if (combined_xy) memset(combined_xy, 0, 64); *accept = 1; return BPPP_OK; }
  KeyJob K;
  int rc = key_checks(K, rp, "rp_excess_verify_keys_batch", nkeys, d_keys, d_msgs, d_sigs, !seed); if (rc) return rc;
  if (combined_xy) memset(combined_xy, 0, 64);
  hipStream_t st = ctx->stream;
  const size_t C = keys_chunk(rp, nkeys);
  KeyWork W;
  if ((rc = key_carve(rp, C, true, W))) return rc;
  const ExDomain dc = challenge_domain(rp);
  BPPP_HIP(ctx, hipMemcpyAsync(W.seed, seed, 32, hipMemcpyHostToDevice, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.any, 0, 16, st));
  BatchParts parts;                             // one combined point per pass
  for (size_t o = 0; o < nkeys; o += C) {
    const size_t n = std::min(C, nkeys - o);
    if ((rc = key_stage(K, W, o, n, dc))) return rc;
    if ((rc = batch_chunk(rp, n, index_offset + o, W.seed, K.sigs + o * EX_SIG, W.X, K.msgs + o * EX_MSG, W.pre, W.c, W.sp, W.R, W.prods, W.red, W.sc3, W.msm_sc, W.msm_pt, W.any,
                          parts))) return rc;
  }
  uint32_t any = 0;
  BPPP_HIP(ctx, hipMemcpy(&any, W.any, 4, hipMemcpyDeviceToHost));
  if ((rc = parts.finish(ctx, any != 0, combined_xy, accept))) return rc;
  if (!status) return BPPP_OK;
  if (*accept) { memset(status, 0, nkeys * 4); return BPPP_OK; }
  return verify_keys_each_pass(K, status);      // one exact pass, whatever the number of bad signatures
}

int sums_each_device(bppp_rp *rp, size_t rows, const void *d_coms, size_t nsums, const void *d_start, const void *d_entries, size_t nnz, const void *d_amt, const void *d_ty,
                     const void *d_off, size_t nkeys, const void *d_key_start, const void *d_keys, uint32_t *status, uint64_t *sums_xy) {
  if (!rp) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  SumsJob S;
  int rc = sums_checks(S, rp, "rp_excess_sums_each", rows, d_coms, nsums, d_start, d_entries, nnz, d_amt, d_ty, d_off, nkeys, d_key_start, d_keys, !status); if (rc) return rc;
  const Ext E = sums_ext(S);
  return each_pass(S.J, status, sums_xy, &E);
}

int sums_batch_device(bppp_rp *rp, size_t rows, const void *d_coms, size_t nsums, const void *d_start, const void *d_entries, size_t nnz, const void *d_amt, const void *d_ty,
                      const void *d_off, size_t nkeys, const void *d_key_start, const void *d_keys, uint64_t index_offset, const uint8_t seed[32], int *accept, uint32_t *status,
                      uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  if (!nsums) { if (combined_xy) memset(combined_xy, 0, 64); *accept = 1; return BPPP_OK; }
  SumsJob S;
  int rc = sums_checks(S, rp, "rp_excess_sums_batch", rows, d_coms, nsums, d_start, d_entries, nnz, d_amt, d_ty, d_off, nkeys, d_key_start, d_keys, !seed); if (rc) return rc;
  const Ext E = sums_ext(S);
  return batch_run(S.J, index_offset, seed, accept, status, combined_xy, &E);
}

// ---- host variants: upload, the _device variant, download
struct HostKeys {
  DevBuf keys, msgs, sigs;
  int up(bppp_rp *rp, size_t nkeys, const uint8_t *k, const uint8_t *m, const uint8_t *s) {
    bppp_ctx *ctx = rp->ctx;
    if (nkeys > RPP_LIM31) return BPPP_OK;     // the _device variant refuses this size before it reads anything
    hipSetDevice(ctx->device);
    int rc = keys.up(ctx, k, nkeys * EX_KEY);
    if (!rc) rc = msgs.up(ctx, m, nkeys * EX_MSG);
    if (!rc) rc = sigs.up(ctx, s, nkeys * EX_SIG);
    return rc;
  }
};
// the tally's arrays (the third claim: the offsets) and the keys of the sums
struct HostSums : HostCsr {
  DevBuf kstart, keys;
  int up(bppp_rp *rp, size_t rows, const void *h_coms, size_t nsums, const uint32_t *sum_start, const uint32_t *ent, size_t nnz, const uint64_t *ca, const uint64_t *cty,
         const uint64_t *co, size_t nkeys, const uint32_t *key_start, const uint8_t *k) {
    if (!rpp_sizes_ok(rp, rows, nsums, nnz, nkeys)) return BPPP_OK;
    int rc = HostCsr::up(rp, rows, h_coms, rp->D.coms_bytes, nsums, sum_start, ent, nnz, ca, cty, co, nsums * 32);
    if (!rc) rc = kstart.up(rp->ctx, key_start, (nsums + 1) * 4);
    if (!rc) rc = keys.up(rp->ctx, k, nkeys * EX_KEY);
    return rc;
  }
};

}  // namespace

extern "C" {

int bppp_rp_excess_keys_device(bppp_rp *rp, size_t nsums, const void *d_claim_blinds, void *d_keys, uint32_t *key_status) {
  return keys_device(rp, nsums, d_claim_blinds, d_keys, key_status);
}

int bppp_rp_excess_keys(bppp_rp *rp, size_t nsums, const uint64_t *claim_blinds, uint8_t *keys, uint32_t *key_status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  DevBuf bl, k;
  if (nsums <= RPP_LIM31) {
    hipSetDevice(ctx->device);
    int rc = bl.up(ctx, claim_blinds, nsums * 32);
    if (!rc) rc = k.out(ctx, keys, nsums * EX_KEY);
    if (rc) return rc;
  }
  int rc = keys_device(rp, nsums, bl.p, k.p, key_status);
  return rpp_download_refused(ctx, rc, "rp_excess_keys: sum ", keys, k.p, nsums * EX_KEY);
}

int bppp_rp_excess_verify_keys_each_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_sigs, uint32_t *status) {
  return verify_keys_each_device(rp, nkeys, d_keys, d_msgs, d_sigs, status);
}

int bppp_rp_excess_verify_keys_each(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *sigs, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (!nkeys) return BPPP_OK;
  HostKeys H;
  int rc = H.up(rp, nkeys, keys, msgs, sigs);
  if (rc) return rc;
  return verify_keys_each_device(rp, nkeys, H.keys.p, H.msgs.p, H.sigs.p, status);
}

int bppp_rp_excess_verify_keys_batch_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_sigs, uint64_t index_offset, const uint8_t seed[32],
                                            int *accept, uint32_t *status, uint64_t *combined_xy) {
  return verify_keys_batch_device(rp, nkeys, d_keys, d_msgs, d_sigs, index_offset, seed, accept, status, combined_xy);
}

int bppp_rp_excess_verify_keys_batch(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *sigs, const uint8_t seed[32], int *accept,
                                     uint32_t *status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  HostKeys H;
  if (nkeys) {
    int rc = H.up(rp, nkeys, keys, msgs, sigs);
    if (rc) return rc;
  }
  return verify_keys_batch_device(rp, nkeys, H.keys.p, H.msgs.p, H.sigs.p, 0, seed, accept, status, combined_xy);
}

int bppp_rp_excess_sums_each_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                                    const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_offsets, size_t nkeys, const void *d_key_start, const void *d_keys,
                                    uint32_t *status, uint64_t *sums_xy) {
  return sums_each_device(rp, rows, d_coms_files, nsums, d_sum_start, d_entries, nnz, d_claim_amounts, d_claim_types, d_claim_offsets, nkeys, d_key_start, d_keys, status, sums_xy);
}

int bppp_rp_excess_sums_each(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                             const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_offsets, size_t nkeys, const uint32_t *key_start,
                             const uint8_t *keys, uint32_t *status, uint64_t *sums_xy) {
  if (!rp) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  HostSums H;
  int rc = H.up(rp, rows, coms_files, nsums, sum_start, entries, nnz, claim_amounts, claim_types, claim_offsets, nkeys, key_start, keys);
  if (rc) return rc;
  return sums_each_device(rp, rows, H.coms.p, nsums, H.start.p, H.entries.p, nnz, H.a.p, H.ty.p, H.e.p, nkeys, H.kstart.p, H.keys.p, status, sums_xy);
}

int bppp_rp_excess_sums_batch_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                                     const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_offsets, size_t nkeys, const void *d_key_start,
                                     const void *d_keys, uint64_t index_offset, const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy) {
  return sums_batch_device(rp, rows, d_coms_files, nsums, d_sum_start, d_entries, nnz, d_claim_amounts, d_claim_types, d_claim_offsets, nkeys, d_key_start, d_keys, index_offset,
                           seed, accept, status, combined_xy);
}

int bppp_rp_excess_sums_batch(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                              const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_offsets, size_t nkeys, const uint32_t *key_start,
                              const uint8_t *keys, const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  HostSums H;
  if (nsums) {
    int rc = H.up(rp, rows, coms_files, nsums, sum_start, entries, nnz, claim_amounts, claim_types, claim_offsets, nkeys, key_start, keys);
    if (rc) return rc;
  }
  return sums_batch_device(rp, rows, H.coms.p, nsums, H.start.p, H.entries.p, nnz, H.a.p, H.ty.p, H.e.p, nkeys, H.kstart.p, H.keys.p, 0, seed, accept, status, combined_xy);
}

}  // extern "C"
