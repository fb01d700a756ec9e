// rpexagg.hip — half-aggregate excess signatures: bppp_rp_excess_halfagg*, bppp_rp_excess_halfagg_verify* (include/bppp.h states every message),
// and what bppp_rp_verify_block_agg (csrc/rpblock.hip) takes from here through csrc/rpexagg.hip.h.
//   aggregate  the n rows of R as the signatures hold them, then put (s_agg), s_agg = sum z_i s_i
//   z_i        decode (SHA-256 (Dz || root || le64 (n) || le64 (i))) mod n, 1 for 0; root: the SHA-256 tree over leaf_i = SHA-256 (Dl || R_i ||
//              the canonical 33 bytes of X_i || msg_i), so every z_i is fixed by the whole job
//   equation   s_agg B - sum z_i (c_i X_i + R_i) = identity, one MSM per pass of keys_chunk keys; s_agg B is term 2n of the FIRST pass alone
// The leaves of the whole job are hashed before any pass (the canonical key bytes need no square root), then the tree, then the passes run as
// those of bppp_rp_excess_verify_keys_batch: exkeys::key_stage over the R rows widened to 65-byte signatures with s = 0 (the aggregator: over the
// signatures themselves), the weights here, BatchParts::msm.
// Kernels (one lane per key or per node unless said otherwise):
//   k_rp_exagg_leaf        three compressions a key; the digest as eight big-endian words
//   k_rp_exagg_tree        a workgroup reduces an aligned tile of TREE_TILE nodes through LDS to one; launches repeat until one node is left
//   k_rp_exagg_expand      R row -> row || put (0), the 65 bytes k_rp_excess_sigs and k_rp_exkeys_challenge read
//   k_rp_exagg_weights     z_i (times rho_A in the block call), the two MSM terms in k_rp_excess_weights' layout, the product column - z_i s_i
//   k_rp_exagg_sagg        one lane: the 32 bytes of s_agg -> a scalar and "s_agg >= n"
//   k_rp_exagg_rho         one lane: rho_A of the block call and rho_A s_agg
//   k_rp_exagg_accumulate  one lane: the column sum of a pass added to the job's
//   k_rp_exagg_encode      the R rows copied, put (s_agg) behind them
// Every kernel is bounds-checked on its own index, reads the 33- and 65-byte rows bytewise and writes with ordinary vector stores; there is no atomic.
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
#include "rpexagg.hip.h"
#include "sha256.hip.h"

namespace bppp {

using exagg::AGG_ROW;
using exagg::TREE_TILE;

// leaves [n][8].  The canonical bytes of the key: put (x mod p) and the sign byte as it stands — no lift, so a key without a point has a leaf too
// (its verdict is taken by the stage that lifts it)
__global__ void __launch_bounds__(64) k_rp_exagg_leaf(uint32_t n, ExDomain dl, const uint8_t *__restrict__ keys, const uint8_t *__restrict__ msgs,
                                                      const uint8_t *__restrict__ rrows, uint32_t rstride, uint32_t *__restrict__ leaves) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint8_t *key = keys + (size_t)t * EX_KEY, *r = rrows + (size_t)t * rstride, *msg = msgs + (size_t)t * EX_MSG;
  uint32_t xw[8], st[8];
  fe_store(xw, load_field_be<0>(key));
  const uint32_t sign = key[32];
  ex_digest<3>(32 + 33 + 33 + EX_MSG, [&](uint32_t k) -> uint32_t {
    if (k < 32) return ex_dom_byte(dl, k);
    if (k < 65) return r[k - 32];
    if (k < 97) return enc_be_byte(xw, k - 65);
    if (k < 98) return sign;
    return msg[k - 98];
  }, st);
  for (int q = 0; q < 8; q++) leaves[(size_t)t * 8 + q] = st[q];
}

// workgroup b: nodes [b TILE, (b + 1) TILE) of a level of `count` -> out[b], their subtree's top.  The tile is aligned to a power of two, so the
// pairs inside it are the pairs of the whole level, and a short last tile moves its odd nodes up as the definition says.  m, the nodes left, is
// the same in every lane: the barriers are uniform.
__global__ void __launch_bounds__(TREE_TILE) k_rp_exagg_tree(uint32_t count, ExDomain dn, const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
  __shared__ uint32_t lds[TREE_TILE * 8];
  const uint32_t base = blockIdx.x * TREE_TILE, j = threadIdx.x;
  if (base >= count) return;                            // the whole workgroup alike
  uint32_t m = count - base < TREE_TILE ? count - base : TREE_TILE;
  if (j < m) for (int q = 0; q < 8; q++) lds[j * 8 + q] = in[(size_t)(base + j) * 8 + q];
  __syncthreads();
  while (m > 1) {
    const uint32_t half = (m + 1) / 2;
    uint32_t st[8];
    if (j < half) {
      uint32_t a[8], b[8];
      for (int q = 0; q < 8; q++) a[q] = lds[2 * j * 8 + q];
      if (2 * j + 1 < m) {
        for (int q = 0; q < 8; q++) b[q] = lds[(2 * j + 1) * 8 + q];
        ex_digest<2>(96, [&](uint32_t k) -> uint32_t { return k < 32 ? ex_dom_byte(dn, k) : k < 64 ? ex_word_byte(a, k - 32) : ex_word_byte(b, k - 64); }, st);
      } else {
        for (int q = 0; q < 8; q++) st[q] = a[q];
      }
    }
    __syncthreads();
    if (j < half) for (int q = 0; q < 8; q++) lds[j * 8 + q] = st[q];
    __syncthreads();
    m = half;
  }
  if (j < 8) out[(size_t)blockIdx.x * 8 + j] = lds[j];
}

__global__ void __launch_bounds__(64) k_rp_exagg_expand(uint32_t n, const uint8_t *__restrict__ rrows, uint8_t *__restrict__ sigx) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint8_t *r = rrows + (size_t)t * AGG_ROW;
  uint8_t *sig = sigx + (size_t)t * EX_SIG;
  for (uint32_t o = 0; o < EX_SIG; o++) sig[o] = o < AGG_ROW ? r[o] : (uint8_t)0;
}

// key i0 + t of a job of ntotal; pre, c, in_sc, X, R as exkeys::key_stage left them.  w = z (rho NULL) or z rho[0].  Terms 2t and 2t + 1:  n - w c  on
// X,  n - w  on R; a key whose verdict is already taken puts in zero scalars and the infinity encoding and raises any[0].  prods [n][3][8]:  - z s  in
// column 0 (rpp_negated_column_sums negates the sum back), without rho.  (sc, pt) and prods may each be NULL.
__global__ void __launch_bounds__(64) k_rp_exagg_weights(uint32_t n, uint32_t slot, uint64_t i0, uint64_t ntotal, ExDomain dz, const uint32_t *__restrict__ root,
                                                         const uint32_t *__restrict__ rho, const uint32_t *__restrict__ X, const uint32_t *__restrict__ pre,
                                                         const uint32_t *__restrict__ c, const uint32_t *__restrict__ in_sc, const uint32_t *__restrict__ R,
                                                         uint32_t *__restrict__ prods, uint32_t *__restrict__ sc, uint32_t *__restrict__ pt, uint32_t *__restrict__ any) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const bool part = pre[t] == EX_EVAL;
  fe zs = fe_zero(), wc = fe_zero(), w1 = fe_zero();
  if (part) {
    const uint64_t i = i0 + t;
    uint32_t rt[8], st[8];
    for (int q = 0; q < 8; q++) rt[q] = root[q];
    ex_digest<2>(32 + 32 + 8 + 8, [&](uint32_t k) -> uint32_t {
      if (k < 32) return ex_dom_byte(dz, k);
      if (k < 64) return ex_word_byte(rt, k - 32);
      if (k < 72) return (uint32_t)(ntotal >> (8 * (k - 64)));
      return (uint32_t)(i >> (8 * (k - 72)));
    }, st);
    fe z = ex_digest_scalar(st);
    if (fe_is_zero(z)) z = fe_one();
    zs = fe_neg<1>(fe_mul<1>(z, fe_load(in_sc + ((size_t)t * 3 + slot) * 8)));
    const fe w = rho ? fe_mul<1>(z, fe_load(rho)) : z;
    wc = fe_neg<1>(fe_mul<1>(w, fe_load(c + (size_t)t * 8)));
    w1 = fe_neg<1>(w);
  } else any[0] = 1u;                                   // every lane that stores here stores the same word
  if (prods) { fe_store(prods + (size_t)t * 24, zs); fe_store(prods + (size_t)t * 24 + 8, fe_zero()); fe_store(prods + (size_t)t * 24 + 16, fe_zero()); }
  if (!sc) return;
  fe_store(sc + (size_t)t * 16, wc); fe_store(sc + (size_t)t * 16 + 8, w1);
  for (int k = 0; k < 16; k++) {
    pt[(size_t)t * 32 + k] = part ? X[(size_t)t * 16 + k] : 0u;
    pt[(size_t)t * 32 + 16 + k] = part ? R[(size_t)t * 16 + k] : 0u;
  }
}

// sagg [8]: s_agg, zero when the 32 bytes hold no scalar; flag[0]: they hold none
__global__ void __launch_bounds__(64) k_rp_exagg_sagg(const uint8_t *__restrict__ s32, uint32_t *__restrict__ sagg, uint32_t *__restrict__ flag) {
  if (blockIdx.x || threadIdx.x) return;
  const fe s = load_field_be_raw(s32);
  const bool bad = !wi_canonical(s);
  fe_store(sagg, bad ? fe_zero() : s);
  flag[0] = bad ? 1u : 0u;
}
// rho [2][8]: rho_A = decode (SHA-256 (seed || le64 (ntotal) || root || the 32 bytes as they stand)) mod n, 1 for 0: 104 bytes; then rho_A s_agg
__global__ void __launch_bounds__(64) k_rp_exagg_rho(const uint8_t *__restrict__ seed, uint64_t ntotal, const uint32_t *__restrict__ root, const uint8_t *__restrict__ s32,
                                                     const uint32_t *__restrict__ sagg, uint32_t *__restrict__ rho) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t rt[8], st[8];
  for (int q = 0; q < 8; q++) rt[q] = root[q];
  ex_digest<2>(32 + 8 + 32 + 32, [&](uint32_t k) -> uint32_t {
    if (k < 32) return seed[k];
    if (k < 40) return (uint32_t)(ntotal >> (8 * (k - 32)));
    if (k < 72) return ex_word_byte(rt, k - 40);
    return s32[k - 72];
  }, st);
  fe r = ex_digest_scalar(st);
  if (fe_is_zero(r)) r = fe_one();
  fe_store(rho, r);
  fe_store(rho + 8, fe_mul<1>(r, fe_load(sagg)));
}
// acc [8] = (first ? 0 : acc) + sc3 [0]: the job's sum z s over its passes
__global__ void __launch_bounds__(64) k_rp_exagg_accumulate(const uint32_t *__restrict__ sc3, uint32_t *__restrict__ acc, uint32_t first) {
  if (blockIdx.x || threadIdx.x) return;
  fe_store(acc, first ? fe_load(sc3) : fe_add<1>(fe_load(acc), fe_load(sc3)));
}
// lane t < n: row t of the aggregate, the first 33 bytes of signature t; lane n: put (s_agg) behind the rows
__global__ void __launch_bounds__(64) k_rp_exagg_encode(uint32_t n, const uint8_t *__restrict__ sigs, const uint32_t *__restrict__ acc, uint8_t *__restrict__ agg) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > n) return;
  uint8_t *out = agg + (size_t)t * AGG_ROW;
  if (t < n) {
    const uint8_t *sig = sigs + (size_t)t * EX_SIG;
    for (uint32_t o = 0; o < AGG_ROW; o++) out[o] = sig[o];
    return;
  }
  uint32_t sw[8];
  for (int q = 0; q < 8; q++) sw[q] = acc[q];
  for (uint32_t o = 0; o < 32; o++) out[o] = enc_be_byte(sw, o);
}

}  // namespace bppp

namespace bppp {
namespace exagg {

using namespace bppp::excess;
using namespace bppp::exkeys;

static size_t tiles(size_t n) { return (n + TREE_TILE - 1) / TREE_TILE; }

void agg_carve(Carver &cv, size_t nkeys, size_t chunk, AggWork &W) {
  W.leaves = cv.take<uint32_t>(nkeys * 8); W.lvl[0] = cv.take<uint32_t>(tiles(nkeys) * 8); W.lvl[1] = cv.take<uint32_t>(tiles(tiles(nkeys)) * 8);
  W.sagg = cv.take<uint32_t>(8); W.rho = cv.take<uint32_t>(16); W.flag = cv.take<uint32_t>(4); W.sigx = cv.take<uint8_t>(chunk * EX_SIG);
  W.root = nullptr;
}

int commit_tree(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *rrows, uint32_t rstride, AggWork &W) {
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  k_rp_exagg_leaf<<<dim3((unsigned)((nkeys + 63) / 64)), dim3(64), 0, st>>>((uint32_t)nkeys, domain("bppp/excess/halfagg/leaf/v1", rp->tag), keys, msgs, rrows, rstride, W.leaves);
  BPPP_HIP(ctx, hipGetLastError());
  const ExDomain dn = domain("bppp/excess/halfagg/node/v1", rp->tag);
  const uint32_t *cur = W.leaves;
  int s = 0;
  for (size_t count = nkeys; count > 1; count = tiles(count), s ^= 1) {      // level sizes: n, then ceil (n / 256), ...: lvl[s] holds tiles (count) nodes
    k_rp_exagg_tree<<<dim3((unsigned)tiles(count)), dim3(TREE_TILE), 0, st>>>((uint32_t)count, dn, cur, W.lvl[s]);
    BPPP_HIP(ctx, hipGetLastError());
    cur = W.lvl[s];
  }
  W.root = cur;
  return BPPP_OK;
}

int sagg_launch(bppp_ctx *ctx, const uint8_t *s32, const AggWork &W) {
  k_rp_exagg_sagg<<<dim3(1), dim3(64), 0, ctx->stream>>>(s32, W.sagg, W.flag);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}
int rho_launch(bppp_ctx *ctx, const uint8_t *d_seed, size_t nkeys, const uint8_t *s32, const AggWork &W) {
  k_rp_exagg_rho<<<dim3(1), dim3(64), 0, ctx->stream>>>(d_seed, (uint64_t)nkeys, W.root, s32, W.sagg, W.rho);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}
int expand_launch(bppp_ctx *ctx, size_t n, const uint8_t *rrows, uint8_t *sigx) {
  k_rp_exagg_expand<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>((uint32_t)n, rrows, sigx);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}
int weights_launch(bppp_rp *rp, size_t n, uint64_t i0, uint64_t ntotal, const uint32_t *root, const uint32_t *rho, const uint32_t *X, const uint32_t *pre, const uint32_t *c,
                   const uint32_t *sp, const uint32_t *R, uint32_t *prods, uint32_t *sc, uint32_t *pt, uint32_t *any) {
  bppp_ctx *ctx = rp->ctx;
  k_rp_exagg_weights<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>((uint32_t)n, blind_slot(rp), i0, ntotal, domain("bppp/excess/halfagg/coef/v1", rp->tag), root, rho, X,
                                                                                   pre, c, sp, R, prods, sc, pt, any);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

// the workspace of both calls, carved from rp->pwork: the job's tree, then a pass of C keys.  `terms`: the verifier's MSM input; else the aggregator's
// product column and its sums (acc: the job's sum z s)
struct PassWork { AggWork A; KeyWork K; uint32_t *acc; };
static int pass_carve(bppp_rp *rp, size_t nkeys, size_t C, bool terms, bool sigx, PassWork &W) {
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    agg_carve(cv, nkeys, sigx ? C : 0, W.A);
    KeyWork &K = W.K;
    K = KeyWork{};
    K.sp = cv.take<uint32_t>(C * 24); K.R = cv.take<uint32_t>(C * 16); K.X = cv.take<uint32_t>(C * 16); K.bits = cv.take<uint32_t>(C); K.pre = cv.take<uint32_t>(C);
    K.c = cv.take<uint32_t>(C * 8); K.any = cv.take<uint32_t>(4);
    K.prods = cv.take<uint32_t>(terms ? 0 : C * 24); K.red = cv.take<uint32_t>(terms ? 0 : (size_t)RPP_REDUCE_BLOCKS * 24); K.sc3 = cv.take<uint32_t>(24);
    K.msm_sc = cv.take<uint32_t>(terms ? (2 * C + 1) * 8 : 0); K.msm_pt = cv.take<uint32_t>(terms ? (2 * C + 1) * 16 : 0);
    W.acc = cv.take<uint32_t>(8);
    if (!pass) { int rc = rpp_ensure_pwork(rp, cv.off); if (rc) return rc; }
  }
  return BPPP_OK;
}

int verify_run(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *agg, int *accept, uint32_t *status, uint64_t *combined_xy) {
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  const size_t C = keys_chunk(rp, nkeys);
  PassWork W;
  int rc;
  if ((rc = pass_carve(rp, nkeys, C, true, true, W))) return rc;
  const ExDomain dc = challenge_domain(rp);
  const uint32_t slot = blind_slot(rp);
  BPPP_HIP(ctx, hipMemsetAsync(W.K.any, 0, 16, st));
  if ((rc = commit_tree(rp, nkeys, keys, msgs, agg, AGG_ROW, W.A)) || (rc = sagg_launch(ctx, agg + nkeys * AGG_ROW, W.A))) return rc;
  std::vector<uint32_t> h_pre(status ? nkeys : 0);
  BatchParts parts;                             // one combined point per pass
  for (size_t o = 0; o < nkeys; o += C) {
    const size_t n = std::min(C, nkeys - o), nt = 2 * n + (o ? 0 : 1);
    const KeyJob K{rp, n, keys + o * EX_KEY, msgs + o * EX_MSG, W.A.sigx};
    if ((rc = expand_launch(ctx, n, agg + o * AGG_ROW, W.A.sigx)) || (rc = key_stage(K, W.K, 0, n, dc))) return rc;
    if ((rc = weights_launch(rp, n, o, nkeys, W.A.root, nullptr, W.K.X, W.K.pre, W.K.c, W.K.sp, W.K.R, nullptr, W.K.msm_sc, W.K.msm_pt, W.K.any))) return rc;
    if (!o) {                                   // s_agg B: once for the job
      BPPP_HIP(ctx, hipMemcpyAsync(W.K.msm_sc + 2 * n * 8, W.A.sagg, 32, hipMemcpyDeviceToDevice, st));
      BPPP_HIP(ctx, hipMemcpyAsync(W.K.msm_pt + 2 * n * 16, rp->d_basis + 16 * slot, 64, hipMemcpyDeviceToDevice, st));
    }
    if (status) BPPP_HIP(ctx, hipMemcpyAsync(h_pre.data() + o, W.K.pre, n * 4, hipMemcpyDeviceToHost, st));
    if ((rc = parts.msm(ctx, W.K.msm_sc, W.K.msm_pt, nt))) return rc;
  }
  uint32_t any = 0, bad_s = 0;
  BPPP_HIP(ctx, hipMemcpy(&any, W.K.any, 4, hipMemcpyDeviceToHost));
  BPPP_HIP(ctx, hipMemcpy(&bad_s, W.A.flag, 4, hipMemcpyDeviceToHost));
  uint64_t xy[8];
  if ((rc = parts.finish(ctx, any != 0 || bad_s != 0, xy, accept))) return rc;
  if (combined_xy) memcpy(combined_xy, xy, 64);
  if (!status) return BPPP_OK;
  const uint32_t open = bad_s ? (uint32_t)BPPP_RP_OPEN_NOT_CANONICAL : rp_point_is_inf(xy) ? (uint32_t)BPPP_RP_OPEN_OK : (uint32_t)BPPP_RP_OPEN_MISMATCH;
  for (size_t k = 0; k < nkeys; k++) status[k] = h_pre[k] == EX_EVAL ? open : h_pre[k];
  return BPPP_OK;
}

}  // namespace exagg
}  // namespace bppp

using namespace bppp;
using namespace bppp::excess;
using namespace bppp::exkeys;
using namespace bppp::exagg;

namespace {

const char *agg_status_text(uint32_t s) {
  return s == BPPP_RP_EXCESS_BAD_KEY       ? "the key's sign byte is above 1, or its x has no curve point"
         : s == BPPP_RP_OPEN_NOT_CANONICAL ? "s is not canonical (>= n)"
                                           : "the sign byte of R is not 0 or 1, or R.x has no curve point";
}

int halfagg_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_sigs, void *d_agg, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nkeys) return BPPP_OK;
  KeyJob J;
  int rc = key_checks(J, rp, "rp_excess_halfagg", nkeys, d_keys, d_msgs, d_sigs, !d_agg); if (rc) return rc;
  hipStream_t st = ctx->stream;
  const size_t C = keys_chunk(rp, nkeys);
  PassWork W;
  if ((rc = pass_carve(rp, nkeys, C, false, false, W))) return rc;
  const ExDomain dc = challenge_domain(rp);
  BPPP_HIP(ctx, hipMemsetAsync(W.K.any, 0, 16, st));
  if ((rc = commit_tree(rp, nkeys, J.keys, J.msgs, J.sigs, EX_SIG, W.A))) return rc;
  std::vector<uint32_t> h_status(nkeys);
  for (size_t o = 0; o < nkeys; o += C) {
    const size_t n = std::min(C, nkeys - o);
    if ((rc = key_stage(J, W.K, o, n, dc))) return rc;
    if ((rc = weights_launch(rp, n, o, nkeys, W.A.root, nullptr, W.K.X, W.K.pre, W.K.c, W.K.sp, W.K.R, W.K.prods, nullptr, nullptr, W.K.any))) return rc;
    if ((rc = rpp_negated_column_sums(rp, n, W.K.prods, W.K.red, W.K.sc3))) return rc;
    k_rp_exagg_accumulate<<<dim3(1), dim3(64), 0, st>>>(W.K.sc3, W.acc, o ? 0u : 1u);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(h_status.data() + o, W.K.pre, n * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  bool refused = false;
  for (auto &s : h_status) { if (s == EX_EVAL) s = BPPP_RP_OPEN_OK; else refused = true; }
  const size_t bytes = BPPP_RP_EXCESS_AGG_BYTES(nkeys);
  if (refused) BPPP_HIP(ctx, hipMemsetAsync(d_agg, 0, bytes, st));
  else {
    k_rp_exagg_encode<<<dim3((unsigned)((nkeys + 64) / 64)), dim3(64), 0, st>>>((uint32_t)nkeys, J.sigs, W.acc, (uint8_t *)d_agg);
    BPPP_HIP(ctx, hipGetLastError());
  }
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  return rpp_report_refusals(ctx, "rp_excess_halfagg", "key", h_status.data(), nkeys, status, agg_status_text);
}

int halfagg_verify_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_agg, int *accept, uint32_t *status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  if (!nkeys) { if (combined_xy) memset(combined_xy, 0, 64); *accept = 1; return BPPP_OK; }
  KeyJob J;
  int rc = key_checks(J, rp, "rp_excess_halfagg_verify", nkeys, d_keys, d_msgs, d_agg, false); if (rc) return rc;
  if (combined_xy) memset(combined_xy, 0, 64);
  return verify_run(rp, nkeys, J.keys, J.msgs, (const uint8_t *)d_agg, accept, status, combined_xy);
}

// keys, messages and a third array of `third` bytes of a host call in HBM
struct HostAgg {
  DevBuf keys, msgs, third;
  int up(bppp_rp *rp, size_t nkeys, const uint8_t *k, const uint8_t *m, const uint8_t *t, size_t third_bytes) {
    bppp_ctx *ctx = rp->ctx;
    hipSetDevice(ctx->device);
    int rc = keys.up(ctx, k, nkeys * EX_KEY);
    if (!rc) rc = msgs.up(ctx, m, nkeys * EX_MSG);
    if (!rc) rc = third.up(ctx, t, third_bytes);
    return rc;
  }
};

}  // namespace

extern "C" {

int bppp_rp_excess_halfagg_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_sigs, void *d_agg, uint32_t *status) {
  return halfagg_device(rp, nkeys, d_keys, d_msgs, d_sigs, d_agg, status);
}

int bppp_rp_excess_halfagg(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *sigs, uint8_t *agg, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nkeys) return BPPP_OK;
  HostAgg H;
  DevBuf a;
  if (nkeys <= RPP_LIM31) {                     // the _device variant refuses a larger size before it reads anything
    int rc = H.up(rp, nkeys, keys, msgs, sigs, nkeys * EX_SIG);
    if (!rc) rc = a.out(ctx, agg, BPPP_RP_EXCESS_AGG_BYTES(nkeys));
    if (rc) return rc;
  }
  const int rc = halfagg_device(rp, nkeys, H.keys.p, H.msgs.p, H.third.p, a.p, status);
  return rpp_download_refused(ctx, rc, "rp_excess_halfagg: key ", agg, a.p, BPPP_RP_EXCESS_AGG_BYTES(nkeys));
}

int bppp_rp_excess_halfagg_verify_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_agg, int *accept, uint32_t *status,
                                         uint64_t *combined_xy) {
  return halfagg_verify_device(rp, nkeys, d_keys, d_msgs, d_agg, accept, status, combined_xy);
}

int bppp_rp_excess_halfagg_verify(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *agg, int *accept, uint32_t *status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  HostAgg H;
  if (nkeys && nkeys <= RPP_LIM31) {
    int rc = H.up(rp, nkeys, keys, msgs, agg, BPPP_RP_EXCESS_AGG_BYTES(nkeys));
    if (rc) return rc;
  }
  return halfagg_verify_device(rp, nkeys, H.keys.p, H.msgs.p, H.third.p, accept, status, combined_xy);
}

}  // extern "C"
