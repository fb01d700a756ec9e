// rpcommit.hip — input commitments outside the prover: bppp_rp_commit_batch*, bppp_rp_open_each*, bppp_rp_open_batch* (include/bppp.h),
// and the fixed-base window table of (g, H0, H1) that they share with the provers.
//
//   commit   scalarPairRPW' / com (src/RangeProof/Internal.hs:59-60): C = v g + ty H0 + bl H1 (RangeProof.Binary: v g + bl h0, scalarRPW'
//            :56-57), then encodeCommitments (src/Encoding.hs:130-134).  No witness is involved: any amount has a commitment.
//   open     decodeCommitments (Encoding.hs:119-128) by the verifier's decoders (csrc/rpdecode.hip.h through rp_decode_coms, csrc/rp.hip), the
//            same commitment recomputed from the claimed (amount, type, blinding), and either a comparison per commitment (open_each) or
//            one weighted combination for the whole batch (open_batch: one MSM over the decoded points, three reduced scalars on g, H0, H1).
// Kernels:
//   k_rp_commit_inputs  three-term commitments through the window table (the provers' kernel, moved here from csrc/rpprove.hip unchanged)
//   k_rp_claim_scalars  (amount, type, blinding) as given -> the three canonical scalars of a commitment in base order, a flag when the
//                       type or the blinding is not canonical
//   k_rp_encode_coms    affine commitments -> files: one workgroup per row, one lane per output byte
//   k_rp_open_compare   decoded point against recomputed point -> one status word per commitment
//   k_rp_open_weights   rho_j = decode (SHA-256 (the weight message of include/bppp.h)) and rho_j times the three scalars, one lane each
//   k_rp_open_reduce    the three product columns summed mod n: wavefront tree by cross-lane moves, one partial per workgroup through
//                       LDS, a last one-workgroup launch over the partials
// Every kernel is bounds-checked on its own index and writes with ordinary vector stores.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ec.hip.h"
#include "comb.hpp"
#include "rp_internal.hpp"
#include "rphostcall.hpp"
#include "rpprove_host.hpp"
#include "rpwords.hip.h"
#include "sha256.hip.h"

namespace bppp {

// ---- input commitments  v g + ty H0 + bl H1  (scalarPairRPW', src/RangeProof/Internal.hs:59-60) by fixed-base windows:
// table[base][w][d - 1] = d 16^w P_base (affine), 3 x 64 x 15 points; a commitment is at most 192 mixed additions, no doubling.
static constexpr int FB_BASES = 3, FB_WIN = 64, FB_DIG = 15;
__global__ void __launch_bounds__(64) k_rp_commit_inputs(const uint32_t *__restrict__ table, const uint32_t *__restrict__ sc, uint64_t n,
                                                         uint32_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  xyzz acc = xyzz_inf();
  for (int base = 0; base < FB_BASES; base++) {
    const fe s = fe_load(sc + (i * FB_BASES + base) * 8);
    if (fe_is_zero(s)) continue;
#pragma unroll 1
    for (int w = 0; w < FB_WIN; w++) {
      uint32_t limb = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) if ((w >> 3) == k) limb = s.v[k];
      const uint32_t d = (limb >> (4 * (w & 7))) & 15u;
      if (d) xyzz_madd(acc, aff_load(table + ((size_t)(base * FB_WIN + w) * FB_DIG + (d - 1)) * 16));
    }
  }
  aff_store(out + i * 16, xyzz_to_aff(acc));
}

// ---- the claimed (amount, type, blinding) of commitment i -> in_sc[i][3][8], the scalars on (g, H0, H1): typed (v mod n, ty, bl), binary
// (v mod n, bl, 0) — what the witness kernels hand the provers (csrc/rpwitness.hip.h).  A type or blinding >= n sets flag[i] and any[0]
// and leaves zero scalars behind, so nothing downstream ever walks a table with a digit of a value it was not built for.
__global__ void __launch_bounds__(256) k_rp_claim_scalars(uint64_t n, uint32_t binary, const uint32_t *__restrict__ amounts, const uint32_t *__restrict__ types,
                                                          const uint32_t *__restrict__ blinds, uint32_t *__restrict__ in_sc, uint32_t *__restrict__ flag,
                                                          uint32_t *__restrict__ any) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe v = wi_smod_n(fe_load(amounts + i * 8)), bl = fe_load(blinds + i * 8), ty = binary ? fe_zero() : fe_load(types + i * 8);
  const bool bad = !wi_canonical(bl) || !wi_canonical(ty);
  if (bad) { v = fe_zero(); ty = fe_zero(); bl = fe_zero(); atomicOr(any, 1u); }
  fe_store(in_sc + i * 24, v); fe_store(in_sc + i * 24 + 8, binary ? bl : ty); fe_store(in_sc + i * 24 + 16, binary ? ty : bl);
  flag[i] = bad ? 1u : 0u;
}

// ---- encodeCommitments (Encoding.hs:130-134) of row b (the workgroup): sign bits packed (bit i & 7 of byte i >> 3: y > p - y), then the
// 32-byte x values.  One lane per output byte, so a sign byte is assembled from its eight points by the one lane that stores it.  The row's
// verdict comes first: refused rows are written as zero bytes.
__global__ void __launch_bounds__(256) k_rp_encode_coms(uint32_t nr, uint32_t coms_bytes, uint32_t binary, const uint32_t *__restrict__ in_pt,
                                                        const uint32_t *__restrict__ flag, uint32_t *__restrict__ row_status, uint8_t *__restrict__ files) {
  const size_t b = blockIdx.x;
  const uint32_t t = threadIdx.x;
  const uint32_t *pts = in_pt + b * nr * 16;
  uint32_t f = 0;
  for (uint32_t i = t; i < nr; i += 256) {
    uint32_t o = 0;
    for (int k = 0; k < 16; k++) o |= pts[(size_t)i * 16 + k];
    f |= (flag[b * nr + i] ? 1u : 0u) | (o ? 0u : 2u);
  }
  const int not_canonical = __syncthreads_or((int)(f & 1u)), infinity = __syncthreads_or((int)(f & 2u));
  const uint32_t st = not_canonical ? (binary ? (uint32_t)BPPP_RP_WIT_BIN_NOT_CANONICAL : (uint32_t)BPPP_RP_WIT_NOT_CANONICAL)
                      : infinity    ? (uint32_t)BPPP_RP_COMMIT_INFINITY
                                    : (uint32_t)BPPP_RP_WIT_OK;
  if (t == 0) row_status[b] = st;
  const uint32_t ns = (nr + 7) / 8;
  uint8_t *file = files + b * coms_bytes;
  for (uint32_t o = t; o < coms_bytes; o += 256) {
    uint8_t v = 0;
    if (st == BPPP_RP_WIT_OK) {
      if (o < ns) { for (uint32_t i = 8 * o; i < 8 * o + 8 && i < nr; i++) v |= (uint8_t)(enc_sign(pts + (size_t)i * 16) << (i & 7)); }
      else v = enc_be_byte(pts + (size_t)((o - ns) >> 5) * 16, (o - ns) & 31);
    }
    file[o] = v;
  }
}

// ---- one opening: the decoded point (sign applied by the decoder; the infinity encoding = the x had no curve point) against the
// recomputed one.  The file is judged before the claim: MALFORMED, then NOT_CANONICAL, then the comparison.
__global__ void __launch_bounds__(256) k_rp_open_compare(uint64_t n, const uint32_t *__restrict__ dec, const uint32_t *__restrict__ rec,
                                                         const uint32_t *__restrict__ flag, uint32_t *__restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t any = 0, diff = 0;
  for (int k = 0; k < 16; k++) { const uint32_t d = dec[i * 16 + k]; any |= d; diff |= d ^ rec[i * 16 + k]; }
  status[i] = !any ? (uint32_t)BPPP_RP_OPEN_MALFORMED : flag[i] ? (uint32_t)BPPP_RP_OPEN_NOT_CANONICAL : diff ? (uint32_t)BPPP_RP_OPEN_MISMATCH : (uint32_t)BPPP_RP_OPEN_OK;
}

// ---- the weight of an opening (include/bppp.h states the message): 169 bytes, three SHA-256 blocks.  Byte k of the message of the
// commitment at job position j, read where the parts lie: the seed, the file (x bytes as they are, not reduced) and in_sc (canonical)
static constexpr uint32_t OPEN_MSG_BYTES = 32 + 8 + 32 + 1 + 3 * 32;
BPPP_DI uint32_t open_msg_byte(uint32_t k, const uint8_t *seed, uint64_t j, const uint8_t *x, uint32_t sign, const uint32_t *v, const uint32_t *ty, const uint32_t *bl) {
  if (k < 32) return seed[k];
  if (k < 40) return (uint32_t)(j >> (8 * (k - 32))) & 0xFFu;
  if (k < 72) return x[k - 40];
  if (k == 72) return sign;
  if (k < 105) return enc_be_byte(v, k - 73);
  if (k < 137) return ty ? enc_be_byte(ty, k - 105) : 0u;
  if (k < OPEN_MSG_BYTES) return enc_be_byte(bl, k - 137);
  return k == OPEN_MSG_BYTES ? 0x80u : 0u;
}
// one lane per commitment i of this launch (row i / nr of `coms`, job position j0 + i): rho[i], prods[i][s] = rho[i] * in_sc[i][s] mod n
__global__ void __launch_bounds__(64) k_rp_open_weights(uint64_t n, uint32_t nr, uint32_t coms_bytes, uint32_t binary, uint64_t j0, const uint8_t *__restrict__ seed,
                                                        const uint8_t *__restrict__ coms, const uint32_t *__restrict__ in_sc, uint32_t *__restrict__ rho,
                                                        uint32_t *__restrict__ prods) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = i / nr;
  const uint32_t c = (uint32_t)(i % nr);
  const uint8_t *file = coms + b * coms_bytes, *x = file + (nr + 7) / 8 + (size_t)c * 32;
  const uint32_t sign = (file[c >> 3] >> (c & 7)) & 1u;
  // the message names (v, ty, bl); in_sc is in base order: typed (v, ty, bl), binary (v, bl, 0) with no type at all
  const uint32_t *sc = in_sc + i * 24, *v = sc, *ty = binary ? nullptr : sc + 8, *bl = binary ? sc + 8 : sc + 16;
  uint32_t st[8], w[16];
  sha256_init(st);
#pragma unroll
  for (uint32_t blk = 0; blk < 3; blk++) {
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) {
      uint32_t word = 0;
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) word = (word << 8) | open_msg_byte(64 * blk + 4 * q + r, seed, j0 + i, x, sign, v, ty, bl);
      w[q] = word;
    }
    if (blk == 2) w[15] = OPEN_MSG_BYTES * 8;
    sha256_compress(st, w);
  }
  fe r; sha256_digest_to_limbs(st, r.v);
  r = wi_umod_n(r);
  if (fe_is_zero(r)) r = fe_one();
  fe_store(rho + i * 8, r);
  for (int s = 0; s < 3; s++) fe_store(prods + i * 24 + s * 8, fe_mul<1>(r, fe_load(sc + s * 8)));
}

// ---- out[blockIdx.x][s] = sum over this workgroup's share of in[i][s] mod n, s < 3; negate: the additive inverse instead (the last
// launch writes the scalars of g, H0, H1 in E = C - v g - ty H0 - bl H1 straight into the MSM's scalar array).  256 threads a workgroup.
BPPP_DI fe fe_shfl_down(const fe &a, int d) { fe r; for (int k = 0; k < 8; k++) r.v[k] = __shfl_down(a.v[k], d); return r; }
__global__ void __launch_bounds__(256) k_rp_open_reduce(uint64_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t negate) {
  __shared__ uint32_t part[4][24];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  fe acc[3] = {fe_zero(), fe_zero(), fe_zero()};
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + t; i < n; i += (uint64_t)gridDim.x * 256)
    for (int s = 0; s < 3; s++) acc[s] = fe_add<1>(acc[s], fe_load(in + i * 24 + s * 8));
  for (int d = 32; d >= 1; d >>= 1)
    for (int s = 0; s < 3; s++) acc[s] = fe_add<1>(acc[s], fe_shfl_down(acc[s], d));
  if (lane == 0) for (int s = 0; s < 3; s++) for (int k = 0; k < 8; k++) part[wave][s * 8 + k] = acc[s].v[k];
  __syncthreads();
  if (wave) return;
  for (int s = 0; s < 3; s++) for (int k = 0; k < 8; k++) acc[s].v[k] = lane < 4 ? part[lane & 3][s * 8 + k] : 0u;
  for (int d = 2; d >= 1; d >>= 1)
    for (int s = 0; s < 3; s++) acc[s] = fe_add<1>(acc[s], fe_shfl_down(acc[s], d));
  if (lane == 0) for (int s = 0; s < 3; s++) fe_store(out + (size_t)blockIdx.x * 24 + s * 8, negate ? fe_neg<1>(acc[s]) : acc[s]);
}

// ---- the window table and its launches
// the fixed-base table of (g, H0, H1): [3][64][15] affine points, built once per setup on the host (2880 additions, one batch inversion)
int rpp_build_fixed_table(bppp_rp *rp) {
  using namespace bppp_host;
  if (rp->d_fixed) return BPPP_OK;
  bppp_ctx *ctx = rp->ctx;
  const Mod &Q = FQ();
  std::vector<HJac> jac;
  jac.reserve(FB_BASES * FB_WIN * FB_DIG);
  const uint64_t *bases[3] = {rp->h_g.data(), rp->h_H.data(), rp->h_H.data() + 8};
  for (int b = 0; b < FB_BASES; b++) {
    HJac cur = hj_from_aff(HAff{U256::load(bases[b]), U256::load(bases[b] + 4)});
    for (int w = 0; w < FB_WIN; w++) {
      HJac acc = cur;
      for (int d = 1; d <= FB_DIG; d++) { jac.push_back(acc); acc = hj_add(acc, cur); }
      cur = acc;                                   // 16 * cur
    }
  }
  std::vector<U256> zs(jac.size());
  for (size_t i = 0; i < jac.size(); i++) zs[i] = jac[i].Z;
  batch_minv(zs.data(), zs.size(), Q);
  std::vector<uint64_t> host(jac.size() * 8, 0);
  for (size_t i = 0; i < jac.size(); i++) {
    if (jac[i].inf()) continue;                    // cannot happen for points of prime order; kept as the infinity encoding
    const U256 zi2 = fqmul(zs[i], zs[i]);
    fqmul(jac[i].X, zi2).store(&host[8 * i]);
    fqmul(jac[i].Y, fqmul(zi2, zs[i])).store(&host[8 * i + 4]);
  }
  BPPP_HIP(ctx, hipMalloc(&rp->d_fixed, host.size() * 8));
  BPPP_HIP(ctx, hipMemcpy(rp->d_fixed, host.data(), host.size() * 8, hipMemcpyHostToDevice));
  return BPPP_OK;
}
int rpp_commit_inputs_fixed(bppp_rp *rp, const uint32_t *d_in_sc, size_t n, uint32_t *d_out) {
  bppp_ctx *ctx = rp->ctx;
  k_rp_commit_inputs<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream>>>(rp->d_fixed, d_in_sc, (uint64_t)n, d_out);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}
int rpp_commit_inputs(bppp_rp *rp, const uint32_t *d_in_sc, size_t n, uint32_t *d_out) {
  bppp_ctx *ctx = rp->ctx;
  // bppp_rp_prove_mixed committed the inputs of the whole family in one launch (csrc/rpshare.hip): they are complete in HBM
  if (rp->pre_inputs) { BPPP_HIP(ctx, hipMemcpyAsync(d_out, rp->pre_inputs, n * 64, hipMemcpyDeviceToDevice, ctx->stream)); return BPPP_OK; }
  // g, H0, H1 are the first three points of the registered basis: with its comb table a commitment is <= 3 x 17 additions, not 3 x 64
  if (rp->comb) { int rc = comb_lanes(rp->comb, d_in_sc, FB_BASES, n, d_out, ctx->stream); return rc ? fail(ctx, rc, bppp_last_error(rp->comb->ctx)) : BPPP_OK; }
  return rpp_commit_inputs_fixed(rp, d_in_sc, n, d_out);
}
int rpp_claim_scalars(bppp_rp *rp, uint64_t n, const uint32_t *amounts, const uint32_t *types, const uint32_t *blinds, uint32_t *in_sc, uint32_t *flag, uint32_t *any) {
  bppp_ctx *ctx = rp->ctx;
  k_rp_claim_scalars<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(n, rp->st.kind == 1, amounts, types, blinds, in_sc, flag, any);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}
int rpp_negated_column_sums(bppp_rp *rp, uint64_t n, const uint32_t *prods, uint32_t *part, uint32_t *out) {
  bppp_ctx *ctx = rp->ctx;
  const unsigned G = (unsigned)std::min<uint64_t>((n + 255) / 256, RPP_REDUCE_BLOCKS);
  k_rp_open_reduce<<<dim3(G), dim3(256), 0, ctx->stream>>>(n, prods, part, 0u);
  k_rp_open_reduce<<<dim3(1), dim3(256), 0, ctx->stream>>>(G, part, out, 1u);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

int rpp_report_refusals(bppp_ctx *ctx, const char *who, const char *noun, const uint32_t *h_status, size_t n, uint32_t *out_status, const char *(*text)(uint32_t)) {
  if (out_status) { memcpy(out_status, h_status, n * 4); return BPPP_OK; }
  for (size_t i = 0; i < n; i++)
    if (h_status[i]) return fail(ctx, BPPP_ERR_ARG, std::string(who) + ": " + noun + " " + std::to_string(i) + ": " + text(h_status[i]));
  return BPPP_OK;
}
int BatchParts::msm(bppp_ctx *ctx, const void *sc, const void *pt, size_t n) {
  xy.resize(xy.size() + 8);
  const int rc = msm_run(ctx, sc, pt, n, 1, 0, 0, &xy[xy.size() - 8]);
  if (rc) hipStreamSynchronize(ctx->stream);
  return rc;
}
int BatchParts::finish(bppp_ctx *ctx, bool reject, uint64_t *combined_xy, int *accept) {
  uint64_t sum[8];
  const int rc = bppp_sum_points(ctx, xy.data(), xy.size() / 8, sum);
  if (rc) return rc;
  if (combined_xy) memcpy(combined_xy, sum, 64);
  *accept = (rp_point_is_inf(sum) && !reject) ? 1 : 0;
  return BPPP_OK;
}

}  // namespace bppp

using namespace bppp;

namespace {

const char *commit_status_text(uint32_t s) {
  return s == BPPP_RP_COMMIT_INFINITY ? "the commitment is the point at infinity (amount, type and blinding are all zero mod n)" : bppp_rps::wit_status_text(s);
}

// the workspace of one chunk of R rows, carved from rp->pwork; `open` adds the decoded points and `weights` the arrays of open_batch
struct Work {
  uint32_t *in_sc, *flag, *rec, *row_status, *dec, *bad, *any, *status, *rho, *prods, *part;
  uint8_t *seed;
};
int carve(bppp_rp *rp, size_t R, bool open, bool weights, Work &W) {
  const size_t nr = rp->D.nr, n = R * nr;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    W.in_sc = cv.take<uint32_t>(n * 24); W.flag = cv.take<uint32_t>(n); W.rec = cv.take<uint32_t>(n * 16); W.row_status = cv.take<uint32_t>(R);
    W.any = cv.take<uint32_t>(2);
    W.dec = cv.take<uint32_t>(open ? (n + 3) * 16 : 0); W.bad = cv.take<uint32_t>(open ? R : 0); W.status = cv.take<uint32_t>(open ? n : 0);
    W.rho = cv.take<uint32_t>(weights ? (n + 3) * 8 : 0); W.prods = cv.take<uint32_t>(weights ? n * 24 : 0);
    W.part = cv.take<uint32_t>(weights ? (size_t)RPP_REDUCE_BLOCKS * 24 : 0); W.seed = cv.take<uint8_t>(32);
    if (!pass) { int rc = rpp_ensure_pwork(rp, cv.off); if (rc) return rc; }
  }
  return BPPP_OK;
}
// rows per pass over the workspace: a larger batch goes through in chunks of whole rows (~300 bytes of workspace a commitment)
size_t chunk_rows(const bppp_rp *rp, size_t batch) { return std::max<size_t>(1, std::min(batch, rpp_flat_chunk(rp) / rp->D.nr)); }

// the checks every entry point makes on a non-empty batch
int entry_checks(bppp_rp *rp, size_t batch, const char *who, bool bad_args) {
  bppp_ctx *ctx = rp->ctx;
  if (bad_args) return fail(ctx, BPPP_ERR_ARG, std::string(who) + ": null input");
  if (!rp->D.nr || batch > RPP_LIM31 / rp->D.nr) return fail(ctx, BPPP_ERR_ARG, std::string(who) + ": batch * nranges must be below 2^31");
  hipSetDevice(ctx->device);
  return BPPP_OK;
}

// rows [0, n) of one chunk: claimed scalars and their commitments in W.rec
int claim_and_commit(bppp_rp *rp, const Work &W, size_t rows, const uint32_t *amt, const uint32_t *ty, const uint32_t *bl) {
  bppp_ctx *ctx = rp->ctx;
  const uint64_t n = (uint64_t)rows * rp->D.nr;
  k_rp_claim_scalars<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(n, rp->st.kind == 1, amt, ty, bl, W.in_sc, W.flag, W.any + 1);
  BPPP_HIP(ctx, hipGetLastError());
  return rpp_commit_inputs(rp, W.in_sc, n, W.rec);
}

int commit_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds, uint32_t *commit_status, void *d_coms_files) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!batch) return BPPP_OK;
  const bool binary = rp->st.kind == 1;
  int rc = entry_checks(rp, batch, "rp_commit_batch", !d_amounts || (!d_types && !binary) || !d_blinds || !d_coms_files); if (rc) return rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const size_t nr = rp->D.nr, cb = rp->D.coms_bytes, R = chunk_rows(rp, batch);
  Work W;
  if ((rc = carve(rp, R, false, false, W))) return rc;
  std::vector<uint32_t> status(batch);
  for (size_t o = 0; o < batch; o += R) {
    const size_t rows = std::min(R, batch - o);
    const uint32_t *amt = (const uint32_t *)d_amounts + o * nr * 8, *ty = binary ? nullptr : (const uint32_t *)d_types + o * nr * 8, *bl = (const uint32_t *)d_blinds + o * nr * 8;
    BPPP_HIP(ctx, hipMemsetAsync(W.any, 0, 8, ctx->stream));
    if ((rc = claim_and_commit(rp, W, rows, amt, ty, bl))) return rc;
    k_rp_encode_coms<<<dim3((unsigned)rows), dim3(256), 0, ctx->stream>>>((uint32_t)nr, (uint32_t)cb, binary, W.rec, W.flag, W.row_status, (uint8_t *)d_coms_files + o * cb);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(status.data() + o, W.row_status, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return rpp_report_refusals(ctx, "rp_commit_batch", "proof", status.data(), batch, commit_status, commit_status_text);
}

// decode + claim + commit of one chunk, in W.dec / W.rec / W.flag; W.any = (some x had no point, some claim was not canonical)
int open_chunk(bppp_rp *rp, const Work &W, size_t rows, size_t o, const void *d_coms, const void *d_amounts, const void *d_types, const void *d_blinds, bool recompute) {
  bppp_ctx *ctx = rp->ctx;
  const size_t nr = rp->D.nr;
  const bool binary = rp->st.kind == 1;
  const uint32_t *amt = (const uint32_t *)d_amounts + o * nr * 8, *ty = binary ? nullptr : (const uint32_t *)d_types + o * nr * 8, *bl = (const uint32_t *)d_blinds + o * nr * 8;
  BPPP_HIP(ctx, hipMemsetAsync(W.any, 0, 8, ctx->stream));
  BPPP_HIP(ctx, hipMemsetAsync(W.bad, 0, rows * 4, ctx->stream));
  rp_decode_coms(rp, rows, (const uint8_t *)d_coms + o * rp->D.coms_bytes, W.dec, W.bad, W.any);
  BPPP_HIP(ctx, hipGetLastError());
  if (recompute) return claim_and_commit(rp, W, rows, amt, ty, bl);
  const uint64_t n = (uint64_t)rows * nr;
  k_rp_claim_scalars<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(n, binary, amt, ty, bl, W.in_sc, W.flag, W.any + 1);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

// every opening decided on its own: open_status [batch][nranges] on the host.  The arguments are checked by the callers.
int open_each_pass(bppp_rp *rp, size_t batch, const void *d_coms, const void *d_amounts, const void *d_types, const void *d_blinds, uint32_t *open_status) {
  bppp_ctx *ctx = rp->ctx;
  int rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const size_t nr = rp->D.nr, R = chunk_rows(rp, batch);
  Work W;
  if ((rc = carve(rp, R, true, false, W))) return rc;
  for (size_t o = 0; o < batch; o += R) {
    const size_t rows = std::min(R, batch - o);
    const uint64_t n = (uint64_t)rows * nr;
    if ((rc = open_chunk(rp, W, rows, o, d_coms, d_amounts, d_types, d_blinds, true))) return rc;
    k_rp_open_compare<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(n, W.dec, W.rec, W.flag, W.status);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(open_status + o * nr, W.status, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return BPPP_OK;
}

int open_each_device(bppp_rp *rp, size_t batch, const void *d_coms, const void *d_amounts, const void *d_types, const void *d_blinds, uint32_t *open_status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!batch) return BPPP_OK;
  int rc = entry_checks(rp, batch, "rp_open_each", !d_coms || !d_amounts || (!d_types && rp->st.kind != 1) || !d_blinds || !open_status);
  return rc ? rc : open_each_pass(rp, batch, d_coms, d_amounts, d_types, d_blinds, open_status);
}

int open_batch_device(bppp_rp *rp, size_t batch, uint64_t index_offset, const void *d_coms, const void *d_amounts, const void *d_types, const void *d_blinds,
                      const uint8_t seed[32], int *accept, uint32_t *open_status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  if (combined_xy) memset(combined_xy, 0, 64);
  if (!batch) { *accept = 1; return BPPP_OK; }
  const bool binary = rp->st.kind == 1;
  int rc = entry_checks(rp, batch, "rp_open_batch", !d_coms || !d_amounts || (!d_types && !binary) || !d_blinds || !seed); if (rc) return rc;
  const size_t nr = rp->D.nr, cb = rp->D.coms_bytes, R = chunk_rows(rp, batch);
  hipStream_t st = ctx->stream;
  Work W;
  if ((rc = carve(rp, R, true, true, W))) return rc;
  BPPP_HIP(ctx, hipMemcpyAsync(W.seed, seed, 32, hipMemcpyHostToDevice, st));
  BatchParts parts;                             // one combined point per chunk
  uint32_t any[2] = {0, 0};
  for (size_t o = 0; o < batch; o += R) {
    const size_t rows = std::min(R, batch - o);
    const uint64_t n = (uint64_t)rows * nr;
    if ((rc = open_chunk(rp, W, rows, o, d_coms, d_amounts, d_types, d_blinds, false))) return rc;
    k_rp_open_weights<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st>>>(n, (uint32_t)nr, (uint32_t)cb, binary, (index_offset + o) * nr, W.seed,
                                                                           (const uint8_t *)d_coms + o * cb, W.in_sc, W.rho, W.prods);
    BPPP_HIP(ctx, hipGetLastError());
    if ((rc = rpp_negated_column_sums(rp, n, W.prods, W.part, W.rho + n * 8))) return rc;   // - sum rho v, - sum rho ty, - sum rho bl: the scalars of g, H0, H1
    BPPP_HIP(ctx, hipMemcpyAsync(W.dec + n * 16, rp->d_basis, 3 * 64, hipMemcpyDeviceToDevice, st));   // [g | H0 | H1 ...]: the registered basis starts with them
    uint32_t chunk_any[2];
    BPPP_HIP(ctx, hipMemcpyAsync(chunk_any, W.any, 8, hipMemcpyDeviceToHost, st));
    if ((rc = parts.msm(ctx, W.rho, W.dec, n + 3))) return rc;
    any[0] |= chunk_any[0]; any[1] |= chunk_any[1];
  }
  if ((rc = parts.finish(ctx, any[0] || any[1], combined_xy, accept))) return rc;
  if (!open_status) return BPPP_OK;
  if (*accept) { memset(open_status, 0, batch * nr * 4); return BPPP_OK; }
  return open_each_pass(rp, batch, d_coms, d_amounts, d_types, d_blinds, open_status);      // one exact pass, whatever the number of bad openings
}

// ---- host variants: upload, the _device variant, download
// the claimed arrays of a host call are batch * nranges scalars each; types stays NULL where the caller passed none
size_t claim_bytes(const bppp_rp *rp, size_t batch) { return batch * rp->D.nr * 32; }
size_t files_bytes(const bppp_rp *rp, size_t batch) { return batch * (size_t)rp->D.coms_bytes; }

}  // namespace

extern "C" {

int bppp_rp_commit_batch_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds, uint32_t *commit_status,
                                void *d_coms_files) {
  return commit_device(rp, batch, d_amounts, d_types, d_blinds, commit_status, d_coms_files);
}

int bppp_rp_commit_batch(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, uint32_t *commit_status,
                         uint8_t *coms_files) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!batch) return BPPP_OK;
  int rc = entry_checks(rp, batch, "rp_commit_batch", !amounts || (!types && rp->st.kind != 1) || !blinds || !coms_files); if (rc) return rc;
  DevBuf amt, ty, bl, files;
  const size_t cl = claim_bytes(rp, batch);
  if ((rc = amt.up(ctx, amounts, cl)) || (rc = ty.up(ctx, types, cl)) || (rc = bl.up(ctx, blinds, cl)) || (rc = files.out(ctx, coms_files, files_bytes(rp, batch)))) return rc;
  rc = commit_device(rp, batch, amt.p, ty.p, bl.p, commit_status, files.p);
  return rpp_download_refused(ctx, rc, nullptr, coms_files, files.p, files_bytes(rp, batch));     // entry_checks has refused everything but a commitment
}

int bppp_rp_open_each_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_amounts, const void *d_types, const void *d_blinds,
                             uint32_t *open_status) {
  return open_each_device(rp, batch, d_coms_files, d_amounts, d_types, d_blinds, open_status);
}

int bppp_rp_open_each(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds,
                      uint32_t *open_status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!batch) return BPPP_OK;
  int rc = entry_checks(rp, batch, "rp_open_each", !coms_files || !amounts || (!types && rp->st.kind != 1) || !blinds || !open_status); if (rc) return rc;
  DevBuf amt, ty, bl, files;
  const size_t cl = claim_bytes(rp, batch);
  if ((rc = amt.up(ctx, amounts, cl)) || (rc = ty.up(ctx, types, cl)) || (rc = bl.up(ctx, blinds, cl)) || (rc = files.up(ctx, coms_files, files_bytes(rp, batch)))) return rc;
  return open_each_device(rp, batch, files.p, amt.p, ty.p, bl.p, open_status);
}

int bppp_rp_open_batch_device(bppp_rp *rp, size_t batch, uint64_t index_offset, const void *d_coms_files, const void *d_amounts, const void *d_types,
                              const void *d_blinds, const uint8_t seed[32], int *accept, uint32_t *open_status, uint64_t *combined_xy) {
  return open_batch_device(rp, batch, index_offset, d_coms_files, d_amounts, d_types, d_blinds, seed, accept, open_status, combined_xy);
}

int bppp_rp_open_batch(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds,
                       const uint8_t seed[32], int *accept, uint32_t *open_status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  if (combined_xy) memset(combined_xy, 0, 64);
  if (!batch) { *accept = 1; return BPPP_OK; }
  int rc = entry_checks(rp, batch, "rp_open_batch", !coms_files || !amounts || (!types && rp->st.kind != 1) || !blinds || !seed); if (rc) return rc;
  DevBuf amt, ty, bl, files;
  const size_t cl = claim_bytes(rp, batch);
  if ((rc = amt.up(ctx, amounts, cl)) || (rc = ty.up(ctx, types, cl)) || (rc = bl.up(ctx, blinds, cl)) || (rc = files.up(ctx, coms_files, files_bytes(rp, batch)))) return rc;
  return open_batch_device(rp, batch, 0, files.p, amt.p, ty.p, bl.p, seed, accept, open_status, combined_xy);
}

}  // extern "C"
