// rptally.hip — signed sums of commitments against claimed openings: bppp_rp_tally_each*, bppp_rp_tally_batch*, bppp_rp_tally_claims*
// (include/bppp.h).  The homomorphic check next to commit / open (csrc/rpcommit.hip): sum t of a job adds and subtracts commitments
// gathered from a pool of commitments files, and must equal  a_t g + ty_t H0 + e_t H1  (a binary handle: a_t g + e_t h0).
//   pool     decodeCommitments (Encoding.hs:119-128) of every row, once per call, by the verifier's decoder (rp_decode_coms, csrc/rp.hip):
//            64 bytes a commitment, the infinity encoding for an x without a curve point
//   sums     CSR: sum_start [nsums + 1], entries [nnz] (bits 0..30 the flat index row * nranges + i, bit 31 = subtract)
// Kernels:
//   k_rp_tally_validate  the CSR conditions, before anything reads through the arrays: the first offending position of each kind
//   k_rp_tally_sum       the segmented signed point sum: route 0 one lane per short sum, route 1 one workgroup per piece of a long sum
//                        (strided shares, then a tree over LDS), route 2 the same over the partial points of the pieces
//   k_rp_tally_compare   XYZZ sum against the recomputed affine claim, cross-multiplied -> one status word per sum
//   k_rp_tally_affine    the sums as affine points, after one batch inversion of their ZZ ZZZ (batch_inverse_run, csrc/rounds.hip)
//   k_rp_tally_weights   rho_t = decode (SHA-256 (the weight message of include/bppp.h)) and rho_t times the three claimed scalars
//   k_rp_tally_terms     per entry: scalar +-rho_t and the gathered point, the MSM's input
//   k_rp_tally_claims    the builder's side: signed sums mod n of the referenced (amount, type, blinding), one wavefront per sum
// Every kernel is bounds-checked on its own index, takes its loop bounds from validated arrays only, and writes with ordinary vector stores.
// The job's checks, the decoded pool, the plan of a pass and the k_rp_tally_sum launches are declared in rp_internal.hpp (bppp::tally): the excess
// signatures (csrc/rpexcess.hip) run the same stage.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ec.hip.h"
#include "rp_internal.hpp"
#include "rphostcall.hpp"
#include "rpprove_host.hpp"
#include "rptally_plan.hpp"
#include "rpwords.hip.h"
#include "sha256.hip.h"

namespace bppp {

static constexpr uint32_t TALLY_LANES = 256;
static constexpr uint32_t TALLY_FINAL = 0x80000000u;     // an item's destination: bit 31 = the sum itself, else a partial point
static constexpr uint32_t TALLY_NONE = 0xFFFFFFFFu;

// ---- flag[0] = the lowest position whose sum_start breaks "non-decreasing from 0 to nnz", flag[1] = the lowest position of an entry whose
// index is >= total; both start as TALLY_NONE.  The bounds nsums and nnz are the caller's arguments, never device data.
__global__ void __launch_bounds__(256) k_rp_tally_validate(uint32_t nsums, uint32_t nnz, uint32_t total, const uint32_t *__restrict__ start,
                                                           const uint32_t *__restrict__ entries, uint32_t *__restrict__ flag) {
  const uint64_t n = (uint64_t)nsums + 1 > nnz ? (uint64_t)nsums + 1 : nnz;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    if (i <= nsums) {
      const uint32_t s = start[i];
      if ((i == 0 && s != 0) || (i == nsums && s != nnz) || (i > 0 && s < start[i - 1])) atomicMin(flag, (uint32_t)i);
    }
    if (i < nnz && (entries[i] & ~TALLY_FINAL) >= total) atomicMin(flag + 1, (uint32_t)i);
  }
}

// ---- the segmented signed sum.  An entry gathers its affine point from the pool and negates it on load (y -> p - y); an entry that
// gathers the infinity encoding marks its sum malformed.  Every addition is the complete law of ec.hip.h: P + P, P - P and infinity
// operands are ordinary input here.
//   route 0   lane t of the launch is sum t of the chunk (count sums, start = sum_start + the chunk's first sum); a sum longer than
//             short_max is left to route 1
//   route 1   workgroup i is item i: entries [x, y) of one sum, lane l takes x + l, x + l + 256, ...; the lanes' points are added by a tree
//             over LDS (160 B a lane, word-major so that a wavefront's accesses fall on distinct banks)
//   route 2   the same over the partial points src[x .. y) that an earlier launch left
// items[i] = (x, y, destination, slot): the destination is sum `d & 0x7FFFFFFF` of the chunk when bit 31 is set, else partial point d of
// dst; slot is the sum whose malformed flag the item raises.
BPPP_DI void tally_gather(xyzz &acc, uint32_t &bad, uint32_t ent, const uint32_t *__restrict__ pool) {
  const aff P = aff_load(pool + (size_t)(ent & ~TALLY_FINAL) * 16);
  if (aff_is_inf(P)) { bad = 1; return; }
  xyzz_madd(acc, aff_cneg(P, (ent >> 31) != 0));
}
__global__ void __launch_bounds__(256) k_rp_tally_sum(uint32_t route, uint32_t count, uint32_t short_max, const uint32_t *__restrict__ start,
                                                      const uint32_t *__restrict__ entries, const uint32_t *__restrict__ pool,
                                                      const uint4 *__restrict__ items, const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                      uint32_t *__restrict__ sums, uint32_t *__restrict__ malformed) {
  __shared__ uint32_t sh[XYZZ_WORDS * TALLY_LANES];
  const uint32_t l = threadIdx.x;
  xyzz acc = xyzz_inf();
  uint32_t bad = 0;
  if (route == 0) {
    const uint64_t t = (uint64_t)blockIdx.x * TALLY_LANES + l;
    if (t >= count) return;
    const uint32_t b = start[t], e = start[t + 1];
    if (e - b > short_max) return;
    for (uint32_t p = b; p < e; p++) tally_gather(acc, bad, entries[p], pool);
    xyzz_store(sums + t * XYZZ_WORDS, acc);
    if (bad) malformed[t] = 1u;
    return;
  }
  if (blockIdx.x >= count) return;
  const uint4 it = items[blockIdx.x];
  if (route == 1) for (uint32_t p = it.x + l; p < it.y; p += TALLY_LANES) tally_gather(acc, bad, entries[p], pool);
  else for (uint32_t p = it.x + l; p < it.y; p += TALLY_LANES) xyzz_add(acc, xyzz_load(src + (size_t)p * XYZZ_WORDS));
  for (uint32_t d = TALLY_LANES / 2; d >= 1; d >>= 1) {
    // lanes [d, 2d) hand their points to lanes [0, d)
    if (l >= d && l < 2 * d) {
#pragma unroll
      for (int k = 0; k < 10; k++) {
        sh[k * TALLY_LANES + l] = acc.X.n[k]; sh[(10 + k) * TALLY_LANES + l] = acc.Y.n[k];
        sh[(20 + k) * TALLY_LANES + l] = acc.ZZ.n[k]; sh[(30 + k) * TALLY_LANES + l] = acc.ZZZ.n[k];
      }
    }
    __syncthreads();
    if (l < d) {
      xyzz o;
#pragma unroll
      for (int k = 0; k < 10; k++) {
        o.X.n[k] = sh[k * TALLY_LANES + l + d]; o.Y.n[k] = sh[(10 + k) * TALLY_LANES + l + d];
        o.ZZ.n[k] = sh[(20 + k) * TALLY_LANES + l + d]; o.ZZZ.n[k] = sh[(30 + k) * TALLY_LANES + l + d];
      }
      xyzz_add(acc, o);
    }
  }
  const int any_bad = __syncthreads_or((int)bad);
  if (l) return;
  if (any_bad) atomicOr(malformed + it.w, 1u);
  if (it.z & TALLY_FINAL) xyzz_store(sums + (size_t)(it.z & ~TALLY_FINAL) * XYZZ_WORDS, acc);
  else xyzz_store(dst + (size_t)it.z * XYZZ_WORDS, acc);
}

// ---- sum t against its recomputed claim rec[t] (affine, the infinity encoding for a zero claim): X = x ZZ and Y = y ZZZ, no inversion.
// The pool is judged before the claim: MALFORMED, then NOT_CANONICAL, then the comparison.  zz (may be NULL): ZZ ZZZ of the sum for
// the batch inversion, zero for infinity and for a malformed sum.
__global__ void __launch_bounds__(256) k_rp_tally_compare(uint32_t n, const uint32_t *__restrict__ sums, const uint32_t *__restrict__ rec,
                                                          const uint32_t *__restrict__ flag, const uint32_t *__restrict__ malformed,
                                                          uint32_t *__restrict__ status, uint32_t *__restrict__ zz) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const xyzz S = xyzz_load(sums + (size_t)t * XYZZ_WORDS);
  const aff R = aff_load(rec + (size_t)t * 16);
  const bool s_inf = xyzz_is_inf(S), bad = malformed[t] != 0;
  bool eq;
  if (aff_is_inf(R)) eq = s_inf;
  else if (s_inf) eq = false;
  else eq = fq_normalizes_to_zero(fq_sub<5>(fq_mul(R.x, S.ZZ), S.X)) && fq_normalizes_to_zero(fq_sub<3>(fq_mul(R.y, S.ZZZ), S.Y));
  status[t] = bad ? (uint32_t)BPPP_RP_OPEN_MALFORMED : flag[t] ? (uint32_t)BPPP_RP_OPEN_NOT_CANONICAL : eq ? (uint32_t)BPPP_RP_OPEN_OK : (uint32_t)BPPP_RP_OPEN_MISMATCH;
  if (zz) fe_store(zz + (size_t)t * 8, (bad || s_inf) ? fe_zero() : fq_to_fe(fq_mul(S.ZZ, S.ZZZ)));
}
// x = X / ZZ = X ZZZ / (ZZ ZZZ), y = Y / ZZZ = Y ZZ / (ZZ ZZZ) with zinv[t] = 1 / (ZZ ZZZ), zero -> the all-zero point
__global__ void __launch_bounds__(256) k_rp_tally_affine(uint32_t n, const uint32_t *__restrict__ sums, const uint32_t *__restrict__ zinv, uint32_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const fe zi = fe_load(zinv + (size_t)t * 8);
  aff r = aff_inf();
  if (!fe_is_zero(zi)) {
    const xyzz S = xyzz_load(sums + (size_t)t * XYZZ_WORDS);
    const fq z = fq_from_fe(zi);
    r.x = fq_mul(S.X, fq_mul(z, S.ZZZ));
    r.y = fq_mul(S.Y, fq_mul(z, S.ZZ));
  }
  aff_store(out + (size_t)t * 16, r);
}

// ---- the weight of sum t (include/bppp.h states the message): 136 bytes, three SHA-256 blocks; in_sc holds the canonical claim in base
// order: typed (a, ty, e), binary (a, e, 0) with a zero type in the message
static constexpr uint32_t TALLY_MSG_BYTES = 32 + 8 + 3 * 32;
BPPP_DI uint32_t tally_msg_byte(uint32_t k, const uint8_t *seed, uint64_t j, const uint32_t *a, const uint32_t *ty, const uint32_t *e) {
  if (k < 32) return seed[k];
  if (k < 40) return (uint32_t)(j >> (8 * (k - 32))) & 0xFFu;
  if (k < 72) return enc_be_byte(a, k - 40);
  if (k < 104) return ty ? enc_be_byte(ty, k - 72) : 0u;
  if (k < TALLY_MSG_BYTES) return enc_be_byte(e, k - 104);
  return k == TALLY_MSG_BYTES ? 0x80u : 0u;
}
__global__ void __launch_bounds__(64) k_rp_tally_weights(uint32_t n, uint32_t binary, uint64_t j0, const uint8_t *__restrict__ seed, const uint32_t *__restrict__ in_sc,
                                                         uint32_t *__restrict__ rho, uint32_t *__restrict__ prods) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t *sc = in_sc + (size_t)t * 24, *a = sc, *ty = binary ? nullptr : sc + 8, *e = binary ? sc + 8 : sc + 16;
  uint32_t st[8], w[16];
  sha256_init(st);
#pragma unroll
  for (uint32_t blk = 0; blk < 3; blk++) {
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) {
      uint32_t word = 0;
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) word = (word << 8) | tally_msg_byte(64 * blk + 4 * q + r, seed, j0 + t, a, ty, e);
      w[q] = word;
    }
    if (blk == 2) w[15] = TALLY_MSG_BYTES * 8;
    sha256_compress(st, w);
  }
  fe r; sha256_digest_to_limbs(st, r.v);
  r = wi_umod_n(r);
  if (fe_is_zero(r)) r = fe_one();
  fe_store(rho + (size_t)t * 8, r);
  for (int s = 0; s < 3; s++) fe_store(prods + (size_t)t * 24 + s * 8, fe_mul<1>(r, fe_load(sc + s * 8)));
}

// ---- entry e0 + i of the job -> term i of the MSM: the sum it lies in is the last t < ns with start[t] <= e0 + i (start = sum_start + the
// chunk's first sum, validated: the search takes at most 32 steps), its scalar rho_t or n - rho_t, its point the gathered one as decoded.
// any[0] is raised when the gathered point is the infinity encoding.
__global__ void __launch_bounds__(256) k_rp_tally_terms(uint32_t n, uint32_t e0, const uint32_t *__restrict__ start, uint32_t ns, const uint32_t *__restrict__ entries,
                                                        const uint32_t *__restrict__ pool, const uint32_t *__restrict__ rho, uint32_t *__restrict__ sc,
                                                        uint32_t *__restrict__ pt, uint32_t *__restrict__ any) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = e0 + i, ent = entries[p];
  uint32_t lo = 0, hi = ns - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (start[mid] <= p) lo = mid; else hi = mid - 1;
  }
  const fe r = fe_load(rho + (size_t)lo * 8);
  fe_store(sc + (size_t)i * 8, (ent >> 31) ? fe_neg<1>(r) : r);
  const uint32_t *src = pool + (size_t)(ent & ~TALLY_FINAL) * 16;
  uint32_t o = 0;
  for (int k = 0; k < 16; k++) { const uint32_t v = src[k]; o |= v; pt[(size_t)i * 16 + k] = v; }
  if (!o) atomicOr(any, 1u);
}

// ---- the claims of the builder: wavefront w of the launch is sum w; its lanes share the entries, add or subtract the referenced
// (amount mod n, type, blinding) mod n and meet in a tree of cross-lane moves.  A referenced type or blinding >= n lowers flag[0] to its sum.
// The amount is written as the representative that the entry points read back as itself: a below 2^255, else a - n in two's complement.
BPPP_DI fe tally_fe_shfl_down(const fe &a, int d) { fe r; for (int k = 0; k < 8; k++) r.v[k] = __shfl_down(a.v[k], d); return r; }
__global__ void __launch_bounds__(256) k_rp_tally_claims(uint32_t nsums, uint32_t binary, const uint32_t *__restrict__ start, const uint32_t *__restrict__ entries,
                                                         const uint32_t *__restrict__ amounts, const uint32_t *__restrict__ types, const uint32_t *__restrict__ blinds,
                                                         uint32_t *__restrict__ out_a, uint32_t *__restrict__ out_ty, uint32_t *__restrict__ out_e, uint32_t *__restrict__ flag) {
  const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (t >= nsums) return;                      // whole wavefronts leave together
  fe acc[3] = {fe_zero(), fe_zero(), fe_zero()};
  bool bad = false;
  for (uint32_t p = start[t] + lane, e = start[t + 1]; p < e; p += 64) {
    const uint32_t ent = entries[p];
    const size_t j = (size_t)(ent & ~TALLY_FINAL) * 8;
    fe v[3] = {wi_smod_n(fe_load(amounts + j)), binary ? fe_zero() : fe_load(types + j), fe_load(blinds + j)};
    if (!wi_canonical(v[1]) || !wi_canonical(v[2])) { bad = true; continue; }
    for (int s = 0; s < 3; s++) acc[s] = (ent >> 31) ? fe_sub<1>(acc[s], v[s]) : fe_add<1>(acc[s], v[s]);
  }
  if (bad) atomicMin(flag, (uint32_t)t);
  for (int d = 32; d >= 1; d >>= 1)
    for (int s = 0; s < 3; s++) acc[s] = fe_add<1>(acc[s], tally_fe_shfl_down(acc[s], d));
  if (lane) return;
  fe a = acc[0];
  if (wi_neg(a)) raw_sub(a, acc[0], fr_modulus());
  fe_store(out_a + (size_t)t * 8, a);
  if (out_ty) fe_store(out_ty + (size_t)t * 8, acc[1]);
  fe_store(out_e + (size_t)t * 8, acc[2]);
}

}  // namespace bppp

namespace bppp {
namespace tally {

void fill(Job &J, bppp_rp *rp, const char *who, size_t rows, const void *coms, size_t nsums, const void *start, const void *entries, size_t nnz, const void *amt,
          const void *ty, const void *bl) {
  J.rp = rp; J.who = who; J.rows = rows; J.nsums = nsums; J.nnz = nnz;
  J.coms = (const uint8_t *)coms; J.start = (const uint32_t *)start; J.entries = (const uint32_t *)entries;
  J.amt = (const uint32_t *)amt; J.ty = rp->st.kind == 1 ? nullptr : (const uint32_t *)ty; J.bl = (const uint32_t *)bl;
}

// the call-level checks of a non-empty job; then the CSR conditions by k_rp_tally_validate, its flag read back before anything gathers
int tally_checks(Job &J, bool null_args, bool claims) {
  bppp_rp *rp = J.rp;
  bppp_ctx *ctx = rp->ctx;
  const std::string who = J.who;
  const size_t nr = rp->D.nr, lim = RPP_LIM31;
  if (!nr || J.rows > lim / nr) return fail(ctx, BPPP_ERR_ARG, who + ": rows * nranges must be below 2^31");
  if (J.nnz > lim || J.nsums > lim) return fail(ctx, BPPP_ERR_ARG, who + ": nnz and nsums must be below 2^31");
  if (null_args || !J.start || (J.nnz && !J.entries)) return fail(ctx, BPPP_ERR_ARG, who + ": null input");
  if (claims) {
    const bool binary = rp->st.kind == 1;
    const int given = (J.amt ? 1 : 0) + (J.bl ? 1 : 0) + ((!binary && J.ty) ? 1 : 0), all = binary ? 2 : 3;
    if (given && given != all) return fail(ctx, BPPP_ERR_ARG, who + ": claim_amounts, claim_types and " + J.bl_name + " must be given together or all be NULL");
    J.zero_claims = !given;
  }
  hipSetDevice(ctx->device);
  int rc = rpp_ensure_pwork(rp, 256); if (rc) return rc;
  uint32_t *flag = (uint32_t *)rp->pwork, h[2];
  hipStream_t st = ctx->stream;
  BPPP_HIP(ctx, hipMemsetAsync(flag, 0xFF, 8, st));
  const uint64_t n = std::max<uint64_t>(J.nsums + 1, J.nnz), total = (uint64_t)J.rows * nr;
  k_rp_tally_validate<<<dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, st>>>((uint32_t)J.nsums, (uint32_t)J.nnz, (uint32_t)total, J.start, J.entries, flag);
  BPPP_HIP(ctx, hipGetLastError());
  BPPP_HIP(ctx, hipMemcpyAsync(h, flag, 8, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  if (h[0] != TALLY_NONE) {                     // h[0] <= nsums: one word of an array of nsums + 1
    uint32_t v = 0;
    BPPP_HIP(ctx, hipMemcpy(&v, J.start + h[0], 4, hipMemcpyDeviceToHost));
    return fail(ctx, BPPP_ERR_ARG, who + ": sum_start[" + std::to_string(h[0]) + "] = " + std::to_string(v) + " is not non-decreasing from 0 to nnz = " + std::to_string(J.nnz));
  }
  if (h[1] != TALLY_NONE) {                     // h[1] < nnz
    uint32_t v = 0;
    BPPP_HIP(ctx, hipMemcpy(&v, J.entries + h[1], 4, hipMemcpyDeviceToHost));
    return fail(ctx, BPPP_ERR_ARG, who + ": entries[" + std::to_string(h[1]) + "]: index " + std::to_string(v & ~TALLY_FINAL) + " is not below rows * nranges = " + std::to_string(total));
  }
  J.h_start.resize(J.nsums + 1);
  BPPP_HIP(ctx, hipMemcpy(J.h_start.data(), J.start, (J.nsums + 1) * 4, hipMemcpyDeviceToHost));
  return BPPP_OK;
}

static_assert(sizeof(bppp_tally::Item) == sizeof(uint4), "an item is the kernel's uint4");
std::vector<size_t> chunk_bounds(const Job &J) { return bppp_tally::chunk_bounds(J.h_start.data(), J.nsums, J.rp->tally_chunk); }
Levels plan_levels(const Job &J, size_t t0, size_t t1) {
  return bppp_tally::plan_levels(J.h_start.data(), t0, t1, (uint32_t)std::min<size_t>(J.rp->tally_short_max, 0xFFFFFFFFu), (uint32_t)std::min<size_t>(J.rp->tally_piece, 0x7FFFFFFFu));
}
Plan make_plan(const Job &J) {
  Plan P;
  P.cb = chunk_bounds(J);
  for (size_t c = 0; c + 1 < P.cb.size(); c++) {
    P.plans.push_back(plan_levels(J, P.cb[c], P.cb[c + 1]));
    P.ns_max = std::max(P.ns_max, P.cb[c + 1] - P.cb[c]); P.ni = std::max(P.ni, P.plans[c].nitems);
    for (int k = 0; k < 2; k++) P.np[k] = std::max(P.np[k], P.plans[c].npart[k]);
  }
  return P;
}

// ns: the sums of the largest chunk; each: the per-sum pass (ni items, np[2] partial points); batch: the weighted combination (ne entries a MSM);
// extra: bytes behind everything else for the caller's own arrays (csrc/rpexcess.hip), so that the arrays above lie where they lay without them;
// J.tail: points behind the decoded pool that the caller fills (csrc/rpexkeys.hip), none in a plain tally
int carve(const Job &J, size_t ns, bool each, size_t ni, const size_t np[2], bool batch, size_t ne, Work &W, size_t extra) {
  bppp_rp *rp = J.rp;
  const size_t total = J.rows * rp->D.nr, R = std::max<size_t>(1, std::min<size_t>(J.rows, ((size_t)1 << 22) / rp->D.nr));
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    W.pool = cv.take<uint32_t>((total + J.tail) * 16 + 16); W.bad = cv.take<uint32_t>(R); W.any = cv.take<uint32_t>(4);
    W.in_sc = cv.take<uint32_t>(ns * 24); W.flag = cv.take<uint32_t>(ns); W.zero = cv.take<uint32_t>(J.zero_claims ? ns * 8 : 0);
    W.sums = cv.take<uint32_t>(each ? ns * XYZZ_WORDS : 0); W.malformed = cv.take<uint32_t>(each ? ns : 0); W.rec = cv.take<uint32_t>(each ? ns * 16 : 0);
    W.status = cv.take<uint32_t>(each ? ns : 0); W.zz = cv.take<uint32_t>(each ? ns * 8 : 0); W.zinv = cv.take<uint32_t>(each ? ns * 8 : 0);
    W.xy = cv.take<uint32_t>(each ? ns * 16 : 0); W.items = cv.take<uint4>(each ? ni : 0);
    for (int k = 0; k < 2; k++) W.part[k] = cv.take<uint32_t>(each ? np[k] * XYZZ_WORDS : 0);
    W.rho = cv.take<uint32_t>(batch ? ns * 8 : 0); W.prods = cv.take<uint32_t>(batch ? ns * 24 : 0); W.red = cv.take<uint32_t>(batch ? (size_t)RPP_REDUCE_BLOCKS * 24 : 0);
    W.sc3 = cv.take<uint32_t>(24); W.msm_sc = cv.take<uint32_t>(batch ? (ne + 3) * 8 : 0); W.msm_pt = cv.take<uint32_t>(batch ? (ne + 3) * 16 : 0);
    W.seed = cv.take<uint8_t>(32); W.extra = cv.take<uint8_t>(extra);
    if (!pass) { int rc = rpp_ensure_pwork(rp, cv.off); if (rc) return rc; }
  }
  return BPPP_OK;
}

// the pool decoded once: W.pool [rows][nranges][16]; which rows hold an x without a point is not kept — a sum learns it from what it gathers
int decode_pool(const Job &J, const Work &W) {
  bppp_rp *rp = J.rp;
  bppp_ctx *ctx = rp->ctx;
  const size_t nr = rp->D.nr, R = std::max<size_t>(1, std::min<size_t>(J.rows, ((size_t)1 << 22) / nr));
  for (size_t o = 0; o < J.rows; o += R) {
    const size_t rows = std::min(R, J.rows - o);
    BPPP_HIP(ctx, hipMemsetAsync(W.bad, 0, rows * 4, ctx->stream));
    rp_decode_coms(rp, rows, J.coms + o * rp->D.coms_bytes, W.pool + o * nr * 16, W.bad, W.any + 2);
    BPPP_HIP(ctx, hipGetLastError());
  }
  return BPPP_OK;
}

// the signed sums of [t0, t0 + ns) into W.sums, their malformed flags into W.malformed: one lane a short sum, then the plan's levels
int sum_launches(const Job &J, const Work &W, size_t t0, size_t ns, const Levels &L) {
  bppp_rp *rp = J.rp;
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  const uint32_t smax = (uint32_t)rp->tally_short_max;
  BPPP_HIP(ctx, hipMemsetAsync(W.malformed, 0, ns * 4, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.any, 0, 8, st));
  k_rp_tally_sum<<<dim3((unsigned)((ns + TALLY_LANES - 1) / TALLY_LANES)), dim3(TALLY_LANES), 0, st>>>(0u, (uint32_t)ns, smax, J.start + t0, J.entries, W.pool, nullptr, nullptr, nullptr,
                                                                                                    W.sums, W.malformed);
  size_t io = 0;
  for (size_t k = 0; k < L.lv.size(); k++) {
    const std::vector<bppp_tally::Item> &items = L.lv[k];
    BPPP_HIP(ctx, hipMemcpyAsync(W.items + io, items.data(), items.size() * sizeof(uint4), hipMemcpyHostToDevice, st));
    k_rp_tally_sum<<<dim3((unsigned)items.size()), dim3(TALLY_LANES), 0, st>>>(k ? 2u : 1u, (uint32_t)items.size(), smax, J.start + t0, J.entries, W.pool, W.items + io,
                                                                             W.part[(k + 1) & 1], W.part[k & 1], W.sums, W.malformed);
    io += items.size();
  }
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

int affine_launch(bppp_ctx *ctx, size_t n, const uint32_t *sums, const uint32_t *zinv, uint32_t *out) {
  k_rp_tally_affine<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>((uint32_t)n, sums, zinv, out);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

}  // namespace tally
}  // namespace bppp

namespace bppp {
namespace tally {

// sums [t0, t0 + ns): the claimed scalars in W.in_sc / W.flag, W.any[1] raised by a non-canonical one
int claim_scalars(const Job &J, const Work &W, size_t t0, size_t ns) {
  bppp_ctx *ctx = J.rp->ctx;
  if (J.zero_claims) {
    BPPP_HIP(ctx, hipMemsetAsync(W.zero, 0, ns * 32, ctx->stream));
    return rpp_claim_scalars(J.rp, ns, W.zero, W.zero, W.zero, W.in_sc, W.flag, W.any + 1);
  }
  return rpp_claim_scalars(J.rp, ns, J.amt + t0 * 8, J.ty ? J.ty + t0 * 8 : nullptr, J.bl + t0 * 8, W.in_sc, W.flag, W.any + 1);
}

// every sum decided on its own: status [nsums] and, when not NULL, sums_xy [nsums][8], both on the host.  The job has passed tally_checks.
// ext (rp_internal.hpp): what the stated keys add; nullptr queues a plain tally's launches
int each_pass(const Job &J0, uint32_t *status, uint64_t *sums_xy, const Ext *ext) {
  Job Jx;
  if (ext) Jx = J0;                             // prepare points its copy at the merged arrays
  const Job &J = ext ? Jx : J0;
  bppp_rp *rp = J.rp;
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  int rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const Plan P = make_plan(J);
  Work W;
  if ((rc = carve(J, P.ns_max, true, P.ni, P.np, false, 0, W, ext ? ext->extra : 0)) || (rc = decode_pool(J, W))) return rc;
  if (ext && (rc = ext->prepare(Jx, W))) return rc;
  for (size_t c = 0; c + 1 < P.cb.size(); c++) {
    const size_t t0 = P.cb[c], ns = P.cb[c + 1] - t0;
    if ((rc = sum_launches(J, W, t0, ns, P.plans[c]))) return rc;
    if ((rc = claim_scalars(J, W, t0, ns)) || (rc = rpp_commit_inputs(rp, W.in_sc, ns, W.rec))) return rc;
    k_rp_tally_compare<<<dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st>>>((uint32_t)ns, W.sums, W.rec, W.flag, W.malformed, W.status, sums_xy ? W.zz : nullptr);
    BPPP_HIP(ctx, hipGetLastError());
    if (ext && (rc = ext->judge(W, t0, ns, sums_xy != nullptr))) return rc;
    BPPP_HIP(ctx, hipMemcpyAsync(status + t0, W.status, ns * 4, hipMemcpyDeviceToHost, st));
    if (sums_xy) {
      if ((rc = batch_inverse_run(ctx, W.zz, ns, 0, W.zinv))) return rc;
      if ((rc = affine_launch(ctx, ns, W.sums, W.zinv, W.xy))) return rc;
      BPPP_HIP(ctx, hipMemcpyAsync(sums_xy + t0 * 8, W.xy, ns * 64, hipMemcpyDeviceToHost, st));
    }
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return BPPP_OK;
}

// the assembly of a pass's MSM, apart from the MSM itself (rp_internal.hpp): batch_run below queues these, and so does the block call
// (csrc/rpblock.hip) into its own buffers
int batch_weights(const Job &J, const Work &W, size_t t0, size_t ns, uint64_t j0) {
  bppp_rp *rp = J.rp;
  bppp_ctx *ctx = rp->ctx;
  int rc;
  if ((rc = claim_scalars(J, W, t0, ns))) return rc;
  k_rp_tally_weights<<<dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, ctx->stream>>>((uint32_t)ns, rp->st.kind == 1, j0, W.seed, W.in_sc, W.rho, W.prods);
  BPPP_HIP(ctx, hipGetLastError());
  return rpp_negated_column_sums(rp, ns, W.prods, W.red, W.sc3);        // - sum rho a, - sum rho ty, - sum rho e: the scalars of g, H0, H1
}
int batch_terms(const Job &J, const Work &W, size_t t0, size_t ns, size_t e0, size_t n, uint32_t *sc, uint32_t *pt) {
  bppp_ctx *ctx = J.rp->ctx;
  if (n) k_rp_tally_terms<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>((uint32_t)n, (uint32_t)e0, J.start + t0, (uint32_t)ns, J.entries, W.pool, W.rho, sc, pt, W.any);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

// all sums by one weighted combination per pass: *accept, status (NULL, or [nsums]: one exact pass when rejected) and combined_xy (NULL or [8]), on
// the host.  The job has passed tally_checks and *accept is 0.  ext as for each_pass.
int batch_run(const Job &J0, uint64_t index_offset, const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy, const Ext *ext) {
  Job Jx;
  if (ext) Jx = J0;
  const Job &J = ext ? Jx : J0;
  bppp_rp *rp = J.rp;
  bppp_ctx *ctx = rp->ctx;
  const size_t nsums = J.nsums, nnz = J.nnz;
  int rc;
  if (combined_xy) memset(combined_xy, 0, 64);
  hipStream_t st = ctx->stream;
  const std::vector<size_t> cb = chunk_bounds(J);
  const size_t E = std::max<size_t>(1, rp->tally_chunk), no_parts[2] = {0, 0};
  size_t ns_max = 0;
  for (size_t c = 0; c + 1 < cb.size(); c++) ns_max = std::max(ns_max, cb[c + 1] - cb[c]);
  Work W;
  if ((rc = carve(J, ns_max, false, 0, no_parts, true, std::min(E, std::max<size_t>(1, nnz)), W, ext ? ext->extra : 0)) || (rc = decode_pool(J, W))) return rc;
  if (ext && (rc = ext->prepare(Jx, W))) return rc;
  BPPP_HIP(ctx, hipMemcpyAsync(W.seed, seed, 32, hipMemcpyHostToDevice, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.any, 0, 8, st));
  BatchParts parts;                             // one combined point per MSM
  for (size_t c = 0; c + 1 < cb.size(); c++) {
    const size_t t0 = cb[c], ns = cb[c + 1] - t0;
    if ((rc = batch_weights(J, W, t0, ns, index_offset + t0))) return rc;
    // the entries of the chunk, at most E to a MSM (a chunk of more is one long sum); the three claim terms ride with the first
    size_t e0 = J.h_start[t0];
    const size_t e1 = J.h_start[t0 + ns];
    bool first = true;
    do {
      const size_t n = std::min(E, e1 - e0);
      if ((rc = batch_terms(J, W, t0, ns, e0, n, W.msm_sc, W.msm_pt))) return rc;
      if (first) BPPP_HIP(ctx, hipMemcpyAsync(W.msm_sc + n * 8, W.sc3, 96, hipMemcpyDeviceToDevice, st));
      else BPPP_HIP(ctx, hipMemsetAsync(W.msm_sc + n * 8, 0, 96, st));
      BPPP_HIP(ctx, hipMemcpyAsync(W.msm_pt + n * 16, rp->d_basis, 3 * 64, hipMemcpyDeviceToDevice, st));   // [g | H0 | H1 ...]: the registered basis starts with them
      if ((rc = parts.msm(ctx, W.msm_sc, W.msm_pt, n + 3))) return rc;
      e0 += n; first = false;
    } while (e0 < e1);
  }
  uint32_t any[2];
  BPPP_HIP(ctx, hipMemcpy(any, W.any, 8, hipMemcpyDeviceToHost));
  bool reject = false;
  if (ext && (rc = ext->rejects(W, reject))) return rc;
  if ((rc = parts.finish(ctx, any[0] || any[1] || reject, combined_xy, accept))) return rc;
  if (!status) return BPPP_OK;
  if (*accept) { memset(status, 0, nsums * 4); return BPPP_OK; }
  return each_pass(J0, status, nullptr, ext);   // one exact pass, whatever the number of bad sums
}

}  // namespace tally
}  // namespace bppp

using namespace bppp;
using namespace bppp::tally;

namespace {

int tally_each_device(bppp_rp *rp, size_t rows, const void *d_coms, size_t nsums, const void *d_start, const void *d_entries, size_t nnz, const void *d_amt, const void *d_ty,
                      const void *d_bl, uint32_t *status, uint64_t *sums_xy) {
  if (!rp) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  Job J;
  fill(J, rp, "rp_tally_each", rows, d_coms, nsums, d_start, d_entries, nnz, d_amt, d_ty, d_bl);
  int rc = tally_checks(J, (rows && !d_coms) || !status, true);
  return rc ? rc : each_pass(J, status, sums_xy);
}

int tally_batch_device(bppp_rp *rp, size_t rows, const void *d_coms, size_t nsums, const void *d_start, const void *d_entries, size_t nnz, const void *d_amt, const void *d_ty,
                       const void *d_bl, uint64_t index_offset, const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  if (!nsums) { if (combined_xy) memset(combined_xy, 0, 64); *accept = 1; return BPPP_OK; }
  Job J;
  fill(J, rp, "rp_tally_batch", rows, d_coms, nsums, d_start, d_entries, nnz, d_amt, d_ty, d_bl);
  int rc = tally_checks(J, (rows && !d_coms) || !seed, true); if (rc) return rc;
  return batch_run(J, index_offset, seed, accept, status, combined_xy, nullptr);
}

int tally_claims_device(bppp_rp *rp, size_t rows, const void *d_amt, const void *d_ty, const void *d_bl, size_t nsums, const void *d_start, const void *d_entries, size_t nnz,
                        void *d_out_a, void *d_out_ty, void *d_out_e) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  const bool binary = rp->st.kind == 1;
  Job J;
  fill(J, rp, "rp_tally_claims", rows, nullptr, nsums, d_start, d_entries, nnz, nullptr, nullptr, nullptr);
  int rc = tally_checks(J, (rows && (!d_amt || (!d_ty && !binary) || !d_bl)) || !d_out_a || (!d_out_ty && !binary) || !d_out_e, false); if (rc) return rc;
  hipStream_t st = ctx->stream;
  uint32_t *flag = (uint32_t *)rp->pwork, bad = TALLY_NONE;      // tally_checks made sure of 256 bytes
  BPPP_HIP(ctx, hipMemsetAsync(flag, 0xFF, 4, st));
  k_rp_tally_claims<<<dim3((unsigned)((nsums + 3) / 4)), dim3(256), 0, st>>>((uint32_t)nsums, binary, J.start, J.entries, (const uint32_t *)d_amt, (const uint32_t *)d_ty,
                                                                          (const uint32_t *)d_bl, (uint32_t *)d_out_a, (uint32_t *)d_out_ty, (uint32_t *)d_out_e, flag);
  BPPP_HIP(ctx, hipGetLastError());
  BPPP_HIP(ctx, hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  if (bad != TALLY_NONE) return fail(ctx, BPPP_ERR_ARG, "rp_tally_claims: sum " + std::to_string(bad) + ": a referenced type or blinding is not canonical (>= n)");
  return BPPP_OK;
}

}  // namespace

extern "C" {

int bppp_rp_tally_each_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                              const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_blinds, uint32_t *tally_status, uint64_t *sums_xy) {
  return tally_each_device(rp, rows, d_coms_files, nsums, d_sum_start, d_entries, nnz, d_claim_amounts, d_claim_types, d_claim_blinds, tally_status, sums_xy);
}

int bppp_rp_tally_each(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                       const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_blinds, uint32_t *tally_status, uint64_t *sums_xy) {
  if (!rp) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  HostCsr H;
  if (rpp_sizes_ok(rp, rows, nsums, nnz)) {
    int rc = H.up(rp, rows, coms_files, rp->D.coms_bytes, nsums, sum_start, entries, nnz, claim_amounts, claim_types, claim_blinds, nsums * 32);
    if (rc) return rc;
  }
  return tally_each_device(rp, rows, H.coms.p, nsums, H.start.p, H.entries.p, nnz, H.a.p, H.ty.p, H.e.p, tally_status, sums_xy);
}

int bppp_rp_tally_batch_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                               const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_blinds, uint64_t index_offset, const uint8_t seed[32],
                               int *accept, uint32_t *tally_status, uint64_t *combined_xy) {
  return tally_batch_device(rp, rows, d_coms_files, nsums, d_sum_start, d_entries, nnz, d_claim_amounts, d_claim_types, d_claim_blinds, index_offset, seed, accept,
                            tally_status, combined_xy);
}

int bppp_rp_tally_batch(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                        const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_blinds, const uint8_t seed[32], int *accept,
                        uint32_t *tally_status, uint64_t *combined_xy) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  *accept = 0;
  HostCsr H;
  if (nsums && rpp_sizes_ok(rp, rows, nsums, nnz)) {
    int rc = H.up(rp, rows, coms_files, rp->D.coms_bytes, nsums, sum_start, entries, nnz, claim_amounts, claim_types, claim_blinds, nsums * 32);
    if (rc) return rc;
  }
  return tally_batch_device(rp, rows, H.coms.p, nsums, H.start.p, H.entries.p, nnz, H.a.p, H.ty.p, H.e.p, 0, seed, accept, tally_status, combined_xy);
}

int bppp_rp_tally_claims_device(bppp_rp *rp, size_t rows, const void *d_amounts, const void *d_types, const void *d_blinds, size_t nsums, const void *d_sum_start,
                                const void *d_entries, size_t nnz, void *d_claim_amounts, void *d_claim_types, void *d_claim_blinds) {
  return tally_claims_device(rp, rows, d_amounts, d_types, d_blinds, nsums, d_sum_start, d_entries, nnz, d_claim_amounts, d_claim_types, d_claim_blinds);
}

int bppp_rp_tally_claims(bppp_rp *rp, size_t rows, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, size_t nsums, const uint32_t *sum_start,
                         const uint32_t *entries, size_t nnz, uint64_t *claim_amounts, uint64_t *claim_types, uint64_t *claim_blinds) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  HostCsr H;
  DevBuf oa, oty, oe;
  if (rpp_sizes_ok(rp, rows, nsums, nnz)) {
    int rc = H.up(rp, 0, nullptr, 0, nsums, sum_start, entries, nnz, amounts, types, blinds, rows * rp->D.nr * 32);
    if (!rc) rc = oa.out(ctx, claim_amounts, nsums * 32);
    if (!rc) rc = oty.out(ctx, claim_types, nsums * 32);
    if (!rc) rc = oe.out(ctx, claim_blinds, nsums * 32);
    if (rc) return rc;
  }
  int rc = tally_claims_device(rp, rows, H.a.p, H.ty.p, H.e.p, nsums, H.start.p, H.entries.p, nnz, oa.p, oty.p, oe.p);
  if (rc) return rc;
  BPPP_HIP(ctx, hipMemcpy(claim_amounts, oa.p, nsums * 32, hipMemcpyDeviceToHost));
  if (oty.p) BPPP_HIP(ctx, hipMemcpy(claim_types, oty.p, nsums * 32, hipMemcpyDeviceToHost));
  BPPP_HIP(ctx, hipMemcpy(claim_blinds, oe.p, nsums * 32, hipMemcpyDeviceToHost));
  return BPPP_OK;
}

}  // extern "C"
