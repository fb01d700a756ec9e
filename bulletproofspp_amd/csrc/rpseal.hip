// rpseal.hip — sealed outputs: a one-sided receive and the view-key scan of an output set: bppp_rp_seal*, bppp_rp_scan* (include/bppp.h
// states the protocol and every message).
//   seal   R = r B by the window table the commitments use, P = r A by the quad walk (csrc/rpexcess.hip.h: a scalar and a point of its own per
//          row), then the shared secret, the view tag, the blindings and the memos, one lane per row and one per (row, range)
//   scan   passes of bounded workspace over the rows: R lifted (csrc/rplift.hip.h), a R by the FIXED-SCALAR walk (csrc/rpseal.hip.h: one lane
//          per row, the recoded view secret a kernel argument), affine P with the shared secret and the tag, the tag's survivors compacted,
//          and for survivors only: pads, the decrypted opening, its commitment over the table csrc/rpcommit.hip shares, the comparison with
//          the lifted commitment of the file and the scatter of verdicts and openings.  A foreign row costs the walk and two hashes.
// Kernels (one lane per row unless said otherwise):
//   k_rp_seal_check    the view key lifted, the verdict of the row, the scalar row of R and the walk's scalar (zero for a refused row)
//   k_rp_seal_mul      one QUAD per row: P = r A
//   k_rp_seal_shared   ss and the first 34 bytes of the seal
//   k_rp_seal_memo     one lane per (row, range): bl_i and memo_i
//   k_rp_scan_lift     the hint lifted; BAD_HINT or still open
//   k_rp_scan_walk     a R, XYZZ; a workgroup is one wavefront with its table in LDS
//   k_rp_scan_tag      affine P, ss, the tag; FOREIGN, or a slot among the survivors
//   k_rp_scan_open     one lane per (survivor, range): pads, the decrypted (v, ty, bl) as the three scalars of a commitment, the file's
//                      commitment lifted
//   k_rp_scan_judge    one lane per survivor: OWNED and the opening scattered, or TAG_ONLY
// Every kernel is bounds-checked on its own index, reads the seals and the files bytewise, takes the survivors' count as an argument read
// back by the host, and writes with ordinary vector stores.  All workspace is carved from rp->pwork.
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
#include "rpseal.hip.h"
#include "rpsealhash.hip.h"
#include "sha256.hip.h"

namespace bppp {

// ---- seal
__global__ void __launch_bounds__(64) k_rp_seal_check(uint32_t n, uint32_t nr, uint32_t binary, uint32_t slot, const uint8_t *__restrict__ keys,
                                                      const uint32_t *__restrict__ eph, const uint32_t *__restrict__ types, uint32_t *__restrict__ A,
                                                      uint32_t *__restrict__ c, uint32_t *__restrict__ in_sc, uint32_t *__restrict__ status) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  aff K;
  const bool key_ok = exk_lift(keys + (size_t)b * EX_KEY, K);
  const fe r = fe_load(eph + (size_t)b * 8);
  bool canon = wi_canonical(r);
  if (!binary) for (uint32_t i = 0; i < nr; i++) canon = canon && wi_canonical(fe_load(types + ((size_t)b * nr + i) * 8));
  const uint32_t st = !key_ok ? (uint32_t)BPPP_RP_EXCESS_BAD_KEY : !canon ? (uint32_t)BPPP_RP_SEAL_NOT_CANONICAL : fe_is_zero(r) ? (uint32_t)BPPP_RP_SEAL_ZERO : (uint32_t)BPPP_RP_SEAL_OK;
  const fe rr = st == BPPP_RP_SEAL_OK ? r : fe_zero();
  aff_store(A + (size_t)b * 16, K);
  fe_store(c + (size_t)b * 8, rr);
  for (uint32_t s = 0; s < 3; s++) fe_store(in_sc + ((size_t)b * 3 + s) * 8, s == slot ? rr : fe_zero());
  status[b] = st;
}
__global__ void __launch_bounds__(64) k_rp_seal_mul(uint32_t n, const uint32_t *__restrict__ c, const uint32_t *__restrict__ A, uint32_t *__restrict__ P) {
  const uint32_t b = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (b >= n) return;
  const xyzz acc = excess_mul_quad(fe_load(c + (size_t)b * 8), aff_load(A + (size_t)b * 16));
  if (quad_lane() == 0) aff_store(P + (size_t)b * 16, xyzz_to_aff(acc));
}
__global__ void __launch_bounds__(64) k_rp_seal_shared(uint32_t n, uint32_t seal_bytes, SealDomains D, const uint32_t *__restrict__ P, const uint32_t *__restrict__ R,
                                                       const uint32_t *__restrict__ status, uint32_t *__restrict__ ssbuf, uint8_t *__restrict__ seals) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  uint8_t *seal = seals + (size_t)b * seal_bytes;
  if (status[b] != BPPP_RP_SEAL_OK) { for (uint32_t o = 0; o < SEAL_HEAD; o++) seal[o] = 0; return; }
  const uint32_t *Rb = R + (size_t)b * 16;
  uint32_t ss[8];
  seal_shared(D.ds, P + (size_t)b * 16, [&](uint32_t o) -> uint32_t { return ex_pt_byte(Rb, o); }, ss);
  for (uint32_t o = 0; o < EX_KEY; o++) seal[o] = (uint8_t)ex_pt_byte(Rb, o);
  seal[EX_KEY] = (uint8_t)seal_view_tag(D.dt, ss);
  for (int k = 0; k < 8; k++) ssbuf[(size_t)b * 8 + k] = ss[k];
}
__global__ void __launch_bounds__(64) k_rp_seal_memo(uint64_t n, uint32_t nr, uint32_t seal_bytes, uint32_t binary, SealDomains D, const uint32_t *__restrict__ amounts,
                                                     const uint32_t *__restrict__ types, const uint32_t *__restrict__ status, const uint32_t *__restrict__ ssbuf,
                                                     uint8_t *__restrict__ seals, uint32_t *__restrict__ blinds) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t b = j / nr;
  const uint32_t i = (uint32_t)(j % nr);
  uint8_t *memo = seals + b * seal_bytes + SEAL_HEAD + (size_t)i * SEAL_MEMO;
  if (status[b] != BPPP_RP_SEAL_OK) {
    for (uint32_t o = 0; o < SEAL_MEMO; o++) memo[o] = 0;
    fe_store(blinds + j * 8, fe_zero());
    return;
  }
  uint32_t ss[8], pad[16];
  for (int k = 0; k < 8; k++) ss[k] = ssbuf[b * 8 + k];
  seal_pad(D.dm, ss, i, pad);
  const fe v = wi_smod_n(fe_load(amounts + j * 8)), ty = binary ? fe_zero() : fe_load(types + j * 8);
  for (uint32_t o = 0; o < SEAL_MEMO; o++) memo[o] = (uint8_t)((o < 32 ? enc_be_byte(v.v, o) : enc_be_byte(ty.v, o - 32)) ^ ex_word_byte(pad, o));
  fe_store(blinds + j * 8, seal_blind(D.db, ss, i));
}

// ---- scan
__global__ void __launch_bounds__(64) k_rp_scan_lift(uint32_t n, uint32_t seal_bytes, const uint8_t *__restrict__ seals, uint32_t *__restrict__ R, uint32_t *__restrict__ status) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  aff H;
  const bool ok = exk_lift(seals + (size_t)b * seal_bytes, H);
  aff_store(R + (size_t)b * 16, H);
  status[b] = ok ? SCAN_OPEN : (uint32_t)BPPP_RP_SCAN_BAD_HINT;
}
__global__ void __launch_bounds__(64) k_rp_scan_walk(uint32_t n, ScanWalk W, const uint32_t *__restrict__ R, uint32_t *__restrict__ acc) {
  __shared__ ScanTab tab[SCAN_TAB_WORDS];
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n) return;
  xyzz_store(acc + (size_t)b * XYZZ_WORDS, scan_mul_lane(W, aff_load(R + (size_t)b * 16), tab, threadIdx.x));
}
// survivors: surv[0 .. count) in no particular order — every result is scattered by its row
__global__ void __launch_bounds__(64) k_rp_scan_tag(uint32_t n, uint32_t seal_bytes, SealDomains D, const uint8_t *__restrict__ seals, const uint32_t *__restrict__ acc,
                                                    uint32_t *__restrict__ status, uint32_t *__restrict__ ssbuf, uint32_t *__restrict__ surv, uint32_t *__restrict__ count) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n || status[b] != SCAN_OPEN) return;
  const uint8_t *seal = seals + (size_t)b * seal_bytes;
  uint32_t P[16], ss[8];
  scan_affine_lane(acc + (size_t)b * XYZZ_WORDS, P);
  seal_shared(D.ds, P, [&](uint32_t o) -> uint32_t { return seal[o]; }, ss);
  if (seal_view_tag(D.dt, ss) != seal[EX_KEY]) { status[b] = BPPP_RP_SCAN_FOREIGN; return; }
  for (int k = 0; k < 8; k++) ssbuf[(size_t)b * 8 + k] = ss[k];
  surv[atomicAdd(count, 1u)] = b;
}
__global__ void __launch_bounds__(64) k_rp_scan_open(uint64_t n, uint32_t nr, uint32_t seal_bytes, uint32_t coms_bytes, uint32_t binary, SealDomains D,
                                                     const uint8_t *__restrict__ seals, const uint8_t *__restrict__ coms, const uint32_t *__restrict__ surv,
                                                     const uint32_t *__restrict__ ssbuf, uint32_t *__restrict__ in_sc, uint32_t *__restrict__ flag, uint32_t *__restrict__ dec) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t b = surv[j / nr], i = (uint32_t)(j % nr);
  const uint8_t *memo = seals + (size_t)b * seal_bytes + SEAL_HEAD + (size_t)i * SEAL_MEMO;
  uint32_t ss[8], pad[16];
  for (int k = 0; k < 8; k++) ss[k] = ssbuf[(size_t)b * 8 + k];
  seal_pad(D.dm, ss, i, pad);
  uint8_t plain[SEAL_MEMO];
  for (uint32_t o = 0; o < SEAL_MEMO; o++) plain[o] = (uint8_t)(memo[o] ^ ex_word_byte(pad, o));
  fe v = load_field_be_raw(plain), ty = load_field_be_raw(plain + 32), bl = seal_blind(D.db, ss, i);
  const bool bad = !wi_canonical(v) || !wi_canonical(ty) || (binary && !fe_is_zero(ty));
  if (bad) { v = fe_zero(); ty = fe_zero(); bl = fe_zero(); }
  fe_store(in_sc + j * 24, v); fe_store(in_sc + j * 24 + 8, binary ? bl : ty); fe_store(in_sc + j * 24 + 16, binary ? ty : bl);
  flag[j] = bad ? 1u : 0u;
  // commitment i of the row's file, as decodeCommitments lifts it: the infinity encoding when the x has no curve point
  const uint8_t *file = coms + (size_t)b * coms_bytes;
  bool ok;
  aff C = rp_lift_x(load_field_be<0>(file + (nr + 7) / 8 + (size_t)i * 32), ((file[i >> 3] >> (i & 7)) & 1u) != 0, ok);
  if (!ok) C = aff_inf();
  aff_store(dec + j * 16, C);
}
__global__ void __launch_bounds__(64) k_rp_scan_judge(uint32_t n, uint32_t nr, uint32_t binary, const uint32_t *__restrict__ surv, const uint32_t *__restrict__ in_sc,
                                                      const uint32_t *__restrict__ flag, const uint32_t *__restrict__ dec, const uint32_t *__restrict__ rec,
                                                      uint32_t *__restrict__ status, uint32_t *__restrict__ amounts, uint32_t *__restrict__ types, uint32_t *__restrict__ blinds) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint32_t b = surv[s];
  bool owned = true;
  for (uint32_t i = 0; i < nr; i++) {
    const size_t j = (size_t)s * nr + i;
    uint32_t any = 0, diff = 0;
    for (int k = 0; k < 16; k++) { const uint32_t d = dec[j * 16 + k]; any |= d; diff |= d ^ rec[j * 16 + k]; }
    owned = owned && !flag[j] && any && !diff;
  }
  status[b] = owned ? (uint32_t)BPPP_RP_SCAN_OWNED : (uint32_t)BPPP_RP_SCAN_TAG_ONLY;
  if (!owned) return;
  for (uint32_t i = 0; i < nr; i++) {
    const size_t j = (size_t)s * nr + i, o = ((size_t)b * nr + i) * 8;
    const uint32_t *sc = in_sc + j * 24;                // base order: typed (v, ty, bl), binary (v, bl, 0)
    for (int k = 0; k < 8; k++) {
      if (amounts) amounts[o + k] = sc[k];
      if (types) types[o + k] = binary ? 0u : sc[8 + k];
      if (blinds) blinds[o + k] = binary ? sc[8 + k] : sc[16 + k];
    }
  }
}

}  // namespace bppp

using namespace bppp;
using namespace bppp::excess;

namespace bppp {
SealDomains seal_domains(const bppp_rp *rp) {
  return {domain("bppp/seal/shared/v1", rp->tag), domain("bppp/seal/tag/v1", rp->tag), domain("bppp/seal/blind/v1", rp->tag), domain("bppp/seal/memo/v1", rp->tag)};
}
void scan_lift_launch(bppp_rp *rp, uint32_t n, const uint8_t *d_seals, uint32_t *R, uint32_t *status) {
  k_rp_scan_lift<<<dim3((n + 63) / 64), dim3(64), 0, rp->ctx->stream>>>(n, (uint32_t)BPPP_RP_SEAL_BYTES(rp->D.nr), d_seals, R, status);
}
}  // namespace bppp

namespace {

size_t seal_row_bytes(const bppp_rp *rp) { return BPPP_RP_SEAL_BYTES(rp->D.nr); }
// rows per pass over the workspace, as the commit and open calls count them
size_t pass_rows(const bppp_rp *rp, size_t rows) { return std::max<size_t>(1, std::min(rows, rpp_flat_chunk(rp) / rp->D.nr)); }

const char *seal_status_text(uint32_t s) {
  return s == BPPP_RP_EXCESS_BAD_KEY        ? "the view key's sign byte is above 1, or its x has no curve point"
         : s == BPPP_RP_SEAL_NOT_CANONICAL ? "the ephemeral secret or a type is not canonical (>= n)"
                                           : "the ephemeral secret is zero";
}

int checks(bppp_rp *rp, size_t rows, const char *who, bool null_args) {
  bppp_ctx *ctx = rp->ctx;
  if (null_args) return fail(ctx, BPPP_ERR_ARG, std::string(who) + ": null input");
  if (!rp->D.nr || rows > RPP_LIM31 / rp->D.nr) return fail(ctx, BPPP_ERR_ARG, std::string(who) + ": rows * nranges must be below 2^31");
  hipSetDevice(ctx->device);
  return BPPP_OK;
}

int seal_device(bppp_rp *rp, size_t batch, const void *d_keys, const void *d_eph, const void *d_amounts, const void *d_types, void *d_seals, void *d_blinds,
                uint32_t *seal_status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!batch) return BPPP_OK;
  const bool binary = rp->st.kind == 1;
  int rc = checks(rp, batch, "rp_seal", !d_keys || !d_eph || !d_amounts || (!d_types && !binary) || !d_seals || !d_blinds); if (rc) return rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const size_t nr = rp->D.nr, sb = seal_row_bytes(rp), C = pass_rows(rp, batch);
  uint32_t *A = nullptr, *c = nullptr, *in_sc = nullptr, *R = nullptr, *P = nullptr, *ss = nullptr, *status = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    A = cv.take<uint32_t>(C * 16); c = cv.take<uint32_t>(C * 8); in_sc = cv.take<uint32_t>(C * 24); R = cv.take<uint32_t>(C * 16); P = cv.take<uint32_t>(C * 16);
    ss = cv.take<uint32_t>(C * 8); status = cv.take<uint32_t>(C);
    if (!pass && (rc = rpp_ensure_pwork(rp, cv.off))) return rc;
  }
  hipStream_t st = ctx->stream;
  const SealDomains D = seal_domains(rp);
  std::vector<uint32_t> h_status(batch);
  for (size_t o = 0; o < batch; o += C) {
    const size_t n = std::min(C, batch - o);
    const dim3 rows_grid((unsigned)((n + 63) / 64));
    const uint32_t *ty = binary ? nullptr : (const uint32_t *)d_types + o * nr * 8;
    uint8_t *seals = (uint8_t *)d_seals + o * sb;
    k_rp_seal_check<<<rows_grid, dim3(64), 0, st>>>((uint32_t)n, (uint32_t)nr, binary, blind_slot(rp), (const uint8_t *)d_keys + o * EX_KEY, (const uint32_t *)d_eph + o * 8, ty, A, c,
                                                    in_sc, status);
    BPPP_HIP(ctx, hipGetLastError());
    if ((rc = rpp_commit_inputs(rp, in_sc, n, R))) return rc;
    k_rp_seal_mul<<<dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, st>>>((uint32_t)n, c, A, P);
    k_rp_seal_shared<<<rows_grid, dim3(64), 0, st>>>((uint32_t)n, (uint32_t)sb, D, P, R, status, ss, seals);
    k_rp_seal_memo<<<dim3((unsigned)((n * nr + 63) / 64)), dim3(64), 0, st>>>((uint64_t)n * nr, (uint32_t)nr, (uint32_t)sb, binary, D, (const uint32_t *)d_amounts + o * nr * 8, ty,
                                                                               status, ss, seals, (uint32_t *)d_blinds + o * nr * 8);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(h_status.data() + o, status, n * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return rpp_report_refusals(ctx, "rp_seal", "row", h_status.data(), batch, seal_status, seal_status_text);
}

struct ScanWork { uint32_t *R, *acc, *ss, *status, *surv, *count, *in_sc, *flag, *dec, *rec; };

int scan_device(bppp_rp *rp, const uint64_t view_secret[4], size_t rows, const void *d_coms, const void *d_seals, uint32_t *scan_status, void *d_amounts, void *d_types,
                void *d_blinds, size_t *nowned) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (nowned) *nowned = 0;
  if (!view_secret) return fail(ctx, BPPP_ERR_ARG, "rp_scan: null view secret");
  {
    const bppp_host::U256 a = bppp_host::U256::load(view_secret);
    if (a.is_zero() || bppp_host::cmp(a, bppp_host::FR().m) >= 0) return fail(ctx, BPPP_ERR_ARG, "rp_scan: the view secret must be in [1, n)");
  }
  if (!rows) return BPPP_OK;
  int rc = checks(rp, rows, "rp_scan", !d_coms || !d_seals || !scan_status); if (rc) return rc;
  ScanWalk W;
  if (!scan_recode(view_secret, W)) return fail(ctx, BPPP_ERR_ARG, "rp_scan: the view secret's halves do not fit the walk");
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const bool binary = rp->st.kind == 1;
  const size_t nr = rp->D.nr, sb = seal_row_bytes(rp), cb = rp->D.coms_bytes, C = pass_rows(rp, rows);
  ScanWork K;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    K.R = cv.take<uint32_t>(C * 16); K.acc = cv.take<uint32_t>(C * XYZZ_WORDS); K.ss = cv.take<uint32_t>(C * 8); K.status = cv.take<uint32_t>(C); K.surv = cv.take<uint32_t>(C);
    K.count = cv.take<uint32_t>(4); K.in_sc = cv.take<uint32_t>(C * nr * 24); K.flag = cv.take<uint32_t>(C * nr); K.dec = cv.take<uint32_t>(C * nr * 16);
    K.rec = cv.take<uint32_t>(C * nr * 16);
    if (!pass && (rc = rpp_ensure_pwork(rp, cv.off))) return rc;
  }
  hipStream_t st = ctx->stream;
  const SealDomains D = seal_domains(rp);
  // every row that is not owned receives zeros
  for (void *out : {d_amounts, d_types, d_blinds}) if (out) BPPP_HIP(ctx, hipMemsetAsync(out, 0, rows * nr * 32, st));
  size_t owned = 0;
  for (size_t o = 0; o < rows; o += C) {
    const size_t n = std::min(C, rows - o);
    const dim3 grid((unsigned)((n + 63) / 64));
    const uint8_t *seals = (const uint8_t *)d_seals + o * sb, *coms = (const uint8_t *)d_coms + o * cb;
    BPPP_HIP(ctx, hipMemsetAsync(K.count, 0, 16, st));
    k_rp_scan_lift<<<grid, dim3(64), 0, st>>>((uint32_t)n, (uint32_t)sb, seals, K.R, K.status);
    k_rp_scan_walk<<<grid, dim3(64), 0, st>>>((uint32_t)n, W, K.R, K.acc);
    k_rp_scan_tag<<<grid, dim3(64), 0, st>>>((uint32_t)n, (uint32_t)sb, D, seals, K.acc, K.status, K.ss, K.surv, K.count);
    BPPP_HIP(ctx, hipGetLastError());
    uint32_t ns = 0;
    BPPP_HIP(ctx, hipMemcpyAsync(&ns, K.count, 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
    if (ns > n) return fail(ctx, BPPP_ERR_HIP, "rp_scan: more survivors than rows");
    if (ns) {
      const uint64_t m = (uint64_t)ns * nr;
      k_rp_scan_open<<<dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st>>>(m, (uint32_t)nr, (uint32_t)sb, (uint32_t)cb, binary, D, seals, coms, K.surv, K.ss, K.in_sc, K.flag, K.dec);
      BPPP_HIP(ctx, hipGetLastError());
      if ((rc = rpp_commit_inputs(rp, K.in_sc, m, K.rec))) return rc;
      k_rp_scan_judge<<<dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, st>>>(ns, (uint32_t)nr, binary, K.surv, K.in_sc, K.flag, K.dec, K.rec, K.status,
                                                                            d_amounts ? (uint32_t *)d_amounts + o * nr * 8 : nullptr, d_types ? (uint32_t *)d_types + o * nr * 8 : nullptr,
                                                                            d_blinds ? (uint32_t *)d_blinds + o * nr * 8 : nullptr);
      BPPP_HIP(ctx, hipGetLastError());
    }
    BPPP_HIP(ctx, hipMemcpyAsync(scan_status + o, K.status, n * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
    for (size_t b = 0; b < n; b++) owned += scan_status[o + b] == BPPP_RP_SCAN_OWNED;
  }
  if (nowned) *nowned = owned;
  return BPPP_OK;
}

}  // namespace

extern "C" {

int bppp_rp_seal_device(bppp_rp *rp, size_t batch, const void *d_view_keys, const void *d_eph, const void *d_amounts, const void *d_types, void *d_seals, void *d_blinds,
                        uint32_t *seal_status) {
  return seal_device(rp, batch, d_view_keys, d_eph, d_amounts, d_types, d_seals, d_blinds, seal_status);
}

int bppp_rp_seal(bppp_rp *rp, size_t batch, const uint8_t *view_keys, const uint64_t *eph, const uint64_t *amounts, const uint64_t *types, uint8_t *seals, uint64_t *blinds,
                 uint32_t *seal_status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!batch) return BPPP_OK;
  int rc = checks(rp, batch, "rp_seal", !view_keys || !eph || !amounts || (!types && rp->st.kind != 1) || !seals || !blinds); if (rc) return rc;
  DevBuf k, e, amt, ty, s, bl;
  const size_t cl = batch * rp->D.nr * 32, sbytes = batch * seal_row_bytes(rp);
  if ((rc = k.up(ctx, view_keys, batch * EX_KEY)) || (rc = e.up(ctx, eph, batch * 32)) || (rc = amt.up(ctx, amounts, cl)) || (rc = ty.up(ctx, types, cl)) ||
      (rc = s.out(ctx, seals, sbytes)) || (rc = bl.out(ctx, blinds, cl))) return rc;
  rc = seal_device(rp, batch, k.p, e.p, amt.p, ty.p, s.p, bl.p, seal_status);
  const int r1 = rpp_download_refused(ctx, rc, "rp_seal: row ", seals, s.p, sbytes);          // a refusal: both outputs go down and the error stands
  return r1 != rc ? r1 : rpp_download_refused(ctx, rc, "rp_seal: row ", blinds, bl.p, cl);
}

int bppp_rp_scan_device(bppp_rp *rp, const uint64_t view_secret[4], size_t rows, const void *d_coms_files, const void *d_seals, uint32_t *scan_status, void *d_amounts,
                        void *d_types, void *d_blinds, size_t *nowned) {
  return scan_device(rp, view_secret, rows, d_coms_files, d_seals, scan_status, d_amounts, d_types, d_blinds, nowned);
}

int bppp_rp_scan(bppp_rp *rp, const uint64_t view_secret[4], size_t rows, const uint8_t *coms_files, const uint8_t *seals, uint32_t *scan_status, uint64_t *amounts,
                 uint64_t *types, uint64_t *blinds, size_t *nowned) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  DevBuf c, s, amt, ty, bl;
  if (rows && rp->D.nr && rows <= RPP_LIM31 / rp->D.nr) {
    hipSetDevice(ctx->device);
    const size_t cl = rows * rp->D.nr * 32;
    int rc;
    if ((rc = c.up(ctx, coms_files, rows * (size_t)rp->D.coms_bytes)) || (rc = s.up(ctx, seals, rows * seal_row_bytes(rp))) || (rc = amt.out(ctx, amounts, cl)) ||
        (rc = ty.out(ctx, types, cl)) || (rc = bl.out(ctx, blinds, cl))) return rc;
  }
  int rc = scan_device(rp, view_secret, rows, c.p, s.p, scan_status, amt.p, ty.p, bl.p, nowned);
  if (rc || !rows) return rc;
  const size_t cl = rows * rp->D.nr * 32;
  if (amounts) BPPP_HIP(ctx, hipMemcpy(amounts, amt.p, cl, hipMemcpyDeviceToHost));
  if (types) BPPP_HIP(ctx, hipMemcpy(types, ty.p, cl, hipMemcpyDeviceToHost));
  if (blinds) BPPP_HIP(ctx, hipMemcpy(blinds, bl.p, cl, hipMemcpyDeviceToHost));
  return BPPP_OK;
}

}  // extern "C"
