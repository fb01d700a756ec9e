// rpcut.hip — cut-through: bppp_rp_cut_through* (include/bppp.h).  The tally's job of T transactions, one sum each, becomes the one sum of a block:
// entries that add and subtract the same commitment are dropped in pairs, the pool and the entries are compacted, the claims are added up.
// The kernels are in csrc/rpcut.hip.h; this file holds the call: the tally's own checks (tally_checks, csrc/rptally.hip), the workspace carved from
// the handle's grow-only pwork, the launches in order, four small read-backs (the CSR verdict, the claims, the number of groups, the counts) and
// the outputs.  Nothing is written to an output before the last kernel has been queued without an error.
#include <string.h>
#include <algorithm>
#include <random>
#include <string>
#include "rp_internal.hpp"
#include "rphostcall.hpp"
#include "rpprove_host.hpp"
#include "rpcut.hip.h"

namespace bppp {
namespace {

// the scratch of one scan of n counts, in words: the workgroups' totals, and their scan level by level
size_t cut_scan_words(size_t n) {
  const size_t nb = (n + 1 + CUT_SCAN_TILE - 1) / CUT_SCAN_TILE;
  return nb <= 1 ? 1 : nb + (nb + 1) + cut_scan_words(nb);
}
int cut_scan(bppp_ctx *ctx, const uint32_t *in, size_t n, uint32_t *out, uint32_t *ws) {
  const size_t nb = (n + 1 + CUT_SCAN_TILE - 1) / CUT_SCAN_TILE;
  hipStream_t st = ctx->stream;
  k_cut_scan_tile<<<dim3((unsigned)nb), dim3(256), 0, st>>>((uint64_t)n, in, out, ws);
  BPPP_HIP(ctx, hipGetLastError());
  if (nb <= 1) return BPPP_OK;
  uint32_t *tsc = ws + nb;
  int rc = cut_scan(ctx, ws, nb, tsc, tsc + nb + 1);
  if (rc) return rc;
  k_cut_scan_add<<<dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st>>>((uint64_t)n, tsc, out);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

size_t cut_pow2_at_least(size_t n) { size_t s = 1; while (s < n) s <<= 1; return s; }

struct CutWork {
  uint32_t *flag, *err, *tot, *res, *claims, *part;
  uint32_t *idw, *slot, *win, *lead, *keep, *pos, *key, *startk, *endk, *perm[2], *status, *tab, *hist, *hoff, *scan;
  uint64_t *hs;
  uint32_t *rowmark, *F, *P, *row_map, *rowinv;
};

unsigned cut_grid(size_t n) { return (unsigned)((n + 255) / 256); }

int cut_through_device(bppp_rp *rp, size_t rows, const void *d_coms, size_t nsums, const void *d_start, const void *d_entries, size_t nnz, const void *d_amt,
                       const void *d_ty, const void *d_off, uint32_t *entry_status, uint32_t *row_map, void *d_new_coms, void *d_new_entries, uint64_t *block_claims,
                       bppp_rp_cut_counts *counts) {
  if (!rp || !counts) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums || !nnz) {
    memset(counts, 0, sizeof *counts);
    if (block_claims) memset(block_claims, 0, 96);
    return BPPP_OK;
  }
  tally::Job J;
  tally::fill(J, rp, "rp_cut_through", rows, d_coms, nsums, d_start, d_entries, nnz, d_amt, d_ty, d_off);
  J.bl_name = "claim_offsets";
  const bool any_claim = J.amt || J.ty || J.bl;
  int rc = tally::tally_checks(J, (rows && !d_coms) || !d_new_entries || (any_claim != (block_claims != nullptr)), true);
  if (rc) return rc;
  const bool binary = rp->st.kind == 1;
  const size_t nr = rp->D.nr, cb = rp->D.coms_bytes;
  hipStream_t st = ctx->stream;

  // the table: at least 2 nnz slots; the test hook may ask for fewer, never fewer than nnz
  size_t slots = cut_pow2_at_least(2 * nnz);
  if (rp->cut_table_bits > 0) slots = std::max(cut_pow2_at_least(nnz), (size_t)1 << std::min(rp->cut_table_bits, 32));
  const size_t nb = (nnz + CUT_SORT_TILE - 1) / CUT_SORT_TILE, scan_n = std::max(std::max(nnz, 2 * rows), 256 * nb);
  CutWork W;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    W.flag = cv.take<uint32_t>(64); W.err = W.flag + 4; W.tot = W.flag + 8; W.res = W.flag + 16; W.claims = W.flag + 32;
    W.part = cv.take<uint32_t>((size_t)CUT_CLAIM_BLOCKS * 24);
    W.idw = cv.take<uint32_t>(nnz * 8); W.hs = cv.take<uint64_t>(nnz);
    W.slot = cv.take<uint32_t>(nnz); W.win = cv.take<uint32_t>(nnz); W.lead = cv.take<uint32_t>(nnz);
    W.keep = cv.take<uint32_t>(nnz); W.pos = cv.take<uint32_t>(nnz + 1); W.key = cv.take<uint32_t>(nnz);
    W.startk = cv.take<uint32_t>(2 * nnz); W.endk = cv.take<uint32_t>(2 * nnz);
    W.perm[0] = cv.take<uint32_t>(nnz); W.perm[1] = cv.take<uint32_t>(nnz); W.status = cv.take<uint32_t>(nnz);
    W.tab = cv.take<uint32_t>(slots); W.hist = cv.take<uint32_t>(256 * nb); W.hoff = cv.take<uint32_t>(256 * nb + 1);
    W.scan = cv.take<uint32_t>(cut_scan_words(scan_n));
    W.rowmark = cv.take<uint32_t>(rows); W.F = cv.take<uint32_t>(2 * rows); W.P = cv.take<uint32_t>(2 * rows + 1);
    W.row_map = cv.take<uint32_t>(rows); W.rowinv = cv.take<uint32_t>(rows);
    if (!pass && (rc = rpp_ensure_pwork(rp, cv.off))) return rc;
  }
  const uint32_t n32 = (uint32_t)nnz, r32 = (uint32_t)rows, nr32 = (uint32_t)nr;
  BPPP_HIP(ctx, hipMemsetAsync(W.flag, 0, 256, st));

  // ---- the claims first: a type or an offset >= n is the call's error, before anything is matched
  uint32_t h_claims[24];
  if (!J.zero_claims) {
    const unsigned blocks = std::min<unsigned>(cut_grid(nsums), CUT_CLAIM_BLOCKS);
    uint32_t bad = CUT_NONE;
    BPPP_HIP(ctx, hipMemsetAsync(W.flag, 0xFF, 4, st));
    k_cut_claims<<<dim3(blocks), dim3(256), 0, st>>>((uint32_t)nsums, binary, J.amt, J.ty, J.bl, W.part, W.flag);
    k_cut_claims_fin<<<dim3(1), dim3(256), 0, st>>>(blocks, W.part, W.claims);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(&bad, W.flag, 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipMemcpyAsync(h_claims, W.claims, 96, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
    if (bad != CUT_NONE) return fail(ctx, BPPP_ERR_ARG, "rp_cut_through: sum " + std::to_string(bad) + ": a claimed type or offset is not canonical (>= n)");
  }

  // ---- identities, the table, the groups
  uint64_t k[2];
  if (rp->cut_salt_pinned) memcpy(k, rp->cut_salt, 16);
  else { std::random_device rd; for (int i = 0; i < 2; i++) k[i] = ((uint64_t)rd() << 32) | (uint32_t)rd(); }
  BPPP_HIP(ctx, hipMemsetAsync(W.tab, 0xFF, slots * 4, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.lead, 0xFF, nnz * 4, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.rowmark, 0, std::max<size_t>(rows, 1) * 4, st));
  k_cut_ident<<<dim3(cut_grid(nnz)), dim3(256), 0, st>>>(n32, nr32, (uint32_t)cb, J.entries, J.coms, k[0], k[1], rp->cut_same_hash ? 1u : 0u, W.idw, W.hs);
  k_cut_insert<<<dim3(cut_grid(nnz)), dim3(256), 0, st>>>(n32, (uint32_t)(slots - 1), W.idw, W.hs, W.tab, W.slot, W.err);
  k_cut_lead<<<dim3(cut_grid(nnz)), dim3(256), 0, st>>>(n32, (uint32_t)(slots - 1), W.tab, W.slot, W.win, W.lead);
  k_cut_first<<<dim3(cut_grid(nnz)), dim3(256), 0, st>>>(n32, W.win, W.lead, W.slot, W.keep);      // W.slot: now the first position of the group
  BPPP_HIP(ctx, hipGetLastError());
  if ((rc = cut_scan(ctx, W.keep, nnz, W.pos, W.scan))) return rc;
  k_cut_key<<<dim3(cut_grid(nnz)), dim3(256), 0, st>>>(n32, J.entries, W.slot, W.pos, W.key);
  BPPP_HIP(ctx, hipGetLastError());
  uint32_t h_g[2] = {0, 0};                     // groups, and the table's "walked off the end" word
  BPPP_HIP(ctx, hipMemcpyAsync(h_g, W.pos + nnz, 4, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipMemcpyAsync(h_g + 1, W.err, 4, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  const size_t ngroups = h_g[0];
  if (h_g[1] || !ngroups || ngroups > nnz) return fail(ctx, BPPP_ERR_HIP, "rp_cut_through: the table did not place every entry");
  BPPP_HIP(ctx, hipMemsetAsync(W.startk, 0, 2 * ngroups * 4, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.endk, 0, 2 * ngroups * 4, st));

  // ---- ranks: the stable sort of the positions on the key, 8 bits a pass
  size_t passes = 1;
  while (passes < 4 && ((2 * ngroups - 1) >> (8 * passes))) passes++;
  const uint32_t *in = nullptr;
  for (size_t p = 0; p < passes; p++) {
    uint32_t *out = W.perm[p & 1];
    k_cut_hist<<<dim3((unsigned)nb), dim3(64), 0, st>>>(n32, (uint32_t)(8 * p), W.key, in, (uint32_t)nb, W.hist);
    BPPP_HIP(ctx, hipGetLastError());
    if ((rc = cut_scan(ctx, W.hist, 256 * nb, W.hoff, W.scan))) return rc;
    k_cut_scatter<<<dim3((unsigned)nb), dim3(64), 0, st>>>(n32, (uint32_t)(8 * p), W.key, in, (uint32_t)nb, W.hoff, out);
    BPPP_HIP(ctx, hipGetLastError());
    in = out;
  }

  // ---- verdicts, the two compactions, the new pool
  k_cut_bounds<<<dim3(cut_grid(nnz)), dim3(256), 0, st>>>(n32, in, W.key, W.startk, W.endk);
  k_cut_status<<<dim3(cut_grid(nnz)), dim3(256), 0, st>>>(n32, nr32, in, W.key, W.startk, W.endk, J.entries, W.status, W.keep, W.rowmark, W.tot);
  BPPP_HIP(ctx, hipGetLastError());
  if ((rc = cut_scan(ctx, W.keep, nnz, W.pos, W.scan))) return rc;
  if (rows) k_cut_rowflags<<<dim3(cut_grid(rows)), dim3(256), 0, st>>>(r32, W.rowmark, W.F);
  BPPP_HIP(ctx, hipGetLastError());
  if ((rc = cut_scan(ctx, W.F, 2 * rows, W.P, W.scan))) return rc;
  if (rows) k_cut_rowmap<<<dim3(cut_grid(rows)), dim3(256), 0, st>>>(r32, W.rowmark, W.P, W.row_map, W.rowinv);
  k_cut_counts<<<dim3(1), dim3(64), 0, st>>>(n32, r32, W.pos, W.P, W.tot, W.res);
  BPPP_HIP(ctx, hipGetLastError());
  uint32_t res[5];
  BPPP_HIP(ctx, hipMemcpyAsync(res, W.res, 20, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  const size_t new_rows = res[0], out_rows = res[1], new_nnz = res[2];
  if (new_rows > rows || out_rows > new_rows || new_nnz > nnz) return fail(ctx, BPPP_ERR_HIP, "rp_cut_through: inconsistent counts");
  k_cut_entries<<<dim3(cut_grid(nnz)), dim3(256), 0, st>>>(n32, nr32, r32, J.entries, W.keep, W.pos, W.rowinv, (uint32_t *)d_new_entries);
  if (d_new_coms && new_rows) {
    const uint64_t total = (uint64_t)new_rows * cb;
    k_cut_gather<<<dim3(cut_grid((total + 15) / 16)), dim3(256), 0, st>>>(total, (uint32_t)cb, r32, W.row_map, J.coms, (uint8_t *)d_new_coms);
  }
  BPPP_HIP(ctx, hipGetLastError());
  if (entry_status) BPPP_HIP(ctx, hipMemcpyAsync(entry_status, W.status, nnz * 4, hipMemcpyDeviceToHost, st));
  if (row_map && new_rows) BPPP_HIP(ctx, hipMemcpyAsync(row_map, W.row_map, new_rows * 4, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  if (block_claims) memcpy(block_claims, h_claims, 96);
  counts->new_rows = new_rows; counts->out_rows = out_rows; counts->new_nnz = new_nnz; counts->ncut = res[3]; counts->nagain = res[4];
  rp->cut_slots = slots; rp->cut_groups = ngroups; rp->cut_passes = passes;
  return BPPP_OK;
}

}  // namespace
}  // namespace bppp

using namespace bppp;

extern "C" {

int bppp_rp_cut_through_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                               const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_offsets, uint32_t *entry_status, uint32_t *row_map,
                               void *d_new_coms_files, void *d_new_entries, uint64_t *block_claims, bppp_rp_cut_counts *counts) {
  return cut_through_device(rp, rows, d_coms_files, nsums, d_sum_start, d_entries, nnz, d_claim_amounts, d_claim_types, d_claim_offsets, entry_status, row_map,
                            d_new_coms_files, d_new_entries, block_claims, counts);
}

int bppp_rp_cut_through(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                        const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_offsets, uint32_t *entry_status, uint32_t *row_map,
                        uint8_t *new_coms_files, uint32_t *new_entries, uint64_t *block_claims, bppp_rp_cut_counts *counts) {
  if (!rp || !counts) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  HostCsr H;
  DevBuf nc, ne;
  if (nsums && nnz && rpp_sizes_ok(rp, rows, nsums, nnz)) {
    int rc = H.up(rp, rows, coms_files, rp->D.coms_bytes, nsums, sum_start, entries, nnz, claim_amounts, claim_types, claim_offsets, nsums * 32);
    if (!rc) rc = nc.out(ctx, new_coms_files, rows * (size_t)rp->D.coms_bytes);
    if (!rc) rc = ne.out(ctx, new_entries, nnz * 4);
    if (rc) return rc;
  }
  bppp_rp_cut_counts c;
  int rc = cut_through_device(rp, rows, H.coms.p, nsums, H.start.p, H.entries.p, nnz, H.a.p, H.ty.p, H.e.p, entry_status, row_map, nc.p, ne.p, block_claims, &c);
  if (rc) return rc;
  if (nc.p && c.new_rows) BPPP_HIP(ctx, hipMemcpy(new_coms_files, nc.p, c.new_rows * (size_t)rp->D.coms_bytes, hipMemcpyDeviceToHost));
  if (ne.p && c.new_nnz) BPPP_HIP(ctx, hipMemcpy(new_entries, ne.p, c.new_nnz * 4, hipMemcpyDeviceToHost));
  *counts = c;
  return BPPP_OK;
}

}  // extern "C"
