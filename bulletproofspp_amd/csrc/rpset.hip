// rpset.hip — set commitments: an append-only Merkle mountain range over opaque rows, its root, its peaks and membership paths (bppp_rp_set_*,
// include/bppp.h states every message).  The set is the device-resident thing: a full store keeps every node in HBM as grow-only level arrays
// (lvl[k][j][8] words, 64 bytes a row in the limit), a frontier-only set keeps the peaks alone (front[k][8], the peak of level k).  Every entry
// point takes host buffers: an internal function on HBM pointers (set_*_dev: no export, no declaration) and a thin wrapper over DevBuf.
// The kernels are in csrc/rpset.hip.h, the index arithmetic in csrc/rpset_plan.hpp.
//   append of m rows onto n   k_rp_set_leaf, then one k_rp_set_tree per pass of csrc/rpset_plan.hpp's append_passes (eight levels a pass, a pass
//                             per level 8q that has a new node: at most ceil (bit_length (n + m) / 8)), then, frontier-only, k_rp_set_front_merge
//   root, peaks               k_rp_set_bags (one lane, popcount (n) hashes)
//   paths                     k_rp_set_bags (the right-bag of every peak position once), k_rp_set_paths
//   verify_paths              k_rp_set_verify
// Scratch (a frontier-only append's leaves and tile tops, the bags, the small outputs) is carved from the handle's pwork; the store and the frontier
// belong to the set.  Everything that can refuse or fail to allocate happens before the first launch of a call, and n moves last.
#include <string.h>
#include <string>
#include <vector>
#include "rp_internal.hpp"
#include "rphostcall.hpp"
#include "rpprove_host.hpp"
#include "rpexcess_shared.hip.h"
#include "rpset_plan.hpp"
#include "rpset.hip.h"

using namespace bppp;
using namespace bppp::set;
using bppp::excess::domain;

struct bppp_rp_set {
  bppp_rp *rp = nullptr;
  bppp_ctx *ctx = nullptr;
  uint32_t row_bytes = 0;
  bool keep = false;
  uint64_t n = 0;
  SetDomains D;
  bppp_set::LevelStore store;           // a full store: the level arrays, their capacities in nodes, and the table of their addresses in HBM
  uint32_t **tab = nullptr;
  uint32_t *front = nullptr;            // frontier-only: [MAX_LEVELS][8]
};

namespace {

SetDomains set_domains(const bppp_rp *rp) {
  return SetDomains{domain("bppp/set/leaf/v1", rp->tag), domain("bppp/set/node/v1", rp->tag), domain("bppp/set/bag/v1", rp->tag), domain("bppp/set/root/v1", rp->tag)};
}
SetNodes nodes_of(const bppp_rp_set *s) { return SetNodes{s->tab, s->front, s->keep ? 1u : 0u}; }
bool set_closed(const bppp_rp_set *s) { return !s || ctx_closed(s->ctx); }
size_t store_bytes_of(const bppp_rp_set *s) {
  if (!s->keep) return (size_t)bppp_set::MAX_LEVELS * 32;
  size_t b = 0;
  for (uint32_t k = 0; k < bppp_set::FULL_LEVELS; k++) b += (size_t)s->store.cap[k] * 32;
  return b;
}
int row_bytes_ok(bppp_ctx *ctx, const char *who, size_t row_bytes) {
  if (row_bytes < 1 || row_bytes > bppp_set::MAX_ROW_BYTES)
    return fail(ctx, BPPP_ERR_ARG, std::string(who) + ": row_bytes = " + std::to_string(row_bytes) + " is outside 1 .. " + std::to_string(bppp_set::MAX_ROW_BYTES));
  return BPPP_OK;
}

// the level arrays hold a set of N rows; what they hold of the n rows there are is kept.  All or nothing (csrc/rpset_plan.hpp: grow_levels): a
// failure leaves the arrays, their capacities and the table in HBM as they were
struct HipLevelOps {
  bppp_rp_set *s; hipError_t err = hipSuccess;
  void *alloc(size_t bytes) { void *p = nullptr; err = hipMalloc(&p, bytes); return err == hipSuccess ? p : nullptr; }
  void release(void *p) { hipFree(p); }
  bool copy(void *dst, const void *src, size_t bytes) {
    err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s->ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(s->ctx->stream);
    return err == hipSuccess;
  }
  bool publish(uint32_t *const *table) {
    const hipError_t e = hipMemcpy(s->tab, table, sizeof(s->store.lvl), hipMemcpyHostToDevice);
    if (e != hipSuccess) err = e;
    return e == hipSuccess;
  }
};
int ensure_levels(bppp_rp_set *s, uint64_t N) {
  HipLevelOps ops{s};
  const bppp_set::GrowResult r = bppp_set::grow_levels(s->store, s->n, N, ops);
  if (r == bppp_set::GROW_OK) return BPPP_OK;
  (void)hipGetLastError();
  return fail(s->ctx, BPPP_ERR_HIP, std::string("rp_set: the level arrays could not grow (") + (r == bppp_set::GROW_ALLOC_FAILED ? "hipMalloc" : r == bppp_set::GROW_COPY_FAILED ? "copy" : "table upload") +
                                        "): " + hipGetErrorString(ops.err) + "; the set is as it was");
}

// rows [m][row_bytes] in HBM appended; m >= 1, the sizes checked by the caller
int set_append_dev(bppp_rp_set *s, uint64_t m, const uint8_t *rows) {
  bppp_ctx *ctx = s->ctx;
  hipStream_t st = ctx->stream;
  const uint64_t n = s->n, N = n + m;
  const std::vector<bppp_set::Pass> passes = bppp_set::append_passes(n, m);
  uint32_t *leaves = nullptr, *tops[2] = {nullptr, nullptr}, *front_new = nullptr;
  if (s->keep) { int rc = ensure_levels(s, N); if (rc) return rc; }
  else {
    for (int pass = 0; pass < 2; pass++) {
      Carver cv(pass ? s->rp->pwork : nullptr, s->rp->pwork_bytes);
      leaves = cv.take<uint32_t>(m * 8); tops[0] = cv.take<uint32_t>(bppp_set::tops_nodes(m, 0) * 8); tops[1] = cv.take<uint32_t>(bppp_set::tops_nodes(m, 1) * 8);
      front_new = cv.take<uint32_t>(bppp_set::MAX_LEVELS * 8);
      if (!pass) { int rc = rpp_ensure_pwork(s->rp, cv.off); if (rc) return rc; }
    }
  }
  k_rp_set_leaf<<<dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st>>>((uint32_t)m, s->row_bytes, s->D.leaf, rows, s->keep ? s->store.lvl[0] + n * 8 : leaves);
  BPPP_HIP(ctx, hipGetLastError());
  const SetNodes S = nodes_of(s);
  const uint32_t *in = leaves;
  for (size_t q = 0; q < passes.size(); q++) {
    const bppp_set::Pass &P = passes[q];
    uint32_t *out = tops[q & 1];                      // sized by bppp_set::tops_nodes
    const TreePass A{n, N, P.tile0, P.L, in, n >> P.L, out, bppp_set::shr(n, P.L + bppp_set::TILE_BITS), front_new};
    k_rp_set_tree<<<dim3((unsigned)P.tiles), dim3(bppp_set::TILE), 0, st>>>(A, S, s->D.node);
    BPPP_HIP(ctx, hipGetLastError());
    in = out;
  }
  if (!s->keep) {
    uint64_t mask = 0;
    for (uint32_t k = 0; k < 64; k++) if (bppp_set::peak_is_new(n, N, k)) mask |= (uint64_t)1 << k;
    k_rp_set_front_merge<<<dim3(bppp_set::MAX_LEVELS * 8 / 64), dim3(64), 0, st>>>(mask, front_new, s->front);
    BPPP_HIP(ctx, hipGetLastError());
  }
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  s->n = N;
  return BPPP_OK;
}

// the scratch of k_rp_set_bags in pwork: peaks, right-bags, and the two small outputs as bytes
struct BagWork { uint32_t *pk, *rbag, *peaks_out, *root_out; };
int bag_carve(bppp_rp_set *s, BagWork &W) {
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? s->rp->pwork : nullptr, s->rp->pwork_bytes);
    W.pk = cv.take<uint32_t>(bppp_set::MAX_LEVELS * 8); W.rbag = cv.take<uint32_t>(bppp_set::MAX_LEVELS * 8);
    W.peaks_out = cv.take<uint32_t>(bppp_set::MAX_LEVELS * 8); W.root_out = cv.take<uint32_t>(8);
    if (!pass) { int rc = rpp_ensure_pwork(s->rp, cv.off); if (rc) return rc; }
  }
  return BPPP_OK;
}
int set_bags_dev(bppp_rp_set *s, const BagWork &W) {
  k_rp_set_bags<<<dim3(1), dim3(64), 0, s->ctx->stream>>>(s->n, s->row_bytes, nodes_of(s), s->D.bag, s->D.root, W.pk, W.rbag, W.peaks_out, W.root_out);
  BPPP_HIP(s->ctx, hipGetLastError());
  return BPPP_OK;
}

// paths [nq][32 L] of idx [nq] (all below n) in HBM; L = bit_length (n) >= 1
int set_paths_dev(bppp_rp_set *s, uint64_t nq, const uint64_t *idx, uint32_t *paths) {
  BagWork W;
  int rc;
  if ((rc = bag_carve(s, W)) || (rc = set_bags_dev(s, W))) return rc;
  const uint32_t L = bppp_set::bit_length(s->n);
  k_rp_set_paths<<<dim3((unsigned)((nq * L + 63) / 64)), dim3(64), 0, s->ctx->stream>>>(nq, s->n, L, nodes_of(s), W.pk, W.rbag, idx, paths);
  BPPP_HIP(s->ctx, hipGetLastError());
  return BPPP_OK;
}

int set_verify_dev(bppp_rp *rp, uint32_t row_bytes, uint64_t n, const ExDomain &root, uint64_t nq, const uint64_t *idx, const uint8_t *rows, const uint8_t *paths,
                   uint32_t *status, uint32_t *any) {
  bppp_ctx *ctx = rp->ctx;
  BPPP_HIP(ctx, hipMemsetAsync(any, 0, 4, ctx->stream));
  k_rp_set_verify<<<dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, ctx->stream>>>(nq, n, row_bytes, bppp_set::bit_length(n), set_domains(rp), root, idx, rows, paths, status, any);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

int set_make(bppp_rp *rp, const char *who, size_t row_bytes, bool keep, bppp_rp_set **out) {
  bppp_ctx *ctx = rp->ctx;
  int rc = row_bytes_ok(ctx, who, row_bytes); if (rc) return rc;
  hipSetDevice(ctx->device);
  bppp_rp_set *s = new bppp_rp_set();
  s->rp = rp; s->ctx = ctx; s->row_bytes = (uint32_t)row_bytes; s->keep = keep; s->D = set_domains(rp);
  const hipError_t e = keep ? hipMalloc((void **)&s->tab, sizeof(s->store.lvl)) : hipMalloc((void **)&s->front, (size_t)bppp_set::MAX_LEVELS * 32);
  if (e != hipSuccess) { delete s; return fail(ctx, BPPP_ERR_HIP, std::string(who) + ": hipMalloc: " + hipGetErrorString(e)); }
  ctx_retain(ctx);
  *out = s;
  return BPPP_OK;
}

}  // namespace

extern "C" {

int bppp_rp_set_create(bppp_rp *rp, size_t row_bytes, int keep_nodes, bppp_rp_set **set) {
  if (set) *set = nullptr;
  if (!rp || !set) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (keep_nodes != 0 && keep_nodes != 1) return fail(rp->ctx, BPPP_ERR_ARG, "rp_set_create: keep_nodes is 0 (the frontier alone) or 1 (every node)");
  return set_make(rp, "rp_set_create", row_bytes, keep_nodes == 1, set);
}

int bppp_rp_set_restore(bppp_rp *rp, size_t row_bytes, uint64_t n, const uint8_t *peaks, bppp_rp_set **set) {
  if (set) *set = nullptr;
  if (!rp || !set) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (n > bppp_set::FRONTIER_MAX_N) return fail(ctx, BPPP_ERR_ARG, "rp_set_restore: n is 2^63 or more");
  if (n && !peaks) return fail(ctx, BPPP_ERR_ARG, "rp_set_restore: peaks is NULL");
  bppp_rp_set *s = nullptr;
  int rc = set_make(rp, "rp_set_restore", row_bytes, false, &s); if (rc) return rc;
  std::vector<uint32_t> h(bppp_set::MAX_LEVELS * 8, 0u);
  for (uint32_t p = 0; p < bppp_set::popcount(n); p++) {
    const uint32_t k = bppp_set::peak_level(n, p);
    for (uint32_t q = 0; q < 8; q++) {
      const uint8_t *b = peaks + 32 * p + 4 * q;
      h[k * 8 + q] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
    }
  }
  const hipError_t e = hipMemcpy(s->front, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { bppp_rp_set_destroy(s); return fail(ctx, BPPP_ERR_HIP, std::string("rp_set_restore: hipMemcpy: ") + hipGetErrorString(e)); }
  s->n = n;
  *set = s;
  return BPPP_OK;
}

void bppp_rp_set_destroy(bppp_rp_set *set) {
  if (!set) return;
  bppp_ctx *ctx = set->ctx;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  for (uint32_t k = 0; k < bppp_set::LEVEL_SLOTS; k++) if (set->store.lvl[k]) hipFree(set->store.lvl[k]);
  if (set->tab) hipFree(set->tab);
  if (set->front) hipFree(set->front);
  delete set;
  ctx_release(ctx);
}

int bppp_rp_set_append(bppp_rp_set *set, size_t nrows, const uint8_t *rows) {
  if (set_closed(set)) return BPPP_ERR_ARG;
  bppp_ctx *ctx = set->ctx;
  if (!nrows) return BPPP_OK;
  if (!rows) return fail(ctx, BPPP_ERR_ARG, "rp_set_append: rows is NULL");
  const uint64_t lim = set->keep ? bppp_set::FULL_MAX_N : bppp_set::FRONTIER_MAX_N;
  if (nrows > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, "rp_set_append: nrows = " + std::to_string(nrows) + " is 2^31 or more: append in several calls");
  if ((uint64_t)nrows > lim - set->n)
    return fail(ctx, BPPP_ERR_ARG, "rp_set_append: " + std::to_string(set->n) + " + " + std::to_string(nrows) + (set->keep ? " rows: a full store holds fewer than 2^31" : " rows: a set holds fewer than 2^63"));
  hipSetDevice(ctx->device);
  DevBuf r;
  int rc = r.up(ctx, rows, nrows * (size_t)set->row_bytes); if (rc) return rc;
  rc = set_append_dev(set, nrows, (const uint8_t *)r.p);
  if (rc) ctx_drain(ctx);
  return rc;
}

int bppp_rp_set_info(const bppp_rp_set *set, uint64_t *n, size_t *row_bytes, size_t *npeaks, size_t *store_bytes) {
  if (!set) return BPPP_ERR_ARG;
  if (n) *n = set->n;
  if (row_bytes) *row_bytes = set->row_bytes;
  if (npeaks) *npeaks = bppp_set::popcount(set->n);
  if (store_bytes) *store_bytes = store_bytes_of(set);
  return BPPP_OK;
}

int bppp_rp_set_root(bppp_rp_set *set, uint8_t root[32]) {
  if (set_closed(set)) return BPPP_ERR_ARG;
  bppp_ctx *ctx = set->ctx;
  if (!root) return fail(ctx, BPPP_ERR_ARG, "rp_set_root: root is NULL");
  hipSetDevice(ctx->device);
  BagWork W;
  int rc;
  if ((rc = bag_carve(set, W)) || (rc = set_bags_dev(set, W))) return rc;
  BPPP_HIP(ctx, hipMemcpyAsync(root, W.root_out, 32, hipMemcpyDeviceToHost, ctx->stream));
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return BPPP_OK;
}

int bppp_rp_set_peaks(bppp_rp_set *set, uint8_t *peaks) {
  if (set_closed(set)) return BPPP_ERR_ARG;
  bppp_ctx *ctx = set->ctx;
  const uint32_t m = bppp_set::popcount(set->n);
  if (!m) return BPPP_OK;
  if (!peaks) return fail(ctx, BPPP_ERR_ARG, "rp_set_peaks: peaks is NULL");
  hipSetDevice(ctx->device);
  BagWork W;
  int rc;
  if ((rc = bag_carve(set, W)) || (rc = set_bags_dev(set, W))) return rc;
  BPPP_HIP(ctx, hipMemcpyAsync(peaks, W.peaks_out, (size_t)32 * m, hipMemcpyDeviceToHost, ctx->stream));
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return BPPP_OK;
}

size_t bppp_rp_set_path_bytes(uint64_t n) { return bppp_set::path_bytes(n); }

int bppp_rp_set_paths(bppp_rp_set *set, size_t nq, const uint64_t *idx, uint8_t *paths) {
  if (set_closed(set)) return BPPP_ERR_ARG;
  bppp_ctx *ctx = set->ctx;
  if (!set->keep) return fail(ctx, BPPP_ERR_ARG, "rp_set_paths: the set keeps its frontier alone (keep_nodes = 0): it has no nodes to serve a path from");
  if (!nq) return BPPP_OK;
  if (!idx || !paths) return fail(ctx, BPPP_ERR_ARG, std::string("rp_set_paths: ") + (idx ? "paths" : "idx") + " is NULL");
  if (nq > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, "rp_set_paths: nq is 2^31 or more");
  for (size_t q = 0; q < nq; q++)
    if (idx[q] >= set->n) return fail(ctx, BPPP_ERR_ARG, "rp_set_paths: idx[" + std::to_string(q) + "] = " + std::to_string(idx[q]) + " is not below n = " + std::to_string(set->n));
  hipSetDevice(ctx->device);
  const size_t bytes = nq * bppp_set::path_bytes(set->n);
  DevBuf i, p;
  int rc = i.up(ctx, idx, nq * 8);
  if (!rc) rc = p.out(ctx, paths, bytes);
  if (!rc) rc = set_paths_dev(set, nq, (const uint64_t *)i.p, (uint32_t *)p.p);
  if (rc) { ctx_drain(ctx); return rc; }
  BPPP_HIP(ctx, hipMemcpyAsync(paths, p.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return BPPP_OK;
}

int bppp_rp_set_verify_paths(bppp_rp *rp, size_t row_bytes, uint64_t n, const uint8_t root[32], size_t nq, const uint64_t *idx, const uint8_t *rows, const uint8_t *paths,
                             uint32_t *status, int *accept) {
  if (!rp || !accept) return BPPP_ERR_ARG;
  *accept = 0;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  int rc = row_bytes_ok(ctx, "rp_set_verify_paths", row_bytes); if (rc) return rc;
  if (n > bppp_set::FRONTIER_MAX_N) return fail(ctx, BPPP_ERR_ARG, "rp_set_verify_paths: n is 2^63 or more");
  if (!root) return fail(ctx, BPPP_ERR_ARG, "rp_set_verify_paths: root is NULL");
  if (!nq) { *accept = 1; return BPPP_OK; }
  if (nq > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, "rp_set_verify_paths: nq is 2^31 or more");
  const size_t pb = bppp_set::path_bytes(n);
  if (!idx || !rows || (pb && !paths)) return fail(ctx, BPPP_ERR_ARG, std::string("rp_set_verify_paths: ") + (!idx ? "idx" : !rows ? "rows" : "paths") + " is NULL");
  ExDomain rt;
  for (uint32_t q = 0; q < 8; q++) rt.w[q] = ((uint32_t)root[4 * q] << 24) | ((uint32_t)root[4 * q + 1] << 16) | ((uint32_t)root[4 * q + 2] << 8) | root[4 * q + 3];
  hipSetDevice(ctx->device);
  DevBuf i, r, p, s, any;
  rc = i.up(ctx, idx, nq * 8);
  if (!rc) rc = r.up(ctx, rows, nq * row_bytes);
  if (!rc) rc = p.up(ctx, paths ? paths : (const uint8_t *)"", nq * pb);
  if (!rc) rc = s.out(ctx, status, nq * 4);
  if (!rc) rc = any.out(ctx, accept, 4);
  if (!rc) rc = set_verify_dev(rp, (uint32_t)row_bytes, n, rt, nq, (const uint64_t *)i.p, (const uint8_t *)r.p, (const uint8_t *)p.p, (uint32_t *)s.p, (uint32_t *)any.p);
  if (rc) { ctx_drain(ctx); return rc; }
  uint32_t h_any = 1;
  if (status) BPPP_HIP(ctx, hipMemcpyAsync(status, s.p, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
  BPPP_HIP(ctx, hipMemcpyAsync(&h_any, any.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *accept = h_any ? 0 : 1;
  return BPPP_OK;
}

}  // extern "C"
