// rpscan_keys.hip — the view-key scan of an output set under MANY view secrets in one call: bppp_rp_scan_keys{,_device} (include/bppp.h states
// the contract: for every key k and row i, exactly what bppp_rp_scan under view_secrets[k] reports for row i).
// Rows are the outer loop and tiles of kt keys the inner one (csrc/rpscan_keys_plan.hpp: the geometry, the recoding, the merge of hits), so
// that what does not depend on the key is paid once per row:
//   per pass    the hints lifted (k_rp_scan_lift of csrc/rpseal.hip, as it is) and the walk's table of every row, R, 3R, 5R, 7R affine by one
//               inversion a row (csrc/rpscan_keys.hip.h), written to HBM
//   per tile    ONE launch walks the tile's keys over every row; one inversion a row makes the tile's kt shared points affine; the shared
//               secret and the tag of every (row, key); the tag's survivors compacted as (row, key, ss)
//   survivors   chunk by chunk: pads, the decrypted opening, its commitment over the table csrc/rpcommit.hip shares, the comparison with the
//               lifted commitment of the file; a verdict per SURVIVOR (two keys may judge one row differently), read back with the survivors
//   per pass    the owned pairs sorted by (row, key) on the host and, for those that still fit under cap, their openings made again from ss
//               (the hashes only, no commitment) straight into their slots
// Kernels:
//   k_rp_scan_table_keys    one lane per row: the table of R; a row whose hint did not lift gets the table of infinity
//   k_rp_scan_walk_keys     one lane per row, a workgroup is one wavefront with its table in LDS: a strided loop over the tile's keys (the launch
//                           gives each key a workgroup of its own), a_k R in XYZZ
//   k_rp_scan_affine_keys   one lane per row: the kt accumulators of the row made affine by Montgomery's trick
//   k_rp_scan_tag_keys      one lane per (row, key): ss, the tag; nothing, or a slot among the survivors
//   k_rp_scan_open_keys     one lane per (survivor, range): k_rp_scan_open with ss by survivor; the file's commitment lifted unless dec is NULL
//   k_rp_scan_judge_keys    one lane per survivor: OWNED or TAG_ONLY into verdict[survivor]
//   k_rp_scan_emit_keys     one lane per (hit, range): the opening into its slot
// Every kernel is bounds-checked on its own index and writes with ordinary vector stores.  No buffer is sized by the 1 / 256 expectation: every
// pair of a tile may survive and be owned.  All workspace is carved from rp->pwork; the recoded keys are wiped, on the host and in HBM, before
// the call returns.
#include <string.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "ec.hip.h"
#include "rp_internal.hpp"
#include "rphostcall.hpp"
#include "rpprove_host.hpp"
#include "rpwords.hip.h"
#include "rplift.hip.h"
#include "rpexcess_shared.hip.h"
#include "rpsealhash.hip.h"
#include "rpscan_keys.hip.h"
#include "sha256.hip.h"

namespace bppp {

// k_rp_scan_table_keys, k_rp_scan_walk_keys and k_rp_scan_affine_keys are in csrc/rpscan_keys.hip.h, which the test hooks share
// survivors: (surv_row, surv_key, ss)[0 .. count) in no particular order; key0: the tile's first key
__global__ void __launch_bounds__(64) k_rp_scan_tag_keys(uint32_t n, uint32_t kt, uint32_t key0, uint32_t seal_bytes, SealDomains D, const uint8_t *__restrict__ seals,
                                                         const uint32_t *__restrict__ status, const uint32_t *__restrict__ P, uint32_t *__restrict__ ssbuf,
                                                         uint32_t *__restrict__ surv_row, uint32_t *__restrict__ surv_key, uint32_t *__restrict__ count) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (uint64_t)n * kt) return;
  const uint32_t b = (uint32_t)(j % n), k = (uint32_t)(j / n);
  if (status[b] != SCAN_OPEN) return;
  const uint8_t *seal = seals + (size_t)b * seal_bytes;
  uint32_t ss[8];
  seal_shared(D.ds, P + j * 16, [&](uint32_t o) -> uint32_t { return seal[o]; }, ss);
  if (seal_view_tag(D.dt, ss) != seal[EX_KEY]) return;
  const uint32_t s = atomicAdd(count, 1u);
  for (int w = 0; w < 8; w++) ssbuf[(size_t)s * 8 + w] = ss[w];
  surv_row[s] = b; surv_key[s] = key0 + k;
}
__global__ void __launch_bounds__(64) k_rp_scan_open_keys(uint64_t n, uint32_t nr, uint32_t seal_bytes, uint32_t coms_bytes, uint32_t binary, SealDomains D,
                                                          const uint8_t *__restrict__ seals, const uint8_t *__restrict__ coms, const uint32_t *__restrict__ surv_row,
                                                          const uint32_t *__restrict__ ssbuf, uint32_t *__restrict__ in_sc, uint32_t *__restrict__ flag, uint32_t *__restrict__ dec) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t s = j / nr;
  const uint32_t b = surv_row[s], i = (uint32_t)(j % nr);
  const uint8_t *memo = seals + (size_t)b * seal_bytes + SEAL_HEAD + (size_t)i * SEAL_MEMO;
  uint32_t ss[8], pad[16];
  for (int k = 0; k < 8; k++) ss[k] = ssbuf[s * 8 + k];
  seal_pad(D.dm, ss, i, pad);
  uint8_t plain[SEAL_MEMO];
  for (uint32_t o = 0; o < SEAL_MEMO; o++) plain[o] = (uint8_t)(memo[o] ^ ex_word_byte(pad, o));
  fe v = load_field_be_raw(plain), ty = load_field_be_raw(plain + 32), bl = seal_blind(D.db, ss, i);
  const bool bad = !wi_canonical(v) || !wi_canonical(ty) || (binary && !fe_is_zero(ty));
  if (bad) { v = fe_zero(); ty = fe_zero(); bl = fe_zero(); }
  fe_store(in_sc + j * 24, v); fe_store(in_sc + j * 24 + 8, binary ? bl : ty); fe_store(in_sc + j * 24 + 16, binary ? ty : bl);
  flag[j] = bad ? 1u : 0u;
  if (!dec) return;
  // commitment i of the row's file, as decodeCommitments lifts it: the infinity encoding when the x has no curve point
  const uint8_t *file = coms + (size_t)b * coms_bytes;
  bool ok;
  aff C = rp_lift_x(load_field_be<0>(file + (nr + 7) / 8 + (size_t)i * 32), ((file[i >> 3] >> (i & 7)) & 1u) != 0, ok);
  if (!ok) C = aff_inf();
  aff_store(dec + j * 16, C);
}
__global__ void __launch_bounds__(64) k_rp_scan_judge_keys(uint32_t n, uint32_t nr, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ dec,
                                                           const uint32_t *__restrict__ rec, uint32_t *__restrict__ verdict) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  bool owned = true;
  for (uint32_t i = 0; i < nr; i++) {
    const size_t j = (size_t)s * nr + i;
    uint32_t any = 0, diff = 0;
    for (int k = 0; k < 16; k++) { const uint32_t d = dec[j * 16 + k]; any |= d; diff |= d ^ rec[j * 16 + k]; }
    owned = owned && !flag[j] && any && !diff;
  }
  verdict[s] = owned ? (uint32_t)BPPP_RP_SCAN_OWNED : (uint32_t)BPPP_RP_SCAN_TAG_ONLY;
}
// in_sc: [n / nr][nr][3] scalars in base order — typed (v, ty, bl), binary (v, bl, 0) — into the slots that begin at the output pointers
__global__ void __launch_bounds__(64) k_rp_scan_emit_keys(uint64_t n, uint32_t binary, const uint32_t *__restrict__ in_sc, uint32_t *__restrict__ amounts,
                                                          uint32_t *__restrict__ types, uint32_t *__restrict__ blinds) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t *sc = in_sc + j * 24;
  for (int k = 0; k < 8; k++) {
    if (amounts) amounts[j * 8 + k] = sc[k];
    if (types) types[j * 8 + k] = binary ? 0u : sc[8 + k];
    if (blinds) blinds[j * 8 + k] = binary ? sc[8 + k] : sc[16 + k];
  }
}

}  // namespace bppp

using namespace bppp;

namespace {

struct KeysWork { uint32_t *R, *status, *tab, *keys, *acc, *P, *count, *surv_row, *surv_key, *ss, *in_sc, *flag, *dec, *rec, *verdict; };

// the recoded keys of a call on the host, wiped with the scope
struct KeyRecs {
  std::vector<ScanKeyRec> v;
  ~KeyRecs() { wipe(); }
  void wipe() {
    volatile uint32_t *p = v.empty() ? nullptr : (volatile uint32_t *)v.data();
    for (size_t i = 0; p && i < v.size() * (SCAN_KEY_WORDS); i++) p[i] = 0;
  }
};

int scan_keys_passes(bppp_rp *rp, const KeyRecs &recs, size_t rows, const void *d_coms, const void *d_seals, uint32_t *row_status, size_t cap, uint32_t *hit_key,
                     uint32_t *hit_row, void *d_amounts, void *d_types, void *d_blinds, size_t *nhits, uint64_t *ntag_only, const ScanKeysGeom &G, const KeysWork &K) {
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  const bool binary = rp->st.kind == 1, want_open = d_amounts || d_types || d_blinds;
  const size_t nkeys = recs.v.size(), nr = rp->D.nr, sb = BPPP_RP_SEAL_BYTES(nr), cb = rp->D.coms_bytes, C = G.rows_pass, S = G.open_chunk;
  const SealDomains D = seal_domains(rp);
  auto at = [&](void *p, size_t slot) -> uint32_t * { return p ? (uint32_t *)p + slot * nr * 8 : nullptr; };
  std::vector<uint32_t> h_status(C), h_verdict, h_row, h_key, h_ss;
  std::vector<uint8_t> seen(C);                          // per row of the pass: bit 0 some key owns it, bit 1 some key's tag matched
  std::vector<ScanHit> hits;
  size_t total = 0;
  uint64_t tag_only = 0;
  int rc;
  for (size_t o = 0; o < rows; o += C) {
    const uint32_t n = (uint32_t)std::min(C, rows - o);
    const dim3 grid((n + 63) / 64);
    const uint8_t *seals = (const uint8_t *)d_seals + o * sb, *coms = (const uint8_t *)d_coms + o * cb;
    scan_lift_launch(rp, n, seals, K.R, K.status);
    k_rp_scan_table_keys<<<grid, dim3(64), 0, st>>>(n, K.R, K.status, SCAN_OPEN, K.tab);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(h_status.data(), K.status, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    std::fill(seen.begin(), seen.end(), 0);
    hits.clear();
    const bool listing = total < cap;                    // rows only grow: once the slots are full no later pass lists a hit
    size_t uncounted = 0;
    for (size_t k0 = 0; k0 < nkeys; k0 += G.kt) {
      const uint32_t kt = (uint32_t)std::min(G.kt, nkeys - k0);
      const uint64_t pairs = (uint64_t)n * kt;
      BPPP_HIP(ctx, hipMemcpyAsync(K.keys, recs.v.data() + k0, (size_t)kt * sizeof(ScanKeyRec), hipMemcpyHostToDevice, st));
      BPPP_HIP(ctx, hipMemsetAsync(K.count, 0, 16, st));
      k_rp_scan_walk_keys<<<dim3(grid.x, kt), dim3(64), 0, st>>>(n, kt, (const ScanKeyRec *)K.keys, K.tab, K.acc);
      k_rp_scan_affine_keys<<<grid, dim3(64), 0, st>>>(n, kt, K.acc, K.P);
      k_rp_scan_tag_keys<<<dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, st>>>(n, kt, (uint32_t)k0, (uint32_t)sb, D, seals, K.status, K.P, K.ss, K.surv_row, K.surv_key, K.count);
      BPPP_HIP(ctx, hipGetLastError());
      uint32_t ns = 0;
      BPPP_HIP(ctx, hipMemcpyAsync(&ns, K.count, 4, hipMemcpyDeviceToHost, st));
      BPPP_HIP(ctx, hipStreamSynchronize(st));
      if (ns > pairs) return fail(ctx, BPPP_ERR_HIP, "rp_scan_keys: more survivors than pairs");
      if (!ns) continue;
      for (size_t c0 = 0; c0 < ns; c0 += S) {
        const uint32_t c = (uint32_t)std::min<size_t>(S, ns - c0);
        const uint64_t m = (uint64_t)c * nr;
        k_rp_scan_open_keys<<<dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st>>>(m, (uint32_t)nr, (uint32_t)sb, (uint32_t)cb, binary, D, seals, coms, K.surv_row + c0, K.ss + c0 * 8,
                                                                                  K.in_sc, K.flag, K.dec);
        BPPP_HIP(ctx, hipGetLastError());
        if ((rc = rpp_commit_inputs(rp, K.in_sc, m, K.rec))) return rc;
        k_rp_scan_judge_keys<<<dim3((c + 63) / 64), dim3(64), 0, st>>>(c, (uint32_t)nr, K.flag, K.dec, K.rec, K.verdict + c0);
        BPPP_HIP(ctx, hipGetLastError());
      }
      h_verdict.resize(ns); h_row.resize(ns); h_key.resize(ns); h_ss.resize((size_t)ns * 8);
      BPPP_HIP(ctx, hipMemcpyAsync(h_verdict.data(), K.verdict, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
      BPPP_HIP(ctx, hipMemcpyAsync(h_row.data(), K.surv_row, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
      BPPP_HIP(ctx, hipMemcpyAsync(h_key.data(), K.surv_key, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
      BPPP_HIP(ctx, hipMemcpyAsync(h_ss.data(), K.ss, (size_t)ns * 32, hipMemcpyDeviceToHost, st));
      BPPP_HIP(ctx, hipStreamSynchronize(st));
      for (uint32_t s = 0; s < ns; s++) {
        if (h_row[s] >= n || h_key[s] < k0 || h_key[s] >= k0 + kt) return fail(ctx, BPPP_ERR_HIP, "rp_scan_keys: a survivor outside its tile");
        if (h_verdict[s] == BPPP_RP_SCAN_OWNED && !listing) {
          uncounted++;                                   // every slot is taken: the hit is counted, nothing of it is kept
          seen[h_row[s]] |= 1;
        } else if (h_verdict[s] == BPPP_RP_SCAN_OWNED) {
          ScanHit h;
          h.row = (uint32_t)(o + h_row[s]); h.key = h_key[s];
          memcpy(h.ss, h_ss.data() + (size_t)s * 8, 32);
          hits.push_back(h);
          seen[h_row[s]] |= 1;
        } else {
          tag_only++;
          seen[h_row[s]] |= 2;
        }
      }
    }
    BPPP_HIP(ctx, hipStreamSynchronize(st));             // h_status, when no tile had a survivor
    if (row_status)
      for (uint32_t b = 0; b < n; b++)
        row_status[o + b] = h_status[b] != SCAN_OPEN ? h_status[b] : (seen[b] & 1) ? BPPP_RP_SCAN_OWNED : (seen[b] & 2) ? BPPP_RP_SCAN_TAG_ONLY : BPPP_RP_SCAN_FOREIGN;
    // the pass's hits in the call's order; those under cap get their openings: pads and blindings again from ss, no commitment
    const size_t first = scan_keys_merge_pass(hits, cap, total, hit_key, hit_row);
    total += uncounted;
    for (size_t c0 = 0; want_open && c0 < hits.size(); c0 += S) {
      const size_t c = std::min(S, hits.size() - c0);
      const uint64_t m = (uint64_t)c * nr;
      h_row.resize(c); h_ss.resize(c * 8);
      for (size_t j = 0; j < c; j++) { h_row[j] = (uint32_t)(hits[c0 + j].row - o); memcpy(h_ss.data() + j * 8, hits[c0 + j].ss, 32); }
      BPPP_HIP(ctx, hipMemcpyAsync(K.surv_row, h_row.data(), c * 4, hipMemcpyHostToDevice, st));
      BPPP_HIP(ctx, hipMemcpyAsync(K.ss, h_ss.data(), c * 32, hipMemcpyHostToDevice, st));
      k_rp_scan_open_keys<<<dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st>>>(m, (uint32_t)nr, (uint32_t)sb, (uint32_t)cb, binary, D, seals, coms, K.surv_row, K.ss, K.in_sc, K.flag,
                                                                                nullptr);
      k_rp_scan_emit_keys<<<dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st>>>(m, binary, K.in_sc, at(d_amounts, first + c0), at(d_types, first + c0), at(d_blinds, first + c0));
      BPPP_HIP(ctx, hipGetLastError());
      BPPP_HIP(ctx, hipStreamSynchronize(st));
    }
  }
  for (size_t h = std::min(total, cap); h < cap; h++) { hit_key[h] = 0; hit_row[h] = 0; }
  *nhits = total;
  if (ntag_only) *ntag_only = tag_only;
  return BPPP_OK;
}

int scan_keys_device(bppp_rp *rp, size_t nkeys, const uint64_t *view_secrets, size_t rows, const void *d_coms, const void *d_seals, uint32_t *row_status, size_t cap,
                     uint32_t *hit_key, uint32_t *hit_row, void *d_amounts, void *d_types, void *d_blinds, size_t *nhits, uint64_t *ntag_only) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (nhits) *nhits = 0;
  if (ntag_only) *ntag_only = 0;
  if (!nhits || !view_secrets || (cap && (!hit_key || !hit_row))) return fail(ctx, BPPP_ERR_ARG, "rp_scan_keys: null input");
  if (!nkeys || nkeys > BPPP_RP_SCAN_MAX_KEYS) return fail(ctx, BPPP_ERR_ARG, "rp_scan_keys: the number of keys must be in [1, 2^20]");
  KeyRecs recs;
  recs.v.resize(nkeys);
  for (size_t k = 0; k < nkeys; k++) {
    const bppp_host::U256 a = bppp_host::U256::load(view_secrets + 4 * k);
    if (a.is_zero() || bppp_host::cmp(a, bppp_host::FR().m) >= 0) return fail(ctx, BPPP_ERR_ARG, "rp_scan_keys: key " + std::to_string(k) + ": the view secret must be in [1, n)");
    if (!scan_keys_recode(view_secrets + 4 * k, recs.v[k])) return fail(ctx, BPPP_ERR_ARG, "rp_scan_keys: key " + std::to_string(k) + ": the view secret's halves do not fit the walk");
  }
  if (!rp->D.nr || rows > RPP_LIM31 / rp->D.nr) return fail(ctx, BPPP_ERR_ARG, "rp_scan_keys: rows * nranges must be below 2^31");
  hipSetDevice(ctx->device);
  const size_t nr = rp->D.nr;
  hipStream_t st = ctx->stream;
  // every slot that no hit fills receives zeros
  for (void *out : {d_amounts, d_types, d_blinds}) if (out && cap) BPPP_HIP(ctx, hipMemsetAsync(out, 0, cap * nr * 32, st));
  if (!rows) {
    for (size_t h = 0; h < cap; h++) { hit_key[h] = 0; hit_row[h] = 0; }
    BPPP_HIP(ctx, hipStreamSynchronize(st));
    return BPPP_OK;
  }
  if (!d_coms || !d_seals) return fail(ctx, BPPP_ERR_ARG, "rp_scan_keys: null input");
  int rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const ScanKeysGeom G = scan_keys_geometry(rpp_flat_chunk(rp), nr, rows, nkeys);
  const ScanKeysCarve Z = scan_keys_carve(G, nr, SCANK_TAB_WORDS, XYZZ_WORDS, SCAN_KEY_WORDS);
  KeysWork K;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    K.R = cv.take<uint32_t>(Z.R); K.status = cv.take<uint32_t>(Z.status); K.tab = cv.take<uint32_t>(Z.tab); K.keys = cv.take<uint32_t>(Z.keys); K.acc = cv.take<uint32_t>(Z.acc);
    K.P = cv.take<uint32_t>(Z.P); K.count = cv.take<uint32_t>(Z.count); K.surv_row = cv.take<uint32_t>(Z.surv_row); K.surv_key = cv.take<uint32_t>(Z.surv_key);
    K.ss = cv.take<uint32_t>(Z.ss); K.in_sc = cv.take<uint32_t>(Z.in_sc); K.flag = cv.take<uint32_t>(Z.flag); K.dec = cv.take<uint32_t>(Z.dec); K.rec = cv.take<uint32_t>(Z.rec);
    K.verdict = cv.take<uint32_t>(Z.verdict);
    if (!pass && (rc = rpp_ensure_pwork(rp, cv.off))) return rc;
  }
  rc = scan_keys_passes(rp, recs, rows, d_coms, d_seals, row_status, cap, hit_key, hit_row, d_amounts, d_types, d_blinds, nhits, ntag_only, G, K);
  // the recoded keys leave HBM whatever happened (the host copies go with recs)
  const bool wiped = hipMemsetAsync(K.keys, 0, Z.keys * 4, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
  if (!rc && !wiped) return fail(ctx, BPPP_ERR_HIP, "rp_scan_keys: the key buffer could not be wiped");
  return rc;
}

}  // namespace

extern "C" {

int bppp_rp_scan_keys_device(bppp_rp *rp, size_t nkeys, const uint64_t *view_secrets, size_t rows, const void *d_coms_files, const void *d_seals, uint32_t *row_status, size_t cap,
                             uint32_t *hit_key, uint32_t *hit_row, void *d_amounts, void *d_types, void *d_blinds, size_t *nhits, uint64_t *ntag_only) {
  return scan_keys_device(rp, nkeys, view_secrets, rows, d_coms_files, d_seals, row_status, cap, hit_key, hit_row, d_amounts, d_types, d_blinds, nhits, ntag_only);
}

int bppp_rp_scan_keys(bppp_rp *rp, size_t nkeys, const uint64_t *view_secrets, size_t rows, const uint8_t *coms_files, const uint8_t *seals, uint32_t *row_status, size_t cap,
                      uint32_t *hit_key, uint32_t *hit_row, uint64_t *amounts, uint64_t *types, uint64_t *blinds, size_t *nhits, uint64_t *ntag_only) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (cap && (!hit_key || !hit_row)) return fail(ctx, BPPP_ERR_ARG, "rp_scan_keys: null input");     // judged here: the _device variant may see a smaller cap
  DevBuf c, s, amt, ty, bl;
  const size_t nr = rp->D.nr;
  // no call has more hits than pairs: the slots in HBM stop there, and the caller's slots beyond are zeroed here
  size_t dcap = 0;
  if (nr && rows <= RPP_LIM31 / nr && nkeys <= BPPP_RP_SCAN_MAX_KEYS) {
    hipSetDevice(ctx->device);
    dcap = std::min(cap, rows * nkeys);
    const size_t cl = dcap * nr * 32;
    int rc;
    if (rows && ((rc = c.up(ctx, coms_files, rows * (size_t)rp->D.coms_bytes)) || (rc = s.up(ctx, seals, rows * BPPP_RP_SEAL_BYTES(nr))))) return rc;
    if (dcap && ((rc = amt.out(ctx, amounts, cl)) || (rc = ty.out(ctx, types, cl)) || (rc = bl.out(ctx, blinds, cl)))) return rc;
  }
  int rc = scan_keys_device(rp, nkeys, view_secrets, rows, c.p, s.p, row_status, dcap, hit_key, hit_row, amt.p, ty.p, bl.p, nhits, ntag_only);
  if (rc) return rc;
  for (size_t h = dcap; h < cap; h++) { if (hit_key) hit_key[h] = 0; if (hit_row) hit_row[h] = 0; }
  const size_t cl = dcap * nr * 32, tail = (cap - dcap) * nr * 32;
  for (auto io : {std::make_pair(amounts, amt.p), std::make_pair(types, ty.p), std::make_pair(blinds, bl.p)}) {
    if (!io.first) continue;
    if (cl) BPPP_HIP(ctx, hipMemcpy(io.first, io.second, cl, hipMemcpyDeviceToHost));
    if (tail) memset((uint8_t *)io.first + cl, 0, tail);
  }
  return BPPP_OK;
}

}  // extern "C"
