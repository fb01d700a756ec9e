// comb.hip — fixed-base comb for THOUSANDS of MSMs over ONE short basis (the prover: range-proof commitments and every round of the
// lockstep argument, 2 x batch instances of ~775 terms each over the setup's [g | H | G]).
//
// The reference commits with `innerProduct` over the setup's fixed points (commitRPW, src/RangeProof/Internal.hs:45-50; the argument's
// round commitments, src/NormArgument.hs:100-128, over a basis that is a known linear image of the setup's).  With the basis fixed
// per setup and 288 GB of HBM, every multiple a signed c-bit digit can ask for is stored once:
//     tab[w][i][d - 1] = d * 2^(c w) * P_i          w < W = ceil(257 / c),   d = 1 .. 2^(c-1)
// (c = 16: 17 x 774 x 32768 entries of 64 B = 27.6 GB — the widest window whose table stays under the caller's budget is taken;
// c = 13: 4.1 GB), and an MSM is then nothing but one mixed addition per non-zero digit into ONE
// accumulator: no digit sort, no buckets, no bucket reduction, no window combine, no doubling — 17 additions per term against
// 29 + sort + reduction on the bucket route at its best window for this shape (csrc/msm.hip, c = 9).
//
// k_comb_msm: one wavefront per instance, lane l takes one term of every 64; the table entry of the NEXT digit is requested
// before the addition of the current one is issued, so the 64-B gathers (random over the table: HBM, not cache) hide under ~2.8 k
// VALU instructions each.  The 64 lane sums meet in a shuffle tree; lane 0 normalises.  VALU-bound like k_acc_points.
//
// k_comb_msm_rows (round 4): thousands of LONG rows of full-width scalars (the argument's rounds) over a table of tens of GB — lane = instance, the
// wavefront walks (term, window) in lockstep and its 64 gathers fall into ONE table row; k_comb_join_rows adds the partial sums of an instance.
// k_comb_msm_packed: thousands of rows of a few dozen terms (8 or 16 lanes per instance).  k_comb_lanes: one lane per three-term instance.
//
// Digits are read in the format of recode.hip.h; comb_gather / CombPipe / comb_walk below are the one table walk the kernels share.
// The kernels, the table fill and the launchers are csrc/comb.hip.h (shared with the test hooks); here: the tables' lifetime and the external entry points.
#include "comb.hip.h"

namespace bppp {

void comb_destroy(CombTable *t) {
  if (!t) return;
  hipSetDevice(t->ctx->device);
  hipStreamSynchronize(t->ctx->stream);
  if (t->tab) hipFree(t->tab);
  ctx_release(t->ctx);
  delete t;
}

int comb_create(bppp_ctx *ctx, const uint32_t *d_points, size_t T, int window_bits, size_t budget_bytes, CombTable **out) {
  if (!ctx || !d_points || !T || !out || T >= (1u << 24)) return BPPP_ERR_ARG;
  hipSetDevice(ctx->device);
  int c = window_bits;
  auto size_of = [&](int cc) { return comb_table_bytes(cc, T); };
  if (!c) { c = 18; while (c > 4 && size_of(c) > budget_bytes) c--; }
  if (c < 4 || c > 18) return fail(ctx, BPPP_ERR_ARG, "comb_create: window_bits must be in [4,18]");
  if (!window_bits && size_of(c) > budget_bytes) return fail(ctx, BPPP_ERR_ARG, "comb_create: no window of 4 bits or more fits the budget (" + std::to_string(size_of(c) >> 20) + " MiB needed)");
  CombTable *t = new CombTable();
  t->ctx = ctx; ctx_retain(ctx); t->T = T; t->c = c; t->W = (257 + c - 1) / c; t->D = 1 << (c - 1); t->tab = nullptr; t->bytes = size_of(c);
  // a failed hipMalloc (or launch) leaves its error in the runtime's last-error slot, which later successful calls do NOT clear on
  // ROCm 7: consume it here, or the next launch check of this context reports a stale out-of-memory
  const std::string err = comb_fill(t, d_points);
  if (!err.empty()) { (void)hipGetLastError(); comb_destroy(t); (void)hipGetLastError(); return fail(ctx, BPPP_ERR_HIP, err); }
  *out = t;
  return BPPP_OK;
}

int comb_lanes(const CombTable *t, const uint32_t *d_scalars, size_t nterms, size_t ninst, uint32_t *d_out_aff, hipStream_t st) {
  return comb_lanes_launch(t, d_scalars, nterms, ninst, d_out_aff, st);
}
int comb_groups(const CombTable *t, const uint32_t *d_scalars, size_t ninst, size_t l0, size_t n0, int L, uint32_t *d_out_aff, size_t out_stride, hipStream_t st) {
  return comb_groups_launch(t, d_scalars, ninst, l0, n0, L, d_out_aff, out_stride, st);
}
int comb_msm(const CombTable *t, const uint32_t *d_scalars, size_t ninst, uint32_t *d_out_aff, hipStream_t st, int rows_hint, size_t nterms, uint32_t *d_scratch,
             size_t scratch_bytes) {
  return comb_msm_launch(t, d_scalars, ninst, d_out_aff, st, rows_hint, nterms, d_scratch, scratch_bytes);
}

}  // namespace bppp
