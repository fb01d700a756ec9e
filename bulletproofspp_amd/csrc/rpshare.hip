// rpshare.hip — one comb table for the prover handles of a basis family (bppp_rp_share_comb, bppp_rp_comb_info) and the prover of a job
// of several setups (bppp_rp_prove_mixed), include/bppp.h.
//
// Every setup's basis [g | H | G] is the prefix ps[1 : 2 + linLen + nrmLen] of the point stream its points came from (csrc/rpmixed.hip),
// and the comb table is laid out tab[w][i][d - 1] (csrc/comb.hpp) with the comb kernels taking the table's stride T and a launch's row
// length as two arguments: the table of the longest basis of a stream serves every shorter one.  A CombTable counts its holders
// (comb_retain / comb_release); a handle holds the table it built or the one it was given (rp_set_comb, csrc/rpprove.hip) and passes
// its own row length to every launch.  Which kernel a borrower's launch takes is decided as for an owner: the lane-per-instance rows
// kernel looks at the TABLE's bytes (csrc/comb.hip), and a borrower's gathers are spread over the whole shared table (stride T per
// window), so it is the shared table's size that counts — same results on either route.
//
// bppp_rp_prove_mixed: families as the mixed verifier forms them; one table per family that reaches its threshold; the input
// commitments v g + ty H0 + bl H1 of ALL groups of such a family in one comb_lanes launch (the first three registered points are the
// same for every setup of a stream); then the groups in order, each through bppp_rp_prove_batch_pub — its routes, its split in two
// halves, its bytes — with rpp_commit_inputs copying the group's share of that launch.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "comb.hpp"
#include "rp_internal.hpp"

using namespace bppp;
using bppp_host::U256;

extern "C" {

int bppp_rp_share_comb(bppp_rp *rp, bppp_rp *donor) {
  if (!rp || !donor) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (donor->ctx != ctx) return fail(ctx, BPPP_ERR_ARG, "rp_share_comb: the handles are on different contexts");
  if (rp_basis_points(donor) < rp_basis_points(rp) || !rp_same_stream(rp, donor))
    return fail(ctx, BPPP_ERR_ARG, "rp_share_comb: the donor's basis (" + std::to_string(rp_basis_points(donor)) + " points) does not extend this handle's (" +
                                       std::to_string(rp_basis_points(rp)) + " points) point by point");
  if (!donor->comb) {
    if (donor->opt.no_comb) return fail(ctx, BPPP_ERR_ARG, "rp_share_comb: the donor's comb table is switched off (COMB_BUDGET 0)");
    donor->comb_failed = false;                 // an explicit request tries again
    const int rc = rp_ensure_comb(donor);
    if (rc) return rc;
    if (!donor->comb) return fail(ctx, BPPP_ERR_HIP, std::string("rp_share_comb: the donor's table could not be built: ") + bppp_last_error(ctx));
  }
  rp_set_comb(rp, donor->comb);
  rp->comb_failed = false;
  return BPPP_OK;
}

int bppp_rp_comb_info(const bppp_rp *rp, int *window_bits, size_t *table_bytes, size_t *table_points, size_t *users) {
  if (!rp) return BPPP_ERR_ARG;
  const CombTable *t = rp->comb;
  if (window_bits) *window_bits = t ? t->c : 0;
  if (table_bytes) *table_bytes = t ? t->bytes : 0;
  if (table_points) *table_points = t ? t->T : 0;
  if (users) *users = t ? (size_t)(t->refs - t->twins) : 0;
  return BPPP_OK;
}

}  // extern "C"

namespace {

struct Family {
  std::vector<size_t> members;     // indices of its non-empty groups, in job order
  bppp_rp *longest = nullptr;      // the handle of its longest basis
};

// the job's argument checks: what bppp_rp_prove_batch_pub refuses before it looks at a proof, and what only a job can get wrong
int mixed_prove_check(const bppp_rp_prove_group *groups, size_t ngroups, bppp_ctx **ctx_out) {
  *ctx_out = nullptr;
  if (ngroups && !groups) return BPPP_ERR_ARG;
  for (size_t s = 0; s < ngroups; s++) if (!groups[s].rp) return BPPP_ERR_ARG;
  if (!ngroups) return BPPP_OK;
  bppp_ctx *ctx = groups[0].rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  *ctx_out = ctx;
  for (size_t s = 0; s < ngroups; s++) {
    const bppp_rp_prove_group &g = groups[s];
    const std::string who = "rp_prove_mixed: group " + std::to_string(s) + ": ";
    if (g.rp->ctx != ctx) return fail(ctx, BPPP_ERR_ARG, who + "the handles are on different contexts");
    for (size_t t = 0; t < s; t++)
      if (groups[t].rp == g.rp) return fail(ctx, BPPP_ERR_ARG, who + "one handle in two groups (merge them into one group)");
    if (!g.batch) continue;
    if (!g.amounts || (!g.types && g.rp->st.kind == 0) || !g.blinds || (g.prefix_len && !g.rand_prefix) || !g.coms_files || !g.proof_files)
      return fail(ctx, BPPP_ERR_ARG, who + "a null buffer in a non-empty group");
    if (g.batch >= (1u << 20) || g.prefix_len > 4096) return fail(ctx, BPPP_ERR_ARG, who + "bad arguments (2^20 proofs or more, or a prefix beyond 4096 bytes)");
  }
  return BPPP_OK;
}

// One table for the family, if it is to have one: the longest existing table that covers its longest basis, else — at the threshold —
// a new one over the longest basis under that handle's options.  Handles with the table switched off are left alone.
int family_table(bppp_ctx *ctx, const bppp_rp_prove_group *groups, const Family &f) {
  CombTable *have = nullptr;
  size_t proofs = 0, comb_min = (size_t)-1;
  bool wanted = false;                           // some member would use a table at all
  for (size_t s : f.members) {
    bppp_rp *rp = groups[s].rp;
    if (rp->comb && rp->comb->T >= rp_basis_points(f.longest) && (!have || rp->comb->T > have->T)) have = rp->comb;
    proofs += groups[s].batch + rp->proved_total;
    if (!rp->opt.no_comb && !rp->opt.host_algebra) { comb_min = std::min(comb_min, rp->opt.comb_min); wanted = true; }
  }
  if (!have) {
    bppp_rp *l = f.longest;
    if (!wanted || proofs < comb_min || l->opt.no_comb || l->comb_failed) return BPPP_OK;      // below the threshold: every handle as on its own
    const int rc = rp_ensure_comb(l);
    if (rc) return rc;
    if (!l->comb) return BPPP_OK;                // no room: the attempt is not repeated (comb_failed), the groups take the bucket route
    have = l->comb;
  }
  for (size_t s : f.members) if (!groups[s].rp->opt.no_comb) rp_set_comb(groups[s].rp, have);
  (void)ctx;
  return BPPP_OK;
}

// v g + ty H0 + bl H1 (typed; binary: v g + bl h0) of every proof of the family's groups that prove over its table: scalars staged on
// the host in job order, ONE comb_lanes launch into ctx->mix, complete on return.  A scalar that is not canonical is staged as zero:
// its group's own checks refuse the proof before anything is written.
int family_inputs(bppp_ctx *ctx, const bppp_rp_prove_group *groups, const Family &f, std::vector<const uint32_t *> &pre) {
  const CombTable *t = nullptr;
  size_t n = 0;
  for (size_t s : f.members) {
    bppp_rp *rp = groups[s].rp;
    if (!rp->comb || rp->opt.host_algebra) continue;
    if (!t) t = rp->comb;
    if (rp->comb == t) n += groups[s].batch * rp->st.rds.size();
  }
  if (!t || !n) return BPPP_OK;
  std::vector<uint64_t> h(n * 12, 0);
  std::vector<size_t> off(f.members.size(), 0);
  size_t at = 0;
  for (size_t m = 0; m < f.members.size(); m++) {
    const bppp_rp_prove_group &g = groups[f.members[m]];
    bppp_rp *rp = g.rp;
    if (rp->comb != t || rp->opt.host_algebra) continue;
    off[m] = at;
    const size_t cnt = g.batch * rp->st.rds.size();
    const bool binary = rp->st.kind == 1;
    rp_parallel(cnt, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) {
        uint64_t *dst = &h[(at + i) * 12];
        bppp_rps::s_mod_n(U256::load(g.amounts + 4 * i)).store(dst);
        const uint64_t *second = binary ? g.blinds + 4 * i : g.types + 4 * i, *third = binary ? nullptr : g.blinds + 4 * i;
        if (bppp_host::scalars_canonical(second, 1)) memcpy(dst + 4, second, 32);
        if (third && bppp_host::scalars_canonical(third, 1)) memcpy(dst + 8, third, 32);
      }
    });
    at += cnt;
  }
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t sc_bytes = (n * 96 + 255) & ~(size_t)255, need = sc_bytes + n * 64;
  if (need > ctx->mix_bytes) {
    BPPP_HIP(ctx, hipStreamSynchronize(st));
    if (ctx->mix) BPPP_HIP(ctx, hipFree(ctx->mix));
    ctx->mix = nullptr; ctx->mix_bytes = 0;
    BPPP_HIP(ctx, hipMalloc(&ctx->mix, need + need / 8));
    ctx->mix_bytes = need + need / 8;
  }
  uint32_t *d_sc = (uint32_t *)ctx->mix, *d_pt = (uint32_t *)((char *)ctx->mix + sc_bytes);
  BPPP_HIP(ctx, hipMemcpyAsync(d_sc, h.data(), n * 96, hipMemcpyHostToDevice, st));
  const int rc = comb_lanes(t, d_sc, 3, n, d_pt, st);
  if (rc) return fail(ctx, rc, bppp_last_error(t->ctx));
  BPPP_HIP(ctx, hipStreamSynchronize(st));       // the groups (and their twins, on streams of their own) read them from here on
  for (size_t m = 0; m < f.members.size(); m++) {
    const bppp_rp *rp = groups[f.members[m]].rp;
    if (rp->comb == t && !rp->opt.host_algebra) pre[f.members[m]] = d_pt + off[m] * 16;
  }
  return BPPP_OK;
}

int mixed_prove_run(bppp_ctx *ctx, const bppp_rp_prove_group *groups, size_t ngroups) {
  std::vector<Family> fams;
  for (size_t s = 0; s < ngroups; s++) {
    if (!groups[s].batch) continue;
    bppp_rp *rp = groups[s].rp;
    Family *f = nullptr;
    for (Family &c : fams) if (rp_same_stream(c.longest, rp)) { f = &c; break; }
    if (!f) { fams.emplace_back(); f = &fams.back(); f->longest = rp; }
    if (rp_basis_points(rp) > rp_basis_points(f->longest)) f->longest = rp;
    f->members.push_back(s);
  }
  // one family's inputs at a time live in ctx->mix: a family's groups run before the next family's launch reuses the buffer
  for (const Family &f : fams) {
    int rc = family_table(ctx, groups, f);
    if (rc) return rc;
    std::vector<const uint32_t *> pre(ngroups, nullptr);
    rc = family_inputs(ctx, groups, f, pre);
    if (rc) return rc;
    for (size_t s : f.members) {
      const bppp_rp_prove_group &g = groups[s];
      g.rp->pre_inputs = pre[s];
      rc = bppp_rp_prove_batch_pub(g.rp, g.batch, g.amounts, g.types, g.blinds, g.public_amounts, g.rand_prefix, g.prefix_len, g.coms_files, g.proof_files);
      g.rp->pre_inputs = nullptr;
      if (rc) return fail(ctx, rc, "rp_prove_mixed: group " + std::to_string(s) + ": " + bppp_last_error(ctx));
    }
  }
  return BPPP_OK;
}

}  // namespace

extern "C" int bppp_rp_prove_mixed(const bppp_rp_prove_group *groups, size_t ngroups) {
  bppp_ctx *ctx;
  int rc = mixed_prove_check(groups, ngroups, &ctx);
  if (rc || !ctx) return rc;
  rc = mixed_prove_run(ctx, groups, ngroups);
  if (rc) ctx_drain(ctx);
  return rc;
}
