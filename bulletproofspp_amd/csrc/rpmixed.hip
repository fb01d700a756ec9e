// rpmixed.hip — batch verification of range proofs of SEVERAL setups (bppp_rp handles: typed-reciprocal or binary, either argument
// flavour) with ONE combined MSM (bppp_rp_verify_mixed*, include/bppp.h).
//
// Every setup's verification basis [g | H | G] is the prefix ps[1 : 2 + linLen + nrmLen] of the point stream its points came from
// (TypedReciprocal.hs:334, :348-349: h : g : hs ++ gs; Binary.hs:147-148: [h, g, h0, h1] ++ gs), and each handle keeps that prefix in
// stream order (rp->d_basis; rp->c_points on the host, index 0 being h).  Handles whose prefixes extend one another form a FAMILY whose
// union basis is its longest member's d_basis; the shared-basis scalars of all its groups are summed onto that union (the merge
// csrc/nlbatch.hip does inside one setup, taken across setups), and unrelated families are concatenated.  The MSM is
//   [family 0 union basis | family 1 ... | group 0 per-proof terms | group 1 ...]
// of sum_f max_{s in f} (1 + llen_s + nlen_s) + sum_s B_s (ninit_s + 2 k_s) terms.
//
// Per group, the single-setup pipeline is reused unchanged: rp_verify_prepare (decode, hashing, public scalars, rho at the group's job
// positions), then the assembly step of nl/ip_verify_batch_run writing into this call's own buffer (ctx->mix: the next group's assembly
// reuses ctx->ws2).  On rejection each group's own combination is evaluated from the arrays its handle still holds and failing groups
// are bisected by the same rp_find_culprits the single-setup verifier uses.
#include <string.h>
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "fe.hip.h"
#include "rp_internal.hpp"

namespace bppp {

static constexpr uint32_t MIX_MEMBERS = 16;           // member groups per launch of k_mix_union_scalars (by value in the kernel arguments)
struct MixMember { const uint32_t *sc; uint32_t llen, nlen; };
struct MixMembers { MixMember m[MIX_MEMBERS]; uint32_t n; };

// One lane per position i of a family's union basis: the sum mod n of every member group's shared scalar on that point.  A group's
// shared scalars are [G (nlen) | H (llen) | g] (nlbatch.hip's order); their stream positions are g -> 0, H_j -> 1 + j, G_j -> 1 + llen + j.
// Gather form, members in job order: deterministic, no atomics.  accumulate: add onto `out` (a family of more than MIX_MEMBERS groups
// takes several launches).
__global__ void __launch_bounds__(256) k_mix_union_scalars(MixMembers M, uint32_t ulen, int accumulate, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ulen) return;
  fe acc = accumulate ? fe_load(out + (size_t)i * 8) : fe_zero();
  for (uint32_t j = 0; j < M.n; j++) {
    const uint32_t llen = M.m[j].llen, nlen = M.m[j].nlen;
    uint32_t idx;
    if (i == 0) idx = nlen + llen;
    else if (i - 1 < llen) idx = nlen + (i - 1);
    else if (i - 1 - llen < nlen) idx = i - 1 - llen;
    else continue;                                       // beyond this member's prefix
    acc = fe_add<1>(acc, fe_load(M.m[j].sc + (size_t)idx * 8));
  }
  fe_store(out + (size_t)i * 8, acc);
}

}  // namespace bppp

using namespace bppp;

namespace {

struct MixGroup {
  bppp_rp *rp;
  RpFiles files;
  size_t B, start;                 // proofs, first job position (relative to index_offset)
  size_t shared, per;              // 1 + llen + nlen shared scalars; ninit + 2k terms per proof
  size_t tail_off, shared_off;     // first MSM term of its per-proof terms; its shared scalars in the mix buffer (in scalars)
  int family;
  RpVerifyArrays A;
};

size_t basis_points(const bppp_rp *rp) { return rp_basis_points(rp); }
bool same_stream(const bppp_rp *a, const bppp_rp *b) { return rp_same_stream(a, b); }      // rp_internal.hpp: shared with the prover's families (csrc/rpshare.hip)

// the checks both entry points make; *ctx_out is the groups' context (null when there is none to report to)
int mixed_check(const bppp_rp_group *groups, size_t ngroups, const uint8_t *seed, int *accept, bppp_ctx **ctx_out, size_t *total_out) {
  *ctx_out = nullptr; *total_out = 0;
  if (!accept || (ngroups && !groups)) return BPPP_ERR_ARG;
  for (size_t s = 0; s < ngroups; s++) if (!groups[s].rp) return BPPP_ERR_ARG;
  if (!ngroups) return BPPP_OK;
  bppp_ctx *ctx = groups[0].rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  *ctx_out = ctx;
  size_t total = 0;
  for (size_t s = 0; s < ngroups; s++) {
    const bppp_rp_group &g = groups[s];
    if (g.rp->ctx != ctx) return fail(ctx, BPPP_ERR_ARG, "rp_verify_mixed: the handles are on different contexts");
    for (size_t t = 0; t < s; t++)
      if (groups[t].rp == g.rp) return fail(ctx, BPPP_ERR_ARG, "rp_verify_mixed: one handle in two groups (merge them into one group)");
    if (g.batch && (!g.coms_files || !g.proof_files)) return fail(ctx, BPPP_ERR_ARG, "rp_verify_mixed: null files for a non-empty group");
    if (g.batch >= (1u << 22) || (total += g.batch) >= (1u << 22)) return fail(ctx, BPPP_ERR_ARG, "rp_verify_mixed: 2^22 proofs or more");
  }
  if (total && !seed) return fail(ctx, BPPP_ERR_ARG, "rp_verify_mixed: null seed");
  *total_out = total;
  return BPPP_OK;
}

// host: the groups' files are on the host, each staged in its handle's buffer (rp_stage_files)
int mixed_run(bppp_ctx *ctx, const bppp_rp_group *groups, size_t ngroups, uint64_t index_offset, bool host, const uint8_t seed[32], int *accept,
              uint32_t *proof_status, uint64_t *combined_xy) {
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  // the job's layout: families of the non-empty groups (host side, once per call), union bases first, then every group's per-proof terms
  std::vector<MixGroup> gs;
  std::vector<bppp_rp *> rep;                            // longest member of each family
  size_t start = 0;
  for (size_t s = 0; s < ngroups; s++) {
    bppp_rp *rp = groups[s].rp;
    const size_t B = groups[s].batch;
    rp->n_combined = rp->n_each = 0;                     // (bppp_test_rp_last_verify_counts: this call's culprit search on the handle)
    if (B) {
      MixGroup g{};
      g.rp = rp; g.files = RpFiles{groups[s].coms_files, groups[s].proof_files}; g.B = B; g.start = start;
      if (host) { const int rc = rp_stage_files(rp, B, groups[s].coms_files, groups[s].proof_files, g.files); if (rc) return rc; }
      g.shared = 1 + rp->st.llen + rp->st.nlen; g.per = rp->D.nrp + rp->D.nr + 2 * (size_t)rp->st.rounds;
      g.family = -1;
      for (size_t f = 0; f < rep.size() && g.family < 0; f++)
        if (same_stream(rep[f], rp)) { g.family = (int)f; if (basis_points(rp) > basis_points(rep[f])) rep[f] = rp; }
      if (g.family < 0) { g.family = (int)rep.size(); rep.push_back(rp); }
      gs.push_back(g);
    }
    start += B;
  }
  std::vector<size_t> fam_off(rep.size());
  size_t T = 0, nshared = 0;
  for (size_t f = 0; f < rep.size(); f++) { fam_off[f] = T; T += basis_points(rep[f]); }
  for (MixGroup &g : gs) { g.tail_off = T; T += g.B * g.per; g.shared_off = nshared; nshared += g.shared; }
  ctx->last_mixed_terms = T;
  // the MSM's scalars and points, the groups' shared scalars, their flag words: ctx->mix, grow-only
  uint32_t *sc = nullptr, *pts = nullptr, *shared = nullptr, *flags = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? ctx->mix : nullptr, ctx->mix_bytes);
    sc = cv.take<uint32_t>((T + 32) * 8); pts = cv.take<uint32_t>(T * 16); shared = cv.take<uint32_t>(nshared * 8); flags = cv.take<uint32_t>(gs.size());
    if (!pass && cv.off > ctx->mix_bytes) {
      BPPP_HIP(ctx, hipStreamSynchronize(st));
      if (ctx->mix) BPPP_HIP(ctx, hipFree(ctx->mix));
      ctx->mix = nullptr; ctx->mix_bytes = 0;
      BPPP_HIP(ctx, hipMalloc(&ctx->mix, cv.off + cv.off / 8));
      ctx->mix_bytes = cv.off + cv.off / 8;
    }
  }
  BPPP_HIP(ctx, hipMemsetAsync(flags, 0, gs.size() * 4, st));
  // per group: the single-setup pipeline up to the MSM, then its assembly into this call's buffers (per-proof terms at their place in the
  // MSM, shared scalars aside for the merge)
  for (size_t i = 0; i < gs.size(); i++) {
    MixGroup &g = gs[i];
    bppp_rp *rp = g.rp;
    int rc = rp_verify_prepare(rp, g.B, index_offset + g.start, g.files, seed, g.A);
    if (rc) return rc;
    const bppp_rps::Setup &S = rp->st;
    const RpDims &D = rp->D;
    const size_t nlen = S.nlen, llen = S.llen, k = S.rounds, ninit = D.nrp + D.nr;
    rc = ensure_scratch(ctx, S.flavour ? ip_verify_batch_scratch(g.B, nlen, llen, k, D.fn) : nl_verify_batch_scratch(g.B, nlen, llen, k));
    if (rc) return rc;
    const RpVerifyArrays &A = g.A;
    auto assemble = S.flavour ? ip_verify_batch_assemble : nl_verify_batch_assemble;
    rc = assemble(ctx, g.B, nlen, llen, k, D.fn, D.fl, ninit, rp->d_g(), rp->d_G(), rp->d_H(), A.rho, A.q, A.sp, A.pub_norm, A.pub_lin_c, A.pub_lin_x, A.es,
                  A.wit_norm, A.wit_lin, A.init_sc, A.init_pts, A.resp_pts, false, shared + g.shared_off * 8, sc + g.tail_off * 8, pts + g.tail_off * 16, false,
                  flags + i);
    if (rc) return rc;
  }
  // the merge: every family's shared scalars summed onto its union basis (stream order), which is its longest member's d_basis
  for (size_t f = 0; f < rep.size(); f++) {
    const uint32_t ulen = (uint32_t)basis_points(rep[f]);
    MixMembers M{};
    int launched = 0;
    for (size_t i = 0; i <= gs.size(); i++) {
      if (i < gs.size() && gs[i].family == (int)f) {
        M.m[M.n++] = MixMember{shared + gs[i].shared_off * 8, (uint32_t)gs[i].rp->st.llen, (uint32_t)gs[i].rp->st.nlen};
        if (M.n < MIX_MEMBERS) continue;
      }
      if (!M.n) continue;
      k_mix_union_scalars<<<dim3((ulen + 255) / 256), dim3(256), 0, st>>>(M, ulen, launched, sc + fam_off[f] * 8);
      launched = 1; M.n = 0;
    }
    BPPP_HIP(ctx, hipMemcpyAsync(pts + fam_off[f] * 16, rep[f]->d_basis, (size_t)ulen * 64, hipMemcpyDeviceToDevice, st));
  }
  BPPP_HIP(ctx, hipGetLastError());
  uint64_t out_xy[8];
  { const int rc = msm_run(ctx, sc, pts, T, 1, 1, 0, out_xy); if (rc) return rc; }
  // (msm_run returned with the stream drained) the inner-product assemblies' flag words, the decode failures of every group
  std::vector<uint32_t> hflags(gs.size());
  BPPP_HIP(ctx, hipMemcpy(hflags.data(), flags, gs.size() * 4, hipMemcpyDeviceToHost));
  bool any_bad = false;
  for (size_t i = 0; i < gs.size(); i++) {
    if (gs[i].rp->st.flavour) { const int rc = ip_verify_batch_flags(ctx, hflags[i]); if (rc) return rc; }
    any_bad |= gs[i].rp->hflag[0] != 0;
  }
  const bool whole = rp_point_is_inf(out_xy);
  if (combined_xy) memcpy(combined_xy, out_xy, 64);
  *accept = (whole && !any_bad) ? 1 : 0;
  if (!proof_status) return BPPP_OK;
  for (const MixGroup &g : gs) {
    uint32_t *status = proof_status + g.start;
    BPPP_HIP(ctx, hipMemcpy(status, g.A.bad, g.B * 4, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < g.B; b++) status[b] = status[b] ? BPPP_RP_MALFORMED : BPPP_RP_VALID;
  }
  if (whole) return BPPP_OK;
  // rejected: each group's own combination from the arrays its handle still holds, the failing ones bisected
  for (const MixGroup &g : gs) {
    const int rc = rp_find_culprits(g.rp, g.A, false, proof_status + g.start);
    if (rc) return rc;
  }
  return BPPP_OK;
}

// both entry points: files on the host (`host`) or in HBM; nothing of the call is in flight once it has returned
int mixed_verify(const bppp_rp_group *groups, size_t ngroups, uint64_t index_offset, bool host, const uint8_t seed[32], int *accept, uint32_t *proof_status,
                 uint64_t *combined_xy) {
  bppp_ctx *ctx;
  size_t total;
  int rc = mixed_check(groups, ngroups, seed, accept, &ctx, &total);
  if (rc) return rc;
  *accept = 0;
  if (combined_xy) memset(combined_xy, 0, 64);
  if (!total) {                                          // an empty job (or only empty groups) is accepted, as batch = 0 is
    if (ctx) ctx->last_mixed_terms = 0;
    *accept = 1;
    return BPPP_OK;
  }
  rc = mixed_run(ctx, groups, ngroups, index_offset, host, seed, accept, proof_status, combined_xy);
  if (rc || host) ctx_drain(ctx);
  return rc;
}

}  // namespace

extern "C" {

int bppp_rp_verify_mixed_device(const bppp_rp_group *groups, size_t ngroups, uint64_t index_offset, const uint8_t seed[32], int *accept,
                                uint32_t *proof_status, uint64_t *combined_xy) {
  return mixed_verify(groups, ngroups, index_offset, false, seed, accept, proof_status, combined_xy);
}

int bppp_rp_verify_mixed(const bppp_rp_group *groups, size_t ngroups, const uint8_t seed[32], int *accept, uint32_t *proof_status, uint64_t *combined_xy) {
  return mixed_verify(groups, ngroups, 0, true, seed, accept, proof_status, combined_xy);
}

}  // extern "C"
