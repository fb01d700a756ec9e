// rpprove_dev.hpp — interface between the two halves of the batch range-proof prover: csrc/rpprove.hip (entry point, witness digits,
// commitments, encoding; the host-algebra reference path) and csrc/rpprove_dev.hip (field algebra and transcript on the device).
#pragma once
#include <stddef.h>
#include <string>
#include <vector>
#include <stdint.h>
#include "rp_internal.hpp"
#include "trrp.hpp"

namespace bppp {

struct PDims { uint32_t nlen, llen, nr, T, nd, has_types, maxb; };     // T = 1 + llen + nlen (one commitment row), nd = random scalars per proof,
// maxb = entries of the per-proof reciprocal table 1 / (e + s), s < maxb: the power of two at or above the setup's widest digit base (16 .. 1024)

// The widest digit base a proof of this setup has digits of, rounded up to the table classes 16, 32, ..., 1024.  An assumed range has no digits
// and no symbols, whatever its base says; a live base is at most 1023 (a shared base b costs b - 1 of the TRRP_MAX_SYMS symbols, an inline one as
// many digits: bppp_rp_create refuses anything wider)
inline uint32_t rpp_table_class(uint32_t widest_base) {        // the power of two at or above the base, 16 at the least (a base fits 32 bits: no overflow below 2^31)
  uint32_t t = 16;
  while (t < widest_base && t < (1u << 31)) t <<= 1;
  return t;
}
inline uint32_t rpp_maxb(const bppp_rps::Setup &S) {
  uint32_t widest = 0;
  for (const bppp_rps::RangeData &rd : S.rds) if (!rd.assumed) widest = std::max(widest, rd.base);
  return rpp_table_class(widest);
}
// dynamic LDS of the two phase kernels (csrc/rpprove_dev.hip), one workgroup per proof, in field elements of 32 bytes.  Phase 2: the values and
// the prefix products of the batch inversion (e, r0, the maxb reciprocals, one entry per range), two scan rows of 64, the base map.  Phase 3: six
// reduction rows of 64, x^(2(j+1)) per range, the base map, four inverses
inline size_t rpp_phase2_lds_bytes(size_t maxb, size_t nr) { return (2 * (2 + maxb + nr) + 128 + (size_t)TRRP_MAX_SLOTS) * 32; }
inline size_t rpp_phase3_lds_bytes(size_t nr) { return ((size_t)6 * 64 + nr + (size_t)TRRP_MAX_SLOTS + 4) * 32; }
// does the device algebra serve this setup?  (csrc/rpprove.hip: what does not fit takes the host-algebra route, same bytes out)
inline bool rpp_phases_fit_lds(const bppp_rps::Setup &S) {
  return rpp_phase2_lds_bytes(rpp_maxb(S), S.rds.size()) <= LDS_MAX_BYTES && rpp_phase3_lds_bytes(S.rds.size()) <= LDS_MAX_BYTES;
}

struct RppHostInputs {
  size_t batch;
  const uint64_t *in_sc;     // [batch][nr][3][4]: amount, type, blinding as field elements
  const uint32_t *dig;       // [batch][nlen]: the digit of every norm position (unused at typing positions)
  const uint32_t *mul;       // [batch][nlen]: the inline multiplicity (0 elsewhere)
  const uint32_t *mss;       // [batch][llen - 6]: the shared multiplicities
  const uint8_t *prefix; size_t prefix_len;
  const uint64_t *pub;       // NULL (the setup's public amounts) or [batch][npub][4] canonical: bppp_rp_prove_batch_pub
};
struct RppOutputs {          // host arrays
  uint64_t *input_coms;      // [batch][nr][8]
  uint64_t *c_dm, *c_m, *c_r, *c_bl;   // [batch][8] each
  uint64_t *resp;            // [batch][rounds][16]: (X, R), last round first
  uint64_t *wit_norm, *wit_lin;        // [batch][fn][4], [batch][fl][4]
};

int rpp_device_prove(bppp_rp *rp, const RppHostInputs &in, RppOutputs &out);

// RangeProof.Binary (csrc/brpprove_dev.hip): proveBRPM + proveBPM of B proofs as one stream of kernels over the handle's comb table
struct BrpHostInputs {
  size_t batch;
  const uint64_t *in_sc;     // [batch][nr][3][4]: amount, blinding, 0 as field elements (scalarRPW', src/RangeProof/Internal.hs:56-57)
  const uint8_t *bits;       // [batch][nlive]: the binary digit of every live norm position (makeDigits, src/RangeProof/Binary.hs:56-69)
  const uint8_t *prefix; size_t prefix_len;
  const uint64_t *pub;       // NULL (the setup's net_public) or [batch][4] canonical: bppp_rp_prove_batch_pub
};
struct BrpOutputs {          // host arrays
  uint64_t *input_coms;      // [batch][nr][8]
  uint64_t *c_d, *c_bl;      // [batch][8] each
  uint64_t *resp;            // [batch][rounds][16]: (X, R) resp. (L, R), last round first
  uint64_t *wit_norm, *wit_lin;
};
int brp_device_prove(bppp_rp *rp, const BrpHostInputs &in, BrpOutputs &out);

// The device workspace of one batch of either prover, carved from rp->pwork (rpp_carve / brp_carve): the inputs of the stream of kernels — in_sc,
// dig, mul, mss (typed) or bits (binary), prefix — are filled by an upload (the host entry points) or by the witness kernel
// (bppp_rp_prove_batch_device, csrc/rpwitness.hip); the rest is the stream's own
struct RppWork {
  uint32_t *in_sc, *in_pt, *dig, *mul, *mss, *rnd, *rows_dm_m, *row_r, *row_bl, *ccbuf, *invtab, *aux, *ch, *es, *tstart, *ptbuf, *a_s, *a_q, *a_lx, *a_nx, *p_sp,
           *p_norm, *p_cs, *p_init, *d_resp, *d_com, *cscratch, *wn, *wl, *status;
  uint8_t *bits, *text, *hdrs;
  const uint8_t *prefix;     // [batch][prefix_len] in HBM: carved (prefix_own), or the caller's buffer
  uint8_t *prefix_own;
};
// what a stream leaves in HBM for k_rp_encode_files: input commitments [batch][nr][16], the range-proof commitments (typed: [dm m] x batch, r x batch,
// bl x batch; binary: d x batch, bl x batch), responses [rounds][batch][2][16] in round order, the final witness [batch][fn][8], [batch][fl][8]
struct RppDevResults { const uint32_t *input_coms, *coms, *resp, *wit_norm, *wit_lin; };
int rpp_carve(bppp_rp *rp, size_t batch, size_t prefix_len, bool own_prefix, RppWork &W);
int brp_carve(bppp_rp *rp, size_t batch, size_t prefix_len, bool own_prefix, RppWork &W);
// the provers' kernels from the randomness to the end of the argument over inputs that lie in W; d_pub: NULL or the batch's canonical public
// amounts in HBM.  Exactly one of `host` (results downloaded, as rpp_device_prove / brp_device_prove return them) and `dev` (results stay in
// HBM; needs the handle's comb table) is given.  Returns with the stream drained.
int rpp_prove_body(bppp_rp *rp, size_t batch, const RppWork &W, size_t prefix_len, const uint32_t *d_pub, RppOutputs *host, RppDevResults *dev);
int brp_prove_body(bppp_rp *rp, size_t batch, const RppWork &W, size_t prefix_len, const uint32_t *d_pub, BrpOutputs *host, RppDevResults *dev);
// proofs [index_base, index_base + batch) of a bppp_rp_prove_batch_device call on a route with a device stream (csrc/rpwitness.hip): every
// buffer in HBM but `pub` (NULL or the half's canonical public amounts, on the host as bppp_rp_prove_batch_pub's halves take them).
// proof_status: NULL (a refused witness fails the call) or the half's [batch] verdicts on the host (bppp_rp_prove_batch_status_device: the refused
// proofs' files are zeroed, the others proved)
int rp_prove_device_half(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds, const uint64_t *pub, const uint8_t *d_prefix,
                         size_t prefix_len, uint8_t *d_coms_files, uint8_t *d_proof_files, size_t index_base, uint32_t *proof_status);

struct RppTranscript;
// proveBPM of the setup's flavour behind the range-proof phases, device-resident (csrc/rpprove_dev.hip)
int rpp_argument_stream(bppp_rp *rp, RppTranscript &tr, size_t first_call, size_t B, const uint32_t *a_s, const uint32_t *a_q, const uint32_t *a_nx, const uint32_t *a_lc,
                        const uint32_t *a_lx, uint32_t *d_resp, uint64_t *resp_out, uint64_t *wn_out, uint64_t *wl_out, const uint32_t *d_extra, size_t extra_points,
                        std::vector<uint64_t> &extra_out, RppDevResults *dev = nullptr, uint32_t *buf_wn = nullptr, uint32_t *buf_wl = nullptr);
// verifyBRPM's public scalars for a batch (k_brp_public, csrc/rp.hip): the binary prover reuses them as the TR prover reuses k_trrp_public
// d_net: NULL (the setup's net_public) or [batch] canonical values, one per proof
int brp_public_device(bppp_rp *rp, size_t batch, const uint32_t *ch, uint32_t *q, uint32_t *sp, uint32_t *pub_norm, uint32_t *pub_lin_c, uint32_t *init_sc,
                      const uint32_t *d_net);

// provided by rpprove.hip
int rpp_ensure_pwork(bppp_rp *rp, size_t bytes);
int rpp_commit_rows(bppp_rp *rp, const uint32_t *d_rows, size_t nrows, uint64_t *host_out);              // synchronises the stream
int nlb_create_impl(bppp_ctx *ctx, size_t batch, const uint64_t *s, const uint64_t *g_xy, const uint64_t *q, const uint64_t *norm_x, const uint64_t *norm_g_xy,
                    size_t nlen, const uint64_t *lin_c, const uint64_t *lin_x, const uint64_t *lin_h_xy, size_t llen, bppp_nlb **out, bool on_device,
                    const struct CombTable *comb);

void rpp_host_oracle(const std::string &tag, std::vector<std::string> &groups, size_t &npoints, const uint64_t *pts, size_t m, int count, uint64_t *out);   // csrc/rpprove.hip
bool nlb_fixed_basis(const bppp_nlb *o);
int nlb_round_commit_dev(bppp_nlb *o, uint32_t *d_XR);
int nlb_round_collapse_dev(bppp_nlb *o, const uint32_t *d_es);
int nlb_witness_dev(bppp_nlb *o, size_t fn, size_t fl, uint32_t *d_wn, uint32_t *d_wl);     // the final witness, canonical, into HBM; asynchronous

}  // namespace bppp

extern "C" {
void bppp_nlb_destroy(bppp_nlb *nlb);
int bppp_nlb_round_commit(bppp_nlb *nlb, uint64_t *sX, uint64_t *X_xy, uint64_t *sR, uint64_t *R_xy);
int bppp_nlb_round_collapse(bppp_nlb *nlb, const uint64_t *es);
int bppp_nlb_get_witness(bppp_nlb *nlb, uint64_t *norm_w, uint64_t *lin_w, uint64_t *s);
}
