// rpwitness.hip — one half-batch of bppp_rp_prove_batch_device on a route with a device stream: the witness kernel on the caller's HBM buffers,
// the status words read back (batch x 4 bytes; a refused proof fails the call before anything else is queued), the provers' stream of kernels
// (rpp_prove_body / brp_prove_body, the same body the host entry points run behind their uploads) and the encoding kernel into the caller's
// file buffers.  The kernels: csrc/rpwitness.hip.h.
// bppp_rp_prove_batch_status_device (proof_status given) keeps going after a refusal: the status words are the answer, and when some are not zero the
// accepted proofs alone are proved, in compact order — the index lists go up (batch x 4 bytes), the workspace is carved again for the G accepted proofs,
// the witness kernel runs once more through src_index, one kernel gathers the prefixes and the public words, the provers' stream runs unchanged on G
// proofs, the encoding kernel writes through dst_index and one kernel zeroes the files of the refused.  A batch without a refusal queues exactly what
// bppp_rp_prove_batch_device queues.
#include <string>
#include <vector>
#include "rpwitness.hip.h"
#include "rpprove_dev.hpp"

namespace bppp {

int rp_prove_device_half(bppp_rp *rp, size_t B, const void *d_amounts, const void *d_types, const void *d_blinds, const uint64_t *pub, const uint8_t *d_prefix,
                         size_t prefix_len, uint8_t *d_coms_files, uint8_t *d_proof_files, size_t index_base, uint32_t *proof_status) {
  bppp_ctx *ctx = rp->ctx;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const bppp_rps::Setup &S = rp->st;
  const bool binary = S.kind == 1;
  const size_t nr = S.rds.size();
  if (!binary && nr >= (1u << 16)) return fail(ctx, BPPP_ERR_ARG, "rp_prove_batch: too many ranges");
  LapTimer timer(rp->opt.timing, binary ? "[rp_prove binary]" : "[rp_prove]");
  RppWork W;
  { int rc = binary ? brp_carve(rp, B, prefix_len, false, W) : rpp_carve(rp, B, prefix_len, false, W); if (rc) return rc; }
  W.prefix = d_prefix;
  const uint32_t *d_pub = nullptr;
  if (pub) { int rc = rp_upload_public(rp, pub, B * rp_public_count(rp) * 4, &d_pub); if (rc) return rc; }
  { int rc = wit_launch(rp, B, d_amounts, d_types, d_blinds, d_pub, W.in_sc, W.dig, W.mul, W.mss, W.bits, W.status); if (rc) return rc; }
  std::vector<uint32_t> status(B);
  BPPP_HIP(ctx, hipMemcpyAsync(status.data(), W.status, B * 4, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  size_t refused = 0;
  for (size_t b = 0; b < B; b++) {
    if (status[b] == WIT_OK) continue;
    if (!proof_status) return fail(ctx, BPPP_ERR_ARG, "rp_prove_batch: proof " + std::to_string(index_base + b) + ": " + wit_status_text(status[b]));
    refused++;
  }
  if (proof_status) memcpy(proof_status, status.data(), B * 4);
  timer.lap("witness (device)");
  const size_t all = B;
  const uint32_t *d_accepted = nullptr;        // NULL (slot b is proof b) or the proofs of the B slots proved below
  std::vector<uint32_t> sel;                   // the accepted proofs, then the refused ones
  // a bound call: the bindings stay where they are, [all][32] in the caller's order; the oracles reach them through the index lists from here on
  struct SelGuard { bppp_rp *rp; ~SelGuard() { rp->bind.sel_h = rp->bind.sel_d = nullptr; } } sel_guard{rp};
  if (refused) {
    B = all - refused;
    for (size_t b = 0; b < all; b++) if (status[b] == WIT_OK) sel.push_back((uint32_t)b);
    for (size_t b = 0; b < all; b++) if (status[b] != WIT_OK) sel.push_back((uint32_t)b);
    const size_t pub_words = d_pub ? rp_public_count(rp) * 8 : 0, lists = (all + 63) & ~(size_t)63, need = (lists + B * pub_words) * 4;
    if (need > rp->d_sel_bytes) {
      if (rp->d_sel) BPPP_HIP(ctx, hipFree(rp->d_sel));
      rp->d_sel = nullptr; rp->d_sel_bytes = 0;
      BPPP_HIP(ctx, hipMalloc(&rp->d_sel, need + need / 8));
      rp->d_sel_bytes = need + need / 8;
    }
    BPPP_HIP(ctx, hipMemcpyAsync(rp->d_sel, sel.data(), all * 4, hipMemcpyHostToDevice, st));
    k_rp_zero_files<<<dim3((unsigned)refused), dim3(256), 0, st>>>(rp->d_sel + B, rp->D.coms_bytes, rp->D.proof_bytes, d_coms_files, d_proof_files);
    BPPP_HIP(ctx, hipGetLastError());
    if (!B) { BPPP_HIP(ctx, hipStreamSynchronize(st)); timer.lap("refused files (device)"); return BPPP_OK; }
    d_accepted = rp->d_sel;
    if (rp->bind.on()) { rp->bind.sel_h = sel.data(); rp->bind.sel_d = d_accepted; }
    { int rc = binary ? brp_carve(rp, B, prefix_len, true, W) : rpp_carve(rp, B, prefix_len, true, W); if (rc) return rc; }
    { int rc = wit_launch(rp, B, d_amounts, d_types, d_blinds, d_pub, W.in_sc, W.dig, W.mul, W.mss, W.bits, W.status, d_accepted); if (rc) return rc; }
    uint32_t *d_pub_own = rp->d_sel + lists;
    k_rp_gather_accepted<<<dim3((unsigned)B), dim3(256), 0, st>>>(d_accepted, d_prefix, (uint32_t)prefix_len, d_pub, (uint32_t)pub_words, W.prefix_own, d_pub_own);
    BPPP_HIP(ctx, hipGetLastError());
    if (d_pub) d_pub = d_pub_own;
    timer.lap("accepted proofs compacted");
  }
  RppDevResults R{};
  { int rc = binary ? brp_prove_body(rp, B, W, prefix_len, d_pub, nullptr, &R) : rpp_prove_body(rp, B, W, prefix_len, d_pub, nullptr, &R); if (rc) return rc; }
  timer.lap("phases + argument (device)");
  EncDims E{};
  E.nr = (uint32_t)nr; E.k = (uint32_t)S.rounds; E.fn = (uint32_t)S.fn; E.fl = (uint32_t)S.fl; E.coms_bytes = rp->D.coms_bytes; E.proof_bytes = rp->D.proof_bytes;
  E.batch = (uint32_t)B;
  const uint32_t Bw = (uint32_t)B;
  if (binary) {                     // blCom dCom (rpp_encode_files' lead of prove_batch_binary_dev)
    E.nlead = 2;
    E.lead_off[0] = Bw; E.lead_stride[0] = 1; E.lead_off[1] = 0; E.lead_stride[1] = 1;
  } else {                          // blCom rCom dmCom mCom (prove_batch_one)
    E.nlead = 4;
    E.lead_off[0] = 3 * Bw; E.lead_stride[0] = 1; E.lead_off[1] = 2 * Bw; E.lead_stride[1] = 1; E.lead_off[2] = 0; E.lead_stride[2] = 2; E.lead_off[3] = 1; E.lead_stride[3] = 2;
  }
  k_rp_encode_files<<<dim3((unsigned)B), dim3(256), 0, st>>>(E, R.input_coms, R.coms, R.resp, R.wit_norm, R.wit_lin, d_coms_files, d_proof_files, d_accepted);
  BPPP_HIP(ctx, hipGetLastError());
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  timer.lap("encode (device)");
  return BPPP_OK;
}

}  // namespace bppp
