// rpbind.hip — per-proof transcript bindings of the bppp_rp_*_bound* entry points (include/bppp.h).
//
// The reference's oracle hashes  tag <> show n <> show (length ps) <> text  (shaOracle, app/Main.hs:75-80; ZKPT.oracle, src/ZKP.hs:96-101) with
// one tag per run.  A bound call gives every proof a tag of its own,  oracle_tag <> binding_b[32]:  the header of an oracle output is then no
// longer the same for every proof of a batch.
//   k_rp_bound_headers   one lane per header word: the 16 big-endian words of  tag <> binding <> show n <> show (length ps)  for every (oracle
//                        output, proof), composed from the unbound header table the hash kernels already read (HashPlan of csrc/rp.hip, RppHdrs
//                        of csrc/rpp_transcript.hip) and the bindings in HBM.  64 bytes written per hash: 3.9 MB at 4096 proofs x 15 hashes.
//   rp_bind_*            the bindings of the call in flight, kept on the handle: fetched to the host for the host oracles, to HBM for the kernel
// The hash kernels' bound forms (k_rp_hash_bound, k_rpp_hash_bound) read a header per lane where the unbound ones read one per oracle output.
#include <string.h>
#include "rp_internal.hpp"

namespace bppp {

__global__ void __launch_bounds__(256) k_rp_bound_headers(const uint32_t *__restrict__ table, RpHdrLayout L, uint32_t nh, uint32_t slots, uint32_t taglen,
                                                         const uint8_t *__restrict__ bindings, const uint32_t *__restrict__ sel, uint32_t *__restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (uint64_t)nh * slots * 16) return;
  const uint32_t w = (uint32_t)(g & 15u);
  const uint64_t is = g >> 4;
  const uint32_t i = (uint32_t)(is / slots), s = (uint32_t)(is % slots);
  const uint32_t *grp = table + (size_t)(i / L.per) * L.group;
  const uint32_t *hdr = grp + (i % L.per) * 16;
  const uint32_t hlen = grp[L.hlen + i % L.per];              // of the unbound header: tag <> digits (0: an output this call does not have)
  const uint8_t *bd = bindings + RP_BINDING_BYTES * (size_t)(sel ? sel[s] : s);
  auto hbyte = [&](uint32_t p) { return (hdr[(p >> 2) & 15u] >> (24 - 8 * (p & 3u))) & 0xFFu; };
  uint32_t v = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t p = 4 * w + j;
    uint32_t byte = 0;
    if (hlen >= taglen && hlen + RP_BINDING_BYTES <= (uint32_t)RP_HDR_MAX) {
      if (p < taglen) byte = hbyte(p);
      else if (p < taglen + RP_BINDING_BYTES) byte = bd[p - taglen];
      else if (p < hlen + RP_BINDING_BYTES) byte = hbyte(p - (uint32_t)RP_BINDING_BYTES);
    }
    v = (v << 8) | byte;
  }
  out[g] = v;                                                 // g = (i * slots + s) * 16 + w
}

int rp_bind_begin(bppp_rp *rp, const void *bindings, bool device, size_t batch, const char *who) {
  rp->bind = RpBind();
  if (!bindings) return BPPP_OK;
  if (rp->hdr_max + RP_BINDING_BYTES > (size_t)RP_HDR_MAX)
    return fail(rp->ctx, BPPP_ERR_ARG, std::string(who) + ": oracle tag too long for per-proof bindings (tag + 32 binding bytes + digits exceed " +
                                           std::to_string(RP_HDR_MAX) + " bytes: the tag may have " + std::to_string(RP_HDR_MAX - RP_BINDING_BYTES - (rp->hdr_max - rp->tag.size())) +
                                           " bytes on this setup)");
  if (device) rp->bind.d = (const uint8_t *)bindings; else rp->bind.h = (const uint8_t *)bindings;
  rp->bind.n = batch;
  return BPPP_OK;
}

int rp_bind_host(bppp_rp *rp) {
  RpBind &b = rp->bind;
  if (!b.on() || b.h) return BPPP_OK;
  bppp_ctx *ctx = rp->ctx;
  hipSetDevice(ctx->device);
  rp->bind_hbuf.resize(b.n * RP_BINDING_BYTES);
  BPPP_HIP(ctx, hipMemcpyAsync(rp->bind_hbuf.data(), b.d, b.n * RP_BINDING_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  b.h = rp->bind_hbuf.data();
  return BPPP_OK;
}

int rp_bind_device(bppp_rp *rp) {
  RpBind &b = rp->bind;
  if (!b.on() || b.d) return BPPP_OK;
  bppp_ctx *ctx = rp->ctx;
  hipSetDevice(ctx->device);
  const size_t bytes = b.n * RP_BINDING_BYTES;
  if (bytes > rp->d_bind_bytes) {
    BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rp->d_bind) BPPP_HIP(ctx, hipFree(rp->d_bind));
    rp->d_bind = nullptr; rp->d_bind_bytes = 0;
    BPPP_HIP(ctx, hipMalloc(&rp->d_bind, bytes + bytes / 8));
    rp->d_bind_bytes = bytes + bytes / 8;
  }
  BPPP_HIP(ctx, hipMemcpyAsync(rp->d_bind, b.h, bytes, hipMemcpyHostToDevice, ctx->stream));
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));           // the source is the caller's (or a buffer of the entry point's)
  b.d = rp->d_bind;
  return BPPP_OK;
}

std::string rp_tag_at(const bppp_rp *rp, size_t s) {
  const RpBind &b = rp->bind;
  if (!b.h) return rp->tag;
  const size_t proof = b.sel_h ? b.sel_h[s] : s;
  return rp->tag + std::string((const char *)b.h + RP_BINDING_BYTES * proof, RP_BINDING_BYTES);
}

int rp_bound_headers(bppp_rp *rp, size_t slots, const uint32_t *d_table, RpHdrLayout L, size_t nh, const uint32_t **out) {
  bppp_ctx *ctx = rp->ctx;
  { int rc = rp_bind_device(rp); if (rc) return rc; }
  const RpBind &b = rp->bind;
  if (!b.d || (b.sel_h && !b.sel_d)) return fail(ctx, BPPP_ERR_ARG, "rp bound call: no bindings in HBM");
  const size_t bytes = nh * slots * 64;
  if (bytes > rp->d_bhdr_bytes) {
    BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rp->d_bhdr) BPPP_HIP(ctx, hipFree(rp->d_bhdr));
    rp->d_bhdr = nullptr; rp->d_bhdr_bytes = 0;
    BPPP_HIP(ctx, hipMalloc(&rp->d_bhdr, bytes + bytes / 8));
    rp->d_bhdr_bytes = bytes + bytes / 8;
  }
  const uint64_t n = (uint64_t)nh * slots * 16;
  k_rp_bound_headers<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(d_table, L, (uint32_t)nh, (uint32_t)slots, (uint32_t)rp->tag.size(), b.d, b.sel_d, rp->d_bhdr);
  BPPP_HIP(ctx, hipGetLastError());
  *out = rp->d_bhdr;
  return BPPP_OK;
}

}  // namespace bppp
