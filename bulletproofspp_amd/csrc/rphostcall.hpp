// rphostcall.hpp — the host-buffer variants of the balance calls (csrc/rpcommit.hip, rptally.hip, rpexcess.hip, rpexkeys.hip): upload, the
// _device variant, download.  Host code only.
#pragma once
#include <string.h>
#include <string>
#include "rp_internal.hpp"

namespace bppp {

// one argument of a host call in HBM, freed with the scope
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) hipFree(p); }
  int up(bppp_ctx *ctx, const void *src, size_t bytes) {
    if (!src) return BPPP_OK;                  // a NULL argument stays NULL: the _device variant judges it
    BPPP_HIP(ctx, hipMalloc(&p, bytes ? bytes : 16));
    if (bytes) BPPP_HIP(ctx, hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    return BPPP_OK;
  }
  int out(bppp_ctx *ctx, const void *want, size_t bytes) {
    if (want) BPPP_HIP(ctx, hipMalloc(&p, bytes ? bytes : 16));
    return BPPP_OK;
  }
};

// the sizes a host variant multiplies before the _device variant has judged them: where this is false nothing is uploaded, and the _device
// variant refuses the sizes before it reads anything
static constexpr size_t RPP_LIM31 = ((size_t)1 << 31) - 1;
inline bool rpp_sizes_ok(const bppp_rp *rp, size_t rows, size_t nsums, size_t nnz, size_t nkeys = 0) {
  const size_t nr = rp->D.nr;
  return nr && rows <= RPP_LIM31 / nr && nsums <= RPP_LIM31 && nnz <= RPP_LIM31 && nkeys <= RPP_LIM31 && rows * nr + nkeys <= RPP_LIM31 && nnz + nkeys <= RPP_LIM31;
}

// the pool, the CSR arrays and up to three claim arrays (claim_bytes each) of a host call in HBM
struct HostCsr {
  DevBuf coms, start, entries, a, ty, e;
  int up(bppp_rp *rp, size_t rows, const void *h_coms, size_t coms_row_bytes, size_t nsums, const uint32_t *sum_start, const uint32_t *ent, size_t nnz,
         const uint64_t *ca, const uint64_t *cty, const uint64_t *ce, size_t claim_bytes) {
    bppp_ctx *ctx = rp->ctx;
    hipSetDevice(ctx->device);
    int rc = coms.up(ctx, h_coms, rows * coms_row_bytes);
    if (!rc) rc = start.up(ctx, sum_start, (nsums + 1) * 4);
    if (!rc) rc = entries.up(ctx, ent, nnz * 4);
    if (!rc) rc = a.up(ctx, ca, claim_bytes);
    if (!rc) rc = ty.up(ctx, cty, claim_bytes);
    if (!rc) rc = e.up(ctx, ce, claim_bytes);
    return rc;
  }
};

// the end of a host builder, rc being what its _device variant returned: a refusal without a status array is the call's error, but the output is
// complete (refused rows zeroed), so it goes down either way and the error stands.  A refusal is BPPP_ERR_ARG with the output in HBM (src) and,
// where who_prefix is given, an error text that begins with it ("<who>: sum "); NULL: the caller made every other argument check before it uploaded.
inline int rpp_download_refused(bppp_ctx *ctx, int rc, const char *who_prefix, void *dst, const void *src, size_t bytes) {
  if (rc && !(rc == BPPP_ERR_ARG && src && (!who_prefix || ctx->err.compare(0, strlen(who_prefix), who_prefix) == 0))) return rc;
  const std::string err = rc ? ctx->err : std::string();
  BPPP_HIP(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return rc ? fail(ctx, rc, err) : BPPP_OK;
}

}  // namespace bppp
