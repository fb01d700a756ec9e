// rpsealhash.hip.h — the messages of a seal (include/bppp.h, sealed outputs) as the device hashes them: shared by the seal and the one-key scan
// (csrc/rpseal.hip) and by the many-key scan (csrc/rpscan_keys.hip).
#pragma once
#include "rpexcess_shared.hip.h"

namespace bppp {

static constexpr uint32_t SEAL_HEAD = 34, SEAL_MEMO = 64;
static constexpr uint32_t SCAN_OPEN = 0xFFFFFFFFu;      // a verdict still open
struct SealDomains { ExDomain ds, dt, db, dm; };

// ss = SHA-256 (Ds || put (P.x) || sign (P) || the 33 bytes of R as stored), as eight big-endian words; P: an affine point in memory
template <class F> BPPP_DI void seal_shared(const ExDomain &ds, const uint32_t *P, F rbyte, uint32_t ss[8]) {
  ex_digest<2>(98u, [&](uint32_t k) -> uint32_t { return k < 32 ? ex_dom_byte(ds, k) : k < 65 ? ex_pt_byte(P, k - 32) : rbyte(k - 65); }, ss);
}
BPPP_DI uint32_t seal_view_tag(const ExDomain &dt, const uint32_t ss[8]) {
  uint32_t st[8];
  ex_digest<2>(64u, [&](uint32_t k) -> uint32_t { return k < 32 ? ex_dom_byte(dt, k) : ex_word_byte(ss, k - 32); }, st);
  return st[0] >> 24;
}
// byte k of  D || ss || le32 (i) [|| half]
BPPP_DI uint32_t seal_range_byte(const ExDomain &d, const uint32_t ss[8], uint32_t i, uint32_t half, uint32_t k) {
  return k < 32 ? ex_dom_byte(d, k) : k < 64 ? ex_word_byte(ss, k - 32) : k < 68 ? (i >> (8 * (k - 64))) & 0xFFu : half;
}
BPPP_DI fe seal_blind(const ExDomain &db, const uint32_t ss[8], uint32_t i) {
  uint32_t st[8];
  ex_digest<2>(68u, [&](uint32_t k) -> uint32_t { return seal_range_byte(db, ss, i, 0, k); }, st);
  return ex_digest_scalar(st);
}
// pad_i as sixteen big-endian words
BPPP_DI void seal_pad(const ExDomain &dm, const uint32_t ss[8], uint32_t i, uint32_t pad[16]) {
  for (uint32_t h = 0; h < 2; h++) ex_digest<2>(69u, [&](uint32_t k) -> uint32_t { return seal_range_byte(dm, ss, i, h, k); }, pad + 8 * h);
}

// what csrc/rpseal.hip lends the many-key scan: the four domains of a handle, and the launch of k_rp_scan_lift (the hints of n seals lifted into
// R [n][16]; status [n]: BPPP_RP_SCAN_BAD_HINT or SCAN_OPEN) on the context's stream
SealDomains seal_domains(const bppp_rp *rp);
void scan_lift_launch(bppp_rp *rp, uint32_t n, const uint8_t *d_seals, uint32_t *R, uint32_t *status);

}  // namespace bppp
