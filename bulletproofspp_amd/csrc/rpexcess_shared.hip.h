// rpexcess_shared.hip.h — what the excess files share: the derived-key path (csrc/rpexcess.hip: the key X_t comes out of the pool), the
// stated-key path (csrc/rpexkeys.hip: the key is 33 bytes next to the signature) and the multi-party signer (csrc/rpexpart.hip: builders
// who each know a part of the blinding sum).  The domains, the three-block hash, the challenge and the lift of 33 bytes are one definition,
// so that the 65 bytes bppp_rp_excess_sign or bppp_rp_excess_part_combine writes verify on either path; the kernels both verifying paths
// run stay in csrc/rpexcess.hip and are reached through the launches declared at the end.
#pragma once
#include <string.h>
#include <string>
#include "ec.hip.h"
#include "rp_internal.hpp"
#include "rpprove_host.hpp"
#include "rpwords.hip.h"
#include "rplift.hip.h"
#include "sha256.hip.h"

namespace bppp {

static constexpr uint32_t EX_SIG = BPPP_RP_EXCESS_SIG_BYTES, EX_MSG = 32, EX_KEY = BPPP_RP_EXCESS_KEY_BYTES;
static constexpr uint32_t EX_EVAL = 0xFFFFFFFFu;       // a verdict still open: the equation decides
struct ExDomain { uint32_t w[8]; };                    // a domain digest as the eight big-endian words it is hashed as

BPPP_DI uint32_t ex_dom_byte(const ExDomain &d, uint32_t k) { return (d.w[k >> 2] >> (24 - 8 * (k & 3))) & 0xFFu; }
// byte o (< 33) of an affine point as a signature, a key and the messages hold it: put (x), then the sign byte (y > p - y)
BPPP_DI uint32_t ex_pt_byte(const uint32_t *pt, uint32_t o) { return o < 32 ? enc_be_byte(pt, o) : enc_sign(pt); }
// the 33 bytes of a key, or of any point held as a signature holds R -> the lifted point; false (and the infinity encoding) for a sign byte
// above 1 or an x without a curve point
BPPP_DI bool exk_lift(const uint8_t *key, aff &X) {
  const uint32_t sign = key[32];
  bool ok;
  X = rp_lift_x(load_field_be<0>(key), sign == 1, ok);
  if (sign > 1 || !ok) { X = aff_inf(); return false; }
  return true;
}
// decode (SHA-256 (message)) mod n of a message of 120 .. 183 bytes (three blocks), byte k of it being at (k)
template <class F> BPPP_DI fe ex_hash3(uint32_t nbytes, F at) {
  uint32_t st[8], w[16];
  sha256_init(st);
#pragma unroll
  for (uint32_t blk = 0; blk < 3; blk++) {
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) {
      uint32_t word = 0;
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) {
        const uint32_t k = 64 * blk + 4 * q + r;
        word = (word << 8) | (k < nbytes ? (at(k) & 0xFFu) : k == nbytes ? 0x80u : 0u);
      }
      w[q] = word;
    }
    if (blk == 2) w[15] = nbytes * 8;
    sha256_compress(st, w);
  }
  fe r; sha256_digest_to_limbs(st, r.v);
  return wi_umod_n(r);
}
// its sibling for the half-aggregate's hash tree (csrc/rpexagg.hip): the RAW digest, as eight big-endian words, of a message of NB blocks
// (64 NB - 72 <= nbytes <= 64 NB - 9: two blocks hold 56 .. 119 bytes, three 120 .. 183), byte k of it being at (k)
template <uint32_t NB, class F> BPPP_DI void ex_digest(uint32_t nbytes, F at, uint32_t st[8]) {
  uint32_t w[16];
  sha256_init(st);
#pragma unroll
  for (uint32_t blk = 0; blk < NB; blk++) {
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) {
      uint32_t word = 0;
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) {
        const uint32_t k = 64 * blk + 4 * q + r;
        word = (word << 8) | (k < nbytes ? (at(k) & 0xFFu) : k == nbytes ? 0x80u : 0u);
      }
      w[q] = word;
    }
    if (blk == NB - 1) w[15] = nbytes * 8;
    sha256_compress(st, w);
  }
}
// byte k of a digest held as big-endian words, and decode (digest) mod n
BPPP_DI uint32_t ex_word_byte(const uint32_t *w, uint32_t k) { return (w[k >> 2] >> (24 - 8 * (k & 3))) & 0xFFu; }
BPPP_DI fe ex_digest_scalar(const uint32_t st[8]) { fe r; sha256_digest_to_limbs(st, r.v); return wi_umod_n(r); }
// c = decode (SHA-256 (Dc || the 33 bytes of R || put (X.x) || sign (X) || msg)) mod n: 130 bytes; rbyte (o): byte o of R as the signature holds it
template <class F> BPPP_DI fe ex_challenge(const ExDomain &dc, F rbyte, const uint32_t *X, const uint8_t *msg) {
  return ex_hash3(32 + 33 + 33 + EX_MSG, [&](uint32_t k) -> uint32_t {
    if (k < 32) return ex_dom_byte(dc, k);
    if (k < 65) return rbyte(k - 32);
    if (k < 98) return ex_pt_byte(X, k - 65);
    return msg[k - 98];
  });
}

namespace excess {

// SHA-256 (label || tag), once per call on the host
inline ExDomain domain(const char *label, const std::string &tag) {
  Sha256 h;
  h.update(label, strlen(label));
  h.update(tag.data(), tag.size());
  ExDomain d;
  h.finish(d.w);
  return d;
}
inline ExDomain challenge_domain(const bppp_rp *rp) { return domain("bppp/excess/challenge/v1", rp->tag); }
inline ExDomain nonce_domain(const bppp_rp *rp) { return domain("bppp/excess/nonce/v1", rp->tag); }
inline uint32_t blind_slot(const bppp_rp *rp) { return rp->st.kind == 1 ? 1u : 2u; }     // B among [g | H0 | H1]: h0 of a binary handle, else H1

// the kernels of csrc/rpexcess.hip that serve the stated keys as they are, queued on the context's stream with the grids its own calls give them:
// k_rp_excess_sigs (s canonical, R lifted), k_rp_excess_mulcheck (the equation, one quad a signature) and, inside batch_chunk, k_rp_excess_weights
int sigs_launch(bppp_ctx *ctx, size_t n, uint32_t slot, const uint8_t *sigs, uint32_t *in_sc, uint32_t *R, uint32_t *bits);
int mulcheck_launch(bppp_ctx *ctx, size_t n, const uint32_t *c, const uint32_t *X, const uint32_t *P, const uint32_t *R, const uint32_t *pre, uint32_t *status);
// one pass of a signature batch over n signatures at job positions j0 ..: the weights and the two MSM terms of each (k_rp_excess_weights; X the keys, sp
// the scalars of s B, as the stage before left them), sum rho s on B as term 2n, and the MSM into parts.  prods [n][24], red [RPP_REDUCE_BLOCKS * 24],
// sc3 [24], msm_sc [2n + 1][8], msm_pt [2n + 1][16] are workspace; any[0] is raised by a signature whose verdict is already taken
int batch_chunk(bppp_rp *rp, size_t n, uint64_t j0, const uint8_t *seed, const uint8_t *sigs, const uint32_t *X, const uint8_t *msgs, const uint32_t *pre, const uint32_t *c,
                const uint32_t *sp, const uint32_t *R, uint32_t *prods, uint32_t *red, uint32_t *sc3, uint32_t *msm_sc, uint32_t *msm_pt, uint32_t *any, BatchParts &parts);

// ... and its assembly alone: everything of batch_chunk but term 2n and the MSM, for a caller that runs the MSM itself (csrc/rpblock.hip)
int batch_assemble(bppp_rp *rp, size_t n, uint64_t j0, const uint8_t *seed, const uint8_t *sigs, const uint32_t *X, const uint8_t *msgs, const uint32_t *pre, const uint32_t *c,
                   const uint32_t *sp, const uint32_t *R, uint32_t *prods, uint32_t *red, uint32_t *sc3, uint32_t *msm_sc, uint32_t *msm_pt, uint32_t *any);

}  // namespace excess

// ---- what the stated keys (csrc/rpexkeys.hip, which defines it) lend to the block call (csrc/rpblock.hip): the jobs after their checks, the stage
// of a signature up to the verdict that needs no equation, and the two exact passes that name the culprits of a rejected job
namespace exkeys {
struct KeyJob { bppp_rp *rp; size_t nkeys; const uint8_t *keys, *msgs, *sigs; };
struct KeyWork { uint32_t *sp, *P, *R, *X, *bits, *pre, *c, *status, *any, *prods, *red, *sc3, *msm_sc, *msm_pt; uint8_t *seed; };
struct SumsJob {
  tally::Job J;                                 // after sums_checks: h_start and nnz merged, tail = nkeys; start and entries the caller's
  size_t nkeys = 0, nnz = 0;                    // nnz: the caller's
  const uint8_t *keys = nullptr; const uint32_t *key_start = nullptr;
};
// keys per pass over the workspace: a quarter of the flat chunk
inline size_t keys_chunk(const bppp_rp *rp, size_t n) { return std::min(n, std::max<size_t>(1, rpp_flat_chunk(rp) / 4)); }
int key_checks(KeyJob &K, bppp_rp *rp, const char *who, size_t nkeys, const void *keys, const void *msgs, const void *sigs, bool null_args);
// keys [o, o + n) up to the verdict that needs no equation: W.X the lifted keys, W.R, W.c, W.pre and W.sp, the scalars of s B
int key_stage(const KeyJob &K, const KeyWork &W, size_t o, size_t n, const ExDomain &dc);
int verify_keys_each_pass(const KeyJob &K, uint32_t *status);
int sums_checks(SumsJob &S, bppp_rp *rp, const char *who, size_t rows, const void *coms, size_t nsums, const void *start, const void *entries, size_t nnz, const void *amt,
                const void *ty, const void *off, size_t nkeys, const void *key_start, const void *keys, bool null_args);
tally::Ext sums_ext(const SumsJob &S);
}  // namespace exkeys
}  // namespace bppp
