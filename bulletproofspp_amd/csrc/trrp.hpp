// trrp.hpp — the static structure of a typed-reciprocal setup as it sits on the device (uploaded by bppp_trrp_create): shared by the
// verifier's public-scalar kernel (csrc/trrp.hip) and the prover's phase kernels (csrc/rpprove_dev.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ctx.hpp"

namespace bppp {
struct TrrpDims { uint32_t nlen, llen, nr, nsyms, npub, has_types, flavour; };
// position kinds (Phase1 constructors, src/RangeProof/TypedReciprocal.hs:56-60)
static constexpr uint32_t K_TYPING = 0, K_INLINE = 1, F_IO = 1u << 8, F_IA = 1u << 9, NO_SYM = 0xFFFFFFFFu;
static constexpr int TRRP_MAX_SLOTS = 16;      // distinct digit bases of one setup (base map x^3, x^5, ...)
static constexpr size_t TRRP_MAX_SYMS = 1022;  // distinct reciprocal symbols of one setup: the digits 1 .. b - 1 of its bases and its public types
static constexpr size_t TRRP_MAX_RANGES = 65535;   // ranges of one setup: every prover route indexes them below 2^16 (csrc/rpprove.hip, csrc/rpwitness.hip)
// dynamic LDS of one workgroup: what a launch gets without asking, and the most hipFuncSetAttribute grants on gfx950
static constexpr size_t LDS_DEFAULT_BYTES = 64 * 1024, LDS_MAX_BYTES = 160 * 1024;

// k_trrp_public<G>'s dynamic LDS for one proof of G lanes, in fr26 words of ten (csrc/trrp.hip: inv [2 + nsyms], two scan rows [G], x2 [nr],
// three slot tables), and for the workgroup of 64 / G proofs
inline size_t trrp_public_lds_words(size_t nsyms, size_t nr, int G) { return (2 + nsyms + 2 * (size_t)G + nr + 3 * (size_t)TRRP_MAX_SLOTS) * 10; }
inline size_t trrp_public_lds_bytes(size_t nsyms, size_t nr, int G) { return trrp_public_lds_words(nsyms, nr, G) * 4 * (size_t)(64 / G); }
// how bppp_trrp_public_device runs a batch.  split: k_trrp_pre / k_trrp_pos / k_trrp_lin, whose per-proof record lies in HBM — batches that fill
// the chip (> 1024 proofs), and every batch of a setup whose one-kernel LDS does not fit a workgroup.  Otherwise k_trrp_public<G>: 32 lanes per
// proof (two proofs per wavefront) unless the LDS of a wavefront's proofs passes 64 KiB; a batch that cannot give every SIMD a wavefront anyway
// (<= 1024 proofs) takes a whole wavefront per proof.  forced_g / force_split: the BPPP_TRRP_G / BPPP_TRRP_SPLIT overrides (0 / -1: none)
struct TrrpPublicPlan { bool split; int G; size_t words_per_proof, lds; };
inline TrrpPublicPlan trrp_public_plan(size_t nsyms, size_t nr, size_t batch, int forced_g = 0, int force_split = -1) {
  TrrpPublicPlan p;
  p.G = forced_g ? forced_g : (batch <= 1024 ? 64 : 32);
  while (p.G < 64 && trrp_public_lds_bytes(nsyms, nr, p.G) > LDS_DEFAULT_BYTES) p.G <<= 1;
  p.words_per_proof = trrp_public_lds_words(nsyms, nr, p.G);
  p.lds = trrp_public_lds_bytes(nsyms, nr, p.G);
  p.split = (force_split >= 0 ? force_split != 0 : batch > 1024) || p.lds > LDS_MAX_BYTES;
  return p;
}
}  // namespace bppp

struct bppp_trrp {
  bppp_ctx *ctx;
  bppp::TrrpDims D;
  uint32_t *pos_kind, *pos_range, *pos_slot, *pos_sym, *pos_coeff, *range_min, *range_assumed, *syms, *cs_slot, *cs_sym, *pub_is_out, *pub_amount, *pub_sym;
  // what the last bppp_trrp_public_device / trrp_public_run on these tables launched (bppp_test_trrp_last_public): 0 nothing yet, 1 k_trrp_public
  // (last_lanes per proof, last_lds bytes of dynamic LDS), 2 the three kernels (lanes and LDS 0)
  int last_route, last_lanes;
  size_t last_lds;
};
namespace bppp {
// bppp_trrp_public_device with per-proof public amounts: d_pub_amounts NULL (the setup's) or [batch][npub] canonical scalars in HBM (csrc/trrp.hip)
int trrp_public_run(bppp_trrp *t, size_t batch, const void *d_challenges, void *d_q, void *d_sp, void *d_pub_norm, void *d_pub_lin_c, void *d_init_scalars,
                    const void *d_pub_amounts);
}  // namespace bppp
