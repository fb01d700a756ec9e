// rpexpart.hip — MULTI-PARTY excess signatures: builders who each know a part e_i of a transaction's blinding sum produce together the 65 bytes
// every verifier of include/bppp.h checks: bppp_rp_excess_part_nonces*, _part_aggregate*, _part_sign*, _part_verify*, _part_combine*.
// Two rounds, two nonces a party (as MuSig2), keys added plainly; include/bppp.h states every message.  With
//   b = decode (SHA-256 (Db || R1agg || R2agg || X || msg)) mod n,    R = R1agg + b R2agg,    c = the single signer's challenge over (R, X, msg):
//   s_i = k_1 + b k_2 + c e_i,     s_i B - b R2_i - c X_i = R1_i,     signature = R || sum s_i.
// Stages (csrc/rpexpart.hip.h holds the joint walk):
//   lift     k_rp_expart_lift       one lane per (part, column): R1_i, R2_i, X_i lifted into HBM; a failure marks the part and its group
//   group    k_rp_expart_sum        one QUAD per (sum, column): the group's affine points added serially (parties per transaction are few), then one
//                                   batch inversion for the affine aggregates; k_rp_expart_judge: the verdict of the sum
//   session  k_rp_expart_coef       one lane per sum: b;  k_rp_expart_session: one QUAD per sum, b R2agg by the walk of csrc/rpexcess.hip.h plus R1agg;
//                                   one batch inversion; k_rp_expart_challenge: R infinity, else c
// and around them, one lane per row unless said otherwise:
//   k_rp_expart_validate   part_start non-decreasing from 0 to nparts, before anything reads through it: the first offending position
//   k_rp_expart_nonce      the verdict on e_i and k_1, k_2; the scalar rows of R1 = k_1 B and R2 = k_2 B
//   k_rp_expart_pubnonce   the 66 bytes of (R1, R2)
//   k_rp_expart_encode     the aggregates as 66 + 33 bytes
//   k_rp_expart_signpre    the signer's verdict, then BAD_KEY / BAD_R of the aggregates it was handed
//   k_rp_expart_respond    s_i as 32 bytes
//   k_rp_expart_partials   s_i canonical, the verdict of a part that needs no equation, the scalar row of s_i B
//   k_rp_expart_mulcheck   one QUAD per part: b R2_i + c X_i by the joint walk, less s_i B, against - R1_i, cross-multiplied
//   k_rp_expart_combine    sum s_i mod n over the group and the 65 bytes
// Every kernel is bounds-checked on its own index, takes its loop bounds from validated arrays only, reads the byte rows bytewise and writes with
// ordinary vector stores.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ec.hip.h"
#include "rp_internal.hpp"
#include "rphostcall.hpp"
#include "rpprove_host.hpp"
#include "rpwords.hip.h"
#include "rplift.hip.h"
#include "rpexcess.hip.h"
#include "rpexpart.hip.h"
#include "rpexcess_shared.hip.h"
#include "sha256.hip.h"

namespace bppp {

static constexpr uint32_t EXP_NONCE = BPPP_RP_EXCESS_PUBNONCE_BYTES, EXP_PARTIAL = BPPP_RP_EXCESS_PARTIAL_BYTES;
static constexpr uint32_t EXP_NONE = 0xFFFFFFFFu;

// flag[0] = the lowest position whose part_start breaks "non-decreasing from 0 to nparts"; it starts as EXP_NONE.  The bounds are the caller's
// arguments, never device data.
__global__ void __launch_bounds__(256) k_rp_expart_validate(uint32_t nsums, uint32_t nparts, const uint32_t *__restrict__ part_start, uint32_t *__restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= nsums; i += (uint64_t)gridDim.x * 256) {
    const uint32_t s = part_start[i];
    if ((i == 0 && s != 0) || (i == nsums && s != nparts) || (i > 0 && s < part_start[i - 1])) atomicMin(flag, (uint32_t)i);
  }
}

// ---- round 1 and the signer's nonces.  k [2n][8]: k_1 of row t, then k_2 of row t at n + t, zero for a refused row; in_sc (may be NULL)
// [2n][3][8]: the scalars of R1_t = k_1 B at row t and of R2_t = k_2 B at row n + t on base `slot`
__global__ void __launch_bounds__(64) k_rp_expart_nonce(uint32_t n, uint32_t slot, ExDomain dm, const uint32_t *__restrict__ blinds, const uint8_t *__restrict__ msgs,
                                                        const uint8_t *__restrict__ aux, uint32_t *__restrict__ k, uint32_t *__restrict__ in_sc,
                                                        uint32_t *__restrict__ status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t *ew = blinds + (size_t)t * 8;
  const uint8_t *msg = msgs + (size_t)t * EX_MSG;
  const fe e = fe_load(ew);
  uint32_t st = !wi_canonical(e) ? (uint32_t)BPPP_RP_EXCESS_NOT_CANONICAL : fe_is_zero(e) ? (uint32_t)BPPP_RP_EXCESS_ZERO : (uint32_t)BPPP_RP_EXCESS_OK;
  fe kj[2] = {fe_zero(), fe_zero()};
  if (st == BPPP_RP_EXCESS_OK) {
#pragma unroll 1
    for (uint32_t j = 0; j < 2; j++) {
      const fe h = ex_hash3(32 + 32 + EX_MSG + 32 + 1, [&](uint32_t b) -> uint32_t {
        if (b < 32) return ex_dom_byte(dm, b);
        if (b < 64) return enc_be_byte(ew, b - 32);
        if (b < 96) return msg[b - 64];
        if (b < 128) return aux[b - 96];
        return j + 1;
      });
      if (j == 0) kj[0] = h; else kj[1] = h;
    }
    if (fe_is_zero(kj[0]) || fe_is_zero(kj[1])) st = BPPP_RP_EXCESS_NONCE;
  }
  const bool ok = st == BPPP_RP_EXCESS_OK;
  for (uint32_t j = 0; j < 2; j++) {
    const fe v = ok ? kj[j] : fe_zero();
    fe_store(k + ((size_t)j * n + t) * 8, v);
    if (in_sc) for (uint32_t b = 0; b < 3; b++) fe_store(in_sc + (((size_t)j * n + t) * 3 + b) * 8, b == slot ? v : fe_zero());
  }
  status[t] = st;
}
// pts [2n][16]: R1 then R2, as in_sc; out [n][66]: the 33 bytes of R1, then those of R2; zero bytes for a refused row
__global__ void __launch_bounds__(64) k_rp_expart_pubnonce(uint32_t n, const uint32_t *__restrict__ pts, const uint32_t *__restrict__ status, uint8_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const bool ok = status[t] == BPPP_RP_EXCESS_OK;
  uint8_t *row = out + (size_t)t * EXP_NONCE;
  for (uint32_t j = 0; j < 2; j++)
    for (uint32_t o = 0; o < 33; o++) row[33 * j + o] = ok ? (uint8_t)ex_pt_byte(pts + ((size_t)j * n + t) * 16, o) : (uint8_t)0;
}

// ---- the lift stage.  Lane col * np + p lifts column col (0: R1, 1: R2, 2: the key) of part p: pts [3][np][16], the infinity encoding where there is no
// point, and bad [3][np].  The part lies in the last sum t < ns with part_start[t] - p0 <= p (validated: at most 32 steps; part_start NULL: every part
// is a group of its own, t = p); the key's lane stores sumof[p] = t, and a failure raises keybad[t] or rbad[t].
__global__ void __launch_bounds__(64) k_rp_expart_lift(uint32_t np, uint32_t ns, uint32_t p0, const uint32_t *__restrict__ part_start, const uint8_t *__restrict__ pubnonces,
                                                       const uint8_t *__restrict__ keys, uint32_t *__restrict__ pts, uint32_t *__restrict__ bad,
                                                       uint32_t *__restrict__ sumof, uint32_t *__restrict__ keybad, uint32_t *__restrict__ rbad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)3 * np) return;
  const uint32_t col = (uint32_t)(i / np), p = (uint32_t)(i % np);
  aff P;
  const bool ok = exk_lift(col == 2 ? keys + (size_t)p * EX_KEY : pubnonces + (size_t)p * EXP_NONCE + 33 * col, P);
  aff_store(pts + ((size_t)col * np + p) * 16, P);
  bad[(size_t)col * np + p] = ok ? 0u : 1u;
  uint32_t lo = p;
  if (part_start) {
    uint32_t hi = ns - 1;
    lo = 0;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1) / 2;
      if (part_start[mid] - p0 <= p) lo = mid; else hi = mid - 1;
    }
  }
  if (col == 2) sumof[p] = lo;
  if (!ok) (col == 2 ? keybad : rbad)[lo] = 1u;            // every lane that stores here stores the same word
}
// ---- the group sum.  Lanes 4q .. 4q + 3 of the launch are (column, sum) q = col * ns + t: the affine points of the group, parts part_start[t] - p0
// up to part_start[t + 1] - p0 of the pass, added one after the other by the complete law (a point without a lift is the infinity encoding and adds
// nothing).  The loop bounds are the same in the four lanes.  Lane 0 stores agg [3][ns][XYZZ_WORDS] and zz [3][ns][8] = ZZ ZZZ, zero for infinity.
__global__ void __launch_bounds__(64) k_rp_expart_sum(uint32_t ns, uint32_t np, uint32_t p0, const uint32_t *__restrict__ part_start, const uint32_t *__restrict__ pts,
                                                      uint32_t *__restrict__ agg, uint32_t *__restrict__ zz) {
  const uint64_t q = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (q >= (uint64_t)3 * ns) return;
  const uint32_t col = (uint32_t)(q / ns), t = (uint32_t)(q % ns);
  const uint32_t lo = part_start[t] - p0, hi = min(part_start[t + 1] - p0, np);
  xyzz acc = xyzz_inf();
#pragma unroll 1
  for (uint32_t p = lo; p < hi; p++) xyzz_add_quad(acc, xyzz_from_aff(aff_load(pts + ((size_t)col * np + p) * 16)));
  if (quad_lane() != 0) return;
  xyzz_store(agg + q * XYZZ_WORDS, acc);
  fe_store(zz + q * 8, xyzz_is_inf(acc) ? fe_zero() : fq_to_fe(fq_mul(acc.ZZ, acc.ZZZ)));
}
// the first verdict of a sum that applies, in the header's order, over aggxy [3][ns][16] (all zeros: infinity)
__global__ void __launch_bounds__(256) k_rp_expart_judge(uint32_t ns, const uint32_t *__restrict__ keybad, const uint32_t *__restrict__ rbad,
                                                         const uint32_t *__restrict__ aggxy, uint32_t *__restrict__ status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ns) return;
  uint32_t any[3] = {0, 0, 0};
  for (uint32_t col = 0; col < 3; col++)
    for (int k = 0; k < 16; k++) any[col] |= aggxy[((size_t)col * ns + t) * 16 + k];
  status[t] = keybad[t]            ? (uint32_t)BPPP_RP_EXCESS_BAD_KEY
              : rbad[t]            ? (uint32_t)BPPP_RP_EXCESS_BAD_R
              : !any[2]            ? (uint32_t)BPPP_RP_EXCESS_NO_KEY
              : (!any[0] || !any[1]) ? (uint32_t)BPPP_RP_EXCESS_NONCE_INFINITY
                                   : (uint32_t)BPPP_RP_EXCESS_OK;
}
// nonces (may be NULL) [ns][66] and keys (may be NULL) [ns][33] of the aggregates; zero bytes for a refused sum
__global__ void __launch_bounds__(64) k_rp_expart_encode(uint32_t ns, const uint32_t *__restrict__ aggxy, const uint32_t *__restrict__ status, uint8_t *__restrict__ nonces,
                                                         uint8_t *__restrict__ keys) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ns) return;
  const bool ok = status[t] == BPPP_RP_EXCESS_OK;
  if (nonces)
    for (uint32_t j = 0; j < 2; j++)
      for (uint32_t o = 0; o < 33; o++) nonces[(size_t)t * EXP_NONCE + 33 * j + o] = ok ? (uint8_t)ex_pt_byte(aggxy + ((size_t)j * ns + t) * 16, o) : (uint8_t)0;
  if (keys)
    for (uint32_t o = 0; o < EX_KEY; o++) keys[(size_t)t * EX_KEY + o] = ok ? (uint8_t)ex_pt_byte(aggxy + ((size_t)2 * ns + t) * 16, o) : (uint8_t)0;
}

// ---- the session stage over xy [3][n][16]: R1agg, R2agg, X of n sums.  It runs where status[t] is OK.
// b = decode (SHA-256 (Db || the 33 bytes of R1agg || of R2agg || of X || msg)) mod n: 163 bytes
__global__ void __launch_bounds__(64) k_rp_expart_coef(uint32_t n, ExDomain db, const uint32_t *__restrict__ xy, const uint8_t *__restrict__ msgs,
                                                       const uint32_t *__restrict__ status, uint32_t *__restrict__ b) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  fe v = fe_zero();
  if (status[t] == BPPP_RP_EXCESS_OK) {
    const uint8_t *msg = msgs + (size_t)t * EX_MSG;
    v = ex_hash3(32 + 3 * 33 + EX_MSG, [&](uint32_t k) -> uint32_t {
      if (k < 32) return ex_dom_byte(db, k);
      if (k < 131) { const uint32_t col = (k - 32) / 33; return ex_pt_byte(xy + ((size_t)col * n + t) * 16, (k - 32) - 33 * col); }
      return msg[k - 131];
    });
  }
  fe_store(b + (size_t)t * 8, v);
}
// lanes 4t .. 4t + 3 are sum t: R = R1agg + b R2agg in XYZZ into Rz [n][XYZZ_WORDS], zz [n][8] = ZZ ZZZ (zero: infinity, or a sum whose verdict is
// taken — that quad leaves as a whole)
__global__ void __launch_bounds__(64) k_rp_expart_session(uint32_t n, const uint32_t *__restrict__ b, const uint32_t *__restrict__ xy, const uint32_t *__restrict__ status,
                                                          uint32_t *__restrict__ Rz, uint32_t *__restrict__ zz) {
  const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (t >= n) return;
  if (status[t] != BPPP_RP_EXCESS_OK) {
    if (quad_lane() == 0) { xyzz_store(Rz + (size_t)t * XYZZ_WORDS, xyzz_inf()); fe_store(zz + (size_t)t * 8, fe_zero()); }
    return;
  }
  xyzz acc = excess_mul_quad(fe_load(b + (size_t)t * 8), aff_load(xy + ((size_t)n + t) * 16));
  xyzz_add_quad(acc, xyzz_from_aff(aff_load(xy + (size_t)t * 16)));
  if (quad_lane() != 0) return;
  xyzz_store(Rz + (size_t)t * XYZZ_WORDS, acc);
  fe_store(zz + (size_t)t * 8, xyzz_is_inf(acc) ? fe_zero() : fq_to_fe(fq_mul(acc.ZZ, acc.ZZZ)));
}
// R [n][16] affine: NONCE_INFINITY where it is all zeros, else c, the single signer's challenge over the canonical bytes of R
__global__ void __launch_bounds__(64) k_rp_expart_challenge(uint32_t n, ExDomain dc, const uint32_t *__restrict__ R, const uint32_t *__restrict__ xy,
                                                            const uint8_t *__restrict__ msgs, uint32_t *__restrict__ status, uint32_t *__restrict__ c) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  fe ch = fe_zero();
  if (status[t] == BPPP_RP_EXCESS_OK) {
    const uint32_t *r = R + (size_t)t * 16;
    uint32_t any = 0;
    for (int k = 0; k < 16; k++) any |= r[k];
    if (!any) status[t] = BPPP_RP_EXCESS_NONCE_INFINITY;
    else ch = ex_challenge(dc, [&](uint32_t o) -> uint32_t { return ex_pt_byte(r, o); }, xy + ((size_t)2 * n + t) * 16, msgs + (size_t)t * EX_MSG);
  }
  fe_store(c + (size_t)t * 8, ch);
}

// ---- round 2
__global__ void __launch_bounds__(256) k_rp_expart_signpre(uint32_t n, const uint32_t *__restrict__ keybad, const uint32_t *__restrict__ rbad, uint32_t *__restrict__ status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n || status[t] != BPPP_RP_EXCESS_OK) return;
  if (keybad[t]) status[t] = BPPP_RP_EXCESS_BAD_KEY;
  else if (rbad[t]) status[t] = BPPP_RP_EXCESS_BAD_R;
}
// s = k_1 + b k_2 + c e mod n as put (s); zero bytes for a refused row
__global__ void __launch_bounds__(64) k_rp_expart_respond(uint32_t n, const uint32_t *__restrict__ blinds, const uint32_t *__restrict__ k, const uint32_t *__restrict__ b,
                                                          const uint32_t *__restrict__ c, const uint32_t *__restrict__ status, uint8_t *__restrict__ partials) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint8_t *row = partials + (size_t)t * EXP_PARTIAL;
  if (status[t] != BPPP_RP_EXCESS_OK) { for (uint32_t o = 0; o < EXP_PARTIAL; o++) row[o] = 0; return; }
  const fe s = fe_add<1>(fe_add<1>(fe_load(k + (size_t)t * 8), fe_mul<1>(fe_load(b + (size_t)t * 8), fe_load(k + ((size_t)n + t) * 8))),
                         fe_mul<1>(fe_load(c + (size_t)t * 8), fe_load(blinds + (size_t)t * 8)));
  uint32_t sw[8];
  fe_store(sw, s);
  for (uint32_t o = 0; o < EXP_PARTIAL; o++) row[o] = enc_be_byte(sw, o);
}

// ---- the partial check.  pre[p]: the first verdict of part p that applies, in the header's order — its own key, its own s_i, its own nonce points,
// then NO_AGGREGATE where another part of its sum does not lift, then the sum's own NO_KEY or NONCE_INFINITY — or EX_EVAL; in_sc [np][3][8]: the scalars of s_i B, zero for an s_i that is no scalar
__global__ void __launch_bounds__(64) k_rp_expart_partials(uint32_t np, uint32_t slot, const uint8_t *__restrict__ partials, const uint32_t *__restrict__ bad,
                                                           const uint32_t *__restrict__ sumof, const uint32_t *__restrict__ sum_status, uint32_t *__restrict__ in_sc,
                                                           uint32_t *__restrict__ pre) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  const fe s = load_field_be_raw(partials + (size_t)p * EXP_PARTIAL);
  const bool bad_s = !wi_canonical(s);
  const uint32_t sst = sum_status[sumof[p]];
  for (uint32_t b = 0; b < 3; b++) fe_store(in_sc + ((size_t)p * 3 + b) * 8, (!bad_s && b == slot) ? s : fe_zero());
  pre[p] = bad[(size_t)2 * np + p]         ? (uint32_t)BPPP_RP_EXCESS_BAD_KEY
           : bad_s                         ? (uint32_t)BPPP_RP_OPEN_NOT_CANONICAL
           : (bad[p] | bad[(size_t)np + p]) ? (uint32_t)BPPP_RP_EXCESS_BAD_R
           : (sst == BPPP_RP_EXCESS_BAD_KEY || sst == BPPP_RP_EXCESS_BAD_R) ? (uint32_t)BPPP_RP_EXCESS_NO_AGGREGATE
           : sst != BPPP_RP_EXCESS_OK      ? sst
                                           : EX_EVAL;
}
// the hot path: lanes 4p .. 4p + 3 of the launch are part p of sum t = sumof[p].  b_t R2_p + c_t X_p by the joint walk, less P_p = s_p B, against
// - R1_p: the equation  s B - b R2 - c X = R1  with both sides negated, cross-multiplied as k_rp_excess_mulcheck does.  A quad past np and a quad
// whose verdict is taken leave as a whole; every branch is on values all four lanes hold alike.
// Two wavefronts a SIMD are asked for: left alone the compiler takes 256 VGPRs and 31 AGPRs — one file of 512 on this chip, so one wavefront a SIMD;
// held to 256 it spills 31 registers (128 bytes a lane) and the issue-bound job is a tenth faster (DESIGN.md has both figures).
__global__ void __launch_bounds__(64, 2) k_rp_expart_mulcheck(uint32_t np, const uint32_t *__restrict__ b, const uint32_t *__restrict__ c, const uint32_t *__restrict__ sumof,
                                                           const uint32_t *__restrict__ pts, const uint32_t *__restrict__ P, const uint32_t *__restrict__ pre,
                                                           uint32_t *__restrict__ status) {
  const uint32_t p = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (p >= np) return;
  const uint32_t st = pre[p];
  if (st != EX_EVAL) { if (quad_lane() == 0) status[p] = st; return; }
  const uint32_t t = sumof[p];
  const fe bt = fe_load(b + (size_t)t * 8), ct = fe_load(c + (size_t)t * 8);
  const aff R2 = aff_load(pts + ((size_t)np + p) * 16), X = aff_load(pts + ((size_t)2 * np + p) * 16);
  xyzz acc = excess_mul2_quad(bt, R2, ct, X);
  xyzz_add_quad(acc, xyzz_from_aff(aff_cneg(aff_load(P + (size_t)p * 16), true)));
  const aff nr = aff_cneg(aff_load(pts + (size_t)p * 16), true);       // R1_p is a curve point here: never infinity
  const bool eq = !xyzz_is_inf(acc) && fq_normalizes_to_zero(fq_sub<5>(fq_mul(nr.x, acc.ZZ), acc.X)) && fq_normalizes_to_zero(fq_sub<3>(fq_mul(nr.y, acc.ZZZ), acc.Y));
  if (quad_lane() == 0) status[p] = eq ? (uint32_t)BPPP_RP_OPEN_OK : (uint32_t)BPPP_RP_OPEN_MISMATCH;
}

// ---- the final signature of sum t: the 33 bytes of R, then put (sum of the group's s_i mod n); each s_i is taken mod n, none is judged.  Zero bytes
// for a refused sum.
__global__ void __launch_bounds__(64) k_rp_expart_combine(uint32_t ns, uint32_t np, uint32_t p0, const uint32_t *__restrict__ part_start, const uint8_t *__restrict__ partials,
                                                          const uint32_t *__restrict__ R, const uint32_t *__restrict__ status, uint8_t *__restrict__ sigs) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ns) return;
  uint8_t *sig = sigs + (size_t)t * EX_SIG;
  if (status[t] != BPPP_RP_EXCESS_OK) { for (uint32_t o = 0; o < EX_SIG; o++) sig[o] = 0; return; }
  const uint32_t lo = part_start[t] - p0, hi = min(part_start[t + 1] - p0, np);
  fe s = fe_zero();
#pragma unroll 1
  for (uint32_t p = lo; p < hi; p++) s = fe_add<1>(s, wi_umod_n(load_field_be_raw(partials + (size_t)p * EXP_PARTIAL)));
  uint32_t sw[8];
  fe_store(sw, s);
  for (uint32_t o = 0; o < 33; o++) sig[o] = (uint8_t)ex_pt_byte(R + (size_t)t * 16, o);
  for (uint32_t o = 0; o < 32; o++) sig[33 + o] = enc_be_byte(sw, o);
}

}  // namespace bppp

using namespace bppp;
using namespace bppp::tally;
using namespace bppp::excess;

namespace {

ExDomain partnonce_domain(const bppp_rp *rp) { return domain("bppp/excess/partnonce/v1", rp->tag); }
ExDomain noncecoef_domain(const bppp_rp *rp) { return domain("bppp/excess/noncecoef/v1", rp->tag); }
// sessions (calls 1 and 3) and parts (calls 2, 4 and 5) per pass over the workspace: a quarter of the flat chunk, as the keys
size_t part_limit(const bppp_rp *rp) { return std::max<size_t>(1, rpp_flat_chunk(rp) / 4); }
dim3 lanes(size_t n, unsigned block = 64) { return dim3((unsigned)((n + block - 1) / block)); }

const char *signer_status_text(uint32_t s) {
  return s == BPPP_RP_EXCESS_NOT_CANONICAL    ? "the blinding part is not canonical (>= n)"
         : s == BPPP_RP_EXCESS_ZERO           ? "the blinding part is zero: its key is the point at infinity and has no encoding"
         : s == BPPP_RP_EXCESS_NONCE          ? "a nonce is zero"
         : s == BPPP_RP_EXCESS_BAD_KEY        ? "the aggregated key has a sign byte above 1 or an x without a curve point"
         : s == BPPP_RP_EXCESS_BAD_R          ? "an aggregated nonce point has a sign byte above 1 or an x without a curve point"
                                              : "the session nonce R1agg + b R2agg is the point at infinity";
}
const char *sum_status_text(uint32_t s) {
  return s == BPPP_RP_EXCESS_BAD_KEY   ? "a key of the group has a sign byte above 1 or an x without a curve point"
         : s == BPPP_RP_EXCESS_BAD_R   ? "a nonce point of the group has a sign byte above 1 or an x without a curve point"
         : s == BPPP_RP_EXCESS_NO_KEY  ? "the keys of the group add up to the point at infinity"
                                       : "the nonce points of the group add up to the point at infinity";
}

// ---- the session stage of n sums whose aggregates lie in xy [3][n][16]: b, R (affine), c; status is overruled where R is infinity
struct SessionWork { uint32_t *b, *c, *Rz, *zz, *zinv, *R; };
void session_carve(Carver &cv, size_t n, SessionWork &S) {
  S.b = cv.take<uint32_t>(n * 8); S.c = cv.take<uint32_t>(n * 8); S.Rz = cv.take<uint32_t>(n * XYZZ_WORDS); S.zz = cv.take<uint32_t>(n * 8); S.zinv = cv.take<uint32_t>(n * 8);
  S.R = cv.take<uint32_t>(n * 16);
}
int session_stage(bppp_rp *rp, size_t n, const uint32_t *xy, const uint8_t *msgs, uint32_t *status, const SessionWork &S, const ExDomain &db, const ExDomain &dc) {
  bppp_ctx *ctx = rp->ctx;
  hipStream_t st = ctx->stream;
  int rc;
  k_rp_expart_coef<<<lanes(n), dim3(64), 0, st>>>((uint32_t)n, db, xy, msgs, status, S.b);
  k_rp_expart_session<<<lanes(4 * n), dim3(64), 0, st>>>((uint32_t)n, S.b, xy, status, S.Rz, S.zz);
  BPPP_HIP(ctx, hipGetLastError());
  if ((rc = batch_inverse_run(ctx, S.zz, n, 0, S.zinv)) || (rc = affine_launch(ctx, n, S.Rz, S.zinv, S.R))) return rc;
  k_rp_expart_challenge<<<lanes(n), dim3(64), 0, st>>>((uint32_t)n, dc, S.R, xy, msgs, status, S.c);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

// ---- calls 1 and 3: n sessions of one party
struct SignerWork { uint32_t *k, *in_sc, *pts, *status, *bad, *sumof, *keybad, *rbad; uint8_t *aux; SessionWork S; };
int signer_carve(bppp_rp *rp, size_t C, bool sign, SignerWork &W) {
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    W.k = cv.take<uint32_t>(2 * C * 8); W.in_sc = cv.take<uint32_t>(sign ? 0 : 2 * C * 24); W.pts = cv.take<uint32_t>((sign ? 3 : 2) * C * 16); W.status = cv.take<uint32_t>(C);
    W.bad = cv.take<uint32_t>(sign ? 3 * C : 0); W.sumof = cv.take<uint32_t>(sign ? C : 0); W.keybad = cv.take<uint32_t>(sign ? C : 0); W.rbad = cv.take<uint32_t>(sign ? C : 0);
    W.aux = cv.take<uint8_t>(32);
    if (sign) session_carve(cv, C, W.S);
    if (!pass) { int rc = rpp_ensure_pwork(rp, cv.off); if (rc) return rc; }
  }
  return BPPP_OK;
}

int nonces_device(bppp_rp *rp, size_t n, const void *d_blinds, const void *d_msgs, const uint8_t aux[32], void *d_pubnonces, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!n) return BPPP_OK;
  if (n > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, "rp_excess_part_nonces: n must be below 2^31");
  if (!d_blinds || !d_msgs || !aux || !d_pubnonces) return fail(ctx, BPPP_ERR_ARG, "rp_excess_part_nonces: null input");
  hipSetDevice(ctx->device);
  int rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  const size_t C = std::min(n, part_limit(rp));
  SignerWork W;
  if ((rc = signer_carve(rp, C, false, W))) return rc;
  hipStream_t st = ctx->stream;
  const ExDomain dm = partnonce_domain(rp);
  const uint32_t slot = blind_slot(rp);
  std::vector<uint32_t> h_status(n);
  BPPP_HIP(ctx, hipMemcpyAsync(W.aux, aux, 32, hipMemcpyHostToDevice, st));
  for (size_t o = 0; o < n; o += C) {
    const size_t m = std::min(C, n - o);
    k_rp_expart_nonce<<<lanes(m), dim3(64), 0, st>>>((uint32_t)m, slot, dm, (const uint32_t *)d_blinds + o * 8, (const uint8_t *)d_msgs + o * EX_MSG, W.aux, W.k, W.in_sc, W.status);
    BPPP_HIP(ctx, hipGetLastError());
    if ((rc = rpp_commit_inputs(rp, W.in_sc, 2 * m, W.pts))) return rc;
    k_rp_expart_pubnonce<<<lanes(m), dim3(64), 0, st>>>((uint32_t)m, W.pts, W.status, (uint8_t *)d_pubnonces + o * EXP_NONCE);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(h_status.data() + o, W.status, m * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return rpp_report_refusals(ctx, "rp_excess_part_nonces", "part", h_status.data(), n, status, signer_status_text);
}

int sign_device(bppp_rp *rp, size_t n, const void *d_blinds, const void *d_msgs, const uint8_t aux[32], const void *d_agg_nonces, const void *d_agg_keys, void *d_partials,
                uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!n) return BPPP_OK;
  if (n > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, "rp_excess_part_sign: n must be below 2^31");
  if (!d_blinds || !d_msgs || !aux || !d_agg_nonces || !d_agg_keys || !d_partials) return fail(ctx, BPPP_ERR_ARG, "rp_excess_part_sign: null input");
  hipSetDevice(ctx->device);
  int rc;
  const size_t C = std::min(n, part_limit(rp));
  SignerWork W;
  if ((rc = signer_carve(rp, C, true, W))) return rc;
  hipStream_t st = ctx->stream;
  const ExDomain dm = partnonce_domain(rp), db = noncecoef_domain(rp), dc = challenge_domain(rp);
  std::vector<uint32_t> h_status(n);
  BPPP_HIP(ctx, hipMemcpyAsync(W.aux, aux, 32, hipMemcpyHostToDevice, st));
  for (size_t o = 0; o < n; o += C) {
    const size_t m = std::min(C, n - o);
    const uint32_t *bl = (const uint32_t *)d_blinds + o * 8;
    const uint8_t *msgs = (const uint8_t *)d_msgs + o * EX_MSG;
    k_rp_expart_nonce<<<lanes(m), dim3(64), 0, st>>>((uint32_t)m, blind_slot(rp), dm, bl, msgs, W.aux, W.k, nullptr, W.status);
    BPPP_HIP(ctx, hipMemsetAsync(W.keybad, 0, m * 4, st));
    BPPP_HIP(ctx, hipMemsetAsync(W.rbad, 0, m * 4, st));
    k_rp_expart_lift<<<lanes(3 * m), dim3(64), 0, st>>>((uint32_t)m, (uint32_t)m, 0u, nullptr, (const uint8_t *)d_agg_nonces + o * EXP_NONCE, (const uint8_t *)d_agg_keys + o * EX_KEY,
                                                       W.pts, W.bad, W.sumof, W.keybad, W.rbad);
    k_rp_expart_signpre<<<lanes(m, 256), dim3(256), 0, st>>>((uint32_t)m, W.keybad, W.rbad, W.status);
    BPPP_HIP(ctx, hipGetLastError());
    if ((rc = session_stage(rp, m, W.pts, msgs, W.status, W.S, db, dc))) return rc;
    k_rp_expart_respond<<<lanes(m), dim3(64), 0, st>>>((uint32_t)m, bl, W.k, W.S.b, W.S.c, W.status, (uint8_t *)d_partials + o * EXP_PARTIAL);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(h_status.data() + o, W.status, m * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return rpp_report_refusals(ctx, "rp_excess_part_sign", "part", h_status.data(), n, status, signer_status_text);
}

// ---- calls 2, 4 and 5: sums over groups of parts
struct GroupJob {
  bppp_rp *rp; std::string who;
  size_t nsums, nparts;
  const uint32_t *part_start; const uint8_t *pubnonces, *keys;
  std::vector<uint32_t> h_start;                // part_start on the host, after validation
  std::vector<size_t> cb;                       // the passes: sums [cb[c], cb[c + 1]), whole groups of at most part_limit parts together
  size_t ns_max = 0, np_max = 0;
};
struct GroupWork { uint32_t *pts, *bad, *sumof, *keybad, *rbad, *agg, *zz, *zinv, *aggxy, *sst, *in_sc, *P, *pre, *pst; SessionWork S; };

// the argument checks of the three calls: the sizes, then part_start by a kernel whose verdict is read back before anything reads through it, then
// the groups on the host: none empty, none longer than a pass ("<who>: part_start: sum N ...": not the "<who>: sum N: ..." of a refusal, after which the
// host variants download)
int group_checks(GroupJob &G, bppp_rp *rp, const char *who, size_t nsums, size_t nparts, const void *part_start, const void *pubnonces, const void *keys, bool null_args) {
  bppp_ctx *ctx = rp->ctx;
  const std::string w = who;
  G.rp = rp; G.who = w; G.nsums = nsums; G.nparts = nparts;
  G.part_start = (const uint32_t *)part_start; G.pubnonces = (const uint8_t *)pubnonces; G.keys = (const uint8_t *)keys;
  if (nsums > RPP_LIM31 || nparts > RPP_LIM31) return fail(ctx, BPPP_ERR_ARG, w + ": nsums and nparts must be below 2^31");
  if (null_args || !part_start || !pubnonces || !keys) return fail(ctx, BPPP_ERR_ARG, w + ": null input");
  hipSetDevice(ctx->device);
  int rc;
  if ((rc = rpp_ensure_pwork(rp, 256))) return rc;
  uint32_t *flag = (uint32_t *)rp->pwork, h = EXP_NONE;
  hipStream_t st = ctx->stream;
  BPPP_HIP(ctx, hipMemsetAsync(flag, 0xFF, 4, st));
  k_rp_expart_validate<<<dim3((unsigned)std::min<size_t>((nsums + 256) / 256, 4096)), dim3(256), 0, st>>>((uint32_t)nsums, (uint32_t)nparts, G.part_start, flag);
  BPPP_HIP(ctx, hipGetLastError());
  BPPP_HIP(ctx, hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, st));
  BPPP_HIP(ctx, hipStreamSynchronize(st));
  if (h != EXP_NONE) {                          // h <= nsums: one word of an array of nsums + 1
    uint32_t v = 0;
    BPPP_HIP(ctx, hipMemcpy(&v, G.part_start + h, 4, hipMemcpyDeviceToHost));
    return fail(ctx, BPPP_ERR_ARG, w + ": part_start[" + std::to_string(h) + "] = " + std::to_string(v) + " is not non-decreasing from 0 to nparts = " + std::to_string(nparts));
  }
  G.h_start.resize(nsums + 1);
  BPPP_HIP(ctx, hipMemcpy(G.h_start.data(), G.part_start, (nsums + 1) * 4, hipMemcpyDeviceToHost));
  const size_t limit = part_limit(rp);
  for (size_t t = 0; t < nsums; t++) {
    const size_t len = G.h_start[t + 1] - G.h_start[t];
    if (!len) return fail(ctx, BPPP_ERR_ARG, w + ": part_start: sum " + std::to_string(t) + " has no part");
    if (len > limit) return fail(ctx, BPPP_ERR_ARG, w + ": part_start: sum " + std::to_string(t) + " has " + std::to_string(len) + " parts, more than the " + std::to_string(limit) + " of one pass");
  }
  G.cb.assign(1, 0);
  for (size_t t = 0; t < nsums; t++)
    if (G.h_start[t + 1] - G.h_start[G.cb.back()] > limit) G.cb.push_back(t);
  G.cb.push_back(nsums);
  for (size_t c = 0; c + 1 < G.cb.size(); c++) {
    G.ns_max = std::max(G.ns_max, G.cb[c + 1] - G.cb[c]);
    G.np_max = std::max<size_t>(G.np_max, G.h_start[G.cb[c + 1]] - G.h_start[G.cb[c]]);
  }
  return BPPP_OK;
}
// session: calls 4 and 5; check: call 4
int group_carve(const GroupJob &G, bool session, bool check, GroupWork &W) {
  bppp_rp *rp = G.rp;
  const size_t NS = G.ns_max, NP = G.np_max;
  for (int pass = 0; pass < 2; pass++) {
    Carver cv(pass ? rp->pwork : nullptr, rp->pwork_bytes);
    W.pts = cv.take<uint32_t>(3 * NP * 16); W.bad = cv.take<uint32_t>(3 * NP); W.sumof = cv.take<uint32_t>(NP); W.keybad = cv.take<uint32_t>(NS); W.rbad = cv.take<uint32_t>(NS);
    W.agg = cv.take<uint32_t>(3 * NS * XYZZ_WORDS); W.zz = cv.take<uint32_t>(3 * NS * 8); W.zinv = cv.take<uint32_t>(3 * NS * 8); W.aggxy = cv.take<uint32_t>(3 * NS * 16);
    W.sst = cv.take<uint32_t>(NS);
    W.in_sc = cv.take<uint32_t>(check ? NP * 24 : 0); W.P = cv.take<uint32_t>(check ? NP * 16 : 0); W.pre = cv.take<uint32_t>(check ? NP : 0); W.pst = cv.take<uint32_t>(check ? NP : 0);
    if (session) session_carve(cv, NS, W.S);
    if (!pass) { int rc = rpp_ensure_pwork(rp, cv.off); if (rc) return rc; }
  }
  return BPPP_OK;
}
// sums [t0, t0 + ns) with their np parts from p0 on: W.pts, W.bad, W.sumof, the affine aggregates W.aggxy and the verdicts W.sst
int group_stage(const GroupJob &G, const GroupWork &W, size_t t0, size_t ns, size_t p0, size_t np) {
  bppp_ctx *ctx = G.rp->ctx;
  hipStream_t st = ctx->stream;
  const uint32_t *ps = G.part_start + t0;
  int rc;
  BPPP_HIP(ctx, hipMemsetAsync(W.keybad, 0, ns * 4, st));
  BPPP_HIP(ctx, hipMemsetAsync(W.rbad, 0, ns * 4, st));
  k_rp_expart_lift<<<lanes(3 * np), dim3(64), 0, st>>>((uint32_t)np, (uint32_t)ns, (uint32_t)p0, ps, G.pubnonces + p0 * EXP_NONCE, G.keys + p0 * EX_KEY, W.pts, W.bad, W.sumof,
                                                      W.keybad, W.rbad);
  k_rp_expart_sum<<<lanes(12 * ns), dim3(64), 0, st>>>((uint32_t)ns, (uint32_t)np, (uint32_t)p0, ps, W.pts, W.agg, W.zz);
  BPPP_HIP(ctx, hipGetLastError());
  if ((rc = batch_inverse_run(ctx, W.zz, 3 * ns, 0, W.zinv)) || (rc = affine_launch(ctx, 3 * ns, W.agg, W.zinv, W.aggxy))) return rc;
  k_rp_expart_judge<<<lanes(ns, 256), dim3(256), 0, st>>>((uint32_t)ns, W.keybad, W.rbad, W.aggxy, W.sst);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

int aggregate_device(bppp_rp *rp, size_t nsums, size_t nparts, const void *d_part_start, const void *d_pubnonces, const void *d_keys, void *d_agg_nonces, void *d_agg_keys,
                     uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  GroupJob G;
  GroupWork W;
  int rc;
  if ((rc = group_checks(G, rp, "rp_excess_part_aggregate", nsums, nparts, d_part_start, d_pubnonces, d_keys, !d_agg_nonces || !d_agg_keys)) || (rc = group_carve(G, false, false, W)))
    return rc;
  hipStream_t st = ctx->stream;
  std::vector<uint32_t> h_status(nsums);
  for (size_t c = 0; c + 1 < G.cb.size(); c++) {
    const size_t t0 = G.cb[c], ns = G.cb[c + 1] - t0, p0 = G.h_start[t0], np = G.h_start[t0 + ns] - p0;
    if ((rc = group_stage(G, W, t0, ns, p0, np))) return rc;
    k_rp_expart_encode<<<lanes(ns), dim3(64), 0, st>>>((uint32_t)ns, W.aggxy, W.sst, (uint8_t *)d_agg_nonces + t0 * EXP_NONCE, (uint8_t *)d_agg_keys + t0 * EX_KEY);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(h_status.data() + t0, W.sst, ns * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return rpp_report_refusals(ctx, "rp_excess_part_aggregate", "sum", h_status.data(), nsums, status, sum_status_text);
}

int verify_device(bppp_rp *rp, size_t nsums, size_t nparts, const void *d_part_start, const void *d_pubnonces, const void *d_keys, const void *d_partials, const void *d_msgs,
                  uint32_t *status, uint32_t *sum_status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  GroupJob G;
  GroupWork W;
  int rc;
  if ((rc = group_checks(G, rp, "rp_excess_part_verify", nsums, nparts, d_part_start, d_pubnonces, d_keys, !d_partials || !d_msgs || !status))) return rc;
  if (!rp->comb && (rc = rpp_build_fixed_table(rp))) return rc;
  if ((rc = group_carve(G, true, true, W))) return rc;
  hipStream_t st = ctx->stream;
  const ExDomain db = noncecoef_domain(rp), dc = challenge_domain(rp);
  for (size_t c = 0; c + 1 < G.cb.size(); c++) {
    const size_t t0 = G.cb[c], ns = G.cb[c + 1] - t0, p0 = G.h_start[t0], np = G.h_start[t0 + ns] - p0;
    if ((rc = group_stage(G, W, t0, ns, p0, np)) || (rc = session_stage(rp, ns, W.aggxy, (const uint8_t *)d_msgs + t0 * EX_MSG, W.sst, W.S, db, dc))) return rc;
    k_rp_expart_partials<<<lanes(np), dim3(64), 0, st>>>((uint32_t)np, blind_slot(rp), (const uint8_t *)d_partials + p0 * EXP_PARTIAL, W.bad, W.sumof, W.sst, W.in_sc, W.pre);
    BPPP_HIP(ctx, hipGetLastError());
    if ((rc = rpp_commit_inputs(rp, W.in_sc, np, W.P))) return rc;
    k_rp_expart_mulcheck<<<lanes(4 * np), dim3(64), 0, st>>>((uint32_t)np, W.S.b, W.S.c, W.sumof, W.pts, W.P, W.pre, W.pst);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(status + p0, W.pst, np * 4, hipMemcpyDeviceToHost, st));
    if (sum_status) BPPP_HIP(ctx, hipMemcpyAsync(sum_status + t0, W.sst, ns * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return BPPP_OK;
}

int combine_device(bppp_rp *rp, size_t nsums, size_t nparts, const void *d_part_start, const void *d_pubnonces, const void *d_keys, const void *d_partials, const void *d_msgs,
                   void *d_sigs, void *d_agg_keys, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  GroupJob G;
  GroupWork W;
  int rc;
  if ((rc = group_checks(G, rp, "rp_excess_part_combine", nsums, nparts, d_part_start, d_pubnonces, d_keys, !d_partials || !d_msgs || !d_sigs)) || (rc = group_carve(G, true, false, W)))
    return rc;
  hipStream_t st = ctx->stream;
  const ExDomain db = noncecoef_domain(rp), dc = challenge_domain(rp);
  std::vector<uint32_t> h_status(nsums);
  for (size_t c = 0; c + 1 < G.cb.size(); c++) {
    const size_t t0 = G.cb[c], ns = G.cb[c + 1] - t0, p0 = G.h_start[t0], np = G.h_start[t0 + ns] - p0;
    if ((rc = group_stage(G, W, t0, ns, p0, np)) || (rc = session_stage(rp, ns, W.aggxy, (const uint8_t *)d_msgs + t0 * EX_MSG, W.sst, W.S, db, dc))) return rc;
    k_rp_expart_combine<<<lanes(ns), dim3(64), 0, st>>>((uint32_t)ns, (uint32_t)np, (uint32_t)p0, G.part_start + t0, (const uint8_t *)d_partials + p0 * EXP_PARTIAL, W.S.R, W.sst,
                                                       (uint8_t *)d_sigs + t0 * EX_SIG);
    if (d_agg_keys) k_rp_expart_encode<<<lanes(ns), dim3(64), 0, st>>>((uint32_t)ns, W.aggxy, W.sst, nullptr, (uint8_t *)d_agg_keys + t0 * EX_KEY);
    BPPP_HIP(ctx, hipGetLastError());
    BPPP_HIP(ctx, hipMemcpyAsync(h_status.data() + t0, W.sst, ns * 4, hipMemcpyDeviceToHost, st));
    BPPP_HIP(ctx, hipStreamSynchronize(st));
  }
  return rpp_report_refusals(ctx, "rp_excess_part_combine", "sum", h_status.data(), nsums, status, sum_status_text);
}

// ---- host variants: upload, the _device variant, download
struct HostSigner {
  DevBuf bl, msgs, aggn, aggk, out;
  int up(bppp_rp *rp, size_t n, const uint64_t *blinds, const uint8_t *m, const uint8_t *an, const uint8_t *ak, const void *want, size_t out_row) {
    bppp_ctx *ctx = rp->ctx;
    if (n > RPP_LIM31) return BPPP_OK;        // the _device variant refuses this size before it reads anything
    hipSetDevice(ctx->device);
    int rc = bl.up(ctx, blinds, n * 32);
    if (!rc) rc = msgs.up(ctx, m, n * EX_MSG);
    if (!rc) rc = aggn.up(ctx, an, n * EXP_NONCE);
    if (!rc) rc = aggk.up(ctx, ak, n * EX_KEY);
    if (!rc) rc = out.out(ctx, want, n * out_row);
    return rc;
  }
};
struct HostGroups {
  DevBuf start, nonces, keys, partials, msgs, out1, out2;
  int up(bppp_rp *rp, size_t nsums, size_t nparts, const uint32_t *part_start, const uint8_t *pn, const uint8_t *k, const uint8_t *pt, const uint8_t *m) {
    bppp_ctx *ctx = rp->ctx;
    if (nsums > RPP_LIM31 || nparts > RPP_LIM31) return BPPP_OK;
    hipSetDevice(ctx->device);
    int rc = start.up(ctx, part_start, (nsums + 1) * 4);
    if (!rc) rc = nonces.up(ctx, pn, nparts * EXP_NONCE);
    if (!rc) rc = keys.up(ctx, k, nparts * EX_KEY);
    if (!rc) rc = partials.up(ctx, pt, nparts * EXP_PARTIAL);
    if (!rc) rc = msgs.up(ctx, m, nsums * EX_MSG);
    return rc;
  }
};

}  // namespace

extern "C" {

int bppp_rp_excess_part_nonces_device(bppp_rp *rp, size_t n, const void *d_part_blinds, const void *d_msgs, const uint8_t aux[32], void *d_pubnonces, uint32_t *status) {
  return nonces_device(rp, n, d_part_blinds, d_msgs, aux, d_pubnonces, status);
}

int bppp_rp_excess_part_nonces(bppp_rp *rp, size_t n, const uint64_t *part_blinds, const uint8_t *msgs, const uint8_t aux[32], uint8_t *pubnonces, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!n) return BPPP_OK;
  HostSigner H;
  int rc = H.up(rp, n, part_blinds, msgs, nullptr, nullptr, pubnonces, EXP_NONCE);
  if (rc) return rc;
  rc = nonces_device(rp, n, H.bl.p, H.msgs.p, aux, H.out.p, status);
  return rpp_download_refused(ctx, rc, "rp_excess_part_nonces: part ", pubnonces, H.out.p, n * EXP_NONCE);
}

int bppp_rp_excess_part_aggregate_device(bppp_rp *rp, size_t nsums, size_t nparts, const void *d_part_start, const void *d_pubnonces, const void *d_keys, void *d_agg_nonces,
                                         void *d_agg_keys, uint32_t *status) {
  return aggregate_device(rp, nsums, nparts, d_part_start, d_pubnonces, d_keys, d_agg_nonces, d_agg_keys, status);
}

int bppp_rp_excess_part_aggregate(bppp_rp *rp, size_t nsums, size_t nparts, const uint32_t *part_start, const uint8_t *pubnonces, const uint8_t *keys, uint8_t *agg_nonces,
                                  uint8_t *agg_keys, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  HostGroups H;
  int rc = H.up(rp, nsums, nparts, part_start, pubnonces, keys, nullptr, nullptr);
  if (!rc && nsums <= RPP_LIM31) rc = H.out1.out(ctx, agg_nonces, nsums * EXP_NONCE);
  if (!rc && nsums <= RPP_LIM31) rc = H.out2.out(ctx, agg_keys, nsums * EX_KEY);
  if (rc) return rc;
  rc = aggregate_device(rp, nsums, nparts, H.start.p, H.nonces.p, H.keys.p, H.out1.p, H.out2.p, status);
  rc = rpp_download_refused(ctx, rc, "rp_excess_part_aggregate: sum ", agg_nonces, H.out1.p, nsums * EXP_NONCE);
  return rpp_download_refused(ctx, rc, "rp_excess_part_aggregate: sum ", agg_keys, H.out2.p, nsums * EX_KEY);
}

int bppp_rp_excess_part_sign_device(bppp_rp *rp, size_t n, const void *d_part_blinds, const void *d_msgs, const uint8_t aux[32], const void *d_agg_nonces, const void *d_agg_keys,
                                    void *d_partials, uint32_t *status) {
  return sign_device(rp, n, d_part_blinds, d_msgs, aux, d_agg_nonces, d_agg_keys, d_partials, status);
}

int bppp_rp_excess_part_sign(bppp_rp *rp, size_t n, const uint64_t *part_blinds, const uint8_t *msgs, const uint8_t aux[32], const uint8_t *agg_nonces, const uint8_t *agg_keys,
                             uint8_t *partials, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!n) return BPPP_OK;
  HostSigner H;
  int rc = H.up(rp, n, part_blinds, msgs, agg_nonces, agg_keys, partials, EXP_PARTIAL);
  if (rc) return rc;
  rc = sign_device(rp, n, H.bl.p, H.msgs.p, aux, H.aggn.p, H.aggk.p, H.out.p, status);
  return rpp_download_refused(ctx, rc, "rp_excess_part_sign: part ", partials, H.out.p, n * EXP_PARTIAL);
}

int bppp_rp_excess_part_verify_device(bppp_rp *rp, size_t nsums, size_t nparts, const void *d_part_start, const void *d_pubnonces, const void *d_keys, const void *d_partials,
                                      const void *d_msgs, uint32_t *status, uint32_t *sum_status) {
  return verify_device(rp, nsums, nparts, d_part_start, d_pubnonces, d_keys, d_partials, d_msgs, status, sum_status);
}

int bppp_rp_excess_part_verify(bppp_rp *rp, size_t nsums, size_t nparts, const uint32_t *part_start, const uint8_t *pubnonces, const uint8_t *keys, const uint8_t *partials,
                               const uint8_t *msgs, uint32_t *status, uint32_t *sum_status) {
  if (!rp) return BPPP_ERR_ARG;
  if (ctx_closed(rp->ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  HostGroups H;
  int rc = H.up(rp, nsums, nparts, part_start, pubnonces, keys, partials, msgs);
  if (rc) return rc;
  return verify_device(rp, nsums, nparts, H.start.p, H.nonces.p, H.keys.p, H.partials.p, H.msgs.p, status, sum_status);
}

int bppp_rp_excess_part_combine_device(bppp_rp *rp, size_t nsums, size_t nparts, const void *d_part_start, const void *d_pubnonces, const void *d_keys, const void *d_partials,
                                       const void *d_msgs, void *d_sigs, void *d_agg_keys, uint32_t *status) {
  return combine_device(rp, nsums, nparts, d_part_start, d_pubnonces, d_keys, d_partials, d_msgs, d_sigs, d_agg_keys, status);
}

int bppp_rp_excess_part_combine(bppp_rp *rp, size_t nsums, size_t nparts, const uint32_t *part_start, const uint8_t *pubnonces, const uint8_t *keys, const uint8_t *partials,
                                const uint8_t *msgs, uint8_t *sigs, uint8_t *agg_keys, uint32_t *status) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!nsums) return BPPP_OK;
  HostGroups H;
  int rc = H.up(rp, nsums, nparts, part_start, pubnonces, keys, partials, msgs);
  if (!rc && nsums <= RPP_LIM31) rc = H.out1.out(ctx, sigs, nsums * EX_SIG);
  if (!rc && nsums <= RPP_LIM31) rc = H.out2.out(ctx, agg_keys, nsums * EX_KEY);
  if (rc) return rc;
  rc = combine_device(rp, nsums, nparts, H.start.p, H.nonces.p, H.keys.p, H.partials.p, H.msgs.p, H.out1.p, H.out2.p, status);
  rc = rpp_download_refused(ctx, rc, "rp_excess_part_combine: sum ", sigs, H.out1.p, nsums * EX_SIG);
  if (agg_keys) rc = rpp_download_refused(ctx, rc, "rp_excess_part_combine: sum ", agg_keys, H.out2.p, nsums * EX_KEY);
  return rc;
}

}  // extern "C"
