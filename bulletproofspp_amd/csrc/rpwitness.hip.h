// rpwitness.hip.h — the two ends of bppp_rp_prove_batch_device that the host entry points do on the host cores: the witness of every proof
// (range and balance checks, digits, multiplicities) from amounts, types and blindings in HBM, and the encoded files from the affine points
// and canonical scalars the prover's stream leaves in HBM.
//   k_rpp_witness      witnessTRRP (src/RangeProof/TypedReciprocal.hs:372-389) + makePhase1s' digits and multiplicities (:125-161, getDsMs
//                      :74-80): what make_witness (csrc/rpprove.hip) fills, in the arrays rpp_device_prove's stream consumes
//   k_brp_witness      witnessBRP (src/RangeProof/Binary.hs:158-166) + makeDigits (:56-69): prove_batch_binary_dev's host loop (csrc/brpprove.hip)
//   k_rp_encode_files  encodeProof' (src/RangeProof.hs:60-66, src/Encoding.hs:81-86, :130-134): rpp_encode_files (csrc/rpprove.hip)
// One workgroup (one wavefront) per proof.  Ranges of a proof are independent (one lane each), the digits of a range are a dependent chain.
// Range arithmetic is on 256-bit INTEGERS in two's complement (csrc/rpsetup.hpp; wi_*, csrc/rpwords.hip.h), not on field elements.  A digit is found by bisection over a
// 256 x 32-bit product for every input: the host's 64-bit fast path (digits_into, csrc/rpsetup.hpp) returns the same digit where it applies
// (a coefficient that does not fit: 0; a zero coefficient: radix - 1).
// The kernels and their launchers live in a header because the test library (csrc/testhooks.hip) runs the witness kernel alone.
#pragma once
#include <vector>
#include "fe.hip.h"
#include "rp_internal.hpp"
#include "rpwords.hip.h"

namespace bppp {

// status word of one proof: 0 = a witness, else the host's refusal (same order of precedence as make_witness / prove_batch_binary_dev)
// — the words and their texts: csrc/rpsetup.hpp, next to the host's witness_status
using bppp_rps::WIT_OK; using bppp_rps::WIT_NOT_CANONICAL; using bppp_rps::WIT_UNBALANCED; using bppp_rps::WIT_OUT_OF_RANGE; using bppp_rps::WIT_BIN_NOT_CANONICAL;
using bppp_rps::WIT_BIN_UNBALANCED; using bppp_rps::wit_status_text;

struct WitDims { uint32_t nr, nlen, nmss, npub, has_types, nlive, conserve, coef_words, pub_words; };
// rp->d_wit: [nr][WR_WORDS] range records | coefficients [..][8] (plain integers) | typed: [npub][WP_WORDS] public (type, amount, is_output);
// binary: net_public [8]
enum : uint32_t { WR_LO = 0, WR_HI = 8, WR_BASE = 16, WR_FLAGS = 17, WR_NCOEF = 18, WR_COEF = 19, WR_POS = 20, WR_MOFF = 21, WR_MOFF2 = 22, WR_WORDS = 24,
                  WF_SHARED = 1, WF_OUTPUT = 2, WF_ASSUMED = 4, WF_BIT = 8, WP_WORDS = 17 };

// a * m for a 32-bit m; true when the product does not fit 256 bits
BPPP_DI bool wi_mul32(fe &r, const fe &a, uint32_t m) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { c += (uint64_t)a.v[i] * m; r.v[i] = (uint32_t)c; c >>= 32; }
  return c != 0;
}
// the largest d <= radix - 1 with d * cf <= n (digits, TypedReciprocal.hs:125-127); n loses d * cf
BPPP_DI uint32_t wi_digit(fe &n, const fe &cf, uint32_t radix) {
  uint32_t lo = 0, hi = radix - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    fe prod;
    const bool ovf = wi_mul32(prod, cf, mid);
    if (!ovf && !wi_ult(n, prod)) lo = mid; else hi = mid - 1;
  }
  if (lo) { fe prod; wi_mul32(prod, cf, lo); raw_sub(n, n, prod); }
  return lo;
}

// amounts / types / blinds [B][nr][8] words as the caller gave them; d_pub NULL or [B][npub][8] canonical.  Out: in_sc [B][nr][3][8] (amount mod n,
// type, blinding), dig / mul [B][nlen], mss [B][nmss], status [B].  The arrays of a proof whose status is not WIT_OK are unspecified.
// src_index: NULL, or slot b (the block) reads proof src_index[b] of amounts / types / blinds / d_pub and writes slot b of every output — the
// accepted proofs of a batch compacted (bppp_rp_prove_batch_status_device, csrc/rpwitness.hip)
__global__ void __launch_bounds__(64) k_rpp_witness(WitDims D, const uint32_t *__restrict__ tab, const uint32_t *__restrict__ amounts, const uint32_t *__restrict__ types,
                                                    const uint32_t *__restrict__ blinds, const uint32_t *__restrict__ d_pub, uint32_t *in_sc, uint32_t *dig, uint32_t *mul,
                                                    uint32_t *mss, uint32_t *__restrict__ status, const uint32_t *__restrict__ src_index) {
  __shared__ uint32_t bad;
  const uint32_t t = threadIdx.x;
  const size_t b = blockIdx.x, src = src_index ? src_index[b] : b;
  const uint32_t *coefs = tab + (size_t)D.nr * WR_WORDS, *pubs = coefs + D.coef_words;
  if (t == 0) bad = 0;
  for (uint32_t i = t; i < D.nlen; i += 64) { dig[b * D.nlen + i] = 0; mul[b * D.nlen + i] = 0; }
  for (uint32_t i = t; i < D.nmss; i += 64) mss[b * D.nmss + i] = 0;
  __syncthreads();
  for (uint32_t i = t; i < D.nr; i += 64) {
    const uint32_t *R = tab + (size_t)i * WR_WORDS;
    const size_t e = b * D.nr + i, se = src * D.nr + i;
    const fe amt = fe_load(amounts + se * 8), ty = fe_load(types + se * 8), bl = fe_load(blinds + se * 8);
    if (!wi_canonical(ty) || !wi_canonical(bl)) atomicOr(&bad, 1u << WIT_NOT_CANONICAL);
    fe_store(in_sc + e * 24, wi_smod_n(amt)); fe_store(in_sc + e * 24 + 8, ty); fe_store(in_sc + e * 24 + 16, bl);
    const uint32_t fl = R[WR_FLAGS];
    if (fl & WF_ASSUMED) continue;
    const fe lo = fe_load(R + WR_LO);
    if (wi_slt(amt, lo) || !wi_slt(amt, fe_load(R + WR_HI))) { atomicOr(&bad, 1u << WIT_OUT_OF_RANGE); continue; }
    fe n;
    raw_sub(n, amt, lo);
    const uint32_t base = R[WR_BASE], nc = R[WR_NCOEF], hb = (fl & WF_BIT) ? 1u : 0u;
    uint32_t *dg = dig + b * D.nlen + R[WR_POS], *ml = mul + b * D.nlen + R[WR_POS], *ms = mss + b * D.nmss;
    for (uint32_t j = 0; j < nc; j++) {
      const bool bit = hb && j == 0;
      const uint32_t d = wi_digit(n, fe_load(coefs + (size_t)(R[WR_COEF] + j) * 8), bit ? 2u : base);
      dg[j] = d;
      if (!d) continue;
      // multiplicities against ns = [1 | has_bit] ++ [1 .. base - 1] (:141-145): the bit itself, then one count per non-zero digit value —
      // shared: in the proof's table of this base (the bit's in base 2's); inline: at the range's own positions, which this lane alone writes
      if (fl & WF_SHARED) atomicAdd(ms + (bit ? R[WR_MOFF2] : R[WR_MOFF] + d - 1), 1u);
      else ml[bit ? 0 : hb + d - 1] += 1;
    }
  }
  __syncthreads();
  if (D.has_types) {
    // every type's amounts balance (:376-381): entry f is a public (type, amount) or a range's (type, amount mod n), outputs negative;
    // lane e sums the entries of ITS type
    const uint32_t ne = D.npub + D.nr;
    for (uint32_t e = t; e < ne; e += 64) {
      const fe te = e < D.npub ? fe_load(pubs + (size_t)e * WP_WORDS) : fe_load(in_sc + (b * D.nr + (e - D.npub)) * 24 + 8);
      fe sum = fe_zero();
      for (uint32_t f = 0; f < ne; f++) {
        fe tf, v;
        bool out;
        if (f < D.npub) {
          const uint32_t *P = pubs + (size_t)f * WP_WORDS;
          tf = fe_load(P); v = d_pub ? fe_load(d_pub + (src * D.npub + f) * 8) : fe_load(P + 8); out = P[16] != 0;
        } else {
          const uint32_t *I = in_sc + (b * D.nr + (f - D.npub)) * 24;
          tf = fe_load(I + 8); v = fe_load(I); out = (tab[(size_t)(f - D.npub) * WR_WORDS + WR_FLAGS] & WF_OUTPUT) != 0;
        }
        if (!fe_eq(tf, te)) continue;
        sum = out ? fe_sub<1>(sum, v) : fe_add<1>(sum, v);
      }
      if (!fe_is_zero(sum)) atomicOr(&bad, 1u << WIT_UNBALANCED);
    }
    __syncthreads();
  }
  if (t == 0) status[b] = bad ? (uint32_t)(__ffs((int)bad) - 1) : WIT_OK;
}

// RangeProof.Binary: amounts / blinds [B][nr][8]; d_pub NULL or [B][8] canonical net_public.  Out: in_sc [B][nr][3][8] (amount mod n, blinding, 0),
// bits [B][nlive] (one byte per live position), status [B]; src_index as for k_rpp_witness
__global__ void __launch_bounds__(64) k_brp_witness(WitDims D, const uint32_t *__restrict__ tab, const uint32_t *__restrict__ amounts, const uint32_t *__restrict__ blinds,
                                                    const uint32_t *__restrict__ d_pub, uint32_t *__restrict__ in_sc, uint8_t *__restrict__ bits,
                                                    uint32_t *__restrict__ status, const uint32_t *__restrict__ src_index) {
  __shared__ uint32_t first_bad;             // (range << 3 | reason) of the lowest-numbered range the host's loop would stop at
  __shared__ uint32_t part[64 * 8];
  const uint32_t t = threadIdx.x;
  const size_t b = blockIdx.x, src = src_index ? src_index[b] : b;
  const uint32_t *coefs = tab + (size_t)D.nr * WR_WORDS, *netp = coefs + D.coef_words;
  if (t == 0) first_bad = 0xFFFFFFFFu;
  __syncthreads();
  fe vsum = fe_zero();
  for (uint32_t i = t; i < D.nr; i += 64) {
    const uint32_t *R = tab + (size_t)i * WR_WORDS;
    const size_t e = b * D.nr + i, se = src * D.nr + i;
    const fe amt = fe_load(amounts + se * 8), bl = fe_load(blinds + se * 8), v = wi_smod_n(amt);
    const uint32_t fl = R[WR_FLAGS];
    vsum = (fl & WF_OUTPUT) ? fe_sub<1>(vsum, v) : fe_add<1>(vsum, v);
    fe_store(in_sc + e * 24, v); fe_store(in_sc + e * 24 + 8, bl); fe_store(in_sc + e * 24 + 16, fe_zero());      // scalarRPW' (Internal.hs:56-57): v g + bl h0
    if (!wi_canonical(bl)) { atomicMin(&first_bad, i << 3 | WIT_BIN_NOT_CANONICAL); continue; }
    if (fl & WF_ASSUMED) continue;
    const fe lo = fe_load(R + WR_LO);
    if (wi_slt(amt, lo) || !wi_slt(amt, fe_load(R + WR_HI))) { atomicMin(&first_bad, i << 3 | WIT_OUT_OF_RANGE); continue; }
    // makeDigits (:56-69, digits_binary_into of csrc/rpsetup.hpp): the top digit takes b_n, the rest are the n1 bits of what is left
    fe n;
    raw_sub(n, amt, lo);
    const uint32_t n1 = R[WR_NCOEF] - 1;
    const fe bn = fe_load(coefs + (size_t)R[WR_COEF] * 8);
    bool over = false;                       // n >> n1 != 0
    for (uint32_t k = 0; k < 8; k++) {
      const uint32_t w = n.v[k];
      if (32 * k >= n1) over |= w != 0;
      else if (32 * (k + 1) > n1) over |= (w >> (n1 - 32 * k)) != 0;
    }
    const bool top = wi_ult(bn, n) || over;
    if (top) raw_sub(n, n, bn);
    uint8_t *o = bits + b * D.nlive + R[WR_POS];
    o[0] = top ? 1 : 0;
    for (uint32_t j = 0; j < n1; j++) { const uint32_t k = n1 - 1 - j; o[1 + j] = (uint8_t)((n.v[k >> 5] >> (k & 31)) & 1u); }
  }
  for (int k = 0; k < 8; k++) part[t * 8 + k] = vsum.v[k];
  __syncthreads();
  if (t == 0) {
    fe s = d_pub ? fe_load(d_pub + src * 8) : fe_load(netp);
    for (uint32_t l = 0; l < 64; l++) { fe p; for (int k = 0; k < 8; k++) p.v[k] = part[l * 8 + k]; s = fe_add<1>(s, p); }
    status[b] = first_bad != 0xFFFFFFFFu ? (first_bad & 7u) : (D.conserve && fe_is_zero(s)) ? WIT_OK : WIT_BIN_UNBALANCED;
  }
}

// ---- encodeProof': one workgroup per proof, one lane per OUTPUT BYTE (consecutive lanes write consecutive bytes of the file)
struct EncDims {
  uint32_t nr, k, fn, fl, nlead, coms_bytes, proof_bytes, batch;
  uint32_t lead_off[4], lead_stride[4];       // leading commitment j of proof b: com + (lead_off[j] + b * lead_stride[j]) * 16 words
};
// in_pt [B][nr][16]; com: the range-proof commitments (EncDims::lead_*); resp [k][B][2][16] in round order (the file lists the LAST round
// first, Bulletproof.hs:359); wn [B][fn][8], wl [B][fl][8] canonical.  coms_files [B][coms_bytes], proof_files [B][proof_bytes]
// dst_index: NULL, or the files of slot b (the block) are those of proof dst_index[b] in the two file buffers
__global__ void __launch_bounds__(256) k_rp_encode_files(EncDims D, const uint32_t *__restrict__ in_pt, const uint32_t *__restrict__ com, const uint32_t *__restrict__ resp,
                                                         const uint32_t *__restrict__ wn, const uint32_t *__restrict__ wl, uint8_t *__restrict__ coms_files,
                                                         uint8_t *__restrict__ proof_files, const uint32_t *__restrict__ dst_index) {
  const size_t b = blockIdx.x, dst = dst_index ? dst_index[b] : b;
  const uint32_t t = threadIdx.x;
  {
    const uint32_t ns = (D.nr + 7) / 8;
    uint8_t *f = coms_files + dst * D.coms_bytes;
    const uint32_t *pts = in_pt + b * D.nr * 16;
    for (uint32_t o = t; o < D.coms_bytes; o += 256) {
      uint8_t v = 0;
      if (o < ns) { for (uint32_t i = 8 * o; i < 8 * o + 8 && i < D.nr; i++) v |= (uint8_t)(enc_sign(pts + (size_t)i * 16) << (i & 7)); }
      else v = enc_be_byte(pts + (size_t)((o - ns) >> 5) * 16, (o - ns) & 31);
      f[o] = v;
    }
  }
  const uint32_t nsc = D.fn + D.fl, np = D.nlead + 2 * D.k, ns = (np + 7) / 8;
  auto point = [&](uint32_t j) -> const uint32_t * {
    if (j < D.nlead) return com + ((size_t)D.lead_off[j] + b * D.lead_stride[j]) * 16;
    const uint32_t r = j - D.nlead, round = D.k - 1 - (r >> 1);
    return resp + (((size_t)round * D.batch + b) * 2 + (r & 1)) * 16;
  };
  uint8_t *f = proof_files + dst * D.proof_bytes;
  for (uint32_t o = t; o < D.proof_bytes; o += 256) {
    uint8_t v = 0;
    if (o < 32 * nsc) {
      const uint32_t i = o >> 5;
      v = enc_be_byte(i < D.fn ? wn + (b * D.fn + i) * 8 : wl + (b * D.fl + (i - D.fn)) * 8, o & 31);
    } else if (o < 32 * nsc + ns) {
      const uint32_t s = o - 32 * nsc;
      for (uint32_t j = 8 * s; j < 8 * s + 8 && j < np; j++) v |= (uint8_t)(enc_sign(point(j)) << (j & 7));
    } else {
      const uint32_t r = o - 32 * nsc - ns;
      v = enc_be_byte(point(r >> 5), r & 31);
    }
    f[o] = v;
  }
}

// ---- a batch with refused proofs (bppp_rp_prove_batch_status_device): the accepted ones are proved in compact order
// slot s (one workgroup) takes the randomness prefix and the canonical public words of proof index[s]: prefix_out [n][prefix_len] bytes, pub_out
// [n][pub_words] (pub NULL or pub_words 0: none)
__global__ void __launch_bounds__(256) k_rp_gather_accepted(const uint32_t *__restrict__ index, const uint8_t *__restrict__ prefix, uint32_t prefix_len,
                                                            const uint32_t *__restrict__ pub, uint32_t pub_words, uint8_t *__restrict__ prefix_out,
                                                            uint32_t *__restrict__ pub_out) {
  const size_t s = blockIdx.x, src = index[s];
  for (uint32_t o = threadIdx.x; o < prefix_len; o += 256) prefix_out[s * prefix_len + o] = prefix[src * prefix_len + o];
  if (pub)
    for (uint32_t o = threadIdx.x; o < pub_words; o += 256) pub_out[s * pub_words + o] = pub[src * pub_words + o];
}
// the two files of every refused proof (one workgroup each, consecutive lanes on consecutive bytes) become zero bytes
__global__ void __launch_bounds__(256) k_rp_zero_files(const uint32_t *__restrict__ index, uint32_t coms_bytes, uint32_t proof_bytes, uint8_t *__restrict__ coms_files,
                                                       uint8_t *__restrict__ proof_files) {
  const size_t dst = index[blockIdx.x];
  for (uint32_t o = threadIdx.x; o < coms_bytes; o += 256) coms_files[dst * coms_bytes + o] = 0;
  for (uint32_t o = threadIdx.x; o < proof_bytes; o += 256) proof_files[dst * proof_bytes + o] = 0;
}

// ---- host side: the per-range data of a setup, uploaded once per handle
inline WitDims wit_dims(const bppp_rp *rp) {
  const bppp_rps::Setup &S = rp->st;
  WitDims D{};
  D.nr = (uint32_t)S.rds.size(); D.nlen = (uint32_t)S.nlen; D.nmss = S.kind == 0 ? (uint32_t)(S.llen - 6) : 0u;
  D.npub = S.kind == 0 && S.has_types ? (uint32_t)S.pubs.size() : 0u; D.has_types = S.has_types ? 1u : 0u; D.nlive = (uint32_t)S.nlive; D.conserve = S.conserve ? 1u : 0u;
  size_t nc = 0;
  for (const bppp_rps::RangeData &rd : S.rds) nc += rd.coeffs.size();
  D.coef_words = (uint32_t)(nc * 8);
  D.pub_words = S.kind == 0 ? D.npub * WP_WORDS : 8u;
  return D;
}
inline int wit_ensure_tables(bppp_rp *rp) {
  if (rp->d_wit) return BPPP_OK;
  bppp_ctx *ctx = rp->ctx;
  const bppp_rps::Setup &S = rp->st;
  const WitDims D = wit_dims(rp);
  std::vector<uint32_t> h((size_t)D.nr * WR_WORDS + D.coef_words + D.pub_words + 8, 0u);
  // offset of a shared base's multiplicities in mss: bases in sorted order, base b holds b - 1 counts (baseMss, TypedReciprocal.hs:363-370)
  auto moff = [&](uint32_t base) {
    uint32_t o = 0;
    for (uint32_t mb : S.m_bases) { if (mb >= base) break; o += mb - 1; }
    return o;
  };
  uint32_t *coefs = h.data() + (size_t)D.nr * WR_WORDS, *tail = coefs + D.coef_words;
  size_t c = 0;
  for (size_t i = 0; i < S.rds.size(); i++) {
    const bppp_rps::RangeData &rd = S.rds[i];
    uint32_t *R = h.data() + i * WR_WORDS;
    memcpy(R + WR_LO, rd.lo.w, 32); memcpy(R + WR_HI, rd.hi.w, 32);
    R[WR_BASE] = rd.base;
    R[WR_FLAGS] = (rd.shared ? WF_SHARED : 0u) | (rd.output ? WF_OUTPUT : 0u) | (rd.assumed ? WF_ASSUMED : 0u) | (rd.has_bit ? WF_BIT : 0u);
    R[WR_NCOEF] = (uint32_t)rd.coeffs.size(); R[WR_COEF] = (uint32_t)c; R[WR_POS] = (uint32_t)S.first_pos[i];
    if (S.kind == 0 && rd.shared && !rd.assumed) { R[WR_MOFF] = moff(rd.base); R[WR_MOFF2] = rd.has_bit ? moff(2) : 0u; }
    for (const bppp_host::U256 &cf : rd.coeffs) memcpy(coefs + 8 * c++, cf.w, 32);
  }
  if (S.kind == 0)
    for (uint32_t j = 0; j < D.npub; j++) {
      memcpy(tail + (size_t)j * WP_WORDS, S.pubs[j].type.w, 32); memcpy(tail + (size_t)j * WP_WORDS + 8, S.pubs[j].amount.w, 32);
      tail[(size_t)j * WP_WORDS + 16] = S.pubs[j].is_output ? 1u : 0u;
    }
  else memcpy(tail, S.net_public.w, 32);
  uint32_t *d = nullptr;
  BPPP_HIP(ctx, hipMalloc(&d, h.size() * 4));
  if (hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); return fail(ctx, BPPP_ERR_HIP, "rp_prove_batch_device: witness table upload"); }
  rp->d_wit = d;
  return BPPP_OK;
}

// the witness kernel of the handle's kind, queued on its stream.  Typed: dig / mul / mss as rpp_device_prove takes them; binary: `bits` [B][nlive]
// bytes (dig / mul / mss unused).  src_index: NULL, or B slots that read the proofs it lists (the kernels' comment)
inline int wit_launch(bppp_rp *rp, size_t B, const void *d_amounts, const void *d_types, const void *d_blinds, const uint32_t *d_pub, uint32_t *in_sc, uint32_t *dig,
                      uint32_t *mul, uint32_t *mss, uint8_t *bits, uint32_t *status, const uint32_t *src_index = nullptr) {
  bppp_ctx *ctx = rp->ctx;
  { int rc = wit_ensure_tables(rp); if (rc) return rc; }
  const WitDims D = wit_dims(rp);
  if (rp->st.kind == 1)
    k_brp_witness<<<dim3((unsigned)B), dim3(64), 0, ctx->stream>>>(D, rp->d_wit, (const uint32_t *)d_amounts, (const uint32_t *)d_blinds, d_pub, in_sc, bits, status, src_index);
  else
    k_rpp_witness<<<dim3((unsigned)B), dim3(64), 0, ctx->stream>>>(D, rp->d_wit, (const uint32_t *)d_amounts, (const uint32_t *)d_types, (const uint32_t *)d_blinds, d_pub,
                                                                  in_sc, dig, mul, mss, status, src_index);
  BPPP_HIP(ctx, hipGetLastError());
  return BPPP_OK;
}

}  // namespace bppp
