// rpprove.hip — batch prover of typed reciprocal range proofs: B proofs of one setup advance in lockstep.
//
// Replaces, with a leading batch dimension, proveM of RangeProof (src/RangeProof.hs:93-97):
//   proveTRRPM                      src/RangeProof/TypedReciprocal.hs:399-446  (phases 1-3: digits and multiplicities, reciprocals,
//                                   blinding — makePhase1s :133-161, makePhase2s :185-205, makeSharedCoeffs :213-216,
//                                   makeErrorTerms :226-243, makePublicConsts :246-274, makeBpCoeffs :391-396)
//   the blinding algebra            src/RangeProof/Internal.hs:118-196 (blindWitness, blindErrWitness, blindBlindingTerm)
//   commitRPW                       src/RangeProof/Internal.hs:45-50
//   proveBPM                        src/Bulletproof.hs:357-359 (the lockstep argument of csrc/nlb.hip)
//   encodeProof'                    src/RangeProof.hs:60-66, src/Encoding.hs:130-134
// Work split: every group operation is on the device — the input commitments through a fixed-base window table of (g, H0, H1)
// (k_rp_commit_inputs, csrc/rpcommit.hip: B x #ranges three-term commitments in one launch), the four range-proof commitments of all proofs as
// batched MSMs over the registered basis (2B, B, B instances of 1 + linLen + nrmLen terms; comb MSMs once the handle has its comb
// table, csrc/comb.hip), the argument through csrc/nlb.hip.  The per-proof field algebra (O(nrmLen) multiplications per phase) and
// the transcript hashing (the CLI's shaOracle and hashToScalar, app/Main.hs:64-87) run on the device (csrc/rpprove_dev.hip;
// prove_batch_host below keeps the first version of this file, with both on the host cores, for comparison); the host extracts
// the digits of the plain amounts, stages inputs in pinned memory and writes the files.  Large batches: two half-batches in flight.
#include <string.h>
#include <array>
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "ec.hip.h"
#include "comb.hpp"
#include "rp_internal.hpp"
#include "rpprove_dev.hpp"
#include "rpprove_host.hpp"
#include "sha256.hip.h"

using namespace bppp;
using namespace bppp_host;
using namespace bppp_rpp;


namespace bppp {
// the same oracle for the device prover's small batches (csrc/rpprove_dev.hip): `groups` / `npoints` are one proof's transcript so far,
// pts [m][8] its new commitments; out[count][4].  A host core hashes a 64by64 transcript in ~50 us; one GPU lane needs ~600 us.
void rpp_host_oracle(const std::string &tag, std::vector<std::string> &groups, size_t &npoints, const uint64_t *pts, size_t m, int count, uint64_t *out) {
  std::string g;
  g.reserve(m * 160);
  for (size_t i = 0; i < m; i++) point_text(g, pts + 8 * i);
  groups.push_back(std::move(g));
  npoints += m;
  for (int n = 1; n <= count; n++) {
    Sha256 h;
    const std::string hdr = tag + std::to_string(n) + std::to_string(npoints);
    h.update(hdr.data(), hdr.size());
    for (size_t k = groups.size(); k-- > 0;) h.update(groups[k].data(), groups[k].size());
    uint32_t d[8];
    h.finish(d);
    digest_to_fr(d).store(out + 4 * (n - 1));
  }
}
}  // namespace bppp
namespace {
// witnessTRRP (TypedReciprocal.hs:372-389) + makePhase1s (:133-161) + getDsMs (:74-80): fills d, mi, pv, ms_shared.  pub: NULL (the
// setup's public amounts) or this proof's [npub][4] canonical amounts (bppp_rp_prove_batch_pub)
bool make_witness(const Setup &st, PState &ps, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint64_t *pub) {
  const size_t nr = st.rds.size();
  // canonical types and blindings, balancing types, amounts in their ranges: one verdict (witness_status, csrc/rpsetup.hpp)
  if (const uint32_t refusal = bppp_rps::witness_status(st, amounts, types, blinds, pub)) { ps.err = bppp_rps::wit_status_text(refusal); return false; }
  ps.v.resize(nr); ps.ty.resize(nr); ps.bl.resize(nr);
  std::vector<U256> amt(nr);
  for (size_t i = 0; i < nr; i++) {
    amt[i] = U256::load(amounts + 4 * i);
    ps.v[i] = bppp_rps::s_mod_n(amt[i]); ps.ty[i] = U256::load(types + 4 * i); ps.bl[i] = U256::load(blinds + 4 * i);
  }
  ps.d.assign(st.nlen, U256::zero()); ps.mi.assign(st.nlen, U256::zero()); ps.pv.assign(st.nlen, U256::one());
  // the shared multiplicities are counts of digits: summed as integers (64 ranges x 255 digit values of modular additions per proof were most of
  // this function's time), converted once at the end
  std::vector<uint32_t> &msc = ps.tmp_msc;
  msc.assign(st.llen - 6, 0u);
  std::vector<size_t> base_off(st.m_bases.size(), 0);
  for (size_t k = 1; k < st.m_bases.size(); k++) base_off[k] = base_off[k - 1] + st.m_bases[k - 1] - 1;
  auto moff = [&](uint32_t base) { size_t k = std::lower_bound(st.m_bases.begin(), st.m_bases.end(), base) - st.m_bases.begin(); return base_off[k]; };
  size_t p = 0;
  if (st.has_types)
    for (size_t i = 0; i < nr; i++, p++) { ps.d[p] = ps.ty[i]; ps.pv[p] = ps.v[i]; }
  for (size_t i = 0; i < nr; i++) {
    const RangeData &rd = st.rds[i];
    if (rd.assumed) continue;
    std::vector<uint32_t> &ds = ps.tmp_ds, &cnt = ps.tmp_cnt, &ms = ps.tmp_ms;       // reused across ranges and proofs
    bppp_rps::digits_into(rd, bppp_rps::u_sub(amt[i], rd.lo), ds);
    const uint32_t b = rd.base;
    const size_t p0 = st.first_pos[i];
    if (rd.shared) {
      // the digits go to their positions; their multiplicities to the shared table of this base (baseMss, :363-370; the bit's to base 2), one
      // count per non-zero digit (ms aligned with ns = [1 | hasBit] ++ [1 .. b-1], :141-145)
      for (size_t j = 0; j < ds.size(); j++) ps.d[p0 + j] = small(ds[j]);
      if (rd.has_bit) msc[moff(2)] += ds[0];
      const size_t o = moff(b);
      for (size_t j = rd.has_bit ? 1 : 0; j < ds.size(); j++) if (ds[j]) msc[o + ds[j] - 1]++;
    } else {
      // ms aligned with ns = [1 | hasBit] ++ [1 .. b-1]: the bit itself, then how often each non-zero digit value occurs (:141-145)
      cnt.assign(b, 0);
      for (size_t j = rd.has_bit ? 1 : 0; j < ds.size(); j++) cnt[ds[j]]++;
      ms.clear();
      if (rd.has_bit) ms.push_back(ds[0]);
      for (uint32_t s = 1; s < b; s++) ms.push_back(cnt[s]);
      const size_t ln = std::max(ds.size(), ms.size());
      for (size_t j = 0; j < ln; j++) {
        if (j < ds.size()) ps.d[p0 + j] = small(ds[j]);
        if (j < ms.size()) ps.mi[p0 + j] = small(ms[j]);
      }
    }
  }
  ps.ms_shared.resize(st.llen - 6);
  for (size_t j = 0; j < msc.size(); j++) ps.ms_shared[j] = small(msc[j]);
  return true;
}

// blindWitness n = 3 (src/RangeProof/Internal.hs:130-139): five fresh scalars with one zero slot, 7 blinding entries in all
RPW blind_witness(int k, const std::vector<U256> &ls, const std::vector<U256> &ns, Rnd &rnd, size_t llen) {
  U256 b[7];
  for (int i = 0; i < 7; i++) b[i] = U256::zero();
  const int zero_at = 2 * 3 - k;                           // insertAt (2n - k) 0
  int j = 0;
  for (int i = 0; i < 5; i++, j++) { if (j == zero_at) j++; b[j] = rnd.next(); }
  RPW w;
  w.sc = b[0];
  w.lin.assign(llen, U256::zero());
  for (int i = 0; i < 6; i++) w.lin[i] = b[1 + i];
  for (size_t i = 0; i < ls.size(); i++) w.lin[6 + i] = ls[i];
  w.nrm = ns;
  return w;
}
// blindErrWitness n = 3 (:142-149): [a, b, c, 0, d] ++ es, padded to 7
RPW blind_err_witness(const U256 &err7, const std::vector<U256> &ns, Rnd &rnd, size_t llen) {
  U256 b[7];
  for (int i = 0; i < 7; i++) b[i] = U256::zero();
  b[0] = rnd.next(); b[1] = rnd.next(); b[2] = rnd.next(); b[4] = rnd.next(); b[5] = err7;
  RPW w;
  w.sc = b[0];
  w.lin.assign(llen, U256::zero());
  for (int i = 0; i < 6; i++) w.lin[i] = b[1 + i];
  w.nrm = ns;
  return w;
}

// makeBaseMap: sortedBases zipped with x^3, x^5, ... (TypedReciprocal.hs:349)
std::vector<U256> base_map(const Setup &st, const U256 &x) {
  std::vector<U256> out(st.sorted_bases.size());
  U256 c = fm(fm(x, x), x), xx = fm(x, x);
  for (size_t k = 0; k < out.size(); k++) { out[k] = c; c = fm(c, xx); }
  return out;
}

// makePhase2s with the private fields (TypedReciprocal.hs:185-205)
void make_phase2(const Setup &st, PState &ps) {
  const size_t n = st.nlen;
  const std::vector<U256> bm = base_map(st, ps.x);
  const U256 xx = fm(ps.x, ps.x);
  std::vector<U256> xpow(st.rds.size());
  { U256 c = xx; for (size_t j = 0; j < xpow.size(); j++) { xpow[j] = c; c = fm(c, xx); } }     // x^(2 (j + 1))
  ps.u.resize(n); ps.vv.resize(n); ps.rr.resize(n); ps.cc.resize(n);
  std::vector<U256> dens(n), ss(n);
  for (size_t i = 0; i < n; i++) {
    const Pos &p = st.pos[i];
    const uint32_t kind = p.kind & 0xFFu;
    const U256 &xi = xpow[p.range];
    dens[i] = fa(ps.e, ps.d[i]);
    ss[i] = U256::zero();
    if (kind == bppp_rps::POS_TYPING) {
      ps.vv[i] = (p.kind & bppp_rps::POS_F_IO) ? fneg(ps.x) : ps.x;
      ps.u[i] = (p.kind & bppp_rps::POS_F_IA) ? U256::zero() : xi;
    } else {
      ps.vv[i] = bm[st.slot_of(p.radix)];
      ps.u[i] = fm(xi, p.coeff);
      if (kind == bppp_rps::POS_INLINE && p.sym_small) ss[i] = fa(ps.e, small(p.sym_small));
    }
  }
  batch_inv(dens); batch_inv(ss);
  for (size_t i = 0; i < n; i++) {
    ps.rr[i] = fm(ps.pv[i], dens[i]);
    ps.cc[i] = ss[i].is_zero() ? U256::zero() : fm(ps.vv[i], fs(ps.e_inv, ss[i]));
  }
}

// makeSharedCoeffs (:213-216)
std::vector<U256> make_shared_coeffs(const Setup &st, const PState &ps) {
  const std::vector<U256> bm = base_map(st, ps.x);
  std::vector<U256> xs, ss;
  for (uint32_t b : st.m_bases)
    for (uint32_t s = 1; s < b; s++) { xs.push_back(bm[st.slot_of(b)]); ss.push_back(fa(ps.e, small(s))); }
  batch_inv(ss);
  for (size_t i = 0; i < xs.size(); i++) xs[i] = fm(xs[i], fs(ps.e_inv, ss[i]));
  return xs;
}

// inputCoeffs (:325-328)
std::vector<U256> input_coeffs(const Setup &st, const U256 &x, const U256 &q0) {
  const size_t nr = st.rds.size();
  std::vector<U256> out(nr);
  const U256 xx = fm(x, x);
  U256 xp = xx, qp = q0;
  for (size_t i = 0; i < nr; i++) {
    U256 c = st.rds[i].assumed ? U256::zero() : xp;
    if (st.has_types) c = fa(c, qp);
    out[i] = c;
    xp = fm(xp, xx); qp = fm(qp, q0);
  }
  return out;
}

// makeErrorTerms (:226-243) with q2 = q0^(i+1), bl = the norm blinding of position i
void make_error_terms(const Setup &st, const PState &ps, const std::vector<U256> &bls_ms, const std::vector<U256> &bls_nrm, U256 tot[6]) {
  for (int k = 0; k < 6; k++) tot[k] = U256::zero();
  U256 s3 = U256::zero();
  for (size_t i = 0; i < ps.shared_cs.size(); i++) s3 = fa(s3, fm(ps.shared_cs[i], bls_ms[i]));
  tot[3] = fdbl(s3);
  U256 q2 = ps.q0;
  for (size_t i = 0; i < st.nlen; i++) {
    const bool is_t = (st.pos[i].kind & 0xFFu) == bppp_rps::POS_TYPING;
    const U256 &d = ps.d[i], &m = ps.mi[i], &u = ps.u[i], &v = ps.vv[i], &r = ps.rr[i], &c = ps.cc[i], &bl = bls_nrm[i];
    const U256 rC = is_t ? fm(ps.xp, fa(u, q2)) : u;
    const U256 dC = fa(v, fm(q2, ps.e));
    const U256 q2d_dC = fa(fm(q2, d), dC), q2r_rC = fa(fm(q2, r), rC), q2bl = fm(q2, bl), q2m = fm(q2, m);
    tot[0] = fa(tot[0], fm(q2bl, bl));
    tot[1] = fa(tot[1], fdbl(fm(q2m, bl)));
    tot[2] = fa(tot[2], fa(fm(q2m, m), fdbl(fm(bl, q2d_dC))));
    tot[3] = fa(tot[3], fdbl(fa(fm(bl, q2r_rC), fm(m, q2d_dC))));
    tot[4] = fa(tot[4], fa(fa(fm(fm(q2, d), d), fdbl(fm(d, dC))), fdbl(fa(fm(bl, c), fm(m, q2r_rC)))));
    tot[5] = fa(tot[5], fa(fa(fm(fm(q2, r), r), fdbl(fm(r, rC))), fdbl(fm(c, d))));
    q2 = fm(q2, ps.q0);
  }
}

// blindBlindingTerm for three earlier witnesses [mWit, dmWit, rWit] (src/RangeProof/Internal.hs:154-196)
RPW blind_blinding_term(const std::vector<U256> &bls_lin, const std::vector<U256> &bls_nrm, const U256 &tC, const PState &ps, const U256 errs[6],
                        const U256 &input_bl, size_t llen) {
  const int n = 3;
  const U256 blT = bls_lin[0];
  const U256 rs_inv = fm(ps.r0_inv, ps.r1_inv);
  // rows: [sc] ++ the first 2n linear entries; the error witness keeps only n + 1 of them (the rest zero)
  U256 rows[3][7];
  const RPW *w1[2] = {&ps.m, &ps.dm};
  for (int a = 0; a < 2; a++) { rows[a][0] = w1[a]->sc; for (int j = 0; j < 6; j++) rows[a][1 + j] = w1[a]->lin[j]; }
  rows[2][0] = ps.r.sc;
  for (int j = 0; j < 6; j++) rows[2][1 + j] = j < n + 1 ? ps.r.lin[j] : U256::zero();
  for (int a = 0; a < 3; a++) for (int j = 2; j < 7; j++) rows[a][j] = fneg(rows[a][j]);
  // errs1 = negate ([errs0 - tC blT] ++ rs_inv * errs[1..])
  U256 table[4][7];
  U256 e1[6];
  e1[0] = fneg(fs(errs[0], fm(tC, blT)));
  for (int j = 1; j < 6; j++) e1[j] = fneg(fm(rs_inv, errs[j]));
  auto scale_errs = [&](U256 *xs6, const U256 &s) { xs6[n + 1] = fm(s, xs6[n + 1]); };     // scaleErrs (:118-121): only entry n + 1 of six
  auto ins = [&](U256 *dst7, const U256 *src6) { for (int j = 0; j < 5; j++) dst7[j] = src6[j]; dst7[5] = U256::zero(); dst7[6] = src6[5]; };   // insertAt (2n - 1) 0
  ins(table[0], e1);
  for (int a = 0; a < 3; a++) {
    U256 r6[6];
    r6[0] = fa(fm(rs_inv, rows[a][0]), fm(fm(rs_inv, tC), rows[a][1]));                      // addConsts
    for (int j = 1; j < 6; j++) r6[j] = rows[a][j + 1];
    scale_errs(r6, ps.r1_inv);
    ins(table[1 + a], r6);
  }
  U256 diag[10];
  for (int k = 0; k < 10; k++) diag[k] = U256::zero();
  for (int a = 0; a < 4; a++) for (int b = 0; b < 7; b++) diag[a + b] = fa(diag[a + b], table[a][b]);     // sumDiagonals (:104-111)
  U256 be[6];
  for (int k = 0, j = 0; k < 7 && j < 6; k++) { if (k == 5) continue; be[j++] = diag[k]; }              // removeAt (2n - 1), take 2n
  scale_errs(be, ps.r1);
  be[5] = fs(be[5], fdbl(input_bl));
  RPW w;
  w.sc = fneg(be[0]);
  w.lin.assign(llen, U256::zero());
  w.lin[0] = blT;
  for (int j = 1; j < 6; j++) w.lin[j] = be[j];
  for (size_t j = 1; j < bls_lin.size(); j++) w.lin[5 + j] = bls_lin[j];
  w.nrm = bls_nrm;
  return w;
}

// makePublicConsts (TypedReciprocal.hs:246-274): returns sc and the norm vector.  pub as for make_witness
void make_public_consts(const Setup &st, const PState &ps, U256 &sc, std::vector<U256> &nrm, const uint64_t *pub) {
  const U256 t2 = fm(ps.t, ps.t), t3 = fm(t2, ps.t), t4 = fm(t2, t2), t5 = fm(t4, ps.t), two_t5 = fdbl(t5);
  const U256 xx = fm(ps.x, ps.x);
  U256 z = U256::zero();
  { U256 xp = xx;
    for (size_t j = 0; j < st.rds.size(); j++) { if (!st.rds[j].assumed) z = fa(z, fm(bppp_rps::s_mod_n(st.rds[j].lo), xp)); xp = fm(xp, xx); } }
  z = fneg(fm(two_t5, z));
  if (st.has_types) {
    std::vector<U256> pr(st.pubs.size());
    for (size_t j = 0; j < pr.size(); j++) pr[j] = fa(ps.e, st.pubs[j].type);
    batch_inv(pr);
    U256 sum = U256::zero();
    for (size_t j = 0; j < pr.size(); j++) {
      const U256 rv = fm(pr[j], pub ? U256::load(pub + 4 * j) : st.pubs[j].amount);
      sum = st.pubs[j].is_output ? fs(sum, rv) : fa(sum, rv);
    }
    z = fs(z, fm(fm(two_t5, ps.x), sum));
  }
  nrm.resize(st.nlen);
  U256 q2 = ps.q0, qi2 = ps.q0_inv, acc = U256::zero();
  for (size_t i = 0; i < st.nlen; i++) {
    const bool is_t = (st.pos[i].kind & 0xFFu) == bppp_rps::POS_TYPING;
    U256 rC, p2C;
    if (is_t) { rC = fm(ps.xp, fa(fm(qi2, ps.u[i]), U256::one())); p2C = U256::zero(); }
    else { rC = fm(qi2, ps.u[i]); p2C = fa(fdbl(q2), fdbl(fm(ps.e_inv, ps.vv[i]))); }
    const U256 pv = fa(fa(fm(t2, fa(ps.e, fm(qi2, ps.vv[i]))), fm(t3, rC)), fm(t4, fm(qi2, ps.cc[i])));
    acc = fa(acc, fa(fm(q2, fm(pv, pv)), fm(t5, p2C)));
    nrm[i] = pv;
    q2 = fm(q2, ps.q0); qi2 = fm(qi2, ps.q0_inv);
  }
  sc = fa(z, acc);
}

int ensure_pwork(bppp_rp *rp, size_t bytes) {
  if (bytes <= rp->pwork_bytes) return BPPP_OK;
  bppp_ctx *ctx = rp->ctx;
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (rp->pwork) BPPP_HIP(ctx, hipFree(rp->pwork));
  rp->pwork = nullptr; rp->pwork_bytes = 0;
  BPPP_HIP(ctx, hipMalloc(&rp->pwork, bytes + bytes / 8));
  rp->pwork_bytes = bytes + bytes / 8;
  return BPPP_OK;
}

}  // namespace

namespace bppp {
int rpp_ensure_pwork(bppp_rp *rp, size_t bytes) { return ensure_pwork(rp, bytes); }
int rpp_ensure_hpin(bppp_rp *rp, size_t bytes) {
  if (bytes <= rp->hpin_bytes) return BPPP_OK;
  bppp_ctx *ctx = rp->ctx;
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (rp->hpin) BPPP_HIP(ctx, hipHostFree(rp->hpin));
  rp->hpin = nullptr; rp->hpin_bytes = 0;
  BPPP_HIP(ctx, hipHostMalloc(&rp->hpin, bytes + bytes / 8, hipHostMallocDefault));
  rp->hpin_bytes = bytes + bytes / 8;
  return BPPP_OK;
}
void rpp_encode_files(const bppp_rp *rp, size_t B, const uint64_t *in_pt, const uint64_t *wn, const uint64_t *wl, std::initializer_list<const uint64_t *> lead,
                      const uint64_t *resp, uint8_t *coms_files, uint8_t *proof_files) {
  const Setup &st = rp->st;
  const RpDims &D = rp->D;
  const size_t nr = st.rds.size(), k = st.rounds;
  rp_parallel(B, [&](size_t lo, size_t hi) {
    std::vector<const uint64_t *> pts;
    for (size_t b = lo; b < hi; b++) {
      pts.assign(nr, nullptr);
      for (size_t i = 0; i < nr; i++) pts[i] = in_pt + (b * nr + i) * 8;
      encode_points(coms_files + b * D.coms_bytes, pts.data(), nr);
      uint8_t *pf = proof_files + b * D.proof_bytes;
      for (size_t i = 0; i < st.fn; i++) put_field(pf + 32 * i, U256::load(wn + (b * st.fn + i) * 4));
      for (size_t i = 0; i < st.fl; i++) put_field(pf + 32 * (st.fn + i), U256::load(wl + (b * st.fl + i) * 4));
      pts.clear();
      for (const uint64_t *c : lead) pts.push_back(c + 8 * b);
      for (size_t j = 0; j < 2 * k; j++) pts.push_back(resp + (b * k) * 16 + 8 * j);
      encode_points(pf + 32 * (st.fn + st.fl), pts.data(), pts.size());
    }
  });
}
int rpp_commit_rows(bppp_rp *rp, const uint32_t *d_rows, size_t nrows, uint64_t *host_out) {
  if (!rp->comb) return bppp_msm_basis(rp->commit_basis, d_rows, 1 + rp->st.llen + rp->st.nlen, nrows, host_out);
  bppp_ctx *ctx = rp->ctx;
  if (nrows > rp->comb_out_rows) {
    BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rp->d_comb_out) BPPP_HIP(ctx, hipFree(rp->d_comb_out));
    rp->d_comb_out = nullptr; rp->comb_out_rows = 0;
    BPPP_HIP(ctx, hipMalloc(&rp->d_comb_out, nrows * 64));
    rp->comb_out_rows = nrows;
  }
  int rc = comb_msm(rp->comb, d_rows, nrows, rp->d_comb_out, ctx->stream, COMB_ROWS_ANY, 1 + rp->st.llen + rp->st.nlen);      // one wavefront per instance (the fold route's small batches); the handle's own row length: the table may be a longer basis's
  if (rc) return fail(ctx, rc, bppp_last_error(rp->comb->ctx));
  BPPP_HIP(ctx, hipMemcpyAsync(host_out, rp->d_comb_out, nrows * 64, hipMemcpyDeviceToHost, ctx->stream));
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return BPPP_OK;
}
}  // namespace bppp

// the comb table of the setup's basis, built at the first large batch: the widest window (<= 18 bits) whose table fits the budget —
// 32 GB by default, BPPP_RP_COMB_GB to change it: 27.6 GB at 774 points (c = 16, built in ~0.3 s), 4.1 GB at c = 13 costs ~15 % more
// additions; BPPP_RP_COMB_BITS forces a width, BPPP_RP_NO_COMB keeps the bucket route
int rp_ensure_comb(bppp_rp *rp) {
  if (rp->comb || rp->opt.no_comb || rp->comb_failed) return BPPP_OK;
  // the table is a persistent allocation of tens of GB: never more than the handle's budget, and never more than half of what is
  // free on the device right now (other handles, other processes on the same GPU); a forced width (comb_bits) skips the budget
  size_t budget = rp->opt.comb_budget, free_b = 0, total_b = 0;
  hipSetDevice(rp->ctx->device);
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, free_b / 2);
  else (void)hipGetLastError();
  int rc = bppp::comb_create(rp->ctx, rp->d_basis, 1 + rp->st.llen + rp->st.nlen, rp->opt.comb_bits, budget, &rp->comb);
  if (rc) {                                  // no room for the table (or no window fits the budget): the bucket route and the point-folding
    rp->comb = nullptr; rp->comb_failed = true;   // argument serve the batch; the reason stays in bppp_last_error, the attempt is not repeated
    (void)hipGetLastError();                 // a failed hipMalloc leaves its error in the runtime's last-error slot: later launch checks must not see it
    return BPPP_OK;
  }
  rp_set_comb(rp->twin, rp->comb);
  return BPPP_OK;
}

void rp_set_comb(bppp_rp *rp, bppp::CombTable *t) {
  if (!rp) return;
  if (rp->comb != t) {
    if (t) { bppp::comb_retain(t); if (rp->is_twin) t->twins++; }
    if (rp->comb) { if (rp->is_twin) rp->comb->twins--; bppp::comb_release(rp->comb); }
    rp->comb = t;
  }
  rp_set_comb(rp->twin, t);
}

static int prove_batch_host(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint8_t *rand_prefix,
                            size_t prefix_len, uint8_t *coms_files, uint8_t *proof_files, size_t index_base, const uint64_t *pub);

static int prove_batch_one(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint8_t *rand_prefix,
                           size_t prefix_len, uint8_t *coms_files, uint8_t *proof_files, size_t index_base, const uint64_t *pub);

// A large batch runs as TWO half-batches in flight, the second on a twin handle with its own context (stream, workspaces) from a host
// thread: the proofs are independent, and the host shares of a half (digits, the argument's half-GCDs and round bookkeeping, the challenge
// round trips) fall under the kernels of the other.  Same bytes out as one batch (tests).  half(h, b0, n) proves proofs [b0, b0 + n) of the
// batch on handle h, naming them from b0 in its errors; a batch below split_min (or on a twin, or with no_split) is one half.
template <class F> static int prove_halves(bppp_rp *rp, size_t batch, size_t split_min, F half) {
  if (batch < split_min || batch < 2 || rp->is_twin || rp->opt.no_split) return half(rp, 0, batch);
  { int rc = rp_ensure_twin(rp); if (rc) return rc; }
  rp_set_comb(rp->twin, rp->comb);                                 // one more holder of the same table
  rp->twin->opt = rp->opt;
  const size_t B0 = (batch + 1) / 2;
  rp->twin->pre_inputs = rp->pre_inputs ? rp->pre_inputs + B0 * rp->st.rds.size() * 16 : nullptr;
  const RpBind whole = rp->bind;                                   // a bound call: the second half starts at its own binding
  rp->twin->bind = whole.from(B0, batch - B0); rp->bind = whole.from(0, B0);
  int rc1 = BPPP_OK;
  std::thread second([&] { rc1 = half(rp->twin, B0, batch - B0); });
  const int rc0 = half(rp, 0, B0);
  second.join();
  rp->twin->pre_inputs = nullptr;
  rp->twin->bind = RpBind(); rp->bind = whole;
  if (rc0) return rc0;
  if (rc1) return fail(rp->ctx, rc1, bppp_last_error(rp->twin_ctx));
  return BPPP_OK;
}

extern "C" int bppp_rp_prove_batch(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint8_t *rand_prefix,
                                   size_t prefix_len, uint8_t *coms_files, uint8_t *proof_files) {
  return bppp_rp_prove_batch_pub(rp, batch, amounts, types, blinds, nullptr, rand_prefix, prefix_len, coms_files, proof_files);
}

// shapes the device algebra does not serve: it looks digits up in a per-proof table of reciprocals held in LDS (16 entries, up to 1024 for wider digit
// bases) beside one entry per range.  A setup whose phase kernels would not fit a workgroup's LDS (the planning functions of csrc/rpprove_dev.hpp, which
// size the launches too), and a wide table with many ranges, take the host-algebra path (prove_batch_one): the same bytes
static bool lds_gate(const Setup &st) {
  return !rpp_phases_fit_lds(st) || (rpp_maxb(st) > 256 && st.rds.size() > 256);
}
// bppp_rp_prove_batch_device: does this call run as one stream of kernels over the handle's comb table (csrc/rpprove_dev.hip, csrc/brpprove_dev.hip)?
// Otherwise its inputs come down and the host-buffer routes below serve it.
static bool has_device_stream(const bppp_rp *rp) {
  return rp->comb && !rp->opt.host_algebra && !rp->opt.fold_points && (rp->st.kind == 1 || !lds_gate(rp->st));
}

// bppp_rp_prove_batch_pub (device = false: every buffer on the host) and bppp_rp_prove_batch_device (device = true: every buffer in HBM); with
// per_proof, their *_status forms: proof_status [batch] on the host takes every proof's verdict, a refused proof's files are zeroed and the rest is
// proved — on a route with a device stream inside each half (csrc/rpwitness.hip), elsewhere here: the accepted proofs' rows are compacted on the
// host, the route below proves them as a batch of its own, and their files are scattered back
// bindings: NULL, or the bppp_rp_prove_bound* entry points' [batch][32] bytes (host / HBM as the other buffers): proof b hashes under tag <> binding_b
static int prove_entry(bppp_rp *rp, size_t batch, const void *amounts_, const void *types_, const void *blinds_, const void *public_amounts, const void *rand_prefix_,
                       size_t prefix_len, void *coms_files_, void *proof_files_, bool device, bool per_proof = false, uint32_t *proof_status = nullptr,
                       const void *bindings = nullptr) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (ctx_closed(ctx)) return BPPP_ERR_ARG;
  if (!batch) return BPPP_OK;
  if (per_proof && !proof_status) return fail(ctx, BPPP_ERR_ARG, "rp_prove_batch_status: proof_status is NULL");
  const uint64_t *amounts = (const uint64_t *)amounts_, *types = (const uint64_t *)types_, *blinds = (const uint64_t *)blinds_;
  const uint8_t *rand_prefix = (const uint8_t *)rand_prefix_;
  uint8_t *coms_files = (uint8_t *)coms_files_, *proof_files = (uint8_t *)proof_files_;
  if (!amounts || (!types && rp->st.kind == 0) || !blinds || (prefix_len && !rand_prefix) || !coms_files || !proof_files || batch >= (1u << 20) || prefix_len > 4096)
    return fail(ctx, BPPP_ERR_ARG, "rp_prove_batch: bad arguments");
  RpBindGuard guard{rp};
  { int rc = rp_bind_begin(rp, bindings, device, batch, "rp_prove_bound"); if (rc) return rc; }
  const size_t npub = rp_public_count(rp);
  std::vector<uint64_t> canon;                  // per-proof public amounts as canonical scalars: what a handle created with them holds
  if (public_amounts) {
    std::vector<uint64_t> raw;
    if (device && npub) {                       // read back and checked on the host, as the verifier's *_pub_device entry points do
      hipSetDevice(ctx->device);
      raw.resize(batch * npub * 4);
      BPPP_HIP(ctx, hipMemcpyAsync(raw.data(), public_amounts, raw.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
      BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    int rc = rp_public_canon(rp, batch, device ? raw.data() : (const uint64_t *)public_amounts, canon); if (rc) return rc;
  }
  const uint64_t *pub = public_amounts ? canon.data() : nullptr;
  auto pub_at = [&](size_t b0) -> const uint64_t * { return pub ? pub + 4 * npub * b0 : nullptr; };
  const size_t comb_min = rp->opt.comb_min;     // default 1024: the table costs ~0.3 s and tens of GB once: worth it for a handle that proves large batches
  // ... or one that has proved that many proofs in smaller batches: with the table in place every batch size is faster (one 64by64 proof:
  // 12 ms against 22 ms; 256: 22 against 48)
  if (!rp->is_twin && !rp->opt.host_algebra) {
    rp->proved_total += batch;
    if (batch >= comb_min || rp->proved_total >= comb_min) { int rc = rp_ensure_comb(rp); if (rc) return rc; }
  }
  const size_t nr = rp->st.rds.size(), cb = rp->D.coms_bytes, pb = rp->D.proof_bytes;
  // the slow path of the device entry point — a route without a device stream: the inputs come down, the host-buffer route proves, the files go up
  std::vector<uint64_t> h_amounts, h_types, h_blinds;
  std::vector<uint8_t> h_prefix, h_coms, h_proofs;
  uint8_t *d_coms_out = nullptr, *d_proofs_out = nullptr;
  if (device && !has_device_stream(rp)) {
    hipSetDevice(ctx->device);
    h_amounts.resize(batch * nr * 4); h_blinds.resize(batch * nr * 4); h_types.resize(types ? batch * nr * 4 : 0); h_prefix.resize(batch * prefix_len);
    h_coms.resize(batch * cb); h_proofs.resize(batch * pb);
    BPPP_HIP(ctx, hipMemcpyAsync(h_amounts.data(), amounts, h_amounts.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    BPPP_HIP(ctx, hipMemcpyAsync(h_blinds.data(), blinds, h_blinds.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (types) BPPP_HIP(ctx, hipMemcpyAsync(h_types.data(), types, h_types.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (prefix_len) BPPP_HIP(ctx, hipMemcpyAsync(h_prefix.data(), rand_prefix, h_prefix.size(), hipMemcpyDeviceToHost, ctx->stream));
    BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    amounts = h_amounts.data(); blinds = h_blinds.data(); types = types ? h_types.data() : nullptr; rand_prefix = prefix_len ? h_prefix.data() : nullptr;
    d_coms_out = coms_files; d_proofs_out = proof_files;
    coms_files = h_coms.data(); proof_files = h_proofs.data();
    device = false;
  }
  // proofs [b0, b0 + n) of the caller's arrays (prove_halves)
  auto prefix_at = [&](size_t b0) { return rand_prefix ? rand_prefix + prefix_len * b0 : nullptr; };
  auto device_half = [&](bppp_rp *h, size_t b0, size_t n) {
    return rp_prove_device_half(h, n, amounts + 4 * nr * b0, types ? types + 4 * nr * b0 : nullptr, blinds + 4 * nr * b0, pub_at(b0), prefix_at(b0), prefix_len,
                                coms_files + cb * b0, proof_files + pb * b0, b0, proof_status ? proof_status + b0 : nullptr);
  };
  auto routes = [&]() -> int {
    // RangeProof.Binary: with the comb table in place the whole proof is a stream of kernels (csrc/brpprove_dev.hip); before that (small
    // batches) and under BPPP_RP_HOST_ALGEBRA the field algebra and the hashing run on the host cores (prove_batch_binary)
    if (rp->st.kind == 1) {
      // two half-batches in flight (as below for the typed-reciprocal proofs): the transcript hashing, the phase and the round kernels of one half —
      // ~14 ms per 1024 proofs of mostly one-lane-per-proof chains — run under the comb additions of the other
      if (device) return prove_halves(rp, batch, rp->opt.split_min_binary, device_half);
      if (rp->comb && !rp->opt.host_algebra && !rp->opt.fold_points)
        return prove_halves(rp, batch, rp->opt.split_min_binary, [&](bppp_rp *h, size_t b0, size_t n) {
          return prove_batch_binary_dev(h, n, amounts + 4 * nr * b0, blinds + 4 * nr * b0, prefix_at(b0), prefix_len, coms_files + cb * b0, proof_files + pb * b0, b0,
                                        pub_at(b0));
        });
      return prove_batch_binary(rp, batch, amounts, blinds, rand_prefix, prefix_len, coms_files, proof_files, pub);
    }
    // inner-product flavour without a table: the range-proof phases with their field algebra on the host cores, then the lockstep argument of
    // ip_argument_lockstep (no basis change, no point fold: every commitment an MSM over the registered original basis)
    if (rp->st.flavour != 0 && (!rp->comb || rp->opt.fold_points))
      return prove_batch_host(rp, batch, amounts, types, blinds, rand_prefix, prefix_len, coms_files, proof_files, 0, pub);
    // split_min: default 4096; measured: 4096 proofs 91-93 ms split against 95-97 ms, but 2048 proofs (128by64) 109 ms split against 104 ms
    if (device) return prove_halves(rp, batch, rp->opt.split_min, device_half);
    return prove_halves(rp, batch, rp->opt.split_min, [&](bppp_rp *h, size_t b0, size_t n) {
      return prove_batch_one(h, n, amounts + 4 * nr * b0, types + 4 * nr * b0, blinds + 4 * nr * b0, prefix_at(b0), prefix_len, coms_files + cb * b0,
                             proof_files + pb * b0, b0, pub_at(b0));
    });
  };
  // per-proof verdicts on host buffers (a device stream takes them from its witness kernel): the refused proofs leave the batch before its route sees it
  std::vector<uint64_t> a_amounts, a_types, a_blinds, a_pub;
  std::vector<uint8_t> a_prefix, a_coms, a_proofs, a_bind;
  std::vector<size_t> accepted;
  const size_t submitted = batch;
  uint8_t *const all_coms = coms_files, *const all_proofs = proof_files;
  if (proof_status && !device) {
    rp_parallel(batch, [&](size_t lo, size_t hi) {
      for (size_t b = lo; b < hi; b++) proof_status[b] = bppp_rps::witness_status(rp->st, amounts + 4 * nr * b, types ? types + 4 * nr * b : nullptr, blinds + 4 * nr * b, pub_at(b));
    });
    for (size_t b = 0; b < batch; b++) if (proof_status[b] == bppp_rps::WIT_OK) accepted.push_back(b);
    if (accepted.size() < batch) {
      const size_t G = accepted.size();
      a_amounts.resize(G * nr * 4); a_blinds.resize(G * nr * 4); a_types.resize(types ? G * nr * 4 : 0); a_pub.resize(pub ? G * npub * 4 : 0);
      a_prefix.resize(G * prefix_len); a_coms.resize(G * cb); a_proofs.resize(G * pb);
      if (rp->bind.on()) { int rcb = rp_bind_host(rp); if (rcb) return rcb; a_bind.resize(G * RP_BINDING_BYTES); }      // the accepted proofs' bindings move with them
      for (size_t s = 0; s < G; s++) {
        const size_t b = accepted[s];
        if (!a_bind.empty()) memcpy(&a_bind[s * RP_BINDING_BYTES], rp->bind.h + b * RP_BINDING_BYTES, RP_BINDING_BYTES);
        memcpy(&a_amounts[s * nr * 4], amounts + 4 * nr * b, nr * 32); memcpy(&a_blinds[s * nr * 4], blinds + 4 * nr * b, nr * 32);
        if (types) memcpy(&a_types[s * nr * 4], types + 4 * nr * b, nr * 32);
        if (pub && npub) memcpy(&a_pub[s * npub * 4], pub + 4 * npub * b, npub * 32);
        if (prefix_len) memcpy(&a_prefix[s * prefix_len], rand_prefix + prefix_len * b, prefix_len);
      }
      amounts = a_amounts.data(); blinds = a_blinds.data(); types = types ? a_types.data() : nullptr; rand_prefix = prefix_len ? a_prefix.data() : nullptr;
      if (pub) pub = a_pub.data();
      coms_files = a_coms.data(); proof_files = a_proofs.data();
      if (!a_bind.empty()) { rp->bind = RpBind(); rp->bind.h = a_bind.data(); rp->bind.n = G; }
      batch = G;
    }
  }
  const int rc = batch ? routes() : BPPP_OK;
  if (!rc && batch < submitted) {
    memset(all_coms, 0, submitted * cb); memset(all_proofs, 0, submitted * pb);
    for (size_t s = 0; s < batch; s++) { memcpy(all_coms + accepted[s] * cb, &a_coms[s * cb], cb); memcpy(all_proofs + accepted[s] * pb, &a_proofs[s * pb], pb); }
  }
  if (rc || !d_coms_out) return rc;
  BPPP_HIP(ctx, hipMemcpyAsync(d_coms_out, h_coms.data(), h_coms.size(), hipMemcpyHostToDevice, ctx->stream));
  BPPP_HIP(ctx, hipMemcpyAsync(d_proofs_out, h_proofs.data(), h_proofs.size(), hipMemcpyHostToDevice, ctx->stream));
  BPPP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return BPPP_OK;
}

extern "C" int bppp_rp_prove_batch_pub(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint64_t *public_amounts,
                                       const uint8_t *rand_prefix, size_t prefix_len, uint8_t *coms_files, uint8_t *proof_files) {
  return prove_entry(rp, batch, amounts, types, blinds, public_amounts, rand_prefix, prefix_len, coms_files, proof_files, false);
}

extern "C" int bppp_rp_prove_batch_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds, const void *d_public_amounts,
                                          const void *d_rand_prefix, size_t prefix_len, void *d_coms_files, void *d_proof_files) {
  return prove_entry(rp, batch, d_amounts, d_types, d_blinds, d_public_amounts, d_rand_prefix, prefix_len, d_coms_files, d_proof_files, true);
}

extern "C" int bppp_rp_prove_batch_status(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint64_t *public_amounts,
                                          const uint8_t *rand_prefix, size_t prefix_len, uint8_t *coms_files, uint8_t *proof_files, uint32_t *proof_status) {
  return prove_entry(rp, batch, amounts, types, blinds, public_amounts, rand_prefix, prefix_len, coms_files, proof_files, false, true, proof_status);
}

extern "C" int bppp_rp_prove_batch_status_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds, const void *d_public_amounts,
                                                 const void *d_rand_prefix, size_t prefix_len, void *d_coms_files, void *d_proof_files, uint32_t *proof_status) {
  return prove_entry(rp, batch, d_amounts, d_types, d_blinds, d_public_amounts, d_rand_prefix, prefix_len, d_coms_files, d_proof_files, true, true, proof_status);
}

extern "C" int bppp_rp_prove_bound(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint64_t *public_amounts,
                                   const uint8_t *bindings, const uint8_t *rand_prefix, size_t prefix_len, uint8_t *coms_files, uint8_t *proof_files,
                                   uint32_t *proof_status) {
  return prove_entry(rp, batch, amounts, types, blinds, public_amounts, rand_prefix, prefix_len, coms_files, proof_files, false, false, proof_status, bindings);
}

extern "C" int bppp_rp_prove_bound_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds, const void *d_public_amounts,
                                          const void *d_bindings, const void *d_rand_prefix, size_t prefix_len, void *d_coms_files, void *d_proof_files,
                                          uint32_t *proof_status) {
  return prove_entry(rp, batch, d_amounts, d_types, d_blinds, d_public_amounts, d_rand_prefix, prefix_len, d_coms_files, d_proof_files, true, false, proof_status, d_bindings);
}

extern "C" const char *bppp_rp_witness_status_text(uint32_t status) { return bppp_rps::wit_status_text(status); }

static int prove_batch_one(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint8_t *rand_prefix,
                           size_t prefix_len, uint8_t *coms_files, uint8_t *proof_files, size_t index_base, const uint64_t *pub) {
  bppp_ctx *ctx = rp->ctx;
  const Setup &st = rp->st;
  // shapes beyond the device algebra's LDS tables (and BPPP_RP_HOST_ALGEBRA=1, kept for comparison) take the host-algebra path: same bytes out
  if (lds_gate(st) || rp->opt.host_algebra || (st.flavour && !rp->comb)) return prove_batch_host(rp, batch, amounts, types, blinds, rand_prefix, prefix_len, coms_files, proof_files, index_base, pub);
  hipSetDevice(ctx->device);
  const size_t B = batch, nr = st.rds.size(), nlen = st.nlen, llen = st.llen, k = st.rounds, T = 1 + llen + nlen, npub = rp_public_count(rp);
  if (nr >= (1u << 16)) return fail(ctx, BPPP_ERR_ARG, "rp_prove_batch: too many ranges");
  { int rc = rpp_build_fixed_table(rp); if (rc) return rc; }
  if (!rp->commit_basis) { int rc = bppp_basis_create_device(ctx, rp->d_basis, T, 0, 4096, &rp->commit_basis); if (rc) return rc; }
  LapTimer timer(rp->opt.timing, "[rp_prove]");
  // ---- the witness on the host: digits and multiplicities are integer work on the plain amounts (TypedReciprocal.hs:125-161)
  // host staging: one pinned grow-only buffer per handle (no page faults on fresh vectors every call; the 50 MB of inputs and the
  // commitments cross PCIe at the pinned rate)
  const size_t n_in_sc = B * nr * 12, n_dig = B * nlen, n_mss = B * (llen - 6) + 1, n_in_pt = B * nr * 8;
  { int rc = rpp_ensure_hpin(rp, (n_in_sc + n_in_pt) * 8 + (2 * n_dig + n_mss) * 4 + 64); if (rc) return rc; }
  uint64_t *h_in_sc = (uint64_t *)rp->hpin, *h_in_pt = h_in_sc + n_in_sc;
  uint32_t *dig = (uint32_t *)(h_in_pt + n_in_pt), *mul = dig + n_dig, *mss = mul + n_dig;
  std::atomic<int> failed{-1};
  std::vector<std::string> errs(B);
  rp_parallel(B, [&](size_t lo, size_t hi) {
    PState p;
    for (size_t b = lo; b < hi; b++) {
      if (!make_witness(st, p, amounts + 4 * nr * b, types + 4 * nr * b, blinds + 4 * nr * b, pub ? pub + 4 * npub * b : nullptr)) { failed = (int)b; errs[b] = p.err; continue; }
      for (size_t i = 0; i < nr; i++) { p.v[i].store(&h_in_sc[(b * nr + i) * 12]); p.ty[i].store(&h_in_sc[(b * nr + i) * 12 + 4]); p.bl[i].store(&h_in_sc[(b * nr + i) * 12 + 8]); }
      for (size_t i = 0; i < nlen; i++) {
        const bool typing = (st.pos[i].kind & 0xFFu) == bppp_rps::POS_TYPING;
        dig[b * nlen + i] = typing ? 0u : (uint32_t)p.d[i].w[0];
        mul[b * nlen + i] = (uint32_t)p.mi[i].w[0];
      }
      for (size_t j = 0; j + 6 < llen; j++) mss[b * (llen - 6) + j] = (uint32_t)p.ms_shared[j].w[0];
    }
  });
  if (failed >= 0) return fail(ctx, BPPP_ERR_ARG, "rp_prove_batch: proof " + std::to_string((size_t)failed + index_base) + ": " + errs[failed]);
  timer.lap("witness digits (host)");
  std::vector<uint64_t> c_dm(B * 8), c_m(B * 8), c_r(B * 8), c_bl(B * 8), resp(B * k * 16), wn(B * st.fn * 4 + 4), wl(B * st.fl * 4 + 4);
  RppHostInputs in{B, h_in_sc, dig, mul, mss, rand_prefix, prefix_len, pub};
  RppOutputs out{h_in_pt, c_dm.data(), c_m.data(), c_r.data(), c_bl.data(), resp.data(), wn.data(), wl.data()};
  { int rc = rpp_device_prove(rp, in, out); if (rc) return rc; }
  timer.lap("phases + argument (device)");
  rpp_encode_files(rp, B, out.input_coms, out.wit_norm, out.wit_lin, {out.c_bl, out.c_r, out.c_dm, out.c_m}, out.resp, coms_files, proof_files);
  timer.lap("encode (host)");
  return BPPP_OK;
}

static int prove_batch_host(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint8_t *rand_prefix,
                            size_t prefix_len, uint8_t *coms_files, uint8_t *proof_files, size_t index_base, const uint64_t *pub) {
  if (!rp) return BPPP_ERR_ARG;
  bppp_ctx *ctx = rp->ctx;
  if (!batch) return BPPP_OK;
  hipSetDevice(ctx->device);
  hipStream_t stream = ctx->stream;
  const Setup &st = rp->st;
  const size_t B = batch, nr = st.rds.size(), nlen = st.nlen, llen = st.llen, k = st.rounds, T = 1 + llen + nlen, npub = rp_public_count(rp);
  if (nr >= (1u << 16)) return fail(ctx, BPPP_ERR_ARG, "rp_prove_batch: too many ranges");
  rp->last_prove_route = 2; rp->last_lds2 = rp->last_lds3 = 0;
  { int rc = rpp_build_fixed_table(rp); if (rc) return rc; }
  // the basis of commitRPW is fixed per setup: registered once with its fixed-base table (one bucket set for all windows)
  if (!rp->commit_basis) { int rc = bppp_basis_create_device(ctx, rp->d_basis, T, 0, 4096, &rp->commit_basis); if (rc) return rc; }
  // device workspace: [input scalars B nr 3 | input commitments B nr | commitment rows 2B T]
  const size_t in_sc = B * nr * 3 * 32, in_pt = B * nr * 64, rows = 2 * B * T * 32;
  { int rc = ensure_pwork(rp, in_sc + in_pt + rows + 1024); if (rc) return rc; }
  uint32_t *d_in_sc = (uint32_t *)rp->pwork, *d_in_pt = (uint32_t *)((char *)rp->pwork + ((in_sc + 255) & ~(size_t)255)),
           *d_rows = (uint32_t *)((char *)d_in_pt + ((in_pt + 255) & ~(size_t)255));

  { int rc = rp_bind_host(rp); if (rc) return rc; }     // a bound call: the oracles below hash under tag <> binding_b
  LapTimer timer(rp->opt.timing, "[rp_prove]");      // BPPP_RP_TIMING=1: wall time of each phase on stderr (tuning aid)
  std::vector<PState> ps(B);
  std::vector<uint64_t> h_in_sc(B * nr * 12), h_in_pt(B * nr * 8), h_rows(2 * B * T * 4), h_com(2 * B * 8);
  std::atomic<int> failed{-1};
  auto put_row = [&](size_t row, const RPW &w) {           // commitRPW's term order: [sc] ++ lin ++ nrm over [g] ++ hs ++ gs
    uint64_t *dst = &h_rows[row * T * 4];
    w.sc.store(dst);
    for (size_t i = 0; i < llen; i++) w.lin[i].store(dst + 4 * (1 + i));
    for (size_t i = 0; i < nlen; i++) w.nrm[i].store(dst + 4 * (1 + llen + i));
  };
  auto commit_rows = [&](size_t nrows) -> int {            // one batched MSM over the registered basis: h_com[row] = commit(row)
    BPPP_HIP(ctx, hipMemcpyAsync(d_rows, h_rows.data(), nrows * T * 32, hipMemcpyHostToDevice, stream));
    return bppp_msm_basis(rp->commit_basis, d_rows, T, nrows, h_com.data());
  };

  // ---- phase 1: witness, dmWit / mWit (TypedReciprocal.hs:402-410)
  rp_parallel(B, [&](size_t lo, size_t hi) {
    for (size_t b = lo; b < hi; b++) {
      PState &p = ps[b];
      p.rnd = Rnd{rand_prefix + b * prefix_len, prefix_len, 0};
      if (!make_witness(st, p, amounts + 4 * nr * b, types + 4 * nr * b, blinds + 4 * nr * b, pub ? pub + 4 * npub * b : nullptr)) { failed = (int)b; continue; }
      for (size_t i = 0; i < nr; i++) { p.v[i].store(&h_in_sc[(b * nr + i) * 12]); p.ty[i].store(&h_in_sc[(b * nr + i) * 12 + 4]); p.bl[i].store(&h_in_sc[(b * nr + i) * 12 + 8]); }
      p.dm = blind_witness(2, p.ms_shared, p.d, p.rnd, llen);
      p.m = blind_witness(1, std::vector<U256>(), p.mi, p.rnd, llen);
      put_row(2 * b, p.dm); put_row(2 * b + 1, p.m);
    }
  });
  if (failed >= 0) return fail(ctx, BPPP_ERR_ARG, "rp_prove_batch: proof " + std::to_string((size_t)failed + index_base) + ": " + ps[failed].err);
  timer.lap("phase 1 host");
  BPPP_HIP(ctx, hipMemcpyAsync(d_in_sc, h_in_sc.data(), in_sc, hipMemcpyHostToDevice, stream));
  {
    { int rc = rpp_commit_inputs_fixed(rp, d_in_sc, B * nr, d_in_pt); if (rc) return rc; }      // this route keeps the 4-bit window table (csrc/rpcommit.hip)
    BPPP_HIP(ctx, hipMemcpyAsync(h_in_pt.data(), d_in_pt, in_pt, hipMemcpyDeviceToHost, stream));
  }
  { int rc = commit_rows(2 * B); if (rc) return rc; }       // synchronises the stream
  timer.lap("inputs + dm/m commits (GPU)");
  std::vector<uint64_t> c_dm(B * 8), c_m(B * 8), c_r(B * 8), c_bl(B * 8);
  for (size_t b = 0; b < B; b++) { memcpy(&c_dm[8 * b], &h_com[16 * b], 64); memcpy(&c_m[8 * b], &h_com[16 * b + 8], 64); }

  // ---- phase 2: (e, x, r0), reciprocals, rWit (:412-419)
  rp_parallel(B, [&](size_t lo, size_t hi) {
    std::vector<const uint64_t *> pts(2 + nr);
    for (size_t b = lo; b < hi; b++) {
      PState &p = ps[b];
      pts[0] = &c_dm[8 * b]; pts[1] = &c_m[8 * b];
      for (size_t i = 0; i < nr; i++) pts[2 + i] = &h_in_pt[(b * nr + i) * 8];
      U256 ch[3];
      oracle(rp_tag_at(rp, b), p, pts.data(), pts.size(), 3, ch);
      p.e = ch[0]; p.x = ch[1]; p.r0 = ch[2];
      p.e_inv = finv(p.e); p.r0_inv = finv(p.r0);
      make_phase2(st, p);
      U256 s = U256::zero();
      for (size_t i = 0; i < nlen; i++) s = fa(s, fdbl(fm(p.rr[i], p.cc[i])));
      const U256 err7 = fm(p.r0_inv, fneg(s));             // err7Term (:209-211)
      p.r = blind_err_witness(err7, p.rr, p.rnd, llen);
      put_row(b, p.r);
    }
  });
  timer.lap("phase 2 host");
  { int rc = commit_rows(B); if (rc) return rc; }
  memcpy(c_r.data(), h_com.data(), B * 64);
  timer.lap("r commit (GPU)");

  // ---- phase 3: (q, x', r1), error terms, the blinding commitment (:421-437)
  rp_parallel(B, [&](size_t lo, size_t hi) {
    for (size_t b = lo; b < hi; b++) {
      PState &p = ps[b];
      const uint64_t *pt = &c_r[8 * b];
      U256 ch[3];
      oracle(rp_tag_at(rp, b), p, &pt, 1, 3, ch);
      p.q = ch[0]; p.xp = ch[1]; p.r1 = ch[2];
      p.q0 = fm(p.q, p.q);                                  // qPowers': powers' (q^2) for the NL norm (NormArgument.hs:148),
      if (st.flavour) p.q0 = fneg(p.q0);                    // powers' (-q^2) for the IP one (InnerProductArgument.hs:231)
      p.q0_inv = finv(p.q0); p.r1_inv = finv(p.r1);
      p.shared_cs = make_shared_coeffs(st, p);
      const U256 tC = st.has_types ? p.xp : U256::zero();
      std::vector<U256> bls_lin(llen - 5), bls_nrm(nlen);
      for (auto &v : bls_lin) v = p.rnd.next();
      for (auto &v : bls_nrm) v = p.rnd.next();
      const std::vector<U256> bls_ms(bls_lin.begin() + 1, bls_lin.end());
      const std::vector<U256> ic = input_coeffs(st, p.x, p.q0);
      p.ns_sc = p.ns_ty = p.ns_bl = U256::zero();
      for (size_t i = 0; i < nr; i++) { p.ns_sc = fa(p.ns_sc, fm(ic[i], p.v[i])); p.ns_ty = fa(p.ns_ty, fm(ic[i], p.ty[i])); p.ns_bl = fa(p.ns_bl, fm(ic[i], p.bl[i])); }
      U256 errs[6];
      make_error_terms(st, p, bls_ms, bls_nrm, errs);
      p.blw = blind_blinding_term(bls_lin, bls_nrm, tC, p, errs, p.ns_bl, llen);
      put_row(b, p.blw);
    }
  });
  timer.lap("phase 3 host");
  { int rc = commit_rows(B); if (rc) return rc; }
  memcpy(c_bl.data(), h_com.data(), B * 64);
  timer.lap("bl commit (GPU)");

  // ---- t, the combined witness and the argument's linear weights (:438-446)
  std::vector<uint64_t> a_s(B * 4), a_q(B * 4), a_nx(B * nlen * 4), a_lc(B * llen * 4), a_lx(B * llen * 4);
  rp_parallel(B, [&](size_t lo, size_t hi) {
    for (size_t b = lo; b < hi; b++) {
      PState &p = ps[b];
      const uint64_t *pt = &c_bl[8 * b];
      oracle(rp_tag_at(rp, b), p, &pt, 1, 1, &p.t);
      U256 psc; std::vector<U256> pn;
      make_public_consts(st, p, psc, pn, pub ? pub + 4 * npub * b : nullptr);
      const U256 t2 = fm(p.t, p.t), t3 = fm(t2, p.t), t4 = fm(t2, t2), t5 = fm(t4, p.t), t6 = fm(t3, t3), two_t5 = fdbl(t5);
      // wit = pub + blWit + t mWit + t^2 dmWit + t^3 rWit + 2 t^5 nWitSum
      U256 sc = fa(fa(psc, p.blw.sc), fa(fa(fm(p.t, p.m.sc), fm(t2, p.dm.sc)), fa(fm(t3, p.r.sc), fm(two_t5, p.ns_sc))));
      sc.store(&a_s[4 * b]); p.q.store(&a_q[4 * b]);
      for (size_t i = 0; i < llen; i++) {
        U256 v = fa(fa(p.blw.lin[i], fm(p.t, p.m.lin[i])), fa(fm(t2, p.dm.lin[i]), fm(t3, p.r.lin[i])));
        if (i == 0) v = fa(v, fm(two_t5, p.ns_ty));
        if (i == 1) v = fa(v, fm(two_t5, p.ns_bl));
        v.store(&a_lx[(b * llen + i) * 4]);
      }
      for (size_t i = 0; i < nlen; i++)
        fa(fa(pn[i], p.blw.nrm[i]), fa(fa(fm(p.t, p.m.nrm[i]), fm(t2, p.dm.nrm[i])), fm(t3, p.r.nrm[i]))).store(&a_nx[(b * nlen + i) * 4]);
      // makeBpCoeffs (:391-396)
      const U256 rs = fm(p.r0, p.r1), two_t3 = fdbl(t3);
      U256 c6[6] = {st.has_types ? fneg(p.xp) : U256::zero(), fm(rs, p.t), fm(rs, t2), fm(rs, t3), fm(p.r0, t4), fm(rs, t6)};
      for (int i = 0; i < 6; i++) c6[i].store(&a_lc[(b * llen + i) * 4]);
      for (size_t i = 0; i < p.shared_cs.size(); i++) fm(two_t3, p.shared_cs[i]).store(&a_lc[(b * llen + 6 + i) * 4]);
      // the phase vectors are no longer needed
      p.dm = RPW(); p.m = RPW(); p.r = RPW(); p.blw = RPW();
      p.u.clear(); p.vv.clear(); p.rr.clear(); p.cc.clear(); p.d.clear(); p.mi.clear(); p.pv.clear();
    }
  });

  timer.lap("witness combination host");
  // ---- proveBPM in lockstep (src/Bulletproof.hs:357-359)
  std::vector<uint64_t> resp(B * (k ? k : 1) * 16), wn(B * st.fn * 4 + 4), wl(B * st.fl * 4 + 4);
  auto argument = st.flavour ? ip_argument_lockstep : nl_argument_lockstep;
  { int rc = argument(rp, B, k, a_s.data(), a_q.data(), a_nx.data(), a_lc.data(), a_lx.data(), [&](size_t b) -> PState & { return ps[b]; }, resp.data(), wn.data(), wl.data());
    if (rc) return rc; }
  timer.lap("argument (lockstep)");
  rpp_encode_files(rp, B, h_in_pt.data(), wn.data(), wl.data(), {c_bl.data(), c_r.data(), c_dm.data(), c_m.data()}, resp.data(), coms_files, proof_files);
  timer.lap("witness download + encode");
  return BPPP_OK;
}

