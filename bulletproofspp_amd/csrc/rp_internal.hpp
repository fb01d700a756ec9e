// rp_internal.hpp — declarations shared by the two halves of the range-proof layer (csrc/rp.hip: setup + batch verifier,
// csrc/rpprove.hip: batch prover).
#pragma once
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include "ctx.hpp"
#include "hostmath.hpp"
#include "rpsetup.hpp"
#include "hostpool.hpp"
#include "rptally_plan.hpp"

struct bppp_trrp;
struct bppp_nlb;
struct bppp_basis;

namespace bppp {

struct RpDims {
  uint32_t nr, k, fn, fl;            // ranges (input commitments), rounds, final witness lengths
  uint32_t nrp, nch;                 // range-proof commitments ahead of the inputs (4: blCom rCom dmCom mCom; Binary 2: blCom dCom) and
                                     // oracle outputs before the argument's rounds (7: e x r0 q x' r1 t; Binary 4: q x r t)
  uint32_t coms_bytes, proof_bytes;  // per-proof file sizes
  uint32_t text_stride;              // bytes reserved per proof for the transcript text (multiple of 16)
};
__host__ __device__ inline uint32_t rp_npts(const RpDims &D) { return D.nrp + D.nr + 2 * D.k; }

static constexpr int RP_HDR_MAX = 64;
struct HashPlan { uint32_t hdr_be[RP_HDR_MAX / 4]; uint32_t hlen, start_pt, out_slot; };   // header as big-endian words, zero-padded
// header bytes -> big-endian words
inline void rp_pack_header(const std::string &h, uint32_t be[RP_HDR_MAX / 4]) {
  for (int i = 0; i < RP_HDR_MAX / 4; i++) be[i] = 0;
  for (size_t i = 0; i < h.size() && i < (size_t)RP_HDR_MAX; i++) be[i >> 2] |= (uint32_t)(uint8_t)h[i] << (24 - 8 * (i & 3));
}   // out_slot: index into ch[7] (< 7) or 7 + index into es[k]

// ---- per-proof transcript bindings (the bppp_rp_*_bound* entry points, include/bppp.h; csrc/rpbind.hip)
// Proof b of a bound call hashes under the tag  oracle_tag <> binding_b[32].  The bindings of one call hang on the handle while the call
// runs (a handle serves one call at a time): every oracle of every route reads them there, so a route that never hears of bindings
// cannot drop them.  h / d: [n][32] bytes as the caller passed them, on the host or in HBM (rp_bind_host / rp_bind_device fetch the
// other copy); both NULL: an unbound call.  sel_h / sel_d: NULL (slot s of the batch in flight is proof s) or the proofs of the slots,
// after the refused proofs of a status call were compacted away (csrc/rpwitness.hip).
static constexpr size_t RP_BINDING_BYTES = 32;
struct RpBind {
  const uint8_t *h = nullptr, *d = nullptr; size_t n = 0;
  const uint32_t *sel_h = nullptr, *sel_d = nullptr;
  bool on() const { return h || d; }
  RpBind from(size_t b0, size_t count) const { RpBind r = *this; if (r.h) r.h += RP_BINDING_BYTES * b0; if (r.d) r.d += RP_BINDING_BYTES * b0; r.n = count; return r; }
};
// where the unbound headers of a kernel's header table lie, in 32-bit words: header i is the 16 words at (i / per) * group + (i % per) * 16, its
// length the word at (i / per) * group + hlen + i % per  (HashPlan: {1, 19, 16}; RppHdrs, csrc/rpp_transcript.hip: {3, 54, 48})
struct RpHdrLayout { uint32_t per, group, hlen; };

// f(lo, hi) on disjoint ranges covering [0, n), one host thread each (at most 16: the GPU box's CPU share per GPU)
template <class F> static void rp_parallel(size_t n, F f) {
  unsigned hw = std::thread::hardware_concurrency();
  size_t nt = std::min<size_t>(std::min<size_t>(hw ? hw : 1, 16), n / 4);
  if (nt <= 1) { f((size_t)0, n); return; }
  std::vector<std::thread> th;
  for (size_t t = 0; t < nt; t++) th.emplace_back([=] { f(n * t / nt, n * (t + 1) / nt); });
  for (auto &x : th) x.join();
}

// BPPP_RP_TIMING's stderr lap timer: lap(what) prints the wall time since the previous lap (or since the timer was made) after `prefix`,
// in milliseconds, or in microseconds with `us`
struct LapTimer {
  bool on; const char *prefix; bool us; double last;
  static double ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  LapTimer(bool on_, const char *prefix_, bool us_ = false) : on(on_), prefix(prefix_), us(us_), last(on_ ? ms() : 0) {}
  void lap(const char *what) {
    if (!on) return;
    const double t = ms();
    if (us) fprintf(stderr, "%s %-24s %7.1f us\n", prefix, what, 1000 * (t - last));
    else fprintf(stderr, "%s %-28s %8.2f ms\n", prefix, what, t - last);
    last = t;
  }
};

int msm_run(bppp_ctx *, const void *, const void *, size_t, size_t, int, int, uint64_t *);
int batch_inverse_run(bppp_ctx *, const void *, size_t, int, void *);      // csrc/rounds.hip
// bppp_{nl,ip}_verify_batch_device with the validation of untrusted inputs optional (csrc/nlbatch.hip)
int nl_verify_batch_run(bppp_ctx *, size_t, size_t, size_t, size_t, size_t, size_t, size_t, const void *, const void *, const void *, const void *, const void *, const void *,
                        const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *, uint64_t *, bool);
int ip_verify_batch_run(bppp_ctx *, size_t, size_t, size_t, size_t, size_t, size_t, size_t, const void *, const void *, const void *, const void *, const void *, const void *,
                        const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *, uint64_t *, bool);
// ... and their first step alone, the assembly of the MSM's input (same arguments up to `validate`, then: shared scalars [G | H | g],
// per-proof scalars [batch][ninit + 2k], points — [G | H | g | per-proof] when gather_shared, else the per-proof ones alone — and the
// flag word read after the MSM).  Scratch: ctx->ws2 of at least {nl,ip}_verify_batch_scratch bytes, made sure of by the caller.
int nl_verify_batch_assemble(bppp_ctx *, size_t, size_t, size_t, size_t, size_t, size_t, size_t, const void *, const void *, const void *, const void *, const void *,
                             const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *,
                             bool validate, uint32_t *sc_shared, uint32_t *sc_tail, uint32_t *pts, bool gather_shared, uint32_t *flags);
int ip_verify_batch_assemble(bppp_ctx *, size_t, size_t, size_t, size_t, size_t, size_t, size_t, const void *, const void *, const void *, const void *, const void *,
                             const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *,
                             bool validate, uint32_t *sc_shared, uint32_t *sc_tail, uint32_t *pts, bool gather_shared, uint32_t *flags);
size_t nl_verify_batch_scratch(size_t batch, size_t nlen, size_t llen, size_t k);
size_t ip_verify_batch_scratch(size_t batch, size_t nlen, size_t llen, size_t k, size_t fn);
int ip_verify_batch_flags(bppp_ctx *, uint32_t hflags);     // the inner-product assembly's flag word -> error code
inline bool rp_point_is_inf(const uint64_t *p) { uint64_t o = 0; for (int i = 0; i < 8; i++) o |= p[i]; return o == 0; }

}  // namespace bppp

extern "C" {
int bppp_trrp_create(bppp_ctx *ctx, int flavour, int has_types, size_t nlen, size_t llen, size_t nranges, const uint32_t *pos_kind, const uint32_t *pos_range,
                     const uint32_t *pos_slot, const uint32_t *pos_sym, const uint64_t *pos_coeff, const uint64_t *range_min, const uint32_t *range_assumed,
                     size_t nsyms, const uint64_t *syms, const uint32_t *cs_slot, const uint32_t *cs_sym, size_t npub, const uint32_t *pub_is_out,
                     const uint64_t *pub_amount, const uint32_t *pub_sym, bppp_trrp **out);
void bppp_trrp_destroy(bppp_trrp *t);
int bppp_trrp_public_device(bppp_trrp *t, size_t batch, const void *d_challenges, void *d_q, void *d_sp, void *d_pub_norm, void *d_pub_lin_c, void *d_init_scalars);
}
namespace bppp {
int trrp_public_run(bppp_trrp *t, size_t batch, const void *d_challenges, void *d_q, void *d_sp, void *d_pub_norm, void *d_pub_lin_c, void *d_init_scalars,
                    const void *d_pub_amounts);      // csrc/trrp.hip: d_pub_amounts NULL or [batch][npub] canonical scalars
}  // namespace bppp


namespace bppp { struct CombTable; void comb_destroy(CombTable *); }
// Tuning knobs of one handle (bppp_rp_set_option, include/bppp.h).  The BPPP_RP_* / BPPP_NLB_* environment variables are read ONCE,
// when the handle is created, as the initial values; no entry point reads the environment per call.
struct RpOptions {
  size_t comb_min = 1024;             // BPPP_RP_COMB_MIN: first batch size (or cumulative proofs) that builds the comb table
  size_t comb_budget = (size_t)32 << 30;   // BPPP_RP_COMB_GB: table budget; also capped by a share of the free HBM (rp_ensure_comb)
  int comb_bits = 0;                  // BPPP_RP_COMB_BITS: force a window width (0 = widest that fits the budget)
  bool no_comb = false;               // BPPP_RP_NO_COMB
  size_t split_min = 4096;            // BPPP_RP_SPLIT_MIN: smallest batch run as two half-batches in flight
  size_t split_min_binary = 1024;     // BPPP_RP_SPLIT_MIN_BINARY: the same for RangeProof.Binary handles (rows of thousands of terms: fewer proofs fill the chip)
  bool no_split = false;              // BPPP_RP_NO_SPLIT
  size_t host_oracle_verify = 8;      // BPPP_RP_HOST_ORACLE_MAX: largest batch whose transcript hashing runs on the host (verifier)
  size_t host_oracle_prove = 64;      //                          ... (prover)
  size_t hash_fork_max = 64;          // BPPP_RP_HASH_FORK_MAX: largest batch whose two hashing halves run side by side on two streams (verifier)
  bool fold_points = false;           // BPPP_NLB_FOLD_POINTS: point-folding argument although a table exists
  bool host_algebra = false;          // BPPP_RP_HOST_ALGEBRA: field algebra and hashing of the prover on the host
  bool timing = false;                // BPPP_RP_TIMING: phase times on stderr
  int culprits = 0;                   // BPPP_RP_OPT_CULPRITS (set_option only): 0 = bisection, 1 = one per-proof pass (csrc/rpeach.hip)
  void from_env();
};
struct bppp_brp_tabs;      // csrc/rp.hip: device tables of a RangeProof.Binary setup
struct bppp_rp {
  bppp_ctx *ctx = nullptr;
  RpOptions opt;
  bppp_brp_tabs *btabs = nullptr;
  bppp_rps::Setup st;
  bppp_trrp *tabs = nullptr;
  std::string tag;
  std::vector<uint64_t> h_g, h_G, h_H;          // the basis on the host (prover: commit inputs, argument start)
  // the registered basis, affine, resident in HBM in commitRPW's term order (src/RangeProof/Internal.hs:45-50):
  // [g (1) | H (llen) | G (nlen)]
  uint32_t *d_basis = nullptr;
  const uint32_t *d_g() const { return d_basis; }
  const uint32_t *d_H() const { return d_basis + 16; }
  const uint32_t *d_G() const { return d_basis + 16 * (1 + st.llen); }
  bppp::HashPlan *d_plan = nullptr;
  uint32_t nhash = 0;
  bppp::RpDims D{};
  // fixed-base window table of g, H[0], H[1] for the input commitments (csrc/rpcommit.hip: the provers and the commit / open entry points);
  // prover workspace (csrc/rpprove.hip), also the commit / open entry points' — a handle serves one call at a time
  uint32_t *d_fixed = nullptr;
  bppp_basis *commit_basis = nullptr;           // [g | H | G] registered with its fixed-base table: the range-proof commitments
  void *pwork = nullptr; size_t pwork_bytes = 0;
  void *awork = nullptr; size_t awork_bytes = 0;   // grow-only workspace of the device-resident inner-product argument (csrc/ipb.hip)
  void *hpin = nullptr; size_t hpin_bytes = 0;     // pinned host staging of the batch prover
  // the creation arguments, kept so that a second handle on its OWN context (stream, workspaces) can be made: a large prove batch
  // runs as two half-batches in flight, the host shares of one under the kernels of the other (csrc/rpprove.hip)
  std::vector<bppp_rp_range> c_ranges; std::vector<bppp_rp_public> c_pubs; std::vector<uint64_t> c_points; int c_has_types = 0;
  int c_conserve = 0; uint64_t c_net_public[4] = {0, 0, 0, 0};      // bppp_rp_create_binary's arguments, for the twin handle
  bppp_rp *twin = nullptr; bppp_ctx *twin_ctx = nullptr; bool is_twin = false;
  // fixed-base comb over [g | H | G] (csrc/comb.hip): the range-proof commitments and the argument's round commitments of large
  // batches.  The table is reference-counted (rp_set_comb): built by this handle, or the table of a LONGER basis of the same point
  // stream that another handle built (bppp_rp_share_comb, bppp_rp_prove_mixed; csrc/rpshare.hip) — every launch passes this handle's own
  // row length next to the table's stride; the twin handle holds its parent's table
  bppp::CombTable *comb = nullptr; bool comb_failed = false; size_t proved_total = 0;
  // bppp_rp_prove_mixed: the input commitments of this handle's group, already computed with its family's in one launch ([batch][nranges]
  // affine points in HBM, complete before the group starts); rpp_commit_inputs copies them instead of launching
  const uint32_t *pre_inputs = nullptr;
  uint32_t *d_comb_out = nullptr; size_t comb_out_rows = 0;   // fixed-base tables of the argument's first round (csrc/nlb.hip)
  // grow-only verifier workspace and the staging buffer of the host-buffer entry point
  bppp::HostPool *pool = nullptr;                // workers of the host oracle (batches of 2 .. host_oracle_verify proofs), made on first use
  hipEvent_t slice_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // one per upload slice of bppp_rp_verify_batch
  uint64_t *hstage = nullptr; size_t hstage_bytes = 0;   // pinned, grow-only: the host oracle's downloads and uploads (a pageable target makes every async copy a blocking one)
  uint32_t *hflag = nullptr;                     // pinned: the verifier's "some proof did not decode" word, copied out while the batch is still in flight
  void *work = nullptr; size_t work_bytes = 0;
  void *stage = nullptr; size_t stage_bytes = 0;
  // per-proof verifier (csrc/rpeach.hip): grow-only workspace, proofs per chunk (0 = from the row budget; a test hook may set it), and
  // what the last verification on this handle ran (combined MSMs, per-proof passes: bppp_test_rp_last_verify_counts)
  void *ework = nullptr; size_t ework_bytes = 0;
  size_t each_chunk = 0;
  uint64_t n_combined = 0, n_each = 0;
  // what the last block call on this handle launched up to its verdict (csrc/rpblock.hip; bppp_test_rp_last_block_counts): MSMs, the terms of
  // the one MSM, keys lifted and commitments square-rooted
  uint64_t blk_msms = 0, blk_terms = 0, blk_key_lifts = 0, blk_coms = 0;
  // what the last typed-reciprocal prove on this handle ran (bppp_test_rp_last_prove): 0 nothing yet, 1 the device algebra (k_rpp_phase2 / k_rpp_phase3
  // with last_lds2 / last_lds3 bytes of dynamic LDS, csrc/rpprove_dev.hip), 2 the host-algebra route (prove_batch_host, csrc/rpprove.hip)
  int last_prove_route = 0; size_t last_lds2 = 0, last_lds3 = 0;
  int last_text_kernel = -1;         // transcript text kernel of the last verification on this handle: 0 k_rp_text, 1 k_rp_text_lds (bppp_test_rp_last_text_kernel)
  // the tally entry points (csrc/rptally.hip): the longest sum one lane walks alone, the entries of one workgroup's piece of a longer sum, and
  // the entries (and sums) of one pass over the workspace; test hooks lower them so that small jobs straddle them (include/bppp_test.h)
  size_t tally_short_max = 16, tally_piece = 4096, tally_chunk = (size_t)1 << 22;
  // the items (commitments, sums, keys) of one pass over the workspace in every balance call that is not planned by the tally's chunk: commit, open,
  // sign, keys and the two key verifiers (rpp_flat_chunk); a test hook lowers it so that a small job takes several passes
  size_t flat_chunk = (size_t)1 << 22;
  // cut-through (csrc/rpcut.hip).  What the test hooks pin (bppp_test_rp_cut_through_force): cut_same_hash makes every routing hash equal, cut_salt_pinned
  // takes cut_salt in place of fresh randomness, cut_table_bits (0: at least 2 nnz slots) asks for 2^bits slots, lifted to the smallest power of two that
  // holds every entry.  And what the last call on this handle ran (bppp_test_rp_cut_through_last): table slots, groups (distinct identities), sort passes
  bool cut_same_hash = false, cut_salt_pinned = false;
  uint8_t cut_salt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int cut_table_bits = 0;
  uint64_t cut_slots = 0, cut_groups = 0, cut_passes = 0;
  // per-proof public amounts of the *_pub entry points (bppp_rp_public_count per proof): grow-only device copy of one call's canonical
  // scalars, [batch][public_count][8] words
  uint32_t *d_pub = nullptr; size_t d_pub_bytes = 0;
  // bppp_rp_prove_batch_device: the per-range data of the witness kernels (csrc/rpwitness.hip.h), uploaded at the first device call
  uint32_t *d_wit = nullptr;
  // bppp_rp_prove_batch_status_device, a batch with refused proofs: the accepted and the refused proofs' indices and the accepted proofs' public
  // words in compact order (csrc/rpwitness.hip), grow-only
  uint32_t *d_sel = nullptr; size_t d_sel_bytes = 0;
  // the bound entry points: the bindings of the call in flight, the copy of them this handle fetched (host: bind_hbuf, HBM: d_bind) and the
  // per-(oracle output, proof) headers the bound hash kernels read (d_bhdr, [headers][batch][16] big-endian words); grow-only.
  // hdr_max: the longest unbound header of this setup (rp_build_plan): a bound call needs hdr_max + 32 <= RP_HDR_MAX
  bppp::RpBind bind;
  std::vector<uint8_t> bind_hbuf;
  uint8_t *d_bind = nullptr; size_t d_bind_bytes = 0;
  uint32_t *d_bhdr = nullptr; size_t d_bhdr_bytes = 0;
  uint32_t hdr_max = 0;
};
namespace bppp {
// a bound entry point's bindings (NULL: nothing to do) on the handle until the guard goes; `who` names the entry point in the tag-length
// error, which rp_bind_begin returns (BPPP_ERR_ARG) when the handle's tag leaves no room for 32 more bytes in a header
int rp_bind_begin(bppp_rp *rp, const void *bindings, bool device, size_t batch, const char *who);
struct RpBindGuard { bppp_rp *rp; ~RpBindGuard() { if (rp) rp->bind = RpBind(); } };
// the bindings of the call in flight where a route needs them: on the host (host oracles) or in HBM (the header kernel); no-ops on an
// unbound call and when that copy is already there
int rp_bind_host(bppp_rp *rp);
int rp_bind_device(bppp_rp *rp);
// the tag slot s of the batch in flight hashes under: oracle_tag, with its binding behind it on a bound call (after rp_bind_host)
std::string rp_tag_at(const bppp_rp *rp, size_t s);
// k_rp_bound_headers: out[(i * slots + s) * 16 ..] = the 16 big-endian words of  tag <> binding of slot s <> the rest of unbound header i, for the
// `nh` headers of a table in HBM (d_table, laid out as L says) — rp->d_bhdr, grown as needed.  Queued on the context's stream.
int rp_bound_headers(bppp_rp *rp, size_t slots, const uint32_t *d_table, RpHdrLayout L, size_t nh, const uint32_t **out);
}  // namespace bppp

// public amounts per proof of the *_pub entry points: npub of a typed handle with types, 1 of a conserved binary handle, else 0
size_t rp_public_count(const bppp_rp *rp);
// the *_pub entry points' amounts of `batch` proofs, as the caller passes them (the creation argument's encoding), checked and made canonical
// scalars [batch][public_count][4] (binary: net_public mod n); BPPP_ERR_ARG names the first bad proof
int rp_public_canon(bppp_rp *rp, size_t batch, const uint64_t *in, std::vector<uint64_t> &out);
// canonical amounts (host) -> rp->d_pub on the handle's stream; returns with the copy done
int rp_upload_public(bppp_rp *rp, const uint64_t *canon, size_t words, const uint32_t **d_out);
// both for a verifier entry point: the amounts from the host (h_in) or from HBM (d_in, downloaded first) into rp->d_pub
int rp_stage_public(bppp_rp *rp, size_t batch, const uint64_t *h_in, const void *d_in, const uint32_t **d_out);

int rp_ensure_twin(bppp_rp *rp);      // csrc/rp.hip

namespace bppp {
// The verifier's per-proof arrays of one prepared batch, carved from the handle's rp->work (csrc/rp.hip).  Every array is [batch][...],
// so proofs [lo, hi) are the same arrays at offset pointers.
struct RpVerifyArrays {
  size_t batch;
  uint32_t *init_pts, *resp_pts, *wit_norm, *wit_lin, *ch, *es, *rho, *q, *sp, *pub_norm, *pub_lin_c, *pub_lin_x, *init_sc, *bad;
};
// the files of one verification: in HBM, or still on the host (h_coms / h_proofs; d_coms / d_proofs are then the handle's staging buffer,
// which the decode stage of rp_verify_prepare fills in slices)
struct RpFiles { const void *d_coms, *d_proofs; const uint8_t *h_coms = nullptr, *h_proofs = nullptr; };
// the host-file entry points' staging: rp->stage grown to `batch` files (coms, then proofs 256-byte aligned), `out` the host files over it
int rp_stage_files(bppp_rp *rp, size_t batch, const void *h_coms, const void *h_proofs, RpFiles &out);
// a single-handle verify entry point after its argument checks: the public amounts (NULL: the handle's own) and the files, both on the
// host (`host`) or in HBM, staged, then rp_verify_prepare.  The caller drains the context (ctx_drain) on failure and after host files.
int rp_verify_start(bppp_rp *rp, size_t batch, uint64_t index_offset, const void *coms, const void *proofs, const void *pub, bool host, const uint8_t seed[32],
                    RpVerifyArrays &A);
// decodeProof, the transcript hashing (device or host oracle, as the handle chooses), the public scalars and the weights rho of the
// proofs at job positions [index_offset, index_offset + batch): everything of the verification but the argument's combination.  Queued
// on the context's stream; bad[b] marks a proof that did not decode and rp->hflag[0] receives "some proof did not" (read it once the
// stream has drained).  The arrays stay valid until the handle's next verification.
// d_pub: NULL (the handle's public amounts) or [batch][public_count] canonical scalars in HBM (rp_upload_public)
int rp_verify_prepare(bppp_rp *rp, size_t batch, uint64_t index_offset, const RpFiles &files, const uint8_t seed[32], RpVerifyArrays &A,
                      const uint32_t *d_pub = nullptr);
// verifyBPM's combination of proofs [lo, lo + n) of a prepared batch: one MSM, returns with the stream drained
int rp_verify_combine(bppp_rp *rp, const RpVerifyArrays &A, size_t lo, size_t n, uint64_t out_xy[8]);
// the culprits of a rejected batch by bisection: a VALID proof_status[b] whose combination fails becomes INVALID.  known_bad: the
// whole batch's combination is already known not to be the identity (otherwise it is evaluated first)
int rp_find_culprits(bppp_rp *rp, const RpVerifyArrays &A, bool known_bad, uint32_t *proof_status);
// every proof of a prepared batch decided on its own (csrc/rpeach.hip): proof_status [A.batch] (VALID / INVALID / MALFORMED) and, when
// proof_xy is not NULL, E_b [A.batch][8] (zeros for infinity and for a malformed proof).  Returns with the stream drained.
int rp_each_pass(bppp_rp *rp, const RpVerifyArrays &A, uint32_t *proof_status, uint64_t *proof_xy);
size_t each_rows_scratch(int flavour, size_t n, size_t llen, size_t k, size_t fn);     // csrc/nlbatch.hip
int each_rows_assemble(bppp_ctx *, int flavour, size_t n, size_t nlen, size_t llen, size_t k, size_t fn, size_t fl, size_t ninit, const uint32_t *ones,
                       const uint32_t *q, const uint32_t *sp, const uint32_t *pub_norm, const uint32_t *pub_lin_c, const uint32_t *pub_lin_x,
                       const uint32_t *es, const uint32_t *wit_norm, const uint32_t *wit_lin, const uint32_t *init_sc, const uint32_t *init_pts,
                       const uint32_t *resp_pts, uint32_t *scratch, uint32_t *rows, uint32_t *tail, uint32_t *pts);
int basis_msm_dev(bppp_basis *h, const void *d_scalars, size_t n_terms, size_t batch, uint32_t *d_out);     // csrc/basis.hip
int msm_batch_dev(bppp_ctx *, const void *, const void *, size_t, size_t, int, int, uint32_t *);           // csrc/msm.hip
}  // namespace bppp
namespace bppp {
// ---- input commitments v g + ty H0 + bl H1 (csrc/rpcommit.hip), shared by the provers and by bppp_rp_commit_batch / bppp_rp_open_*
// the [3][64][15] fixed-base window table of (g, H0, H1), rp->d_fixed: built once per handle, by whichever side needs it first
int rpp_build_fixed_table(bppp_rp *rp);
// d_out[i] = sum_j d_in_sc[i][j] * (g, H0, H1)[j] for n commitments (canonical scalars [n][3][8], affine points [n][16]); asynchronous on the
// context's stream.  rpp_commit_inputs takes the handle's comb table when it has one (and the inputs bppp_rp_prove_mixed already committed),
// else the window table, which the caller has made sure of; rpp_commit_inputs_fixed always takes the window table.  Same points either way.
int rpp_commit_inputs(bppp_rp *rp, const uint32_t *d_in_sc, size_t n, uint32_t *d_out);
int rpp_commit_inputs_fixed(bppp_rp *rp, const uint32_t *d_in_sc, size_t n, uint32_t *d_out);
// decodeCommitments (Encoding.hs:119-128) alone, by the verifier's decoders (csrc/rpdecode.hip.h, launched from csrc/rp.hip): the commitments
// files of nb rows in HBM -> pts [nb][nr][16]; an x without a curve point decodes to the infinity encoding and sets bad[row] and any_bad[0]
// (both OR-ed into: the caller zeroes them).  Queued on the context's stream.
void rp_decode_coms(bppp_rp *rp, size_t nb, const uint8_t *d_coms, uint32_t *pts, uint32_t *bad, uint32_t *any_bad);
// the launches of two of the commit / open kernels (csrc/rpcommit.hip) for the tally entry points (csrc/rptally.hip), queued on the context's stream:
// k_rp_claim_scalars — n claimed (amount, type, blinding) -> in_sc [n][3][8] in base order, flag [n] and any[0] for a type or blinding >= n;
// k_rp_open_reduce twice — the three columns of prods [n][3][8] summed mod n and negated into out [3][8]; part: RPP_REDUCE_BLOCKS * 24 words
static constexpr unsigned RPP_REDUCE_BLOCKS = 1024;
int rpp_claim_scalars(bppp_rp *rp, uint64_t n, const uint32_t *amounts, const uint32_t *types, const uint32_t *blinds, uint32_t *in_sc, uint32_t *flag, uint32_t *any);
int rpp_negated_column_sums(bppp_rp *rp, uint64_t n, const uint32_t *prods, uint32_t *part, uint32_t *out);
// ---- what the passes of the balance calls share (csrc/rpcommit.hip, rptally.hip, rpexcess.hip, rpexkeys.hip)
// the items of one pass over the workspace; a caller whose items are heavier takes a fraction of it
inline size_t rpp_flat_chunk(const bppp_rp *rp) { return rp->flat_chunk; }
// the end of a builder: the statuses of its n items (on the host) go out as they are, or, without a status array, the first refusal is the call's
// error  "<who>: <noun> <position>: <text (status)>"
int rpp_report_refusals(bppp_ctx *ctx, const char *who, const char *noun, const uint32_t *h_status, size_t n, uint32_t *out_status, const char *(*text)(uint32_t));
// the combined points of a batch check, one per MSM.  msm: one more MSM of n terms (msm_run: returns with the stream drained, also when it fails);
// finish: their sum into combined_xy (may be NULL), *accept = the sum is the identity and the caller saw nothing that rejects
struct BatchParts {
  std::vector<uint64_t> xy;
  int msm(bppp_ctx *ctx, const void *sc, const void *pt, size_t n);
  int finish(bppp_ctx *ctx, bool reject, uint64_t *combined_xy, int *accept);
};
}  // namespace bppp
namespace bppp {
// ---- the stage the tally entry points (csrc/rptally.hip, which defines it) and the excess signatures (csrc/rpexcess.hip) share: the job's
// checks, the pool decoded once, the plan of a pass and the segmented signed sums of its sums; and the two passes of a tally themselves, which
// the sums against stated keys (csrc/rpexkeys.hip) run over a pool and a CSR that they extend
namespace tally {
using bppp_tally::Levels;
// one call's arguments, all in HBM, and what the checks established
struct Job {
  bppp_rp *rp; const char *who;
  size_t rows, nsums, nnz;
  const uint8_t *coms; const uint32_t *start, *entries, *amt, *ty, *bl;
  std::vector<uint32_t> h_start;               // sum_start on the host, after validation
  bool zero_claims = false;
  size_t tail = 0;                             // points behind the decoded pool, filled by the caller (Ext::prepare); 0: a plain tally
  const char *bl_name = "claim_blinds";       // what the caller's ABI calls the third claim array, for tally_checks' text
};
struct Work {
  uint32_t *pool, *bad, *any, *sums, *malformed, *in_sc, *flag, *rec, *status, *zz, *zinv, *xy, *zero, *part[2];
  uint4 *items;
  uint32_t *rho, *prods, *red, *sc3, *msm_sc, *msm_pt;
  uint8_t *seed, *extra;
};
// claims: the three claim arrays of a tally are judged too (all given or all NULL)
// the arguments of a call as it names them; the type array of a binary handle is dropped
void fill(Job &J, bppp_rp *rp, const char *who, size_t rows, const void *coms, size_t nsums, const void *start, const void *entries, size_t nnz, const void *amt,
          const void *ty, const void *bl);
int tally_checks(Job &J, bool null_args, bool claims);
std::vector<size_t> chunk_bounds(const Job &J);
Levels plan_levels(const Job &J, size_t t0, size_t t1);
// the passes of a job over the workspace (cb: their bounds), the levels of each and the largest of every size that carve takes
struct Plan { std::vector<size_t> cb; std::vector<Levels> plans; size_t ns_max = 0, ni = 0, np[2] = {0, 0}; };
Plan make_plan(const Job &J);
int carve(const Job &J, size_t ns, bool each, size_t ni, const size_t np[2], bool batch, size_t ne, Work &W, size_t extra = 0);
int decode_pool(const Job &J, const Work &W);
// W.sums [ns][XYZZ_WORDS] and W.malformed [ns] of the sums [t0, t0 + ns), planned as L; zeroes W.any[0..1]
int sum_launches(const Job &J, const Work &W, size_t t0, size_t ns, const Levels &L);
// k_rp_tally_affine: n XYZZ points and the inverses of their ZZ ZZZ (zero: the all-zero point) -> affine
int affine_launch(bppp_ctx *ctx, size_t n, const uint32_t *sums, const uint32_t *zinv, uint32_t *out);
// What a caller adds to the two passes below; with nullptr they are the plain tally, launch for launch.  The job it hands in has passed tally_checks
// over the caller's own CSR and then carries the EXTENDED h_start and nnz (the plan and the sizes come from them) and J.tail; start and entries still
// name the caller's arrays.  prepare runs once per pass over the workspace, after decode_pool and on a copy of the job: it fills the tail of W.pool
// and points the copy's start / entries at extended arrays of its own in W.extra (`extra` bytes).  judge runs in each_pass after k_rp_tally_compare
// of sums [t0, t0 + ns) and may overrule W.status (and W.zz when zz is set).  rejects runs in batch_run after the last pass: what the combined point
// cannot show.
struct Ext {
  size_t extra = 0;
  std::function<int(Job &J, const Work &W)> prepare;
  std::function<int(const Work &W, size_t t0, size_t ns, bool zz)> judge;
  std::function<int(const Work &W, bool &reject)> rejects;
};
// every sum decided on its own: status [nsums] and, when not NULL, sums_xy [nsums][8], both on the host
int each_pass(const Job &J, uint32_t *status, uint64_t *sums_xy, const Ext *ext = nullptr);
// the two steps of batch_run's pass that assemble its MSM, for a caller that runs the MSM itself (csrc/rpblock.hip).  batch_weights: the claimed
// scalars of sums [t0, t0 + ns) (W.in_sc, W.flag; W.any[1] for a non-canonical one), their weights W.rho at job positions j0 .. under W.seed, and the
// three negated column sums W.sc3 (the scalars of g, H0, H1).  batch_terms: entries [e0, e0 + n) of those sums -> n scalars and points; W.any[0] is
// raised by an entry that gathers the infinity encoding.
int claim_scalars(const Job &J, const Work &W, size_t t0, size_t ns);
int batch_weights(const Job &J, const Work &W, size_t t0, size_t ns, uint64_t j0);
int batch_terms(const Job &J, const Work &W, size_t t0, size_t ns, size_t e0, size_t n, uint32_t *sc, uint32_t *pt);
// all sums by one weighted combination per pass; status (may be NULL) by one each_pass when rejected; *accept is 0 on entry
int batch_run(const Job &J, uint64_t index_offset, const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy, const Ext *ext = nullptr);
}  // namespace tally
}  // namespace bppp
int rp_ensure_comb(bppp_rp *rp);      // csrc/rpprove.hip
// the handle (and its twin) proves over table t from now on (nullptr: none): t gains a holder, the table held before loses one and is
// freed with its last holder (csrc/rpprove.hip)
void rp_set_comb(bppp_rp *rp, bppp::CombTable *t);
namespace bppp {
inline size_t rp_basis_points(const bppp_rp *rp) { return rp->c_points.size() / 8 - 1; }     // [g | H | G]: c_points without h
// one handle's basis is a prefix of the other's (compared point by point, never by seed or tag)
inline bool rp_same_stream(const bppp_rp *a, const bppp_rp *b) {
  const size_t n = std::min(rp_basis_points(a), rp_basis_points(b));
  return memcmp(a->c_points.data() + 8, b->c_points.data() + 8, n * 64) == 0;
}
}  // namespace bppp
