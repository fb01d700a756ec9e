/*
 * bppp.h — C ABI of libbppp_hip.so: the MI355X (gfx950) implementation of the Bulletproofs++
 * hot path of Liam-Eagen/BulletproofsPP.  Plain pointers and sizes only; no C++/torch types.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository root).  INTEGRATION.md shows the Haskell `foreign import ccall` stubs that bind
 * these symbols behind the reference's own typeclasses (FastInnerProduct / BPOpening).
 *
 * Data formats (all little-endian, limb 0 least significant):
 *   scalar  Fr : 4 x uint64, canonical integer in [0, n)              (as FastPrime's 4 words,
 *                src/Data/Field/Galois/FastPrime/Internal.hs:152-176; Encoding.hs:75-86)
 *   point      : 8 x uint64 = affine x[4] ++ y[4], canonical in [0, p); infinity = all zero
 *                (what `toA` yields, src/Commitment.hs:172-176; (0,0) is not on y^2 = x^3 + 7)
 *   reduced scalar (ReducedScalar (Prime p) = Integer, Commitment.hs:270): sign flag + 3 x uint64
 *                magnitude (< 2^130; rationalReducedScalarLength = 129, Commitment.hs:286)
 *
 * Buffers named d_* are DEVICE pointers (HBM-resident, 16-byte aligned); everything else is host
 * memory.  A device buffer is exactly as long as its description says ([count][bytes a record],
 * nothing rounded up to 16 bytes or to an allocation's granularity) and needs no alignment above
 * 16 bytes, so buffers may be packed into one arena: no entry point writes behind the stated end
 * of an output or into a buffer declared const (tests/test_gpu_guarded_outputs.py).
 * All calls are synchronous with respect to the caller on return (outputs are valid),
 * matching a Haskell `foreign import ccall safe`.  A context is bound to one GPU and one HIP
 * stream and is not thread-safe; use one context per thread/GPU.
 *
 * Every function returns BPPP_OK (0) or a negative BPPP_ERR_* code; bppp_last_error() gives text.
 *
 * Handle lifetime: every child handle (bppp_nl, bppp_nlb, bppp_ip, bppp_trrp, bppp_rp, bppp_basis) holds a reference on its context.
 * bppp_ctx_destroy closes the context (further calls through it or its children fail with BPPP_ERR_ARG) and drops the caller's
 * reference; the stream and workspaces are released when the last child is destroyed, so finalisers may run in any order.
 *
 * Untrusted input: the verifier entry points that take DECODED values (bppp_nl_verify, bppp_ip_verify, bppp_nl_verify_batch_device)
 * check that proof-supplied scalars are canonical (< n) and points are on the curve (or the infinity encoding) and return
 * BPPP_ERR_ARG / BPPP_ERR_POINT otherwise; the batch weights rho must be non-zero.  The entry points that take the reference's FILES
 * (bppp_rp_verify_batch*, bppp_rp_verify_shard_device) decode them as the reference does: `get` of Binary (Prime p) ends in toP
 * (src/Encoding.hs:76-80), i.e. a coordinate >= p or a scalar >= n is REDUCED, not refused, so a proof has more than one accepted
 * byte encoding (the files are malleable exactly as the reference's are); an x with no curve point is BPPP_RP_MALFORMED.
 *
 * Side channels: the PROVER entry points are not constant-time.  The fixed-base comb walk (csrc/comb.hip) indexes its HBM table by
 * the signed digits of secret scalars (blindings included) and skips zero scalars per lane, and the bucket method sorts by secret
 * digits; memory access pattern and running time depend on the witness.  The reference is not constant-time either (Integer /
 * GMP arithmetic, testBit-driven additions, src/Commitment.hs:325-335); a deployment that shares the GPU with an adversary needs
 * its own isolation.
 */
#ifndef BPPP_H
#define BPPP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)

#define BPPP_OK 0
#define BPPP_ERR_ARG (-1)      /* bad length / null pointer / unsupported parameter */
#define BPPP_ERR_HIP (-2)      /* a HIP runtime call or kernel launch failed */
#define BPPP_ERR_NODEVICE (-3) /* no gfx950 GPU visible */
#define BPPP_ERR_POINT (-4)    /* a proof-supplied point is not on the curve (verifier entry points validate their inputs) */

typedef struct bppp_ctx bppp_ctx;

/* ---- context ---------------------------------------------------------------------------- */
int bppp_ctx_create(int device, bppp_ctx **out);
void bppp_ctx_destroy(bppp_ctx *ctx);
/* run all work of this context on an existing hipStream_t (e.g. torch's current stream);
 * NULL = the context's own stream.  The call returns after the stream bound before has drained.
 * With a caller's stream bound, the d_* inputs of a call may be produced by work the caller enqueued
 * earlier on that stream and need not be complete when the library is entered: whatever reads them,
 * kernels and copies alike, is ordered behind that work.  On return nothing of the call is in flight
 * on any stream - the bound one, the null stream or the context's second stream - for refusals and
 * failing return codes too, so outputs may be read from any stream at once.
 * tests/test_gpu_stream_order.py holds both for every device entry point: inputs delivered late on
 * a busy bound stream, outputs read off-stream on return. */
int bppp_ctx_set_stream(bppp_ctx *ctx, void *hip_stream);
const char *bppp_last_error(const bppp_ctx *ctx);
const char *bppp_version(void);

/* ---- a1: FastInnerProduct.innerProduct / commit --------------------------------------------
 * Replaces `innerProduct :: [(Scalar v, v)] -> v` (src/Commitment.hs:325-335) as reached through
 * `commit` (src/Commitment.hs:416-417): out = sum_i scalars[i] * points[i], as the canonical
 * affine point.  Zero scalars and points at infinity are allowed (dotWith pads with both,
 * Commitment.hs:423-424).  n = 0 returns infinity (the reference would crash on `head []`,
 * Commitment.hs:328 — documented deviation).  Algorithm: signed-digit Pippenger bucket method
 * (a different algorithm from the reference's 256-row Straus loop; same group element). */
int bppp_msm(bppp_ctx *ctx, const uint64_t *scalars, const uint64_t *points_xy, size_t n, uint64_t out_xy[8]);
/* same, inputs already resident in HBM; window_bits = 0 lets the library choose. */
int bppp_msm_device(bppp_ctx *ctx, const void *d_scalars, const void *d_points_xy, size_t n, int window_bits,
                    uint64_t out_xy[8]);
/* `batch` independent MSMs of n terms each in one pass (one per proof: verifyBPM's single commit,
 * src/Bulletproof.hs:377).  d_scalars is [batch][n]; d_points_xy is [batch][n] when shared_points == 0, one [n] basis used
 * by every instance when shared_points == 1, and [batch / d][n] (one basis per d consecutive instances, e.g. the X and R
 * commitments of one proof) when shared_points == d >= 2.  out_xy is [batch][8] on the host. */
int bppp_msm_batch_device(bppp_ctx *ctx, const void *d_scalars, const void *d_points_xy, size_t n, size_t batch,
                          int shared_points, int window_bits, uint64_t *out_xy);
/* Sum of n affine points (complete group law): the local tail of a sharded MSM after the ranks all-gathered their partial points
 * (SURVEY.md 8e).  Host arithmetic, microseconds for the 2..64 points it is meant for. */
int bppp_sum_points(bppp_ctx *ctx, const uint64_t *points_xy, size_t n, uint64_t out_xy[8]);

/* ---- registered basis with fixed-base precomputation (SURVEY.md 8(b) "Ownership": basis points "may be registered once and
 * referenced by handle since G, H are fixed per setup", src/RangeProof/TypedReciprocal.hs:348-359) ---------------------------
 * The handle owns a copy of the n points in HBM plus the table T[w][i] = 2^(c w) P_i (W = 256 / c + 1 rows of n affine points,
 * W * n * 64 bytes; built on the device at creation).  bppp_msm_basis is `innerProduct` (src/Commitment.hs:325-335) over the first
 * n_terms registered points — `batch` instances, d_scalars [batch][n_terms] in HBM, out_xy [batch][8] on the host — with all
 * windows sharing ONE bucket set: one bucket reduction per instance instead of W, no window combine.  Results equal
 * bppp_msm_batch_device over the same points bit for bit.  window_bits = 0 lets the library choose for `batch_hint` instances
 * of n terms.  The arbitrary-point entry points above stay the general route (and the headline of bench.py). */
typedef struct bppp_basis bppp_basis;
int bppp_basis_create(bppp_ctx *ctx, const uint64_t *points_xy, size_t n, int window_bits, size_t batch_hint, bppp_basis **out);
int bppp_basis_create_device(bppp_ctx *ctx, const void *d_points_xy, size_t n, int window_bits, size_t batch_hint, bppp_basis **out);
void bppp_basis_destroy(bppp_basis *basis);
int bppp_basis_info(const bppp_basis *basis, size_t *n, int *window_bits, size_t *table_bytes);
int bppp_msm_basis(bppp_basis *basis, const void *d_scalars, size_t n_terms, size_t batch, uint64_t *out_xy);
/* For MANY instances over a SHORT basis (the prover's commitments: thousands of MSMs of ~775 terms over a setup's points) the handle can
 * also hold every multiple of every window, tab[w][i][d-1] = d 2^(c w) P_i: bppp_msm_basis of >= 64 instances is then one mixed addition
 * per non-zero signed c-bit digit into one accumulator — no sort, no buckets, no reduction, no doubling.  window_bits = 0 takes the widest
 * window (<= 18) whose table fits budget_bytes (W * n * 2^(c-1) * 64 bytes: 27.6 GB for 774 points at c = 16, 4.1 GB at c = 13).  Same
 * results bit for bit. */
int bppp_basis_enable_comb(bppp_basis *basis, int window_bits, size_t budget_bytes, int *window_bits_out, size_t *table_bytes);

/* ---- a7: SplitScalar.rationalReduceScalar (host) ------------------------------------------
 * Replaces rationalReduceScalar for `Prime p` (src/Commitment.hs:242-255, instance :269-288):
 * returns (a, b) with x = a / b (mod n), following the reference's egcd step-for-step (its
 * choice of (a, b) fixes the collapsed basis points, so it must match exactly). */
int bppp_rational_reduce(const uint64_t x[4], uint64_t a_mag[3], int *a_neg, uint64_t b_mag[3], int *b_neg);

/* ---- a8: projectivePairIP via collapsePoints, over a whole vector ---------------------------
 * Replaces `collapsePoints b a gL gR = projectivePairIP (b, gL) (a, gR)` (src/Bulletproof.hs:213-214,
 * src/Commitment.hs:343-353) mapped over adjacent pairs by mapHalves (src/Bulletproof.hs:88-90):
 * out[j] = b * pts[2j] + a * pts[2j+1] for j < ceil(n/2); an odd tail pairs with infinity.
 * The same (a, b) is used for every pair (one uniform add/double schedule per wavefront). */
int bppp_fold_points(bppp_ctx *ctx, const uint64_t b_mag[3], int b_neg, const uint64_t a_mag[3], int a_neg,
                     const uint64_t *points_xy, size_t n, uint64_t *out_xy);
int bppp_fold_points_device(bppp_ctx *ctx, const uint64_t b_mag[3], int b_neg, const uint64_t a_mag[3], int a_neg,
                            const void *d_points_xy, size_t n, void *d_out_xy);

/* ---- a7 / a8, Eisenstein variant: the reference's FastPrime configuration (src/Commitment.hs:293-306) -------------------------
 * ReducedScalar = Eis Integer: a reduced scalar is a0 + a1*w (w^3 = 1; w acts on scalars as lambda, on points as the
 * endomorphism (x, y) -> (beta x, y), src/Data/Curve/CM.hs:25-27) with components of about 65 bits
 * (rationalReducedScalarLength = 65).  bppp_rational_reduce_eis is the class default rationalReduceScalar (Commitment.hs:242-255)
 * over that instance: reducedChar = conjEis . charEis, reduceScalar = decomposeEis (FastPrime.hs:186-205), Euclid with the
 * nearest-integer quotRem of Integral (Eis a) (src/Data/Field/Eis.hs:72-82), stop at the first r with (normEis r)^2 <= 2n.
 * Components: mag[2*k], mag[2*k+1] = the two 64-bit limbs of |component k|, neg[k] its sign (k = 0: rational part, 1: w part).
 * bppp_fold_points_eis_device is projectivePairIP of that configuration (Commitment.hs:343-353 with the FastInnerProduct instance
 * :374-398, 65 rows) mapped over adjacent pairs: out[j] = b' * pts[2j] + a' * pts[2j+1].  Same cost as the integer fold
 * (two 66-row walks instead of one 130-row walk): provided for parity with that configuration, not as the fast path. */
int bppp_rational_reduce_eis(const uint64_t x[4], uint64_t a_mag[4], int a_neg[2], uint64_t b_mag[4], int b_neg[2]);
int bppp_fold_points_eis_device(bppp_ctx *ctx, const uint64_t b_mag[4], const int b_neg[2], const uint64_t a_mag[4], const int a_neg[2],
                                const void *d_points_xy, size_t n, void *d_out_xy);

/* ---- a10/a11/a16: scalar halves of the Norm / Linear round (NL flavour) ---------------------
 * makeScalarsComs scalar sums (src/Bulletproof/NormArgument.hs:113-118 via foldXR :20-29):
 *   sx = sum_j q^(4j) xL_j xR_j,  sr = sum_j q^(4j) xR_j^2   over adjacent pairs (odd tail: xR = 0)
 * The caller applies the 2 n^2 q^3 / n^2 q^4 factors (host glue, one multiplication each). */
int bppp_norm_round_sums_device(bppp_ctx *ctx, const void *d_x, size_t n, const uint64_t q4[4], uint64_t sx[4],
                                uint64_t sr[4]);
/* Linear makeScalarsComs sums (NormArgument.hs:56-59): sx = sum cL xR + cR xL, sr = sum cR xR */
int bppp_lin_round_sums_device(bppp_ctx *ctx, const void *d_c, const void *d_x, size_t n, uint64_t sx[4],
                               uint64_t sr[4]);
/* X / R opening scalars of the Norm round (NormArgument.hs:117): d_xw[2j] = q xR_j,
 * d_xw[2j+1] = qinv xL_j (length 2*ceil(n/2)); d_rw[j] = xR_j (length ceil(n/2)). */
int bppp_norm_round_openings_device(bppp_ctx *ctx, const void *d_x, size_t n, const uint64_t q[4],
                                    const uint64_t qinv[4], void *d_xw, void *d_rw);
/* Linear X / R opening scalars (NormArgument.hs:59): d_xw[2j] = xR_j, d_xw[2j+1] = xL_j; d_rw[j] = xR_j */
int bppp_lin_round_openings_device(bppp_ctx *ctx, const void *d_x, size_t n, void *d_xw, void *d_rw);
/* scalar vector fold of collapse (NormArgument.hs:129 / :71): out[j] = u * x[2j] + v * x[2j+1]
 * with u = b0^-1, v = e q b0^-1 (norm) or e b0^-1 (linear x) or (u, v) = (b0, a0) (linear c). */
int bppp_fold_scalars_device(bppp_ctx *ctx, const uint64_t u[4], const uint64_t v[4], const void *d_x, size_t n,
                             void *d_out);

/* ---- a5: batchInverse ----------------------------------------------------------------------
 * Replaces batchInverse (src/Data/Field/BatchInverse.hs:14-24; used by normalizes, src/Commitment.hs:125, :153, and by
 * the range-proof phases, src/RangeProof/TypedReciprocal.hs:193-195): out[i] = x[i]^-1, with 0 -> 0, over n canonical
 * field elements in HBM.  modulus: 0 = Fq (coordinates), 1 = Fr (scalars).  Montgomery's trick runs along each lane
 * (8 values per inversion); d_out may alias d_x. */
int bppp_batch_inverse_device(bppp_ctx *ctx, const void *d_x, size_t n, int modulus, void *d_out);

/* ---- a15: tensor' (challenge expansion) -----------------------------------------------------
 * Replaces the list instance of tensor' (src/Bulletproof.hs:94-95) as used by expandChallenges
 * (NormArgument.hs:73-81, :131-145): out[i * 2^k + t] = bs[i] * prod over rounds of (q_r or e_r)
 * selected by the bits of t.  es (k challenges, LAST ROUND FIRST as verifyBPM holds them,
 * Bulletproof.hs:374) and qs (k weights, first round first) are host arrays of k scalars. */
int bppp_tensor_device(bppp_ctx *ctx, const uint64_t *bs, size_t nb, const uint64_t *es, const uint64_t *qs,
                       size_t k, void *d_out);

/* ---- a10-a14: the norm-linear argument with device-resident state (BPOpening / BPCollection) ---
 * `bppp_nl` is the device counterpart of `PedersenScalarVector (NormLinear f) v s`
 * (src/Commitment.hs:487-501, src/Bulletproof/NormArgument.hs:153-162): the norm vector x with basis G,
 * the linear vector (c, x) with basis H, the scalar s on g, and the deferred normalisations
 * (BPFrame''.nrmlz'', src/Bulletproof.hs:167).  The Fiat-Shamir oracle stays with the caller
 * (injected in the reference too, src/ZKP.hs:73-77). */
typedef struct bppp_nl bppp_nl;
/* makeNormLinearBP' 1 q cs nss ngs lss lgs (NormArgument.hs:162) inside makePSV s g (Commitment.hs:490-491) */
int bppp_nl_create(bppp_ctx *ctx, const uint64_t s[4], const uint64_t g_xy[8], const uint64_t q[4], const uint64_t *norm_x,
                   const uint64_t *norm_g_xy, size_t nlen, const uint64_t *lin_c, const uint64_t *lin_x, const uint64_t *lin_h_xy,
                   size_t llen, bppp_nl **out);
void bppp_nl_destroy(bppp_nl *nl);
int bppp_nl_lengths(const bppp_nl *nl, size_t *nlen, size_t *llen);
/* first half of proveRoundM (src/Bulletproof.hs:346-350): makeScalarsComs (NormArgument.hs:113-118, :56-59,
 * Bulletproof.hs:258-261) and ac = commit(sX, X-opening), bc = commit(sR, R-opening) as one batched MSM. */
int bppp_nl_round_commit(bppp_nl *nl, uint64_t sX[4], uint64_t X_xy[8], uint64_t sR[4], uint64_t R_xy[8]);
/* second half of proveRoundM (Bulletproof.hs:352-354): (e0, e1) = makeEs e = (e, e^2 - 1); s += e0 sX + e1 sR;
 * collapse e (NormArgument.hs:123-129, :64-71): scalar folds, basis folds by collapsePoints, q <- q^2. */
int bppp_nl_round_collapse(bppp_nl *nl, const uint64_t e[4]);
/* getWitness (NormArgument.hs:121, :62; Bulletproof.hs:264): normalisation applied; lengths from bppp_nl_lengths */
int bppp_nl_get_witness(bppp_nl *nl, uint64_t *norm_w, uint64_t *lin_w);
/* raw current state (vectors NOT multiplied by the normalisations) for parity checks; any pointer may be NULL */
int bppp_nl_download(bppp_nl *nl, uint64_t *norm_x, uint64_t *norm_g_xy, uint64_t *lin_c, uint64_t *lin_x, uint64_t *lin_h_xy,
                     uint64_t s[4], uint64_t q[4], uint64_t norm_nrmlz[4], uint64_t lin_nrmlz[4]);
/* verifyBPM (src/Bulletproof.hs:370-378) after the challenges are known: expandChallenges
 * (NormArgument.hs:73-81, :131-145; Bulletproof.hs:268-269) on the device, then the single commit over
 * verifyWith's term list (Bulletproof.hs:362-368): wit' ++ initCom ++ [e0 X_j, e1 R_j].  `es` and
 * `responses_xy` (k pairs X, R) are LAST ROUND FIRST as the reference holds them (Bulletproof.hs:359, :374).
 * out_xy is the committed point; the proof verifies iff it is infinity (all zero). */
int bppp_nl_verify(bppp_ctx *ctx, const uint64_t q[4], const uint64_t sp[4], const uint64_t g_xy[8], const uint64_t *pub_norm,
                   const uint64_t *norm_g_xy, size_t nlen, const uint64_t *pub_lin_c, const uint64_t *pub_lin_x, const uint64_t *lin_h_xy,
                   size_t llen, const uint64_t *es, size_t k, const uint64_t *wit_norm, size_t fn, const uint64_t *wit_lin, size_t fl,
                   const uint64_t *init_scalars, const uint64_t *init_points_xy, size_t ninit, const uint64_t *responses_xy, uint64_t out_xy[8]);

/* The injected Fiat-Shamir oracle (MonadZKP.oracle, src/ZKP.hs:57, :96-101; app/Main.hs:75-80 is the CLI's SHA-256 one):
 * called with the WHOLE transcript so far, newest commitments first, as affine points; writes the first challenge. */
typedef void (*bppp_oracle_fn)(void *user, const uint64_t *transcript_xy, size_t npoints, uint64_t challenge[4]);
/* proveBPM (src/Bulletproof.hs:357-359): n_rounds x proveRoundM with the caller's oracle; responses and challenges come out
 * LAST ROUND FIRST.  transcript_xy (capacity transcript_cap points) holds *ntranscript earlier commitments on entry and
 * receives the responses (newest first). */
int bppp_nl_prove(bppp_nl *nl, size_t n_rounds, bppp_oracle_fn oracle, void *user, uint64_t *transcript_xy, size_t *ntranscript,
                  size_t transcript_cap, uint64_t *responses_xy, uint64_t *es);
/* the challenge derivation of verifyBPM (src/Bulletproof.hs:374) with the same oracle contract */
int bppp_nl_verify_challenges(bppp_oracle_fn oracle, void *user, const uint64_t *responses_xy, size_t k, uint64_t *transcript_xy,
                              size_t *ntranscript, size_t transcript_cap, uint64_t *es);

/* ---- lockstep batch prover: `batch` norm-linear arguments of one shape advance round by round together ----------------
 * Same functions as bppp_nl_* (proveRoundM, src/Bulletproof.hs:346-355) with a leading batch dimension on every array:
 * one proof cannot fill the chip (its MSMs have < 800 terms, its basis fold is one ~1 ms dependency chain), B proofs
 * share every launch.  The starting basis (g, G, H) is shared; q, s and the vectors are per proof ([batch][...]). */
typedef struct bppp_nlb bppp_nlb;
int bppp_nlb_create(bppp_ctx *ctx, size_t batch, const uint64_t *s, const uint64_t g_xy[8], const uint64_t *q, const uint64_t *norm_x,
                    const uint64_t *norm_g_xy, size_t nlen, const uint64_t *lin_c, const uint64_t *lin_x, const uint64_t *lin_h_xy, size_t llen,
                    bppp_nlb **out);
void bppp_nlb_destroy(bppp_nlb *nlb);
int bppp_nlb_lengths(const bppp_nlb *nlb, size_t *batch, size_t *nlen, size_t *llen);
int bppp_nlb_round_commit(bppp_nlb *nlb, uint64_t *sX, uint64_t *X_xy, uint64_t *sR, uint64_t *R_xy);   /* [batch][4], [batch][8] */
int bppp_nlb_round_collapse(bppp_nlb *nlb, const uint64_t *es);                                         /* [batch][4] */
int bppp_nlb_get_witness(bppp_nlb *nlb, uint64_t *norm_w, uint64_t *lin_w, uint64_t *s);

/* ---- a12: the inner-product flavour (src/Bulletproof/InnerProductArgument.hs; the CLI's default, app/Parse.hs:100)
 * Same contract as bppp_nl_*.  `r` is the argument of makeNorm (:194-206; q = r^4): the norm vector (nlen scalars on nlen
 * points) is re-expressed as ceil(nlen/2) inner-product pairs with the basis change g' = g1 + r g0, h' = g1 - r g0 done
 * on the device (one full scalar multiplication per pair, :204).  makeEs e = (1/e, e) (:68). */
typedef struct bppp_ip bppp_ip;
int bppp_ip_create(bppp_ctx *ctx, const uint64_t s[4], const uint64_t g_xy[8], const uint64_t r[4], const uint64_t *norm_s,
                   const uint64_t *norm_g_xy, size_t nlen, const uint64_t *lin_c, const uint64_t *lin_x, const uint64_t *lin_h_xy,
                   size_t llen, bppp_ip **out);
void bppp_ip_destroy(bppp_ip *ip);
int bppp_ip_lengths(const bppp_ip *ip, size_t *ip_len, size_t *llen);   /* ip_len = number of (x, y) pairs */
/* makeScalarsComs (:70-81, :155-158 via foldLR :17-26) + the two commits of proveRoundM (src/Bulletproof.hs:348-350) */
int bppp_ip_round_commit(bppp_ip *ip, uint64_t sL[4], uint64_t L_xy[8], uint64_t sR[4], uint64_t R_xy[8]);
/* s += e^-1 sL + e sR; collapse (:86-101, :162-170) */
int bppp_ip_round_collapse(bppp_ip *ip, const uint64_t e[4]);
/* getWitness: norm_w holds 2*ip_len scalars (nx x - ny y, nx x + ny y) (:222-223); lin_w llen scalars; s the PSV scalar */
int bppp_ip_get_witness(bppp_ip *ip, uint64_t *norm_w, uint64_t *lin_w, uint64_t s[4]);
/* verifyBPM for this flavour: basis change, expandChallenges (:103-124, :172-181), one MSM; out must be infinity */
int bppp_ip_verify(bppp_ctx *ctx, const uint64_t r[4], const uint64_t sp[4], const uint64_t g_xy[8], const uint64_t *pub_norm,
                   const uint64_t *norm_g_xy, size_t nlen, const uint64_t *pub_lin_c, const uint64_t *pub_lin_x, const uint64_t *lin_h_xy,
                   size_t llen, const uint64_t *es, size_t k, const uint64_t *wit_norm, size_t fn, const uint64_t *wit_lin, size_t fl,
                   const uint64_t *init_scalars, const uint64_t *init_points_xy, size_t ninit, const uint64_t *responses_xy, uint64_t out_xy[8]);

/* ---- batch verifier (BASELINE config 5) --------------------------------------------------------
 * No reference implementation exists (TODO at src/RangeProof/TypedReciprocal.hs:469-472); semantics per
 * out = sum_b rho[b] * MSM(T_b) with T_b the verifyWith term list of proof b
 * (src/Bulletproof.hs:362-368, :375-377).  All proofs share the shape (nlen, llen, k rounds, fn, fl, ninit)
 * and the basis (G, H, g); q, sp, the public vectors, challenges, final openings, initCom terms and responses
 * are per proof, stored [batch][...] contiguously in HBM.  Scalars on the shared basis are summed over the
 * batch on the device; one MSM of (nlen + llen + 1) + batch * (ninit + 2k) terms decides every proof:
 * out is infinity iff all verify (rho random, rho[0] = 1 by convention). */
int bppp_nl_verify_batch_device(bppp_ctx *ctx, size_t batch, size_t nlen, size_t llen, size_t k, size_t fn, size_t fl, size_t ninit,
                                const void *d_g_xy, const void *d_norm_g_xy, const void *d_lin_h_xy, const void *d_rho, const void *d_q,
                                const void *d_sp, const void *d_pub_norm, const void *d_pub_lin_c, const void *d_pub_lin_x,
                                const void *d_es, const void *d_wit_norm, const void *d_wit_lin, const void *d_init_scalars,
                                const void *d_init_points_xy, const void *d_responses_xy, uint64_t out_xy[8]);

/* The same batch check for the inner-product flavour (src/Bulletproof/InnerProductArgument.hs; verifyBPM src/Bulletproof.hs:370-378 with
 * expandChallenges :103-124, :172-181 and makeEs e = (1/e, e) :68).  Same layout and result as bppp_nl_verify_batch_device; d_r holds the
 * per-proof argument of makeNorm (:194-206; the range proofs pass their challenge q), fn counts the SCALARS of the final norm witness
 * (two per inner-product pair, as getWitness :222-223 lays them out).  makeNorm's basis change g' = g1 + r g0, h' = g1 - r g0 depends
 * on the proof, so it is folded into the scalars on the ORIGINAL basis — x' g' + y' h' = r (x' - y') g0 + (x' + y') g1 — and the
 * per-proof scalars still sum onto the one shared basis [G | H | g]: no scalar multiplication per basis pair (the reference's TODO at
 * InnerProductArgument.hs:187-190, :225-227) and one MSM of (nlen + llen + 1) + batch * (ninit + 2k) terms for the whole batch. */
int bppp_ip_verify_batch_device(bppp_ctx *ctx, size_t batch, size_t nlen, size_t llen, size_t k, size_t fn, size_t fl, size_t ninit,
                                const void *d_g_xy, const void *d_norm_g_xy, const void *d_lin_h_xy, const void *d_rho, const void *d_r,
                                const void *d_sp, const void *d_pub_norm, const void *d_pub_lin_c, const void *d_pub_lin_x,
                                const void *d_es, const void *d_wit_norm, const void *d_wit_lin, const void *d_init_scalars,
                                const void *d_init_points_xy, const void *d_responses_xy, uint64_t out_xy[8]);

/* ---- the optional endomorphism (GLV) path ---------------------------------------------------------------
 * bppp_glv_decompose_device: decomposeFastPrimeEis (src/Data/Field/Galois/FastPrime.hs:186-205) for n canonical scalars:
 * x = a + b*lambda (mod n), the reference's own (a, b) including its one-step rounding.  d_a_mag / d_b_mag: [n][4] magnitudes,
 * d_signs: [n] uint32, bit 0 = a negative, bit 1 = b negative (bit 2 would flag a magnitude over 256 bits; it cannot happen).
 * bppp_msm_glv_device: the same group element as bppp_msm_device through that decomposition — 2n half-length terms
 * |a| * (+-P), |b| * (+-(beta x, y)) (SplitScalar / FastInnerProduct of FastPrime, src/Commitment.hs:293-306, :374-398; cmConj,
 * src/Data/Curve/CM.hs:25-27).  Not faster at 2^20 (same number of bucket additions); provided for parity with that option. */
int bppp_glv_decompose_device(bppp_ctx *ctx, const void *d_scalars, size_t n, void *d_a_mag, void *d_b_mag, void *d_signs);
int bppp_msm_glv_device(bppp_ctx *ctx, const void *d_scalars, const void *d_points_xy, size_t n, uint64_t out_xy[8]);

/* ---- range-proof verifier: public scalars from challenges, on the device ----------------------------------------------
 * The scalar work of verifyTRRPM (src/RangeProof/TypedReciprocal.hs:449-467) for a batch of proofs of ONE setup: makePhase2s on
 * the unit witness (:185-205), makeSharedCoeffs (:213-216), makePublicConsts (:246-274), makeBpCoeffs (:391-396) and the opening
 * scalars of TranscriptTRRP (:293-297).  bppp_trrp_create uploads the setup's static structure:
 *   per norm position i < nlen (the verifier's Phase1 list, types first when has_types):
 *     pos_kind[i]  = 0 typing | 1 inline | 2 shared, | 0x100 if the range is an output (typing) | 0x200 if it is assumed (typing)
 *     pos_range[i] = index of the range;  pos_slot[i] = index of the digit's base in the sorted base list (base map x^(3+2 slot));
 *     pos_sym[i]   = index into syms of the inline symbol, or 0xFFFFFFFF;  pos_coeff[i] = the digit coefficient b (4 limbs)
 *   per range: range_min (4 limbs, canonical mod n), range_assumed;  syms: the distinct values s whose 1/(e+s) is needed
 *   cs_slot / cs_sym [llen - 6]: base slot and symbol of each shared-digit linear weight;  public amounts: is_out, amount, type symbol.
 * flavour 0 = NL (q0 = q^2), 1 = IP (q0 = -q^2).
 * bppp_trrp_public_device: d_challenges is [batch][7][4] = (e, x, r0, q, x', r1, t) per proof; outputs, all in HBM:
 *   d_q [batch][4], d_sp [batch][4], d_pub_norm [batch][nlen][4], d_pub_lin_c [batch][llen][4] and
 *   d_init_scalars [batch][4 + nranges][4] in the proof's commitment order blCom, rCom, dmCom, mCom, nComs...
 * — exactly the arrays bppp_nl_verify_batch_device reads (its pub_lin_x is all zero for these proofs).  Synchronous on return
 * like every other call: the five arrays are complete in HBM (it used to return with its kernels queued). */
typedef struct bppp_trrp bppp_trrp;
int bppp_trrp_create(bppp_ctx *ctx, int flavour, int has_types, size_t nlen, size_t llen, size_t nranges, const uint32_t *pos_kind,
                     const uint32_t *pos_range, const uint32_t *pos_slot, const uint32_t *pos_sym, const uint64_t *pos_coeff,
                     const uint64_t *range_min, const uint32_t *range_assumed, size_t nsyms, const uint64_t *syms, const uint32_t *cs_slot,
                     const uint32_t *cs_sym, size_t npub, const uint32_t *pub_is_out, const uint64_t *pub_amount, const uint32_t *pub_sym,
                     bppp_trrp **out);
void bppp_trrp_destroy(bppp_trrp *t);
int bppp_trrp_public_device(bppp_trrp *t, size_t batch, const void *d_challenges, void *d_q, void *d_sp, void *d_pub_norm, void *d_pub_lin_c,
                            void *d_init_scalars);

/* ---- the range-proof layer end to end: encoded proofs in, accept / reject out ------------------
 * `bppp_rp` is one typed-reciprocal setup (setup, src/RangeProof/TypedReciprocal.hs:332-359) resident on the device: the ranges
 * with their digit coefficients (makeRangeData :103-120), the Phase1 layout (:133-169), the round count (optimalWitnessSize,
 * src/Bulletproof/NormArgument.hs:165-178) and the REGISTERED BASIS g, G, H — uploaded once, referenced by every later call
 * (G, H are fixed per setup, TypedReciprocal.hs:348-359).  Argument flavour: 0 = norm-linear (Bulletproof.NormArgument), 1 = inner product
 * (Bulletproof.InnerProductArgument, the CLI's default, app/Parse.hs:100).  Both have the batch verifier and the lockstep batch prover
 * (bppp_rp_prove_batch; flavour 1 proves with every commitment as an MSM over the registered ORIGINAL basis — makeNorm's basis change and
 * every point fold are carried in the scalars, same bytes as the folding route; with the handle's comb table in place the whole proof,
 * argument included, is one stream of kernels (csrc/ipb.hip), before that the field algebra of this flavour runs on the host cores).
 *
 * bppp_rp_create: `ranges` as the schema gives them (app/Parse.hs:125-172): base, min, max (plain INTEGERS in 256-bit two's complement — a minimum may be negative, examples/rec_test — max exclusive
 * as in makeRangeData), flags.  `pubs`: the public (isOutput, type, amount) triples.  `points_xy` = h : g : hs ++ gs, the stream the
 * CLI takes from getPoints (app/Main.hs:68-72, :260); at least 2 + lin_len + norm_len points (validated: on the curve).
 * `oracle_tag` (may be NULL = the reference's input) is prepended to every hashed message (domain separation for tests).
 *
 * Schemas the reference's setup takes and this library refuses with BPPP_ERR_ARG and a message, from every bppp_rp_create*:
 *   - an INLINE range with more reciprocal symbols than digits ((1 if it has a leading bit) + base - 1 > number of digits, e.g. base 16 over
 *     [0, 100)): the reference's own norm vector is then longer than its basis ("... unsupported layout");
 *   - a range of width 2 <= max - min < base, shared, inline or assumed: makeRangeData's leading coefficient max - min - base is negative there and
 *     the other one is 1 under a digit of radix base, so a proof would bound value - min by base, not by max - min ("range narrower than its digit
 *     base: the reference's coefficients do not bound it").  Use a base <= max - min (base 2 fits every width >= 2);
 *   - a range of width 1 ("degenerate range: a digit coefficient is zero").
 * Size limits, checked at creation before anything is built (BPPP_ERR_ARG and a message that names the count and the limit); a setup that
 * bppp_rp_create accepts never fails later for its size:
 *   - at most 65535 ranges ("65536 ranges: at most 65535"): every prover route, the host algebra included, indexes ranges below 2^16;
 *   - at most 16 distinct digit bases among the ranges that are not assumed, a leading bit counting as base 2 ("17 distinct digit bases
 *     (a leading bit counts as base 2): at most 16");
 *   - at most 1022 reciprocal symbols: the digits 1 .. b - 1 of the widest shared or inline base b and the distinct public types that are not
 *     such a digit ("1023 reciprocal symbols (...): at most 1022").  So a shared digit base is at most 1023 — and smaller by the number of
 *     distinct public types; an inline base is bounded by its digits long before (base - 1 of them);
 *   - bppp_rp_create_binary: at most 1024 ranges ("1025 ranges: at most 1024 ranges").
 * bppp_rp_shape_of refuses the same ranges (it knows no public amounts: their types count at creation only).
 * Beyond 2470 ranges of small bases (less with a wider base: the phase kernels' LDS, csrc/rpprove_dev.hpp) a prove takes the HOST_ALGEBRA route
 * by itself, same bytes; beyond 3917 ranges and symbols together a verification computes its public scalars in three kernels over HBM instead
 * of one over LDS, at every batch size (csrc/trrp.hpp), same results.
 *
 * The Fiat-Shamir oracle of these entry points is the CLI's shaOracle (app/Main.hs:64-80) computed natively: challenge n =
 * decode (SHA-256 (tag <> show n <> show (length ps) <> foldMap (show x <> show y) ps)) over the WHOLE transcript, newest first
 * (src/ZKP.hs:96-101); `show` of a coordinate = its decimal integer (parity of that text with galois-field's Show instance is
 * unpinned), `decode` = Binary (Prime p): four big-endian 64-bit words, least significant first (Encoding.hs:75-79).
 * The injectable-oracle route stays available: bppp_trrp_public_device + bppp_nl_verify_batch_device from caller-made challenges. */
#define BPPP_RP_SHARED 1u  /* isShared  */
#define BPPP_RP_OUTPUT 2u  /* isOutput  */
#define BPPP_RP_ASSUMED 4u /* isAssumed */
typedef struct bppp_rp_range { uint32_t base; uint32_t flags; uint64_t min[4]; uint64_t max[4]; } bppp_rp_range;
typedef struct bppp_rp_public { uint32_t is_output; uint32_t reserved; uint64_t type[4]; uint64_t amount[4]; } bppp_rp_public;
typedef struct bppp_rp_shape {
  size_t nranges, norm_len, lin_len, rounds, final_norm, final_lin;
  size_t coms_bytes;            /* the commitments file of one proof: sign bytes + 32 per input commitment (Encoding.hs:130-134) */
  size_t proof_bytes;           /* the proof file: final witness scalars, sign bytes, 4 + 2*rounds x coordinates (RangeProof.hs:60-66) */
  size_t challenges_per_proof;  /* 7 + rounds */
} bppp_rp_shape;
typedef struct bppp_rp bppp_rp;
int bppp_rp_create(bppp_ctx *ctx, int flavour, int has_types, const bppp_rp_range *ranges, size_t nranges, const bppp_rp_public *pubs, size_t npub,
                   const uint64_t *points_xy, size_t npoints, const char *oracle_tag, bppp_rp **out);
/* RangeProof.Binary (src/RangeProof/Binary.hs) behind the same handle: setupBRP (:143-156).  `ranges`: base must be 2 and SHARED must not
 * be set (app/Parse.hs:141-146 refuses both); `conserve` = the schema's "conserved" (inputs, outputs and `net_public` — the net public
 * amount, inputs minus outputs, a plain integer in two's complement — must balance: witnessBRP :158-166 yields a witness only then);
 * `points_xy` = [h, g, h0, h1] ++ gs, at least 4 + nrmLen points (:147-148).  Every entry point that takes a bppp_rp then serves the
 * binary protocol: bppp_rp_info (lin_len = 2; proof file = final witness scalars, then blCom, dCom and the responses;
 * challenges_per_proof = 4 + rounds: q, x, r, t), bppp_rp_verify_batch* / _shard_device (verifyBRPM :206-222 with its two oracle
 * calls, then verifyBPM) and bppp_rp_prove_batch (proveBRPM :169-204 + proveBPM in lockstep; `types` is ignored, a binary proof is
 * untyped; from its first 1024 proofs on — COMB_MIN — the handle keeps a comb table of its basis, 21.5 GB for the 4099 points of 64 outputs of
 * 64 bits, and a proof is one stream of kernels, csrc/brpprove_dev.hip; before that the field algebra runs on the host cores; same bytes).  Both sides take the round count from optimalWitnessSize (the reference's prover uses integerLog 2 nrmLen - 1, which
 * agrees wherever its own proofs verify — SURVEY.md App. D-1). */
int bppp_rp_create_binary(bppp_ctx *ctx, int flavour, int conserve, const bppp_rp_range *ranges, size_t nranges, const uint64_t net_public[4],
                          const uint64_t *points_xy, size_t npoints, const char *oracle_tag, bppp_rp **out);
/* The two constructors with the basis named as the schema names it, by its "basisSeed": each generates the points its counterpart
 * requires for the shape (2 + lin_len + norm_len; 4 + nrmLen) with bppp_points_from_seed from candidate 0 and is the counterpart
 * called with them from there — same handle, same bytes, every argument error of the counterpart with its message, and those of
 * bppp_points_from_seed for the seed.  Handles seeded alike hold prefixes of one stream: bppp_rp_share_comb and the merging of
 * bppp_rp_verify_mixed work on them as on any handles of one basis. */
int bppp_rp_create_seeded(bppp_ctx *ctx, int flavour, int has_types, const bppp_rp_range *ranges, size_t nranges, const bppp_rp_public *pubs,
                          size_t npub, const uint8_t *seed, size_t seed_len, const char *oracle_tag, bppp_rp **out);
int bppp_rp_create_binary_seeded(bppp_ctx *ctx, int flavour, int conserve, const bppp_rp_range *ranges, size_t nranges,
                                 const uint64_t net_public[4], const uint8_t *seed, size_t seed_len, const char *oracle_tag, bppp_rp **out);
void bppp_rp_destroy(bppp_rp *rp);
int bppp_rp_info(const bppp_rp *rp, bppp_rp_shape *out);
/* Tuning knobs of one handle.  Every knob has a measured default; the BPPP_RP_* environment variables of the
 * same names are read ONCE, at bppp_rp_create, as initial values — no entry point reads the environment per call.  None changes a
 * result (asserted byte for byte by the tests).
 *   COMB_MIN        first batch size — or cumulative number of proofs proved — at which the PROVER builds its fixed-base comb table
 *                   (default 1024).  The table is a persistent allocation that lives until bppp_rp_destroy.
 *   COMB_BUDGET     bytes the table may take (default 32 GiB; additionally never more than half of the HBM free at build time);
 *                   0 = never build one (bucket MSMs and the point-folding argument serve every batch).
 *   COMB_BITS       force the table's window width (4..18; skips the budget), 0 = widest that fits.
 *   SPLIT_MIN       smallest prove batch run as two half-batches in flight on a twin context (default 4096); 0 = never split.
 *   HOST_ORACLE_MAX largest batch whose Fiat-Shamir hashing runs on host cores (defaults: 8 proofs verifying, 64 proving; UINT64_MAX
 *                   restores them).  Verifying 2 .. HOST_ORACLE_MAX proofs starts, once per handle, a pool of at most 15 worker threads
 *                   that sleep between calls and end with bppp_rp_destroy.
 *   FOLD_POINTS     1 = the point-folding argument although a table exists;  HOST_ALGEBRA 1 = prover's field algebra on the host;
 *   TIMING          1 = phase times on stderr.
 *   CULPRITS        how a rejected batch finds its invalid proofs (proof_status of bppp_rp_verify_batch*, the failing groups of
 *                   bppp_rp_verify_mixed*): 0 (default) = bisection, O(f log B) combined MSMs for f bad proofs; 1 = one per-proof pass
 *                   (bppp_rp_verify_each's) over the rejected range, whatever f.  Same statuses either way.  Set here only, no
 *                   environment variable. */
#define BPPP_RP_OPT_COMB_MIN 1
#define BPPP_RP_OPT_COMB_BUDGET 2
#define BPPP_RP_OPT_COMB_BITS 3
#define BPPP_RP_OPT_SPLIT_MIN 4
#define BPPP_RP_OPT_HOST_ORACLE_MAX 5
#define BPPP_RP_OPT_FOLD_POINTS 6
#define BPPP_RP_OPT_HOST_ALGEBRA 7
#define BPPP_RP_OPT_TIMING 8
#define BPPP_RP_OPT_CULPRITS 9
int bppp_rp_set_option(bppp_rp *rp, int option, uint64_t value);
/* Host-only helpers (no context, no GPU): the shape `setup` gives a schema (nrmLen, linLen, rounds = optimalWitnessSize, file sizes);
 * `digits` of one value in one range (src/RangeProof/TypedReciprocal.hs:125-127: greedy mixed-radix digits, the first one binary when
 * the range needs a bit; cap = capacity of out_digits); and the CLI's hash-to-field `hash = decode . SHA.hash` (app/Main.hs:64-65:
 * SHA-256, digest read through Binary (Prime p)) — hashToScalar p s = bppp_hash_to_scalar (p <> s) (app/Main.hs:83-84). */
int bppp_rp_shape_of(int flavour, int has_types, const bppp_rp_range *ranges, size_t nranges, bppp_rp_shape *out);
int bppp_rp_digits(const bppp_rp_range *range, const uint64_t amount[4], uint32_t *out_digits, size_t cap, size_t *ndigits, int *has_bit);
int bppp_hash_to_scalar(const uint8_t *data, size_t len, uint64_t out[4]);

/* Batch verification, end to end: for `batch` proofs of this setup, given as the reference's FILES — coms_files [batch][coms_bytes],
 * proof_files [batch][proof_bytes] — decodeProof (src/RangeProof.hs:68-85, src/Encoding.hs:97-128: x-only points, square roots and
 * sign selection on the device), verifyM (src/RangeProof.hs:103-105): verifyTRRPM with its three oracle calls
 * (TypedReciprocal.hs:447-467) and verifyBPM with one per round (src/Bulletproof.hs:370-378), all SHA-256 on the device, then ONE
 * combined MSM over sum_b rho_b T_b.  `seed` = 32 bytes of the VERIFIER's fresh secret randomness (never a constant
 * outside tests); rho_b = decode(SHA-256(seed <> le64(index_offset + b) <> t_b <> e_last_b <> final witness scalars of b)): bound to
 * the seed, to the proof's position in the whole job and to every byte of the proof (t and e_last are transcript hashes over all its
 * commitments and responses), never fixed to 1.  *accept = 1 iff every proof decodes and the combination is the identity.
 * proof_status (may be NULL, [batch]): BPPP_RP_VALID / _INVALID / _MALFORMED (an x coordinate with no curve point: `Nothing` in
 * the reference); when the batch is rejected the culprits are found by bisection over sub-batches (each a combined MSM).
 * challenges_out (may be NULL, [batch][7 + rounds][4]): (e, x, r0, q, x', r1, t) then the argument's challenges LAST ROUND FIRST
 * (src/Bulletproof.hs:374) — what the injected-oracle route would have been given; for parity tests.
 * combined_xy (may be NULL): the combined point sum_b rho_b MSM(T_b) itself (infinity = all zero).
 * _device: the files are already in HBM (the timed configuration of bench.py); the host variant uploads them first.
 * bppp_rp_verify_shard_device: one rank's share of a job sharded proof-per-GPU: this rank holds proofs
 * [index_offset, index_offset + batch) of the job and every rank passes the SAME seed; the ranks all-gather their 64-byte combined
 * points (RCCL) and add them with bppp_sum_points: the job verifies iff that sum is the identity and no rank saw a malformed proof.
 * Because the weights are indexed by the position in the JOB (and bound to the proofs), error terms cannot cancel between ranks: the
 * sum over ranks is the same random linear combination a single rank would have formed over all proofs.  bppp_rp_verify_batch_device
 * is the shard with index_offset = 0. */
#define BPPP_RP_VALID 0u
#define BPPP_RP_INVALID 1u
#define BPPP_RP_MALFORMED 2u
int bppp_rp_verify_batch(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint8_t *proof_files, const uint8_t seed[32], int *accept,
                         uint32_t *proof_status, uint64_t *challenges_out, uint64_t *combined_xy);
int bppp_rp_verify_batch_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_proof_files, const uint8_t seed[32], int *accept,
                                uint32_t *proof_status, uint64_t *challenges_out, uint64_t *combined_xy);
int bppp_rp_verify_shard_device(bppp_rp *rp, size_t batch, uint64_t index_offset, const void *d_coms_files, const void *d_proof_files, const uint8_t seed[32],
                                int *accept, uint32_t *proof_status, uint64_t *challenges_out, uint64_t *combined_xy);
/* Per-proof verification without weights: the same files as bppp_rp_verify_batch, every proof decided on its own.  For proof b,
 * E_b = MSM(T_b) over exactly the term list verifyWith builds for that proof alone (verifyM of one proof); the proof is valid iff
 * E_b is the identity.  No seed, no random weights: the verdict is exact, and its cost does not depend on how many proofs fail
 * (one fixed-base MSM of 1 + linLen + nrmLen terms and one of ninit + 2 rounds distinct points per proof, in chunks of bounded memory).
 * proof_status (required, [batch]): BPPP_RP_VALID / _INVALID / _MALFORMED.  proof_xy (may be NULL, [batch][8]): E_b, infinity as all
 * zeros; zeros for a malformed proof.  Sum_b rho_b E_b with bppp_rp_verify_batch's weights is its combined_xy.
 * Typed-reciprocal and binary handles, both argument flavours.  BPPP_ERR_ARG as bppp_rp_verify_batch (null files with a non-empty batch,
 * a closed context, 2^22 proofs or more); an empty batch returns BPPP_OK.  _device: the files are already in HBM. */
int bppp_rp_verify_each(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint8_t *proof_files, uint32_t *proof_status, uint64_t *proof_xy);
int bppp_rp_verify_each_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_proof_files, uint32_t *proof_status,
                               uint64_t *proof_xy);

/* Batch verification of proofs of SEVERAL setups with one combined MSM: a block or a mempool holds many shapes (32 .. 128 outputs,
 * norm-linear and inner-product argument, typed-reciprocal and binary proofs), each group below one handle of this context.  The job
 * is the groups concatenated in the order given: proof j of group s has job position index_offset + start_s + j (start_s = the earlier
 * groups' batches) and the weight rho bppp_rp_verify_shard_device gives that position, so combined_xy is exactly the sum over groups of
 * bppp_rp_verify_shard_device (rp_s, batch_s, index_offset + start_s, ...)'s combined point with the same seed; a rank's share of a
 * sharded mixed job is this call with its index_offset, the ranks' points added with bppp_sum_points as there.
 * The shared-basis scalars are merged across setups: every setup's verification basis [g | H | G] is the prefix ps[1 : 2 + linLen +
 * nrmLen] of the point stream its points came from (TypedReciprocal.hs:334, :348-349; Binary.hs:147-148), so handles whose bases
 * (points 1.. of the creation's points_xy, compared point by point) extend one another share the longest one's terms; unrelated bases
 * are concatenated.  One MSM of sum over those families of the longest basis + sum_s batch_s (ninit_s + 2 rounds_s) terms.
 * *accept = 1 iff every proof of every group decodes and the one combination is the identity.  proof_status (may be NULL): [total
 * batch] in job order, BPPP_RP_VALID / _INVALID / _MALFORMED; on rejection each group's own combination is evaluated and failing
 * groups are bisected as in bppp_rp_verify_batch.  BPPP_ERR_ARG: handles on different contexts, one handle in two groups, 2^22 proofs
 * or more, null files for a non-empty group.  Empty groups take no part; an empty job is accepted.
 * _device: the files are in HBM; bppp_rp_verify_mixed takes host files, uploads them and runs as _device with index_offset 0. */
typedef struct bppp_rp_group {
  bppp_rp *rp;               /* the setup these proofs claim */
  size_t batch;              /* proofs in this group (0 allowed) */
  const void *coms_files;    /* [batch][coms_bytes of rp] */
  const void *proof_files;   /* [batch][proof_bytes of rp] */
} bppp_rp_group;
int bppp_rp_verify_mixed_device(const bppp_rp_group *groups, size_t ngroups, uint64_t index_offset, const uint8_t seed[32], int *accept,
                                uint32_t *proof_status, uint64_t *combined_xy);
int bppp_rp_verify_mixed(const bppp_rp_group *groups, size_t ngroups, const uint8_t seed[32], int *accept, uint32_t *proof_status,
                         uint64_t *combined_xy);

/* Batch prover: `batch` proofs of this setup in lockstep — proveM of RangeProof (src/RangeProof.hs:93-97) = proveTRRPM
 * (src/RangeProof/TypedReciprocal.hs:399-446; blinding algebra src/RangeProof/Internal.hs:118-196) followed by proveBPM
 * (src/Bulletproof.hs:357-359), then encodeProof' (src/RangeProof.hs:60-66).  Per proof b: amounts / types / blinds are
 * [batch][nranges][4] (amount: a plain integer inside its range, two's complement when negative; type, blinding: canonical scalars), and the prover's randomness
 * is the CLI's: random n = decode(SHA-256(prefix_b <> show n)) for n = 0, 1, ... (hashToScalar, app/Main.hs:83-87, :189;
 * ZKPT.random, src/ZKP.hs:88-92) with prefix_b = rand_prefix[b * prefix_len ..].  The oracle is the setup's shaOracle (see above).
 * Outputs are the reference's files: coms_files [batch][coms_bytes], proof_files [batch][proof_bytes].  Every commitment is
 * computed on the device (input commitments through a fixed-base table of g, H0, H1; the four range-proof commitments of all
 * proofs and the round commitments of the argument), and so are the per-proof field algebra, the randomness and the transcript
 * hashing; the host cores extract the digits of the plain amounts.  MEMORY: at the first batch of 1024 proofs or more, or once it has proved that many in smaller batches (bppp_rp_set_option COMB_MIN), the handle
 * builds a fixed-base comb table over the setup's basis [g | H | G] and keeps it until it is destroyed — the widest window (<= 18
 * bits) whose table fits 32 GB: c = 16, 27.6 GB for the 774 points of 64by64, built in ~0.3 s (BPPP_RP_COMB_GB=<GB> changes the budget:
 * 64 GB (c = 17) and 128 GB (c = 18) measured level with it — the gathers over longer table rows cost what the fewer additions save;
 * BPPP_RP_COMB_BITS=<c> forces a width: c = 13 is 4.1 GB and ~15 % more additions; BPPP_RP_NO_COMB=1 keeps the bucket route and
 * the point-folding argument, which smaller batches use anyway).  A batch of 4096 proofs or more runs as two half-batches in
 * flight, the second on a twin handle with its own context that this handle creates and owns and that shares the table
 * (BPPP_RP_SPLIT_MIN=<n> moves the threshold, BPPP_RP_NO_SPLIT=1 disables it; a RangeProof.Binary handle splits from 1024 proofs,
 * BPPP_RP_SPLIT_MIN_BINARY); a handle serves one call at a time.  Handles whose bases extend one another can prove over ONE table
 * instead of one each (bppp_rp_share_comb, bppp_rp_prove_mixed below); a handle never passed to those builds and keeps its own.  Same
 * randomness and inputs => byte-identical files to the host protocol code (bulletproofspp_amd/rangeproof.py: prove +
 * encoding.encode_proof), on every one of these routes, which the tests assert. */
int bppp_rp_prove_batch(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, const uint8_t *rand_prefix,
                        size_t prefix_len, uint8_t *coms_files, uint8_t *proof_files);

/* ---- per-proof public amounts (fees, deposits, withdrawals) --------------------------------------------------------------------
 * A handle fixes its setup's public amounts at creation: the `amount` of every bppp_rp_public (typed reciprocal, pubSum of
 * TypedReciprocal.hs:235-248) or `net_public` (RangeProof.Binary with conservation, netPub' of Binary.hs:72-87).  In a block of
 * conserved transactions they are each transaction's fee or public deposit and differ from proof to proof.  The *_pub entry points
 * below take them per proof; everything else (ranges, public types and is_output flags, basis, tag) stays the handle's.
 *   bppp_rp_public_count: amounts per proof — npub for a typed handle created with has_types, 1 for a binary handle with `conserve`,
 *                         0 otherwise (an untyped handle, whose public values the protocol ignores, or a binary one without conservation).
 *   public_amounts: [batch][public_count][4] words, encoded as the creation argument is — typed: canonical scalars, in the order of the
 *                   handle's `pubs`; binary: the plain integer in two's complement, as net_public.  NULL = the handle's own amounts:
 *                   the call is then exactly its counterpart without _pub.  _device variants take it in HBM (d_public_amounts); it is
 *                   read back and checked on the host (32 bytes per amount) before any work is queued.
 * Proof b under a *_pub call behaves as proof b under a handle created with the same arguments but proof b's amounts: statuses,
 * challenges, E_b (verify_each), the prover's files and its balance check (witnessTRRP's per-type sum, witnessBRP's netPub + sum v = 0;
 * the first proof that does not balance is named in the BPPP_ERR_ARG message) all match that handle.  The batch weights rho_b are
 * defined exactly as for bppp_rp_verify_shard_device — the amounts are the verifier's own inputs, fixed before it draws its seed — so
 * combined_xy of bppp_rp_verify_shard_pub_device is the sum over b of bppp_rp_verify_shard_device (handle with amounts_b, 1,
 * index_offset + b, ...)'s points.
 * Fiat-Shamir: the reference does not hash the public amounts into the transcript, and neither do these entry points (parity): a proof
 * made for one fee also opens against a setup whose other values agree only where the prover chose them.  The caller must take the
 * amounts from the transaction it is validating, never from the prover — and a caller that wants the proof TIED to that transaction
 * (its fee, recipients, memo, chain id) passes a hash of them as the proof's binding to the bppp_rp_*_bound* entry points below, which
 * put it into every oracle message of that proof.
 * BPPP_ERR_ARG: a non-NULL public_amounts with batch > 0 on a handle whose public_count is 0; a typed amount that is not canonical;
 * every argument error of the counterpart without _pub. */
int bppp_rp_public_count(const bppp_rp *rp, size_t *n);
int bppp_rp_verify_batch_pub(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint8_t *proof_files, const uint64_t *public_amounts,
                             const uint8_t seed[32], int *accept, uint32_t *proof_status, uint64_t *challenges_out, uint64_t *combined_xy);
int bppp_rp_verify_batch_pub_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_proof_files, const void *d_public_amounts,
                                    const uint8_t seed[32], int *accept, uint32_t *proof_status, uint64_t *challenges_out, uint64_t *combined_xy);
int bppp_rp_verify_shard_pub_device(bppp_rp *rp, size_t batch, uint64_t index_offset, const void *d_coms_files, const void *d_proof_files,
                                    const void *d_public_amounts, const uint8_t seed[32], int *accept, uint32_t *proof_status,
                                    uint64_t *challenges_out, uint64_t *combined_xy);
int bppp_rp_verify_each_pub(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint8_t *proof_files, const uint64_t *public_amounts,
                            uint32_t *proof_status, uint64_t *proof_xy);
int bppp_rp_verify_each_pub_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_proof_files, const void *d_public_amounts,
                                   uint32_t *proof_status, uint64_t *proof_xy);
int bppp_rp_prove_batch_pub(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds,
                            const uint64_t *public_amounts, const uint8_t *rand_prefix, size_t prefix_len, uint8_t *coms_files,
                            uint8_t *proof_files);

/* ---- proving from HBM to HBM -------------------------------------------------------------------------------------------------------
 * bppp_rp_prove_batch_device is bppp_rp_prove_batch_pub with every buffer in HBM (16-byte aligned): d_amounts, d_types, d_blinds
 * [batch][nranges][4] words (amounts as plain integers in two's complement; d_types is ignored and may be NULL on a binary handle),
 * d_public_amounts NULL or [batch][public_count][4], d_rand_prefix [batch][prefix_len] bytes (NULL iff prefix_len == 0); out:
 * d_coms_files [batch][coms_bytes], d_proof_files [batch][proof_bytes].  Synchronous: on return the files are complete in HBM.  The
 * two output buffers hold, byte for byte, what bppp_rp_prove_batch_pub writes for the same inputs on the same handle, and the call
 * does the same bookkeeping (the comb table is built at the same point, the options, a shared table and the two half-batches of a
 * large batch apply as they do there; d_public_amounts is read back and checked on the host as the verifier's _pub_device calls do).
 * With the handle's comb table in place (neither HOST_ALGEBRA nor FOLD_POINTS set, and a setup the device algebra serves: its phase kernels fit a
 * workgroup's LDS — 2470 ranges of small bases —, and a digit base above 256 meets at most 256 ranges) nothing of a proof
 * crosses to the host but one status word per proof: a kernel checks the witness (canonical types and blindings, balance, ranges) and
 * extracts digits and multiplicities, the prover's stream of kernels runs on its output, a kernel encodes the files.  Internal
 * thresholds stay (at most HOST_ORACLE_MAX proofs still hash their transcripts on the host cores).  Every other route is the SLOW PATH
 * of this entry point: the inputs are downloaded, the host-buffer route proves, the files are uploaded.
 * Errors: return code and bppp_last_error text of bppp_rp_prove_batch_pub on the same inputs (bad arguments, a public amount that is
 * not canonical, "proof N: value outside its range" ...).  When SEVERAL proofs of a batch are refused the device stream names the
 * LOWEST-numbered one, with the reason the host entry point gives for that proof alone; the host entry point names whichever its
 * worker threads reported last. */
int bppp_rp_prove_batch_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds,
                               const void *d_public_amounts, const void *d_rand_prefix, size_t prefix_len, void *d_coms_files,
                               void *d_proof_files);

/* ---- per-proof witness verdicts: skip the refused proofs, prove the rest ---------------------------------------------------------------
 * bppp_rp_prove_batch_status is bppp_rp_prove_batch_pub, and bppp_rp_prove_batch_status_device is bppp_rp_prove_batch_device, with one
 * more argument: proof_status [batch], in HOST memory on both (as for bppp_rp_verify_each_device), required.  A witness the counterpart
 * would refuse no longer fails the call: proof_status[b] says why (BPPP_RP_WIT_*), the other proofs are proved in the same single
 * lockstep pass.
 * Return code: BPPP_OK whenever the call itself was well formed, however many proofs were refused — all of them included.  The
 * counterpart's call-level errors stay, with its code and message: NULL buffers, batch >= 2^20, prefix_len > 4096, a public amount that
 * is not canonical (or given to a handle whose public_count is 0), a closed context.  A NULL proof_status with batch > 0 is BPPP_ERR_ARG;
 * an empty batch is BPPP_OK.
 * Accepted proofs (proof_status[b] == BPPP_RP_WIT_OK): the two files of proof b are, byte for byte, what bppp_rp_prove_batch_pub writes
 * when given proof b's inputs alone, on every route — a proof's randomness comes from its own prefix and its transcript is its own, so
 * neither its position in the batch nor its neighbours matter.
 * Refused proofs: both files of proof b are all zero bytes (on the host, and in HBM), and proof_status[b] is the reason
 * bppp_rp_prove_batch_pub gives for proof b alone — a typed handle reports the lowest code that applies (canonical types and blindings
 * are checked first, then the balance, then the ranges), a binary handle the first offending range (its blinding, then its bounds) and,
 * if there is none, the balance.  Host and _device variants report identical statuses.  bppp_rp_witness_status_text is the text after
 * "proof N: " in the counterpart's message (a static string; "unknown witness status" for any other value).
 * Bookkeeping: the decision to build the comb table counts the submitted batch, as the counterpart does, before any witness is looked
 * at.  The accepted proofs are proved as a batch of their own: HOST_ORACLE_MAX applies to their number, and so does SPLIT_MIN /
 * SPLIT_MIN_BINARY on the host-buffer routes; on the device stream the submitted batch is split (each half checks and compacts its own
 * proofs in HBM; statuses sit at their indices in the whole batch).  None of this changes a byte.
 * Device stream (bppp_rp_prove_batch_device's conditions): nothing of a proof crosses to the host but its status word; a batch without a
 * refusal queues exactly the kernels of bppp_rp_prove_batch_device.  Otherwise the accepted proofs' indices go up, the witness kernel
 * runs again over them in compact order, and one kernel zeroes the refused proofs' files.
 * Not covered: bppp_rp_prove_mixed; verdicts on public amounts (the caller's own inputs). */
#define BPPP_RP_WIT_OK 0u
#define BPPP_RP_WIT_NOT_CANONICAL 1u      /* typed: a type or blinding >= n */
#define BPPP_RP_WIT_UNBALANCED 2u         /* typed: amounts of some type do not balance */
#define BPPP_RP_WIT_OUT_OF_RANGE 3u       /* either kind */
#define BPPP_RP_WIT_BIN_NOT_CANONICAL 4u  /* binary: a blinding >= n */
#define BPPP_RP_WIT_BIN_UNBALANCED 5u     /* binary: no conserved, balancing schema */
const char *bppp_rp_witness_status_text(uint32_t status);
int bppp_rp_prove_batch_status(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds,
                               const uint64_t *public_amounts, const uint8_t *rand_prefix, size_t prefix_len, uint8_t *coms_files,
                               uint8_t *proof_files, uint32_t *proof_status);
int bppp_rp_prove_batch_status_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds,
                                      const void *d_public_amounts, const void *d_rand_prefix, size_t prefix_len, void *d_coms_files,
                                      void *d_proof_files, uint32_t *proof_status /* host, [batch] */);

/* ---- per-proof transcript bindings: tie each proof to its transaction ------------------------------------------------------------------
 * The oracle of the range-proof entry points is the CLI's shaOracle (app/Main.hs:75-80) over ZKPT's transcript (src/ZKP.hs:96-101): every
 * message is  tag <> show n <> show (length ps) <> text,  and the tag is the handle's oracle_tag, fixed at creation — the only domain
 * separation.  The *_bound* entry points take one more array, bindings: [batch][BPPP_RP_BINDING_BYTES] opaque bytes, which the caller derives
 * from what each proof belongs to (typically SHA-256 of the transaction's public data).  Proof b of a bound call behaves in every respect as
 * a proof under a handle whose oracle tag is  oracle_tag <> binding_b:  every oracle message of that proof is
 *   oracle_tag <> binding_b[32] <> show n <> show (length ps) <> text
 * so a proof lifted from one transaction does not verify inside another.  Nothing else changes: the prover's randomness (rand_prefix), the
 * wire format, the file sizes and the commitments are as before, and the batch weights rho_b keep their formula (they hash t and e_last,
 * which now depend on the binding).  Bindings are raw bytes — 0x00 and bytes >= 0x80 are ordinary values — and two proofs may carry the
 * same one.  bindings == NULL: the call is exactly its unbound counterpart (the same kernels queued, the same bytes, challenges_out and
 * combined_xy).  _device variants take d_bindings in HBM; it stays there whenever the batch hashes its transcripts on the GPU, and is read
 * back (32 bytes per proof) on the routes that hash on host cores (at most HOST_ORACLE_MAX proofs, HOST_ALGEBRA, FOLD_POINTS, a prover
 * without its comb table).  The host variants upload it where the GPU hashes.
 *   bppp_rp_verify_bound         bppp_rp_verify_batch_pub plus bindings
 *   bppp_rp_verify_bound_device  bppp_rp_verify_shard_pub_device plus d_bindings.  index_offset moves the weights only, never the bindings:
 *                                a rank passes the bindings of its own proofs, and the ranks' combined_xy add up as before
 *   bppp_rp_verify_each_bound{,_device}   bppp_rp_verify_each_pub{,_device} plus bindings
 *   bppp_rp_prove_bound{,_device}         with proof_status == NULL: bppp_rp_prove_batch_pub / bppp_rp_prove_batch_device plus bindings (a
 *                                refused witness fails the call); with proof_status ([batch], host memory on both): bppp_rp_prove_batch_status
 *                                {,_device} plus bindings (refused proofs get their BPPP_RP_WIT_* code and zeroed files, the rest are proved,
 *                                each under its own binding wherever it lands in the compacted batch)
 * public_amounts / d_public_amounts may be NULL as in the counterparts.  Typed-reciprocal and binary handles, both argument flavours.
 * The culprit search of a rejected batch (bisection or CULPRITS = 1), the two half-batches of a large prove call and verify_each's chunks
 * all work on each proof's own binding.
 * Tag limit: a header (tag, binding, the decimal digits of n and of the point count) is at most 64 bytes, so a bound call needs
 *   strlen (oracle_tag) <= 64 - 32 - 1 - digits (nranges + 2 rounds + 4)       (binary: nranges + 2 rounds + 2)
 * — 29 bytes while the transcript has fewer than 100 points, 28 below 1000.  On a handle with a longer tag a bound call with bindings
 * returns BPPP_ERR_ARG and bppp_last_error says so; unbound calls on that handle (bindings == NULL included) keep working.
 * Errors otherwise: those of the counterpart, with its codes and texts (NULL files with a non-empty batch, ...); an empty batch is BPPP_OK.
 * What a binding protects: the TRANSCRIPT — a proof verifies only under the binding it was made with.  It does not make the encodings
 * unique (the malleability of the files is as documented for the unbound calls), and it protects nothing if the verifier takes the
 * binding from the prover: derive it from the transaction being validated.
 * Not covered: bppp_rp_verify_mixed*, bppp_rp_prove_mixed (one handle per group there: give each its own tag), and the commit / open entry
 * points, which hash no transcript and so have nothing to bind. */
#define BPPP_RP_BINDING_BYTES 32
int bppp_rp_verify_bound(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint8_t *proof_files, const uint64_t *public_amounts /* NULL ok */,
                         const uint8_t *bindings /* [batch][32], NULL ok */, const uint8_t seed[32], int *accept, uint32_t *proof_status,
                         uint64_t *challenges_out, uint64_t *combined_xy);
int bppp_rp_verify_bound_device(bppp_rp *rp, size_t batch, uint64_t index_offset, const void *d_coms_files, const void *d_proof_files,
                                const void *d_public_amounts, const void *d_bindings, const uint8_t seed[32], int *accept, uint32_t *proof_status,
                                uint64_t *challenges_out, uint64_t *combined_xy);
int bppp_rp_verify_each_bound(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint8_t *proof_files, const uint64_t *public_amounts,
                              const uint8_t *bindings, uint32_t *proof_status, uint64_t *proof_xy);
int bppp_rp_verify_each_bound_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_proof_files, const void *d_public_amounts,
                                     const void *d_bindings, uint32_t *proof_status, uint64_t *proof_xy);
int bppp_rp_prove_bound(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds,
                        const uint64_t *public_amounts, const uint8_t *bindings, const uint8_t *rand_prefix, size_t prefix_len, uint8_t *coms_files,
                        uint8_t *proof_files, uint32_t *proof_status /* may be NULL */);
int bppp_rp_prove_bound_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds,
                               const void *d_public_amounts, const void *d_bindings, const void *d_rand_prefix, size_t prefix_len,
                               void *d_coms_files, void *d_proof_files, uint32_t *proof_status /* host, [batch], may be NULL */);

/* ---- commitments without a proof, and checking their openings ---------------------------------------------------------------------------
 * The input commitments of a transaction exist before its proof does (a receiver makes them, a builder lays out a transaction with them)
 * and are checked after it (an auditor, a receiving wallet, a service re-checking its book of openings).  These entry points are
 * scalarPairRPW' / com (src/RangeProof/Internal.hs:59-60) and encodeCommitments / decodeCommitments (src/Encoding.hs:119-134) on their own:
 *   C = v g + ty H0 + bl H1      (a RangeProof.Binary handle: C = v g + bl h0, scalarRPW' Internal.hs:56-57; it has no types)
 * over the first three points [g | H0 | H1] of the handle's registered basis.  Every call takes a bppp_rp of either kind and either
 * argument flavour (the flavour plays no part).  amounts / types / blinds are laid out as for bppp_rp_prove_batch, [batch][nranges][4]
 * words: an amount is a plain integer in two's complement, reduced mod n as the prover reduces it (so v and v + n name one commitment);
 * a type and a blinding are canonical scalars; `types` is ignored on a binary handle and may be NULL there.  NO WITNESS IS JUDGED: no
 * range check, no balance check, no public amount — any amount has a commitment; bppp_rp_prove_batch_status judges witnesses.
 * The host variants upload, call the _device variant and download; d_* buffers are in HBM, 16-byte aligned; status arrays are host memory.
 *
 * bppp_rp_commit_batch{,_device}: coms_files [batch][coms_bytes], the commitments file of every row.  For every row bppp_rp_prove_batch_pub
 * accepts, the file equals that call's coms_files row byte for byte.  commit_status ([batch], host, may be NULL): BPPP_RP_WIT_OK,
 * BPPP_RP_WIT_NOT_CANONICAL (typed: a type or blinding >= n), BPPP_RP_WIT_BIN_NOT_CANONICAL (binary: a blinding >= n) or
 * BPPP_RP_COMMIT_INFINITY — some commitment of the row is the point at infinity (amount, type and blinding all zero mod n), which has no
 * encoding (encodeCommitments takes affine coordinates).  NOT_CANONICAL is reported before INFINITY.  The file of a refused row is all
 * zero bytes, the others are written.  With commit_status == NULL a refused row is BPPP_ERR_ARG and bppp_last_error names the
 * lowest-numbered one ("proof N: ...") — the files are then as they would be with commit_status given.
 *
 * bppp_rp_open_each{,_device}: open_status [batch][nranges] (required), one exact verdict per commitment, no randomness:
 *   BPPP_RP_OPEN_OK             the decoded point, with its sign applied, equals the recomputed commitment
 *   BPPP_RP_OPEN_MISMATCH       it does not
 *   BPPP_RP_OPEN_MALFORMED      the x has no curve point (decodeCommitments' Nothing; an x >= p is reduced first, as the verifier does)
 *   BPPP_RP_OPEN_NOT_CANONICAL  the claimed type or blinding is >= n (binary: the blinding)
 * The file is judged before the claim: MALFORMED wins over NOT_CANONICAL.
 *
 * bppp_rp_open_batch{,_device}: all openings checked by ONE weighted combination, as bppp_rp_verify_shard_device checks proofs.  The
 * commitment i of row b has job position j = (index_offset + b) * nranges + i (mod 2^64), error term E_j = C_j - v_j g - ty_j H0 - bl_j H1
 * and weight
 *   rho_j = decode (SHA-256 (M_j)) mod n, with 1 in place of 0;  decode = Binary (Prime p): four big-endian 64-bit words, least significant first
 *   M_j   = seed[32] || le64 (j) || the 32 x bytes of the commitment AS THEY STAND IN THE FILE || one byte holding its sign bit (0 or 1)
 *           || put (v_j mod n) || put (ty_j) || put (bl_j)          — 169 bytes;  ty_j = 0 on a binary handle;
 *   put   = Binary (Prime p) put (Encoding.hs:81-86): 32 bytes, the four 64-bit limbs least significant first, each big-endian.
 * combined = sum_j rho_j E_j = sum_j rho_j C_j - (sum rho_j v_j) g - (sum rho_j ty_j) H0 - (sum rho_j bl_j) H1 (binary: bl on H0): one MSM
 * over the decoded points plus three reduced scalars.  *accept = 1 iff no x is malformed, no claimed scalar is non-canonical and
 * combined is the identity.  `seed` is the checker's fresh secret randomness (never a constant outside tests); every rank of a sharded job
 * passes the same seed and its own index_offset, and the ranks' combined points add up (bppp_sum_points) to the one-call point.
 * open_status (may be NULL, [batch][nranges]): all BPPP_RP_OPEN_OK when accepted; on rejection exactly bppp_rp_open_each's verdicts over
 * the same inputs, from one such pass (no bisection).  combined_xy (may be NULL): the combined point, infinity as all zeros; it is defined
 * by the formula above only when nothing is malformed or non-canonical.  bppp_rp_open_batch is the _device call with index_offset 0.
 *
 * Errors, as for the verify entry points: NULL buffers with a non-empty batch, a closed context and batch * nranges >= 2^31 are
 * BPPP_ERR_ARG; an empty batch returns BPPP_OK (bppp_rp_open_batch* with *accept = 1).  A large batch is worked through in chunks of
 * 2^22 commitments of bounded memory. */
#define BPPP_RP_COMMIT_INFINITY 16u
#define BPPP_RP_OPEN_OK 0u
#define BPPP_RP_OPEN_MISMATCH 1u
#define BPPP_RP_OPEN_MALFORMED 2u
#define BPPP_RP_OPEN_NOT_CANONICAL 3u
int bppp_rp_commit_batch(bppp_rp *rp, size_t batch, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, uint32_t *commit_status,
                         uint8_t *coms_files);
int bppp_rp_commit_batch_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds,
                                uint32_t *commit_status /* host, [batch], may be NULL */, void *d_coms_files);
int bppp_rp_open_each(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds,
                      uint32_t *open_status);
int bppp_rp_open_each_device(bppp_rp *rp, size_t batch, const void *d_coms_files, const void *d_amounts, const void *d_types, const void *d_blinds,
                             uint32_t *open_status /* host, [batch][nranges], required */);
int bppp_rp_open_batch(bppp_rp *rp, size_t batch, const uint8_t *coms_files, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds,
                       const uint8_t seed[32], int *accept, uint32_t *open_status, uint64_t *combined_xy);
int bppp_rp_open_batch_device(bppp_rp *rp, size_t batch, uint64_t index_offset, const void *d_coms_files, const void *d_amounts, const void *d_types,
                              const void *d_blinds, const uint8_t seed[32], int *accept, uint32_t *open_status, uint64_t *combined_xy);

/* ---- tallies: signed sums of commitments against claimed openings --------------------------------------------------------------------
 * The homomorphic check next to commit / open: a set of commitments adds up.  A validator checks that inputs - outputs - fee g is a commitment
 * to zero with a known excess blinding; an auditor checks that a book of commitments sums to a stated total.  The shapes that prove balance
 * inside the proof (conserved typed-reciprocal and conserved binary) do not need it; every other shape, and any untyped handle, does.
 * "Known" means TOLD: the claim of a tally includes e_t, the signed sum of the blindings, so these calls serve a checker who is shown the
 * books.  A checker who is not told e_t (a public validator) takes the excess signatures below, bppp_rp_excess_verify_*, over the same pool
 * and the same sums: the builder proves that it knows e_t instead of revealing it.
 *
 * POOL.  coms_files [rows][coms_bytes] of handle rp, exactly as bppp_rp_open_each takes it.  Commitment i of row r has the flat index
 * j = r * nranges + i; rows * nranges < 2^31, so bit 31 of an index is free.  The pool is decoded once per call (64 bytes a commitment in
 * HBM; a pool whose decoded form cannot be allocated is BPPP_ERR_HIP).
 * SUMS.  nsums sums in CSR form: sum_start [nsums + 1] (uint32, non-decreasing, sum_start[0] = 0, sum_start[nsums] = nnz) and entries [nnz]
 * (uint32: bits 0..30 a flat index, bit 31 set = the commitment is subtracted); nnz < 2^31 and nsums < 2^31.  A commitment may appear in any
 * number of sums and more than once in one sum; an empty sum is the identity.  nnz is passed next to entries: it is the length the caller
 * vouches for, and sum_start is checked against it.
 * CLAIM.  Sum t must equal a_t g + ty_t H0 + e_t H1 (a binary handle: a_t g + e_t h0; ty is ignored there and may be NULL).  claim_amounts,
 * claim_types, claim_blinds are [nsums][4] words, encoded as for bppp_rp_open_each: the amount a plain integer in two's complement, reduced
 * mod n; the type and the blinding canonical scalars.  All three NULL: every claim is zero, the pure "these balance to nothing" tally.
 * The host variants upload, call the _device variant and download; d_* buffers are in HBM, 16-byte aligned; status and point arrays are host
 * memory.
 *
 * bppp_rp_tally_each{,_device}: tally_status [nsums] (required), one exact verdict per sum, no randomness — the BPPP_RP_OPEN_* codes:
 *   BPPP_RP_OPEN_OK             the signed sum equals the recomputed claim
 *   BPPP_RP_OPEN_MISMATCH       it does not
 *   BPPP_RP_OPEN_MALFORMED      the x of some commitment the sum references has no curve point
 *   BPPP_RP_OPEN_NOT_CANONICAL  the claimed type or blinding is >= n (binary: the blinding)
 * The file is judged before the claim, as in bppp_rp_open_each: MALFORMED wins over NOT_CANONICAL.  A commitment that no sum references is
 * never judged.  sums_xy (may be NULL, [nsums][8]): the signed sum itself, infinity as all zeros, and zeros for a MALFORMED sum.
 *
 * bppp_rp_tally_batch{,_device}: all sums checked by ONE weighted combination,
 *   combined = sum_t rho_t (S_t - a_t g - ty_t H0 - e_t H1)
 * computed as one MSM over nnz + 3 terms: every entry contributes its decoded point with the scalar +-rho_t, and three reduced scalars go on
 * the first three points of the registered basis (more than 2^22 entries: one such MSM per 2^22, added with bppp_sum_points).  Sum t of this
 * call has job position index_offset + t (mod 2^64) and weight
 *   rho_t = decode (SHA-256 (M_t)) mod n, with 1 in place of 0
 *   M_t   = seed[32] || le64 (index_offset + t) || put (a_t mod n) || put (ty_t) || put (e_t)      — 136 bytes;  ty_t = 0 on a binary handle
 * with decode and put as defined for bppp_rp_open_batch.  The message does not name the pool or the entries: they are the checker's OWN
 * inputs, fixed before it draws the seed — as the public amounts of the *_pub calls are.  `seed` is the checker's fresh secret randomness
 * (never a constant outside tests); a checker that lets another party choose entries after seeing the seed has no guarantee.
 * *accept = 1 iff nothing referenced is malformed, no claim is non-canonical and combined is the identity.  tally_status (may be NULL,
 * [nsums]): all BPPP_RP_OPEN_OK when accepted; on rejection exactly bppp_rp_tally_each's verdicts over the same inputs, from one such pass.
 * combined_xy (may be NULL): the combined point, infinity as all zeros, defined by the formula only when nothing is malformed or
 * non-canonical.  Every rank of a sharded job passes the same seed, its own sums and its own index_offset; the ranks' points add up
 * (bppp_sum_points) to the one-call point.  bppp_rp_tally_batch is the _device call with index_offset 0.
 *
 * bppp_rp_tally_claims{,_device}: the builder's side (pedersen_blind_sum's counterpart).  amounts / types / blinds are the witness rows
 * [rows][nranges][4] in bppp_rp_commit_batch's layout, the CSR arrays as above; claim_amounts, claim_types, claim_blinds [nsums][4] receive
 * the signed sums mod n of the referenced (amount mod n, type, blinding).  The amount is written as the integer the other entry points read
 * back as itself: a when a < 2^255, else a - n in two's complement.  On a binary handle types is ignored and claim_types may be NULL (zeros
 * are written when it is not).  A referenced type or blinding >= n is BPPP_ERR_ARG naming the lowest such sum.  By construction
 * bppp_rp_tally_each over bppp_rp_commit_batch's files of these rows with these claims is all BPPP_RP_OPEN_OK.
 *
 * Errors (BPPP_ERR_ARG, bppp_last_error names the first offender): NULL buffers with a non-empty job; a closed context; rows * nranges,
 * nnz or nsums >= 2^31; a sum_start that is not non-decreasing from 0 to nnz ("sum_start[i] = ..."); an entry whose index is >= rows * nranges
 * ("entries[i]: index ..."); only some of the claim arrays NULL (a binary handle's types do not count).  nsums == 0 is BPPP_OK (tally_batch
 * with *accept = 1).  The CSR conditions are established by a kernel of their own whose verdict is read back BEFORE anything reads through
 * entries, on the host variants too: a bad array is an error code, never an out-of-bounds read, and no output buffer is written.  The
 * sums are worked through in passes of at most 2^22 entries of bounded workspace. */
int bppp_rp_tally_each(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                       const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_blinds, uint32_t *tally_status,
                       uint64_t *sums_xy /* may be NULL */);
int bppp_rp_tally_each_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                              const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_blinds,
                              uint32_t *tally_status /* host, [nsums], required */, uint64_t *sums_xy /* host, [nsums][8], may be NULL */);
int bppp_rp_tally_batch(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                        const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_blinds, const uint8_t seed[32], int *accept,
                        uint32_t *tally_status, uint64_t *combined_xy);
int bppp_rp_tally_batch_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                               const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_blinds, uint64_t index_offset,
                               const uint8_t seed[32], int *accept, uint32_t *tally_status, uint64_t *combined_xy);
int bppp_rp_tally_claims(bppp_rp *rp, size_t rows, const uint64_t *amounts, const uint64_t *types, const uint64_t *blinds, size_t nsums,
                         const uint32_t *sum_start, const uint32_t *entries, size_t nnz, uint64_t *claim_amounts, uint64_t *claim_types,
                         uint64_t *claim_blinds);
int bppp_rp_tally_claims_device(bppp_rp *rp, size_t rows, const void *d_amounts, const void *d_types, const void *d_blinds, size_t nsums,
                                const void *d_sum_start, const void *d_entries, size_t nnz, void *d_claim_amounts, void *d_claim_types,
                                void *d_claim_blinds);

/* ---- excess signatures: a tally checked without revealing the blinding sum -----------------------------------------------------------
 * pedersen_blind_sum's other use: the excess of sum t over its PUBLIC claim,
 *   X_t = S_t - a_t g - ty_t H0 = e_t B            (a binary handle: X_t = S_t - a_t g)
 * is published as a public key and the builder signs the transaction with e_t (Schnorr).  B is the blinding generator: H1 on a typed
 * handle (point 2 of [g | H0 | H1]), h0 on a RangeProof.Binary handle (point 1).  A valid signature shows that X_t has no g (and no H0)
 * component, i.e. that the sum carries exactly the claimed amount and type — without anyone learning e_t.
 *
 * POOL, SUMS, entries: exactly as for bppp_rp_tally_each, the same arrays and the same validation before anything reads through them.
 * PUBLIC CLAIM.  claim_amounts, claim_types [nsums][4], encoded as for the tally; claim_types is ignored on a binary handle and may be NULL
 * there; both NULL: every claim is zero.  There is no claim_blinds.
 * MESSAGE.  msgs [nsums][32], opaque bytes: typically the transaction's binding, the same 32 bytes a *_bound call takes.
 * SIGNATURE.  sigs [nsums][BPPP_RP_EXCESS_SIG_BYTES = 65]: put (R.x), then one sign byte of R (0 or 1: y > p - y, as encodeCommitments
 * defines the sign), then put (s); put and decode as defined for bppp_rp_open_batch.
 * DOMAINS, computed once per call on the host; tag = the handle's oracle tag bytes:
 *   Dc = SHA-256 ("bppp/excess/challenge/v1" || tag)        Dn = SHA-256 ("bppp/excess/nonce/v1" || tag)
 * NONCE (signer).  k_t = decode (SHA-256 (Dn || put (e_t) || msg_t || aux[32])) mod n      — 128 bytes.  aux is the signer's 32 bytes of
 * randomness; it may be constant, the derivation is deterministic in the secret: equal (e, msg, aux) give an equal signature.
 * CHALLENGE.  c_t = decode (SHA-256 (Dc || put (R.x) || sign (R) || put (X_t.x) || sign (X_t) || msg_t)) mod n      — 130 bytes.  The 33 bytes
 * of R are hashed as they stand in the signature, those of X_t are the canonical affine point's.  THE CHALLENGE HASHES X_t: over (R, msg)
 * alone a forger could choose R = r B + d g, compute c, and solve  s B - c X = R  for X = (s - r) / c B - d / c g — an "excess" with a non-zero
 * g component, i.e. an unbalanced sum that verifies.  With X_t under the hash, c is fixed only after X_t is, and the equation then proves
 * knowledge of log_B X_t.
 * RESPONSE.  s_t = k_t + c_t e_t mod n;  the verifier checks  s_t B - c_t X_t = R_t.
 *
 * bppp_rp_excess_sign{,_device}: the builder's side; it takes no pool — claim_blinds [nsums][4] are the e_t bppp_rp_tally_claims returned.
 * sigs receives the signatures, excess_xy (host, may be NULL, [nsums][8]) the points X_t = e_t B.  sign_status (host, may be NULL, [nsums]):
 *   BPPP_RP_EXCESS_OK             signed
 *   BPPP_RP_EXCESS_NOT_CANONICAL  e >= n
 *   BPPP_RP_EXCESS_ZERO           e = 0: the excess is infinity and has no encoding; the plain tally with e = 0 serves this case
 *   BPPP_RP_EXCESS_NONCE          k = 0
 * A refused sum gets 65 zero bytes (and a zero excess_xy row).  With sign_status == NULL a refusal is BPPP_ERR_ARG and bppp_last_error names
 * the lowest such sum ("sum N: ..."), as bppp_rp_commit_batch does; the signatures are then as they would be with sign_status given.
 * No side-channel hardening, as everywhere in this library.
 *
 * bppp_rp_excess_verify_each{,_device}: status [nsums] (required), one exact verdict per sum — the first that applies of
 *   BPPP_RP_OPEN_MALFORMED (2)      an x in a referenced commitment has no curve point
 *   BPPP_RP_OPEN_NOT_CANONICAL (3)  the claimed type is >= n, or s >= n
 *   BPPP_RP_EXCESS_BAD_R (4)        the sign byte is not 0 or 1, or R.x has no curve point
 *   BPPP_RP_EXCESS_NO_KEY (5)       X_t is infinity
 *   BPPP_RP_OPEN_MISMATCH (1) or BPPP_RP_OPEN_OK (0), from the equation.
 * excess_xy (host, may be NULL, [nsums][8]): X_t, zeros for infinity and for a MALFORMED sum.  c_t X_t is a scalar multiplication of a point
 * of its own per sum: four lanes share each (256 doublings and the additions of the set bits, on the complete law).
 *
 * bppp_rp_excess_verify_batch{,_device}: all sums by ONE weighted combination per pass,
 *   combined = sum_t rho_t (s_t B - c_t X_t - R_t)        over the sums whose verdict the equation has to give,
 *   rho_t = decode (SHA-256 (seed[32] || le64 (index_offset + t) || sig_t[65] || put (X_t.x) || sign (X_t) || msg_t)) mod n, 1 in place of 0
 *                                                                                                                      — 170 bytes,
 * as one MSM over 2 ns + 1 terms: (sum rho_t s_t) on B, n - rho_t c_t on X_t, n - rho_t on R_t.  *accept = 1 iff no sum has one of the
 * verdicts 2 .. 5 and combined is the identity.  status (may be NULL): all BPPP_RP_OPEN_OK when accepted; on rejection exactly
 * bppp_rp_excess_verify_each's verdicts, from one such pass (no bisection).  combined_xy (may be NULL): the combined point, infinity as all
 * zeros.  seed, index_offset, shards adding up with bppp_sum_points and the passes of bounded workspace are as in bppp_rp_tally_batch_device;
 * bppp_rp_excess_verify_batch is the _device call with index_offset 0.
 *
 * The host variants upload, call the _device variant and download; status and point arrays are host memory; aux and seed are host memory.
 * nsums == 0 is BPPP_OK (verify_batch with *accept = 1).  Argument errors, CSR errors and their texts are as for bppp_rp_tally_each (only one
 * of claim_amounts / claim_types NULL on a typed handle is BPPP_ERR_ARG); the CSR verdict is read back before anything gathers. */
#define BPPP_RP_EXCESS_SIG_BYTES 65
#define BPPP_RP_EXCESS_OK 0u
#define BPPP_RP_EXCESS_NOT_CANONICAL 1u
#define BPPP_RP_EXCESS_ZERO 2u
#define BPPP_RP_EXCESS_NONCE 3u
#define BPPP_RP_EXCESS_BAD_R 4u
#define BPPP_RP_EXCESS_NO_KEY 5u
int bppp_rp_excess_sign(bppp_rp *rp, size_t nsums, const uint64_t *claim_blinds, const uint8_t *msgs, const uint8_t aux[32], uint8_t *sigs,
                        uint64_t *excess_xy /* may be NULL */, uint32_t *sign_status /* may be NULL */);
int bppp_rp_excess_sign_device(bppp_rp *rp, size_t nsums, const void *d_claim_blinds, const void *d_msgs, const uint8_t aux[32], void *d_sigs,
                               uint64_t *excess_xy /* host, [nsums][8], may be NULL */, uint32_t *sign_status /* host, [nsums], may be NULL */);
int bppp_rp_excess_verify_each(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries,
                               size_t nnz, const uint64_t *claim_amounts, const uint64_t *claim_types, const uint8_t *msgs, const uint8_t *sigs,
                               uint32_t *status, uint64_t *excess_xy /* may be NULL */);
int bppp_rp_excess_verify_each_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries,
                                      size_t nnz, const void *d_claim_amounts, const void *d_claim_types, const void *d_msgs, const void *d_sigs,
                                      uint32_t *status /* host, [nsums], required */, uint64_t *excess_xy /* host, [nsums][8], may be NULL */);
int bppp_rp_excess_verify_batch(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries,
                                size_t nnz, const uint64_t *claim_amounts, const uint64_t *claim_types, const uint8_t *msgs, const uint8_t *sigs,
                                const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy);
int bppp_rp_excess_verify_batch_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries,
                                       size_t nnz, const void *d_claim_amounts, const void *d_claim_types, const void *d_msgs, const void *d_sigs,
                                       uint64_t index_offset, const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy);

/* ---- excess keys: the excess stated as a public key, so that signatures and sums still check after cut-through ------------------------------
 * The calls above derive X_t from the pool, so a signature can only be checked by someone who holds every input and output of its
 * transaction.  Here the transaction PUBLISHES its excess as a key next to the signature.  Then (1) an archive node or a mempool checks (key,
 * message, signature) triples with no commitment in hand, and (2) a block that has merged its transactions and dropped the outputs spent inside
 * it (cut-through) is still checked as one sum: the remaining outputs minus the inputs, minus the fees, minus a revealed offset, equal the sum of
 * the stated keys.  Domains, messages, put, decode, the sign byte and B are those of the excess signatures above; a signature made by
 * bppp_rp_excess_sign verifies under the stated key X_t = e_t B, the same 65 bytes.
 *
 * KEY.  keys [n][BPPP_RP_EXCESS_KEY_BYTES = 33]: put (x), then one sign byte, 0 or 1 (y > p - y) — exactly how a signature holds R.  It is lifted
 * by the decoder the pool and R take (x is reduced mod p; the root of x^3 + 7 with that sign).  EVERY HASH THAT NAMES THE KEY — the challenge c and
 * the weight rho of verify_keys_batch — TAKES THE CANONICAL 33 BYTES OF THE LIFTED POINT (put of the reduced x, the sign of the chosen y), not
 * the bytes as they were passed: that is what the derived-key calls hash, so both paths give one verdict.  Infinity has no encoding, so there is
 * no NO_KEY verdict here.  BPPP_RP_EXCESS_BAD_KEY (6): the sign byte is above 1, or x has no curve point.
 *
 * bppp_rp_excess_keys{,_device}: the builder's side.  claim_blinds [nsums][4] as bppp_rp_excess_sign takes them; keys [nsums][33] receives
 * X_t = e_t B, over the table the signer uses.  key_status (host, may be NULL, [nsums]): BPPP_RP_EXCESS_OK, BPPP_RP_EXCESS_NOT_CANONICAL (e >= n)
 * or BPPP_RP_EXCESS_ZERO (e = 0); a refused row gets 33 zero bytes.  With key_status == NULL a refusal is BPPP_ERR_ARG and bppp_last_error names
 * the lowest refused sum ("sum N: ..."), as bppp_rp_excess_sign does; the keys are then as they would be with key_status given.
 *
 * bppp_rp_excess_verify_keys_each{,_device}: keys, msgs [nkeys][32], sigs [nkeys][65]; status [nkeys] (host, required), the first that applies of
 *   BPPP_RP_EXCESS_BAD_KEY (6)      the key's sign byte is above 1, or its x has no curve point
 *   BPPP_RP_OPEN_NOT_CANONICAL (3)  s >= n
 *   BPPP_RP_EXCESS_BAD_R (4)        the sign byte of R is not 0 or 1, or R.x has no curve point
 *   BPPP_RP_OPEN_MISMATCH (1) or BPPP_RP_OPEN_OK (0), from  s B - c X = R  with
 *   c = decode (SHA-256 (Dc || sig[0..33) || the canonical 33 bytes of X || msg)) mod n      — the CHALLENGE above, 130 bytes.
 * No pool is decoded, no sum is formed and nothing is inverted: one lane lifts a key, four lanes share the walk of c X.
 *
 * bppp_rp_excess_verify_keys_batch{,_device}: all signatures by ONE weighted combination per pass of 2^20 keys,
 *   combined = sum_t rho_t (s_t B - c_t X_t - R_t)        over the keys whose verdict the equation has to give,
 *   rho_t = decode (SHA-256 (seed[32] || le64 (index_offset + t) || sig_t[65] || the canonical 33 bytes of X_t || msg_t)) mod n, 1 in place of 0
 *                                                                                                                      — 170 bytes,
 * as one MSM over 2 nkeys + 1 terms, exactly as bppp_rp_excess_verify_batch.  *accept = 1 iff no key has a verdict other than OK or MISMATCH and
 * combined is the identity (a BAD_KEY contributes no term and still rejects).  status (may be NULL): all OK when accepted; on rejection exactly
 * verify_keys_each's verdicts, from one such pass.  combined_xy (may be NULL): the combined point, infinity as all zeros.  seed, index_offset and
 * shards adding up with bppp_sum_points are as in bppp_rp_tally_batch_device; the host call is the _device call with index_offset 0.
 * nkeys == 0 is BPPP_OK (*accept = 1).
 *
 * bppp_rp_excess_sums_each{,_device}: the tally's job — POOL, SUMS, entries and claims exactly as for bppp_rp_tally_each — plus the keys of every
 * sum: key_start [nsums + 1] (uint32, required, non-decreasing, key_start[0] = 0, key_start[nsums] = nkeys) and keys [nkeys][33]; the keys of sum
 * t are the contiguous rows key_start[t] .. key_start[t + 1].  Sum t must satisfy
 *   S_t - a_t g - ty_t H0 - o_t B - sum of the keys of group t = identity        (a binary handle: no H0 term, claim_types ignored)
 * claim_offsets is the tally's claim_blinds under its protocol name: a REVEALED scalar o_t.  Amounts, types and offsets all NULL: zero claims.
 * status [nsums] (host, required), the first that applies of
 *   BPPP_RP_OPEN_MALFORMED (2)      an x in a referenced commitment has no curve point
 *   BPPP_RP_EXCESS_BAD_KEY (6)      a key of the group has a sign byte above 1 or an x without a curve point
 *   BPPP_RP_OPEN_NOT_CANONICAL (3)  the claimed type or offset is >= n
 *   BPPP_RP_OPEN_MISMATCH (1) or BPPP_RP_OPEN_OK (0).
 * sums_xy (host, may be NULL, [nsums][8]): S_t - sum of the keys of group t; zeros for infinity, for a MALFORMED sum and for a BAD_KEY sum.  A
 * group may be empty: that sum is exactly a tally.  DUPLICATE KEYS ARE NOT REJECTED: a key that stands twice is subtracted twice, in one group or in
 * two — whether a key may be used again is the caller's rule (a chain keeps its own set of seen kernels).  The keys are lifted behind the decoded
 * pool and merged into the sums, so a sum's keys are split into pieces and summed in the same pass as its entries: thousands of keys in one sum cost
 * what thousands of entries cost.
 *
 * bppp_rp_excess_sums_batch{,_device}: combined = sum_t rho_t (S_t - a_t g - ty_t H0 - o_t B - sum of the keys of group t) as one MSM over
 * nnz + nkeys + 3 terms per pass, with rho_t exactly bppp_rp_tally_batch's weight over (seed, index_offset + t, a_t, ty_t, o_t): the keys, like the
 * pool, are the checker's own inputs fixed before the seed is drawn.  accept (a BAD_KEY rejects), status on rejection, combined_xy, index_offset and
 * shards are as in bppp_rp_tally_batch_device.
 *
 * Errors (BPPP_ERR_ARG, bppp_last_error names the offender): those of bppp_rp_tally_each, and rows * nranges + nkeys >= 2^31, nnz + nkeys >= 2^31,
 * a key_start that is not non-decreasing from 0 to nkeys ("key_start[i] = ...").  key_start is validated as sum_start is: by a kernel whose verdict
 * is read back before anything reads through the array — a bad array is an error code, never an out-of-bounds read, and no output buffer is written.
 * nsums == 0 is BPPP_OK (sums_batch with *accept = 1) and nothing else is looked at.  The host variants upload, call the _device variant and
 * download; status and point arrays, aux and seed are host memory. */
#define BPPP_RP_EXCESS_KEY_BYTES 33
#define BPPP_RP_EXCESS_BAD_KEY 6u
int bppp_rp_excess_keys(bppp_rp *rp, size_t nsums, const uint64_t *claim_blinds, uint8_t *keys, uint32_t *key_status /* may be NULL */);
int bppp_rp_excess_keys_device(bppp_rp *rp, size_t nsums, const void *d_claim_blinds, void *d_keys, uint32_t *key_status /* host, [nsums], may be NULL */);
int bppp_rp_excess_verify_keys_each(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *sigs, uint32_t *status);
int bppp_rp_excess_verify_keys_each_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_sigs,
                                           uint32_t *status /* host, [nkeys], required */);
int bppp_rp_excess_verify_keys_batch(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *sigs, const uint8_t seed[32], int *accept,
                                     uint32_t *status /* may be NULL */, uint64_t *combined_xy /* may be NULL */);
int bppp_rp_excess_verify_keys_batch_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_sigs, uint64_t index_offset,
                                            const uint8_t seed[32], int *accept, uint32_t *status /* host, may be NULL */, uint64_t *combined_xy /* may be NULL */);
int bppp_rp_excess_sums_each(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                             const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_offsets, size_t nkeys, const uint32_t *key_start,
                             const uint8_t *keys, uint32_t *status, uint64_t *sums_xy /* may be NULL */);
int bppp_rp_excess_sums_each_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                                    const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_offsets, size_t nkeys, const void *d_key_start,
                                    const void *d_keys, uint32_t *status /* host, [nsums], required */, uint64_t *sums_xy /* host, [nsums][8], may be NULL */);
int bppp_rp_excess_sums_batch(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                              const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_offsets, size_t nkeys, const uint32_t *key_start,
                              const uint8_t *keys, const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy);
int bppp_rp_excess_sums_batch_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                                     const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_offsets, size_t nkeys, const void *d_key_start,
                                     const void *d_keys, uint64_t index_offset, const uint8_t seed[32], int *accept, uint32_t *status, uint64_t *combined_xy);

/* ---- multi-party excess signatures: builders who each know a PART of the blinding sum sign together --------------------------------------------
 * bppp_rp_excess_sign takes e_t whole.  In a transaction between a sender and a receiver nobody knows it whole: party i knows e_{t,i}, the blinding
 * sum of its own inputs and outputs, and e_t = sum_i e_{t,i}.  The calls below let the parties produce the 65 bytes of the SIGNATURE above under the
 * CHALLENGE above, so every verifier of this header accepts the result as it is.  Two rounds with two nonces a party, as in MuSig2: no commitment
 * round is needed for sessions that run at the same time.  Keys add PLAINLY, with no key-aggregation coefficients: the aggregated key has to equal
 * the excess of the commitments, X_t = sum_i X_{t,i} = S_t - a_t g - ty_t H0, and it is the sums check (bppp_rp_excess_sums_*, or the derived key of
 * bppp_rp_excess_verify_*) that binds it to commitments whose range proofs prove knowledge of their blindings.  A stated-key signature ALONE
 * (bppp_rp_excess_verify_keys_* without that check) does not protect against a cosigner who chooses its key as a difference X' - X_1.
 * B, put, decode, the sign byte, the lift of 33 bytes, tag, Dc and the challenge are those of the two blocks above.  New domains, hashed once a call:
 *   Dm = SHA-256 ("bppp/excess/partnonce/v1" || tag)        Db = SHA-256 ("bppp/excess/noncecoef/v1" || tag)
 * Dm is not the single signer's Dn: a party that also signs alone with the same (e, msg, aux) never uses a nonce twice.
 *   party nonces   k_j = decode (SHA-256 (Dm || put (e_i) || msg[32] || aux[32] || byte j)) mod n,  j = 1, 2                          — 129 bytes
 *   public nonce   [BPPP_RP_EXCESS_PUBNONCE_BYTES = 66]: the 33 bytes of R1 = k_1 B, then the 33 bytes of R2 = k_2 B
 *   aggregates     R1agg = sum_i R1_i,  R2agg = sum_i R2_i,  X = sum_i X_i;  X_i = e_i B as 33 bytes comes from bppp_rp_excess_keys
 *   coefficient    b = decode (SHA-256 (Db || canon33 (R1agg) || canon33 (R2agg) || canon33 (X) || msg)) mod n                        — 163 bytes
 *                  canon33: the canonical 33 bytes of the LIFTED point, the rule of every hash that names a key
 *   session        R = R1agg + b R2agg,    c = the CHALLENGE over (canon33 (R), X, msg): the single signer's, byte for byte
 *   partial        [BPPP_RP_EXCESS_PARTIAL_BYTES = 32]: put (s_i),  s_i = k_1 + b k_2 + c e_i mod n
 *   signature      canon33 (R) || put (sum_i s_i mod n)
 *   partial check  s_i B - b R2_i - c X_i = R1_i
 * GROUPS.  part_start [nsums + 1] (uint32, non-decreasing, part_start[0] = 0, part_start[nsums] = nparts): the parts of sum t are the contiguous
 * rows part_start[t] .. part_start[t + 1] of pubnonces [nparts][66], keys [nparts][33] and partials [nparts][32].  It is validated as key_start is:
 * by a kernel whose verdict is read back before anything reads through the array.  A sum with no part is BPPP_ERR_ARG ("part_start: sum N has no part").
 *
 * 1. bppp_rp_excess_part_nonces{,_device}: round 1 for n sessions of ONE party: part_blinds [n][4], msgs [n][32], aux[32] -> pubnonces [n][66].
 *    status (host, may be NULL, [n]): BPPP_RP_EXCESS_OK, _NOT_CANONICAL (e >= n), _ZERO (e = 0) or _NONCE (k_1 or k_2 is 0); a refused row is 66
 *    zero bytes.  With status == NULL a refusal is BPPP_ERR_ARG and bppp_last_error names the lowest refused row ("part N: ..."); the output is then
 *    as it would be with status given.  The secret nonces never leave the call: round 2 derives them again.
 * 2. bppp_rp_excess_part_aggregate{,_device}: the coordinator's step; it needs no secret.  agg_nonces [nsums][66] = (R1agg, R2agg) and agg_keys
 *    [nsums][33] = X.  status (host, may be NULL, [nsums]), the first that applies of
 *      BPPP_RP_EXCESS_BAD_KEY (6)         a key of the group has a sign byte above 1 or an x without a curve point
 *      BPPP_RP_EXCESS_BAD_R (4)           a nonce point of the group has
 *      BPPP_RP_EXCESS_NO_KEY (5)          X is infinity
 *      BPPP_RP_EXCESS_NONCE_INFINITY (7)  R1agg or R2agg is infinity
 *      BPPP_RP_EXCESS_OK (0)
 *    A refused sum gets zero bytes; with status == NULL a refusal is BPPP_ERR_ARG ("sum N: ...").
 * 3. bppp_rp_excess_part_sign{,_device}: round 2 for n sessions of one party: partials [n][32].  It is STATELESS: k_1 and k_2 are derived again from
 *    (e, msg, aux), the aggregates are lifted, and b, R, c and s_i follow.  status (host, may be NULL, [n]), the first that applies of the three
 *    refusals of call 1, BPPP_RP_EXCESS_BAD_KEY (agg_keys does not lift), BPPP_RP_EXCESS_BAD_R (an aggregated nonce point does not),
 *    BPPP_RP_EXCESS_NONCE_INFINITY (R is infinity), BPPP_RP_EXCESS_OK; refusals and a NULL status as in call 1.
 *    TWO RULES THE CALLER MUST KEEP.  (a) aux is FRESH RANDOMNESS for every session.  (b) part_sign is NEVER called twice with one (e, msg, aux) under
 *    different aggregates.  Either mistake yields two responses over the same nonces under different b or c, and they reveal e.  The library is not
 *    hardened against side channels, here as everywhere.
 * 4. bppp_rp_excess_part_verify{,_device}: who misbehaved.  It aggregates by the stage of call 2 itself, so a caller cannot hand it aggregates that
 *    do not belong to the parts.  msgs [nsums][32].  status [nparts] (host, required), per part the first that applies of
 *      BPPP_RP_EXCESS_BAD_KEY (6)         the part's key does not lift
 *      BPPP_RP_OPEN_NOT_CANONICAL (3)     s_i >= n
 *      BPPP_RP_EXCESS_BAD_R (4)           one of the part's nonce points does not lift
 *      BPPP_RP_EXCESS_NO_AGGREGATE (8)    ANOTHER part of its sum has a key or a nonce point that does not lift: the sum has no aggregate and this
 *                                         part no equation to be asked, until that part — the one that reads BAD_KEY or BAD_R — is replaced
 *      the verdict of its sum, if that is not OK: BPPP_RP_EXCESS_NO_KEY (5) or BPPP_RP_EXCESS_NONCE_INFINITY (7; also: R is infinity)
 *      BPPP_RP_OPEN_MISMATCH (1) or BPPP_RP_OPEN_OK (0), from the partial check.
 *    sum_status (host, may be NULL, [nsums]): the verdict of each sum as call 2 gives it, NONCE_INFINITY also for R.
 * 5. bppp_rp_excess_part_combine{,_device}: the final signatures sigs [nsums][65]; agg_keys (may be NULL) [nsums][33].  status (host, may be NULL,
 *    [nsums]) as sum_status of call 4; a refused sum gets zero bytes, and with status == NULL a refusal is BPPP_ERR_ARG ("sum N: ...").  IT DOES NOT
 *    CHECK THE PARTIALS (each is taken mod n): the caller checks the 65 bytes with bppp_rp_excess_verify_keys_each under the aggregated key, and
 *    runs call 4 only when that fails.
 *
 * PASSES.  Calls 2, 4 and 5 cut their passes over the workspace at sum boundaries, 2^20 parts a pass; a single sum with more parts than one pass
 * holds is BPPP_ERR_ARG, and bppp_last_error names the sum and the limit.  A group is added serially by four lanes: parties per transaction are few.
 * Errors (BPPP_ERR_ARG): a NULL buffer, n, nsums or nparts >= 2^31, a part_start that is not non-decreasing from 0 to nparts ("part_start[i] =
 * ..."), an empty or an over-long group; no output buffer is written then.  n == 0 or nsums == 0 is BPPP_OK and nothing else is looked at.  The host
 * variants upload, call the _device variant and download; status arrays and aux are host memory. */
#define BPPP_RP_EXCESS_PUBNONCE_BYTES 66
#define BPPP_RP_EXCESS_PARTIAL_BYTES 32
#define BPPP_RP_EXCESS_NONCE_INFINITY 7u
#define BPPP_RP_EXCESS_NO_AGGREGATE 8u
int bppp_rp_excess_part_nonces(bppp_rp *rp, size_t n, const uint64_t *part_blinds, const uint8_t *msgs, const uint8_t aux[32], uint8_t *pubnonces,
                               uint32_t *status /* may be NULL */);
int bppp_rp_excess_part_nonces_device(bppp_rp *rp, size_t n, const void *d_part_blinds, const void *d_msgs, const uint8_t aux[32], void *d_pubnonces,
                                      uint32_t *status /* host, [n], may be NULL */);
int bppp_rp_excess_part_aggregate(bppp_rp *rp, size_t nsums, size_t nparts, const uint32_t *part_start, const uint8_t *pubnonces, const uint8_t *keys,
                                  uint8_t *agg_nonces, uint8_t *agg_keys, uint32_t *status /* may be NULL */);
int bppp_rp_excess_part_aggregate_device(bppp_rp *rp, size_t nsums, size_t nparts, const void *d_part_start, const void *d_pubnonces, const void *d_keys,
                                         void *d_agg_nonces, void *d_agg_keys, uint32_t *status /* host, [nsums], may be NULL */);
int bppp_rp_excess_part_sign(bppp_rp *rp, size_t n, const uint64_t *part_blinds, const uint8_t *msgs, const uint8_t aux[32], const uint8_t *agg_nonces,
                             const uint8_t *agg_keys, uint8_t *partials, uint32_t *status /* may be NULL */);
int bppp_rp_excess_part_sign_device(bppp_rp *rp, size_t n, const void *d_part_blinds, const void *d_msgs, const uint8_t aux[32], const void *d_agg_nonces,
                                    const void *d_agg_keys, void *d_partials, uint32_t *status /* host, [n], may be NULL */);
int bppp_rp_excess_part_verify(bppp_rp *rp, size_t nsums, size_t nparts, const uint32_t *part_start, const uint8_t *pubnonces, const uint8_t *keys,
                               const uint8_t *partials, const uint8_t *msgs, uint32_t *status, uint32_t *sum_status /* may be NULL */);
int bppp_rp_excess_part_verify_device(bppp_rp *rp, size_t nsums, size_t nparts, const void *d_part_start, const void *d_pubnonces, const void *d_keys,
                                      const void *d_partials, const void *d_msgs, uint32_t *status /* host, [nparts], required */,
                                      uint32_t *sum_status /* host, [nsums], may be NULL */);
int bppp_rp_excess_part_combine(bppp_rp *rp, size_t nsums, size_t nparts, const uint32_t *part_start, const uint8_t *pubnonces, const uint8_t *keys,
                                const uint8_t *partials, const uint8_t *msgs, uint8_t *sigs, uint8_t *agg_keys /* may be NULL */, uint32_t *status /* may be NULL */);
int bppp_rp_excess_part_combine_device(bppp_rp *rp, size_t nsums, size_t nparts, const void *d_part_start, const void *d_pubnonces, const void *d_keys,
                                       const void *d_partials, const void *d_msgs, void *d_sigs, void *d_agg_keys /* may be NULL */,
                                       uint32_t *status /* host, [nsums], may be NULL */);

/* ---- a block in one call: range proofs, key signatures and sums after cut-through as ONE MSM --------------------------------------------
 * A node that receives a block checks the range proofs of its new outputs (bppp_rp_verify_bound), the kernel signatures against their
 * stated keys (bppp_rp_excess_verify_keys_batch) and the balance after cut-through (bppp_rp_excess_sums_batch).  bppp_rp_verify_block runs the
 * three as one weighted combination: one MSM of
 *   T = 1 + llen + nlen + nproofs (ninit + 2k) + nnz + 2 nkeys
 * terms  [ g | H | G | per-proof terms | entry terms | per key: X_k, R_k ]  instead of three MSMs of nkeys + 4 terms more.  Up to the verdict
 * every key is lifted once and the commitments of the proven rows are square-rooted once; the status passes of a REJECTED block are the
 * counterparts' own and lift what they need again (the keys once more for key_status and once more for sum_status).
 *
 * bppp_rp_block, all of one handle (typed-reciprocal or binary, either argument flavour):
 *   POOL        rows, coms_files [rows][coms_bytes] as bppp_rp_tally_each takes them; rows [0, nproofs) are the outputs that carry a proof
 *   PROOFS      nproofs <= rows, proof_files [nproofs][proof_bytes] (NULL allowed when nproofs == 0), bindings [nproofs][32] or NULL (an
 *               unbound call) as bppp_rp_verify_bound takes them.  The proofs verify under the handle's own public amounts.
 *   SUMS        nsums, sum_start, entries, nnz, claim_amounts, claim_types, claim_offsets, nkeys, key_start, keys [nkeys][33] exactly as
 *               bppp_rp_excess_sums_batch takes them
 *   SIGNATURES  msgs [nkeys][32], sigs [nkeys][65]: one per key, as bppp_rp_excess_verify_keys_batch takes them
 *   OFFSETS     proof_offset, key_offset, sum_offset: the job positions of this shard's proofs, keys and sums (0 for a whole block)
 * bppp_rp_verify_block takes host pointers in the struct, bppp_rp_verify_block_device HBM pointers; seed, accept, the status arrays and
 * combined_xy are host memory in both.
 *
 * Part seeds: seed_p = SHA-256 ("bppp block" (10 bytes) || seed[32] || byte p), a message of 43 bytes, with p = 0 for the proofs, 1 for the
 * signatures, 2 for the sums; derived on the host.  The three weight families of the counterpart calls hash messages of different layouts;
 * under separate sub-seeds their independence needs no argument about message lengths.
 * Combined point: combined = V + K + S, where V is the combined_xy of bppp_rp_verify_bound_device over rows [0, nproofs) with index_offset =
 * proof_offset, public_amounts = NULL and seed_0; K that of bppp_rp_excess_verify_keys_batch_device with index_offset = key_offset and seed_1;
 * S that of bppp_rp_excess_sums_batch_device with index_offset = sum_offset and seed_2.  Every weight, challenge and scalar is the counterpart's
 * own formula; key k of sum t carries the ONE scalar  n - rho^K_k c_k - rho^S_t  (mod n)  on X_k.  The point is defined by the formula only when
 * nothing is malformed or non-canonical, as the counterparts say.
 * *accept = 1 iff every proof decodes, no referenced commitment is malformed, no key has a verdict other than OK or MISMATCH, no claim is
 * non-canonical, and combined is the identity.
 * Status (bppp_rp_block_status, host arrays, each may be NULL, as may the struct): proof_status [nproofs], key_status [nkeys], sum_status
 * [nsums].  On acceptance every array given is filled with VALID / OK (zeros).  On rejection each array given receives exactly what the
 * counterpart reports over the same inputs: proof_status by the handle's culprit search (bisection, or one per-proof pass under
 * BPPP_RP_OPT_CULPRITS = 1), key_status by one pass of bppp_rp_excess_verify_keys_each, sum_status by one pass of bppp_rp_excess_sums_each.  A
 * rejected combined point does not say which part failed, so all the arrays asked for are computed.
 * Sharding: ranks pass the same seed, their own slices (rows and entries re-indexed per shard) and offsets; their points add up with
 * bppp_sum_points to the one-call point.
 * Empty parts: any part may be empty and its term of the formula is then the identity; with nsums == 0 the keys belong to no sum and only their
 * signatures are checked.  All three empty returns BPPP_OK with *accept = 1 and looks at nothing else.
 * BPPP_ERR_ARG (bppp_last_error names the offender; no output buffer is written on an error): the errors of the three counterparts, under the name
 * rp_verify_block; nproofs > rows; the tag limit of the bound calls when bindings are given; rows * nranges + nkeys, nnz + nkeys or nsums at
 * or above 2^31; nproofs >= 2^22; and a block that does not fit ONE pass of the handle's limits (nnz + nkeys or nsums above the tally's chunk,
 * nkeys above a quarter of the flat chunk): the block call is one MSM by contract, the text names the limit and says "shard it", and the offsets
 * are the route to larger jobs.  sum_start, entries and key_start are validated by kernels whose verdict is read back before anything reads
 * through the arrays. */
typedef struct bppp_rp_block {
  size_t rows;    const void *coms_files;                 /* [rows][coms_bytes] */
  size_t nproofs; const void *proof_files;                /* [nproofs][proof_bytes]; NULL ok when nproofs == 0 */
  const void *bindings;                                   /* [nproofs][32] or NULL (unbound) */
  size_t nsums; const void *sum_start, *entries; size_t nnz;
  const void *claim_amounts, *claim_types, *claim_offsets;
  size_t nkeys; const void *key_start, *keys;             /* [nsums + 1], [nkeys][33] */
  const void *msgs, *sigs;                                /* [nkeys][32], [nkeys][65] */
  uint64_t proof_offset, key_offset, sum_offset;
} bppp_rp_block;
typedef struct bppp_rp_block_status { uint32_t *proof_status, *key_status, *sum_status; } bppp_rp_block_status;  /* host; each may be NULL */
int bppp_rp_verify_block(bppp_rp *rp, const bppp_rp_block *blk, const uint8_t seed[32], int *accept, const bppp_rp_block_status *status /* may be NULL */,
                         uint64_t *combined_xy /* may be NULL */);
int bppp_rp_verify_block_device(bppp_rp *rp, const bppp_rp_block *blk, const uint8_t seed[32], int *accept, const bppp_rp_block_status *status /* may be NULL */,
                                uint64_t *combined_xy /* may be NULL */);

/* ---- half-aggregate excess signatures: 33 bytes a kernel and one scalar, checked as one MSM ------------------------------------------------
 * After cut-through the kernels (a 33-byte key and a 65-byte signature each) are what a chain keeps for ever.  Non-interactive half-aggregation
 * turns the n signatures (R_i, s_i) of a block into the n nonce points and ONE scalar: BPPP_RP_EXCESS_AGG_BYTES (n) = 33 n + 32 bytes instead
 * of 65 n.  Anyone who holds the signatures can aggregate, with no secret and no interaction; the check is deterministic and takes no seed.
 * put, decode, the sign byte, the lift of 33 bytes, B, tag and the challenge c_i are those of the excess signatures and the stated keys above.
 * The canonical 33 bytes of a key are put (x mod p), then the sign byte as it stands: defined for every row, with no square root.
 *   domains      Dl = SHA-256 ("bppp/excess/halfagg/leaf/v1" || tag), Dn = SHA-256 ("bppp/excess/halfagg/node/v1" || tag),
 *                Dz = SHA-256 ("bppp/excess/halfagg/coef/v1" || tag), hashed once a call on the host
 *   leaf         leaf_i = SHA-256 (Dl || the 33 bytes of R_i as the signature holds them || the canonical 33 bytes of X_i || msg_i)  — 130 bytes;
 *                the raw digest, not reduced
 *   tree         level 0: the n leaves in job order; level k has ceil (count_{k-1} / 2) nodes, node (k, j) = SHA-256 (Dn || node (k-1, 2j) ||
 *                node (k-1, 2j+1)) — 96 bytes — when 2j + 1 < count_{k-1}, else node (k-1, 2j) unchanged; root: the node of the level of one
 *                (n = 1: leaf_0)
 *   coefficient  z_i = decode (SHA-256 (Dz || root || le64 (n) || le64 (i))) mod n, 1 in place of 0                                  — 80 bytes
 *   aggregate    the n rows of 33 bytes of R_i, copied as they stand, then put (s_agg), s_agg = sum_i z_i s_i mod n
 *   equation     s_agg B - sum_i z_i (c_i X_i + R_i) = identity: one MSM per pass over  n - z_i c_i  on X_i,  n - z_i  on R_i, and s_agg on B once
 * The tree commits to every (R, X, msg) and to n before any z_i is fixed, so errors in several s_i cannot be chosen to cancel.
 * THE AGGREGATE CANNOT NAME A CULPRIT: one equation speaks for all keys, and the s_i are gone.  Check the signatures before they are aggregated.
 * INCREMENTAL AGGREGATION IS OUT OF SCOPE: one more signature changes the root and with it every z_i; aggregate a block once, from its signatures.
 * THE AGGREGATE IS NOT SHARDABLE BY KEYS: every z_i depends on all of them, so the verifier takes no index offset.
 *
 * bppp_rp_excess_halfagg{,_device}: keys [nkeys][33], msgs [nkeys][32], sigs [nkeys][65] -> agg [33 nkeys + 32].  status (host, may be NULL,
 * [nkeys]), per signature the first that applies of BPPP_RP_EXCESS_BAD_KEY (6), BPPP_RP_OPEN_NOT_CANONICAL (3: s >= n), BPPP_RP_EXCESS_BAD_R (4),
 * BPPP_RP_OPEN_OK.  IT DOES NOT EVALUATE THE EQUATION of any signature: run bppp_rp_excess_verify_keys_batch over the same buffers first.  If any
 * signature is refused agg is all zero bytes; with status == NULL a refusal is BPPP_ERR_ARG and bppp_last_error names the lowest refused key
 * ("key N: ..."), as bppp_rp_excess_keys does for its sums.
 *
 * bppp_rp_excess_halfagg_verify{,_device}: *accept = 1 iff no key is BAD_KEY, no R row is BAD_R, s_agg < n and the combined point is the
 * identity.  status (host, may be NULL, [nkeys]), per key the first that applies of 6, 4, 3 (for every key still open when s_agg >= n), otherwise
 * the ONE verdict of the equation, BPPP_RP_OPEN_MISMATCH or BPPP_RP_OPEN_OK, for all open keys alike.  combined_xy (host, may be NULL): the left
 * side of the equation over the open keys, infinity as zeros.
 *
 * bppp_rp_verify_block_agg{,_device}: bppp_rp_verify_block with the aggregate in place of the signatures.  blk->sigs must be NULL and
 * blk->key_offset 0 (else BPPP_ERR_ARG); agg [33 nkeys + 32] lies where the struct's pointers lie (host / HBM).  combined = V + K' + S with V and S
 * exactly as in bppp_rp_verify_block under seed_0 and seed_2, and
 *   K' = rho_A (s_agg B - sum_k z_k (c_k X_k + R_k)),
 *   rho_A = decode (SHA-256 (seed_1 || le64 (nkeys) || root || the 32 bytes of s_agg)) mod n, 1 in place of 0                        — 104 bytes.
 * Key k of sum t carries the one scalar  n - rho_A z_k c_k - rho^S_t  on X_k, and every key is lifted once.  On rejection key_status is that of
 * bppp_rp_excess_halfagg_verify; proof_status and sum_status are as in the block call, and so are the one-pass limits, errors and texts.
 *
 * nkeys == 0 is BPPP_OK (*accept = 1; the aggregator writes nothing) and nothing else is looked at.  BPPP_ERR_ARG: a NULL handle or buffer,
 * nkeys >= 2^31.  The host variants upload, call the _device variant and download; status and point arrays are host memory. */
#define BPPP_RP_EXCESS_AGG_BYTES(n) (33 * (size_t)(n) + 32)
int bppp_rp_excess_halfagg(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *sigs, uint8_t *agg, uint32_t *status /* may be NULL */);
int bppp_rp_excess_halfagg_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_sigs, void *d_agg,
                                  uint32_t *status /* host, [nkeys], may be NULL */);
int bppp_rp_excess_halfagg_verify(bppp_rp *rp, size_t nkeys, const uint8_t *keys, const uint8_t *msgs, const uint8_t *agg, int *accept,
                                  uint32_t *status /* may be NULL */, uint64_t *combined_xy /* may be NULL */);
int bppp_rp_excess_halfagg_verify_device(bppp_rp *rp, size_t nkeys, const void *d_keys, const void *d_msgs, const void *d_agg, int *accept,
                                         uint32_t *status /* host, may be NULL */, uint64_t *combined_xy /* may be NULL */);
int bppp_rp_verify_block_agg(bppp_rp *rp, const bppp_rp_block *blk, const uint8_t *agg, const uint8_t seed[32], int *accept,
                             const bppp_rp_block_status *status /* may be NULL */, uint64_t *combined_xy /* may be NULL */);
int bppp_rp_verify_block_agg_device(bppp_rp *rp, const bppp_rp_block *blk, const void *d_agg, const uint8_t seed[32], int *accept,
                                    const bppp_rp_block_status *status /* may be NULL */, uint64_t *combined_xy /* may be NULL */);

/* ---- sealed outputs: a one-sided receive, and the view-key scan of an output set ---------------------------------------------------
 * Every call above assumes that the owner of an output knows its amount, type and blinding.  A SEAL next to an output lets the holder of a view
 * secret find the outputs that are its own in a set of outputs, with their openings, without having been online when they were made.
 * put, decode, the sign byte and the 33-byte point format are those of the excess keys; tag = the handle's oracle tag bytes; B, g, H0 and the
 * commitment C = v g + ty H0 + bl B are bppp_rp_commit_batch's (B = H1, or h0 of a binary handle, which has no H0); n = the group order.
 *
 * KEYS.  The view secret is a, 1 <= a < n; the view key is A = a B as 33 bytes: bppp_rp_excess_keys with claim_blinds = a writes it.
 * DOMAINS, computed once per call on the host:
 *   Ds = SHA-256 ("bppp/seal/shared/v1" || tag), Dt = SHA-256 ("bppp/seal/tag/v1" || tag), Db = SHA-256 ("bppp/seal/blind/v1" || tag),
 *   Dm = SHA-256 ("bppp/seal/memo/v1" || tag).
 * ROW, with the ephemeral secret r (1 <= r < n) and the recipient's key A:
 *   R  = r B, the hint, stored as 33 bytes;  P = r A = a R, the shared point;
 *   ss = SHA-256 (Ds || put (P.x) || sign (P) || the 33 bytes of R as stored)                                                      —  98 bytes
 *   vt = the first byte of SHA-256 (Dt || ss), the view tag                                                                        —  64 bytes
 * and per range i of the row:
 *   bl_i   = decode (SHA-256 (Db || ss || le32 (i))) mod n                                                                         —  68 bytes
 *   pad_i  = SHA-256 (Dm || ss || le32 (i) || 0x00) || SHA-256 (Dm || ss || le32 (i) || 0x01), 64 bytes                            —  69 bytes each
 *   memo_i = (put (v_i mod n) || put (ty_i)) XOR pad_i, with ty_i = 0 on a binary handle.
 * SEAL of a row:  R[33] || vt[1] || memo_0 .. memo_{nranges - 1}  =  BPPP_RP_SEAL_BYTES (nranges) = 34 + 64 nranges bytes.
 *
 * CAVEATS.  The sender knows the blindings, as in every non-interactive output of this kind: the receiver of a one-sided payment re-spends it
 * into an output of its own.  The intended uses are restore-from-seed (the wallet seals to its own key with r derived from its seed) and such
 * one-sided payments.  Script keys, a defence against a sender who re-spends, and rewinding the proof itself are not here.  There is no
 * side-channel hardening, as everywhere in this library.
 *
 * bppp_rp_seal{,_device}: view_keys [batch][33], eph [batch][4] words (r), amounts and types [batch][nranges][4] words laid out and encoded as for
 * bppp_rp_commit_batch (types may be NULL on a binary handle, which ignores it) -> seals [batch][BPPP_RP_SEAL_BYTES (nranges)] and blinds
 * [batch][nranges][4] words: the caller then commits or proves with these blindings, and nothing else changes for the prover.
 * seal_status (host, may be NULL, [batch]), the first that applies:
 *   BPPP_RP_EXCESS_BAD_KEY (6)      the view key's sign byte is above 1, or its x has no curve point (bppp_rp_excess_verify_keys_each's rule)
 *   BPPP_RP_SEAL_NOT_CANONICAL (1)  r or a type is >= n
 *   BPPP_RP_SEAL_ZERO (2)           r = 0
 *   BPPP_RP_SEAL_OK (0)
 * A refused row gets zero bytes and zero blindings.  With seal_status == NULL a refusal is BPPP_ERR_ARG and bppp_last_error names the lowest such
 * row ("rp_seal: row N: ..."), as bppp_rp_commit_batch does; the outputs are complete either way.
 *
 * bppp_rp_scan{,_device}: view_secret [4] words on the host, coms_files [rows][coms_bytes] as bppp_rp_open_each takes them and seals
 * [rows][BPPP_RP_SEAL_BYTES (nranges)] -> scan_status (host, required, [rows]), per row the first that applies:
 *   BPPP_RP_SCAN_BAD_HINT (2)  R's sign byte is not 0 or 1, or its x has no curve point (the rule of BPPP_RP_EXCESS_BAD_R)
 *   BPPP_RP_SCAN_FOREIGN (0)   the view tag differs
 *   BPPP_RP_SCAN_TAG_ONLY (3)  the tag matches (one foreign row in 256 does so by chance), but a decrypted amount or type is >= n (on a binary
 *                              handle: the type is not 0, for its commitments have no type term), or a commitment of the row is malformed, or a
 *                              commitment does not equal v' g + ty' H0 + bl_i B under bppp_rp_open_each's comparison
 *   BPPP_RP_SCAN_OWNED (1)     every commitment of the row opens
 * amounts, types, blinds (each may be NULL; [rows][nranges][4] words; HBM in the _device variant): an owned row receives v' (the scalar in [0, n):
 * a negative amount reads as n - |v|), ty' and bl; every other row receives zeros.  *nowned (host, may be NULL): the number of owned rows.
 * The rows go through in passes of bounded workspace (a R by a walk that takes the one scalar of the call as a kernel argument, one lane per row);
 * a foreign row costs that walk and two hashes.  Rows are independent: a caller with several GPUs slices them.
 * BPPP_ERR_ARG: a NULL handle or required buffer, a = 0 or a >= n, rows * nranges >= 2^31.  rows == 0 (or batch == 0) is BPPP_OK and nothing else
 * is looked at, except that the scan still judges the view secret.  The host variants upload, call the _device variant and download. */
#define BPPP_RP_SEAL_BYTES(nranges) (34 + 64 * (size_t)(nranges))
#define BPPP_RP_SEAL_OK 0u
#define BPPP_RP_SEAL_NOT_CANONICAL 1u
#define BPPP_RP_SEAL_ZERO 2u
#define BPPP_RP_SCAN_FOREIGN 0u
#define BPPP_RP_SCAN_OWNED 1u
#define BPPP_RP_SCAN_BAD_HINT 2u
#define BPPP_RP_SCAN_TAG_ONLY 3u
int bppp_rp_seal(bppp_rp *rp, size_t batch, const uint8_t *view_keys, const uint64_t *eph, const uint64_t *amounts, const uint64_t *types /* may be NULL: binary */,
                 uint8_t *seals, uint64_t *blinds, uint32_t *seal_status /* may be NULL */);
int bppp_rp_seal_device(bppp_rp *rp, size_t batch, const void *d_view_keys, const void *d_eph, const void *d_amounts, const void *d_types, void *d_seals,
                        void *d_blinds, uint32_t *seal_status /* host, [batch], may be NULL */);
int bppp_rp_scan(bppp_rp *rp, const uint64_t view_secret[4], size_t rows, const uint8_t *coms_files, const uint8_t *seals, uint32_t *scan_status,
                 uint64_t *amounts /* may be NULL */, uint64_t *types /* may be NULL */, uint64_t *blinds /* may be NULL */, size_t *nowned /* may be NULL */);
int bppp_rp_scan_device(bppp_rp *rp, const uint64_t view_secret[4], size_t rows, const void *d_coms_files, const void *d_seals, uint32_t *scan_status /* host, [rows] */,
                        void *d_amounts /* may be NULL */, void *d_types /* may be NULL */, void *d_blinds /* may be NULL */, size_t *nowned /* may be NULL */);

/* ---- the scan under MANY view secrets ------------------------------------------------------------------------------------------------
 * A scanning service holds the view secrets of its K accounts and tests every new output against each of them; a wallet restoring several accounts
 * from one seed does the same.  bppp_rp_scan_keys{,_device} gives the verdicts of K scans in one pass over the output set and returns the owned
 * (key, row) pairs as a compact hit list.  Wire formats, domains, hashes and status values are those above; no new bytes are defined.
 *
 * THE SPECIFICATION: for every key index k and row i, bppp_rp_scan_keys reports exactly what bppp_rp_scan with view_secrets[k] reports for row i.
 *
 * view_secrets [nkeys][4] words on the host, 1 <= nkeys <= BPPP_RP_SCAN_MAX_KEYS; coms_files and seals [rows][...] as bppp_rp_scan takes them.
 * HITS.  A hit is a pair (k, i) that bppp_rp_scan under view_secrets[k] calls BPPP_RP_SCAN_OWNED for row i.  *nhits (host, required) is the number
 * of ALL hits of the call, whatever cap is.  Hits are ordered by (row, key) ascending, and the first min (*nhits, cap) of them are written:
 * hit_row[h], hit_key[h] (host, [cap]; may be NULL iff cap == 0) and the opening of row hit_row[h] under key hit_key[h] at slot h of amounts, types
 * and blinds (each may be NULL; [cap][nranges][4] words; HBM in the _device variant) — the values bppp_rp_scan writes for that row.  Slots from
 * *nhits up to cap receive zeros.  A caller that finds *nhits > cap calls again with a larger cap: that case is BPPP_OK, not an error.  Equal
 * secrets in the list are allowed, and each is reported.
 * row_status (host, [rows], may be NULL), the first that applies: BPPP_RP_SCAN_BAD_HINT (key-independent, by the rule of bppp_rp_scan);
 * BPPP_RP_SCAN_OWNED: some key owns the row; BPPP_RP_SCAN_TAG_ONLY: some key's tag matched, but no key owns the row; BPPP_RP_SCAN_FOREIGN.
 * *ntag_only (host, may be NULL): the number of pairs (k, i) that bppp_rp_scan would call BPPP_RP_SCAN_TAG_ONLY (about nkeys * rows / 256 occur
 * by chance); they are counted, never listed.
 * BPPP_ERR_ARG: a NULL handle or required buffer, nkeys == 0, nkeys > BPPP_RP_SCAN_MAX_KEYS, a secret that is 0 or >= n (bppp_last_error names the
 * lowest such index: "rp_scan_keys: key N: ..."), rows * nranges >= 2^31.  With rows == 0 the call still judges the secrets and then returns BPPP_OK
 * with *nhits = 0.  The host variant uploads, calls the _device variant and downloads.
 * The rows go through in passes and the keys in tiles within a pass (rows outer, keys inner), so a pass's seals are lifted once for all keys; one
 * launch walks a tile's keys over every row of the pass, one inversion a row serves the tile, and no buffer is sized by the 1 / 256 expectation:
 * a job whose every pair is owned is answered like any other.  The recoded secrets are wiped, on the host and in HBM, before the call returns;
 * there is no side-channel hardening, as everywhere in this library.  Rows and keys are independent: a caller with several GPUs slices either. */
#define BPPP_RP_SCAN_MAX_KEYS ((size_t)1 << 20)
int bppp_rp_scan_keys(bppp_rp *rp, size_t nkeys, const uint64_t *view_secrets /* host, [nkeys][4] */, size_t rows, const uint8_t *coms_files, const uint8_t *seals,
                      uint32_t *row_status /* host, [rows], may be NULL */, size_t cap, uint32_t *hit_key, uint32_t *hit_row /* host, [cap]; may be NULL iff cap == 0 */,
                      uint64_t *amounts, uint64_t *types, uint64_t *blinds /* each may be NULL; [cap][nranges][4] words */, size_t *nhits /* required */,
                      uint64_t *ntag_only /* may be NULL */);
int bppp_rp_scan_keys_device(bppp_rp *rp, size_t nkeys, const uint64_t *view_secrets /* host, [nkeys][4] */, size_t rows, const void *d_coms_files, const void *d_seals,
                             uint32_t *row_status /* host, [rows], may be NULL */, size_t cap, uint32_t *hit_key, uint32_t *hit_row /* host, [cap] */,
                             void *d_amounts, void *d_types, void *d_blinds /* HBM, each may be NULL; [cap][nranges][4] words */, size_t *nhits /* host, required */,
                             uint64_t *ntag_only /* host, may be NULL */);

/* ---- cut-through: the transactions of a block merged into its one sum -----------------------------------------------------------------------------
 * The block calls above (bppp_rp_excess_sums_*, bppp_rp_verify_block*, bppp_rp_excess_halfagg*) take a block "after cut-through".  This is the step:
 * a miner, a mempool or an aggregator holds T transactions as they arrived, and an output that one of them creates and another spends need not reach
 * the chain.  bppp_rp_cut_through turns the job of the T transactions into the pool, the one sum and the claim of the block.
 *
 * INPUT: the tally's job exactly as bppp_rp_excess_sums_each takes it, one sum per transaction — POOL (rows, coms_files [rows][coms_bytes]), SUMS
 * (nsums, sum_start [nsums + 1], entries [nnz] with bit 31 = subtracted = an input, nnz) and the claims claim_amounts, claim_types, claim_offsets
 * [nsums][4] (all three may be NULL; a binary handle's types do not count).  Keys, messages, signatures, proofs, bindings and seals are not inputs: a
 * block's keys are the transactions' keys, concatenated, in one group (key_start = {0, nkeys}), and whatever belongs to a row is gathered by the caller
 * with row_map.
 *
 * IDENTITY.  Entry e references the commitment with flat index j = r * nranges + i.  The identity of that commitment is 33 bytes: put (x mod p) of
 * commitment i of row r, and bit i of the row's sign bytes.  Two entries reference the same commitment iff these 33 bytes are equal.  So a
 * non-canonical x matches its reduction (x and x + p); unused bits of the sign bytes take no part; two different rows of equal content match (the
 * normal case: transaction 2 brings its own copy of the output it spends); and one flat index used with both signs matches itself.  No square root is
 * taken and nothing is judged for lying on the curve: what survives is judged by the block calls, and what is cut adds and subtracts the same term.
 *
 * WHAT IS CUT.  For every identity let P be its added entries and M its subtracted entries, both in job order (position in `entries`), and
 * m = min (|P|, |M|).  The first m of P and the first m of M are cut; every other entry survives.  This is a multiset rule over the whole job: an
 * output added and subtracted inside one transaction is cut, and the order of the transactions does not matter to the sum — whether a spend may
 * come before its output is the caller's rule.
 *
 * OUTPUTS.
 *   entry_status [nnz] (host, may be NULL)  BPPP_RP_CUT_KEPT (0); BPPP_RP_CUT_SPENT (1): the entry is cut; BPPP_RP_CUT_KEPT_AGAIN (2): it survives and
 *                an EARLIER surviving entry has the same identity — necessarily with the same sign, so 2 marks a duplicate output or a double spend
 *                inside the set.  Both are reported, never refused: the caller's rule, as for duplicate keys above.
 *   row_map [rows] (host, may be NULL)  row_map[k] is the old index of new row k.  A row survives iff a surviving entry references one of its
 *                commitments.  The surviving rows come in two groups, each in ascending old index: first the rows referenced by at least one surviving
 *                ADDED entry — the block's new outputs, the rows [0, nproofs) that bppp_rp_verify_block wants in front —, then the other survivors.
 *   new_coms_files [rows][coms_bytes] (may be NULL; HBM in the _device variant)  the surviving rows, copied byte for byte: the first new_rows rows
 *                are written.  A row of several ranges that is only partly spent stays whole: its proof still speaks for the rest.
 *   new_entries [nnz] (required; HBM in the _device variant)  the surviving entries in job order, in the first new_nnz slots: the sign kept, the
 *                index re-based to the new pool.  The block's sum_start is {0, new_nnz}.
 *   block_claims [3][4] (host; NULL iff the three claim arrays are NULL)  the sums mod n of the amounts, the types and the offsets, in this order
 *                (zeros for the types of a binary handle).  The amount is written as bppp_rp_tally_claims writes it: a below 2^255, else a - n in
 *                two's complement.  A type or an offset >= n is BPPP_ERR_ARG naming the lowest such sum.
 *   counts (host, required)  new_rows, out_rows (the first group), new_nnz, ncut (entries cut, twice the pairs), nagain (entries with status 2).
 * The call is deterministic: the same job gives the same bytes in every output, on every run.
 *
 * HOW.  The job is matched in ONE pass — matching is global and cannot be chunked as the tally chunks its sums.  Entries meet through a hash table of
 * at least 2 nnz 32-bit slots.  The hash only routes: whether two identities are equal is decided by comparing all 33 bytes.  The hash (SipHash-2-4) is
 * keyed with 16 fresh random bytes per call, so the author of a block cannot steer entries into one chain, and no output depends on the key.  Entries
 * of one identity cost one comparison each, however many they are.  Job order within an identity comes from a stable counting sort of the positions,
 * not from the order in which lanes arrive.  The workspace is the handle's, O (nnz + rows): at most 112 bytes an entry and 28 bytes a row.
 *
 * Errors and empties are the tally's: the BPPP_ERR_ARG cases and texts of bppp_rp_tally_each under the name rp_cut_through (NULL buffers with a
 * non-empty job — new_entries and counts are required, block_claims must be given exactly when the claims are; rows * nranges, nnz or nsums >= 2^31;
 * "sum_start[i] = ..."; "entries[i]: index ..."; only some of the claim arrays NULL).  The CSR arrays are validated by a kernel whose verdict is read
 * back before anything reads through them, and no output is written on an error.  nsums == 0 or nnz == 0 is BPPP_OK with all counts zero (and a
 * zeroed block_claims where one is given); nothing else is looked at.  Workspace that cannot be allocated is BPPP_ERR_HIP.  The host variant uploads,
 * calls the _device variant and downloads; d_* buffers are in HBM, 16-byte aligned. */
#define BPPP_RP_CUT_KEPT 0u
#define BPPP_RP_CUT_SPENT 1u
#define BPPP_RP_CUT_KEPT_AGAIN 2u
typedef struct bppp_rp_cut_counts {
  size_t new_rows, out_rows, new_nnz, ncut, nagain;
} bppp_rp_cut_counts;
int bppp_rp_cut_through(bppp_rp *rp, size_t rows, const uint8_t *coms_files, size_t nsums, const uint32_t *sum_start, const uint32_t *entries, size_t nnz,
                        const uint64_t *claim_amounts, const uint64_t *claim_types, const uint64_t *claim_offsets, uint32_t *entry_status /* may be NULL */,
                        uint32_t *row_map /* may be NULL */, uint8_t *new_coms_files /* may be NULL */, uint32_t *new_entries, uint64_t *block_claims,
                        bppp_rp_cut_counts *counts);
int bppp_rp_cut_through_device(bppp_rp *rp, size_t rows, const void *d_coms_files, size_t nsums, const void *d_sum_start, const void *d_entries, size_t nnz,
                               const void *d_claim_amounts, const void *d_claim_types, const void *d_claim_offsets, uint32_t *entry_status /* host, [nnz], may be NULL */,
                               uint32_t *row_map /* host, [rows], may be NULL */, void *d_new_coms_files /* HBM, may be NULL */, void *d_new_entries /* HBM, [nnz] */,
                               uint64_t *block_claims /* host, [3][4] */, bppp_rp_cut_counts *counts /* host, required */);

/* ---- set commitments: an append-only Merkle mountain range, its root and membership paths ----------------------------------------------------------
 * What a block header commits to: "the output set after this block" or "the kernels of this block" as 32 bytes, a proof that a row is in that set,
 * and the check of such proofs by someone who holds the 32 bytes alone.  Rows are opaque byte strings of one length per set, row_bytes in
 * 1 .. BPPP_RP_SET_MAX_ROW_BYTES: a commitments file of any setup, a 33-byte key, a seal.  H = SHA-256.  The four domains are
 * D* = SHA-256 (label || the handle's oracle_tag) for the labels "bppp/set/leaf/v1" (Dl), "bppp/set/node/v1" (Dn), "bppp/set/bag/v1" (Db) and
 * "bppp/set/root/v1" (Dr): sets of handles with different tags have unrelated roots.
 *
 *   leaf_i       = H (Dl || row_i)
 *   node (0, j)  = leaf_j;  node (k, j) = H (Dn || node (k - 1, 2j) || node (k - 1, 2j + 1)), 96 bytes; it covers the leaves [j 2^k, (j + 1) 2^k) and
 *                  exists once (j + 1) 2^k <= n
 *   PEAKS of n rows: for every set bit k of n, from the highest down, P = node (k, (n with its bits <= k cleared) >> k): P_0 .. P_{m-1}, m = popcount (n)
 *   BAG          acc = P_{m-1};  for i = m - 2 .. 0: acc = H (Db || P_i || acc);  32 zero bytes for n = 0
 *   ROOT         = H (Dr || le64 (n) || le32 (row_bytes) || acc), 76 bytes
 *   PATH of leaf i among n >= 1 rows: exactly bit_length (n) hashes of 32 bytes (bppp_rp_set_path_bytes), in this order:
 *                  1. the h siblings of the leaf inside its peak P_p of height h, bottom-up (sibling s is node (s, (i >> s) ^ 1));
 *                  2. if p < m - 1, the bag of P_{p+1} .. P_{m-1} as ONE hash;
 *                  3. P_{p-1}, .., P_0, the nearest first;
 *                  4. zero bytes up to the length (h + p + 1 <= bit_length (n) always).
 *                The verifier hashes upwards: the leaf with its siblings (the path's hash on the left where bit s of i is set), then
 *                acc = H (Db || acc || the right bag), then acc = H (Db || P || acc) for each peak to the left, then the root's message.
 * None of this depends on how the rows were split into appends.
 *
 * THE SET is the device-resident thing; every buffer below is on the host.
 * bppp_rp_set_create: an empty set on rp's context.  keep_nodes = 1 stores every node in HBM — one grow-only array per level, 32 bytes a node, 64 bytes
 *   a row in the limit (an array that must grow at least doubles, so up to twice that is allocated; while an append grows the arrays the old ones
 *   stay alive beside the new ones, transiently up to three times that) — and can serve paths; n < 2^31 rows, subject to HBM.  keep_nodes = 0 stores the peaks alone (2 KB) and can append, give its root and its peaks; n < 2^63.  The set uses rp's workspace for
 *   scratch and its tag for the domains, so it is destroyed BEFORE rp, and like rp it serves one call at a time.
 * bppp_rp_set_restore: a frontier-only set of n rows that continues from exported state, peaks [popcount (n)][32] as bppp_rp_set_peaks wrote them
 *   (may be NULL iff n = 0).  The peaks are taken as they are: a caller who restores checks the root against one it trusts.
 * bppp_rp_set_append: rows [nrows][row_bytes] behind the rows there are.  nrows = 0 is BPPP_OK and touches nothing; nrows < 2^31 a call.  A refused
 *   call (BPPP_ERR_ARG, or workspace or level arrays that cannot be allocated, BPPP_ERR_HIP) leaves the set as it was: the arrays grow all or
 *   nothing, and the set can be used and appended to afterwards.  One launch hashes the leaves (one lane a
 *   row, ceil ((32 + row_bytes + 9) / 64) compressions), then one launch per EIGHT levels that have a new node builds the nodes above them through
 *   LDS, whichever n the append starts from: at most 1 + ceil (bit_length (n + nrows) / 8) launches, one more on a frontier-only set.
 * bppp_rp_set_info: rows, row_bytes, popcount (n) and the bytes of HBM the store (or the frontier) holds; any out pointer may be NULL.
 * bppp_rp_set_root: the 32 bytes of the root of the rows there are.  bppp_rp_set_peaks: peaks [popcount (n)][32], P_0 first; nothing for n = 0.
 * bppp_rp_set_path_bytes: 32 bit_length (n); host only, no handle.
 * bppp_rp_set_paths: paths [nq][bppp_rp_set_path_bytes (n)] of the leaves idx [nq], against the set's current n.  BPPP_ERR_ARG on a frontier-only
 *   set, and for any idx >= n: bppp_last_error names the first such index and nothing is written.  nq < 2^31.
 * bppp_rp_set_verify_paths: stateless — what a light client or a validator holding only a header runs.  Query q: is rows [q][row_bytes] leaf
 *   idx [q] of the set of n rows with this root, by paths [q][bppp_rp_set_path_bytes (n)]?  status [nq] (may be NULL), the first that applies:
 *     BPPP_RP_SET_BAD_INDEX (2)    idx >= n
 *     BPPP_RP_SET_BAD_PADDING (3)  a non-zero byte behind the hashes the path uses
 *     BPPP_RP_SET_MISMATCH (1)     the root computed from the row and the path differs
 *     BPPP_RP_SET_OK (0)
 *   *accept = 1 iff every query is OK (nq = 0: 1).  One lane a query, about 2 bit_length (n) compressions and the leaf's.  n < 2^63, nq < 2^31.
 * Errors: BPPP_ERR_ARG for a NULL handle, set or required buffer, a closed context, row_bytes outside 1 .. 8192 ("row_bytes = .. is outside"),
 * keep_nodes other than 0 or 1, a size at or above its limit ("a full store holds fewer than 2^31", "a set holds fewer than 2^63", "is 2^31 or more").
 * bppp_last_error of the handle's context gives the text. */
#define BPPP_RP_SET_OK 0u
#define BPPP_RP_SET_MISMATCH 1u
#define BPPP_RP_SET_BAD_INDEX 2u
#define BPPP_RP_SET_BAD_PADDING 3u
#define BPPP_RP_SET_MAX_ROW_BYTES 8192
typedef struct bppp_rp_set bppp_rp_set;
int bppp_rp_set_create(bppp_rp *rp, size_t row_bytes, int keep_nodes, bppp_rp_set **set);
int bppp_rp_set_restore(bppp_rp *rp, size_t row_bytes, uint64_t n, const uint8_t *peaks /* [popcount (n)][32] */, bppp_rp_set **set);
void bppp_rp_set_destroy(bppp_rp_set *set);
int bppp_rp_set_append(bppp_rp_set *set, size_t nrows, const uint8_t *rows /* [nrows][row_bytes] */);
int bppp_rp_set_info(const bppp_rp_set *set, uint64_t *n, size_t *row_bytes, size_t *npeaks, size_t *store_bytes);
int bppp_rp_set_root(bppp_rp_set *set, uint8_t root[32]);
int bppp_rp_set_peaks(bppp_rp_set *set, uint8_t *peaks /* [popcount (n)][32] */);
size_t bppp_rp_set_path_bytes(uint64_t n);
int bppp_rp_set_paths(bppp_rp_set *set, size_t nq, const uint64_t *idx /* [nq] */, uint8_t *paths /* [nq][32 bit_length (n)] */);
int bppp_rp_set_verify_paths(bppp_rp *rp, size_t row_bytes, uint64_t n, const uint8_t root[32], size_t nq, const uint64_t *idx, const uint8_t *rows, const uint8_t *paths,
                             uint32_t *status /* [nq], may be NULL */, int *accept);

/* ---- one comb table for the handles of a basis family --------------------------------------------------------------------------
 * Every setup's basis [g | H | G] is a prefix of the point stream its points came from (see bppp_rp_verify_mixed), and the comb table
 * is laid out tab[window][point][multiple]: the table of the longest basis of a stream contains the table of every shorter one (same
 * entries, the longer table's stride).  A service that proves several shapes over one stream therefore needs ONE table, not one of
 * tens of GB per handle.
 * bppp_rp_share_comb: rp proves over donor's comb table from now on.  Both handles on the same context; donor's basis (points 1.. of
 * its creation's points_xy) must extend rp's point by point — the comparison bppp_rp_verify_mixed uses for its families — else
 * BPPP_ERR_ARG.  If donor has no table yet it is built now, under donor's COMB_BUDGET / COMB_BITS options, as donor's own prover would
 * build it (BPPP_ERR_ARG if donor's table is switched off, BPPP_ERR_HIP if it cannot be built; rp is then unchanged).  A table rp held
 * before is released.  The table lives until the last handle using it is destroyed, in any order.  rp == donor is a no-op that only
 * forces the build.  The files rp proves are the same bytes as over a table of its own, on every route; the window may be narrower
 * than rp's own table would have had (the budget is spent on the longer basis).  rp's verify_each uses the table as it uses its own.
 * bppp_rp_comb_info: window bits, bytes and number of registered points of the table this handle proves over, and how many handles
 * (twins not counted) use it; all zero when it has none.  Any out pointer may be NULL. */
int bppp_rp_share_comb(bppp_rp *rp, bppp_rp *donor);
int bppp_rp_comb_info(const bppp_rp *rp, int *window_bits, size_t *table_bytes, size_t *table_points, size_t *users);

/* Proving a job of SEVERAL setups in one call: group s is bppp_rp_prove_batch_pub (rp_s, batch_s, ...) — its files are byte-identical
 * to that call's — with the handles grouped into families as bppp_rp_verify_mixed groups them.  A family whose proofs in this job,
 * together with what its handles proved before, reach the smallest COMB_MIN among its handles gets ONE table, built over the longest
 * basis among the family's handles given here under that handle's COMB_BUDGET / COMB_BITS; all its handles share it afterwards, as
 * after bppp_rp_share_comb.  A family that already has tables keeps the longest one that covers its longest basis.  A handle with the
 * table switched off (COMB_BUDGET 0) stays without.  Families below the threshold (and those whose table cannot be built) prove as
 * bppp_rp_prove_batch_pub does.  The input commitments of all groups of a family with a table are one launch over its first three
 * points; the groups then run in the order given, each as its handle's prover runs it (a large group still splits in two halves).
 * BPPP_ERR_ARG: handles on different contexts, one handle in two groups, a null buffer in a non-empty group, every argument error of
 * bppp_rp_prove_batch_pub (the message names the group and the proof).  Empty groups take no part; an empty job returns BPPP_OK.  On
 * an error nothing is guaranteed about ANY group's output buffers (earlier groups may be complete, later ones untouched). */
typedef struct bppp_rp_prove_group {
  bppp_rp *rp;
  size_t batch;                               /* proofs in this group (0 allowed) */
  const uint64_t *amounts, *types, *blinds;   /* as bppp_rp_prove_batch: [batch][nranges][4] */
  const uint64_t *public_amounts;             /* as bppp_rp_prove_batch_pub, may be NULL */
  const uint8_t *rand_prefix;
  size_t prefix_len;
  uint8_t *coms_files, *proof_files;          /* out: the reference's files, [batch][coms_bytes], [batch][proof_bytes] of rp */
} bppp_rp_prove_group;
int bppp_rp_prove_mixed(const bppp_rp_prove_group *groups, size_t ngroups);

/* ---- harness utility: pointX of getPoints (app/Main.hs:68-72) -------------------------------
 * For each candidate x (n x 4 uint64 in HBM) writes the affine point (x, y) with y the EVEN root of
 * x^3 + 7, or the infinity encoding when x^3 + 7 is a non-residue or x >= p.  (Which root
 * galois-field's `sr` returns cannot be confirmed offline — SURVEY.md 8c; even-y is this build's
 * documented choice.)  An x >= p is NOT reduced: it is "not a point" here, while the decoder of proof and
 * commitments files (Binary (Prime p), src/Encoding.hs:76-80) and the seed stream below reduce mod p first.
 * Used to make synthetic bases on the GPU. */
int bppp_lift_x_device(bppp_ctx *ctx, const void *d_x, size_t n, void *d_points_xy);

/* ---- a setup's basis from its seed: getPoints (app/Main.hs:68-72), the stream h : g : hs ++ gs the CLI hands to setup (:260) -------
 * Candidate n of `seed` is x = decode (SHA-256 (seed <> decimal ASCII of n)) mod p, decode = Binary (Prime p) (src/Encoding.hs:75-79:
 * four big-endian 64-bit words, least significant first); it is a point iff x^3 + 7 is a square, with the EVEN root as y (the choice
 * of bppp_lift_x_device).  The stream is the accepted candidates in increasing n, so every basis of one seed is a prefix of every
 * longer one — what bppp_rp_share_comb and the basis merging of bppp_rp_verify_mixed compare.  The work runs on the GPU in ordered
 * passes (csrc/seedpoints.hip.h: one lane per candidate, ballot / LDS / one scan for the slots, no atomics): the same call writes the
 * same bytes every time.
 *
 * bppp_seed_candidate_x: host only, no context, no GPU: x of candidate n (before the curve test).
 * bppp_points_from_seed{,_device}: `count` consecutive points of the stream, the search starting at candidate `first_candidate`;
 * *next_candidate (may be NULL) = the index after the last accepted candidate, so a later call with it continues the same stream.
 * points_xy: [count][8] words on the host; _device: the same in HBM, ready for bppp_basis_create_device.
 * `seed` may be NULL iff seed_len == 0; seed_len <= 4096.  count == 0 returns BPPP_OK, writes nothing and sets *next_candidate =
 * first_candidate.  BPPP_ERR_ARG: a seed outside those rules, a NULL output with count > 0, a closed context, or a search that would
 * run past the last candidate (the stream ends with candidate 2^64 - 2, so that *next_candidate always names a candidate; nothing is
 * promised about the output then). */
int bppp_seed_candidate_x(const uint8_t *seed, size_t seed_len, uint64_t n, uint64_t out_x[4]);
int bppp_points_from_seed_device(bppp_ctx *ctx, const uint8_t *seed, size_t seed_len, uint64_t first_candidate, size_t count, void *d_points_xy,
                                 uint64_t *next_candidate);
int bppp_points_from_seed(bppp_ctx *ctx, const uint8_t *seed, size_t seed_len, uint64_t first_candidate, size_t count, uint64_t *points_xy,
                          uint64_t *next_candidate);

/* ---- device memory helpers (so a non-HIP host language can keep vectors resident) ---------- */
int bppp_device_alloc(bppp_ctx *ctx, size_t bytes, void **d_ptr);
int bppp_device_free(bppp_ctx *ctx, void *d_ptr);
int bppp_upload(bppp_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int bppp_download(bppp_ctx *ctx, void *dst, const void *d_src, size_t bytes);
/* Page-locked host memory for the buffers a caller hands to the host-buffer entry points (bppp_msm, bppp_rp_verify_batch,
 * bppp_rp_prove_batch, bppp_upload ...): from such a buffer the copies to the device are DMA transfers that run beside the kernels;
 * from ordinary (pageable) memory every copy first passes through a staging buffer at the host's memcpy rate.  Optional: every entry
 * point takes either kind (a Haskell binding would wrap these in a ForeignPtr with bppp_host_free as its finalizer). */
int bppp_host_alloc(bppp_ctx *ctx, size_t bytes, void **ptr);
int bppp_host_free(bppp_ctx *ctx, void *ptr);

/* ---- measurement hooks ---------------------------------------------------------------------
 * When enabled, each MSM call brackets its stages with hipEvents on the context's stream; the
 * accumulated per-stage milliseconds and launch counts can be read back (bench.py's roofline). */
#define BPPP_STAGE_DIGITS 0      /* k_digits */
#define BPPP_STAGE_SORT 1        /* k_hist .. k_scatter + bucket memset */
#define BPPP_STAGE_ACC_POINTS 2  /* k_acc_points alone: the dominant kernel (roofline) */
#define BPPP_STAGE_ACC_RECORDS 3 /* k_merge + k_merge_heavy (buckets that straddle lanes) */
#define BPPP_STAGE_REDUCE 4      /* k_reduce1 + k_reduce2 */
#define BPPP_STAGE_FINISH 5      /* window combine + copy-out */
#define BPPP_NUM_STAGES 6
int bppp_profile_enable(bppp_ctx *ctx, int on);
int bppp_profile_read(bppp_ctx *ctx, double ms[BPPP_NUM_STAGES], uint64_t *calls, int reset);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BPPP_H */
