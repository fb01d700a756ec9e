/*
 * bppp_test.h — test-only hooks exported by libbppp_hip_test.so (a separate library; the product library does not contain them) so the parity tests can exercise the
 * device field and group arithmetic directly (the device counterparts of mulField# / addField# /
 * invField#, src/Data/Field/Galois/FastPrime/Internal.hs:909-988, and of nrmlAdd / dbl',
 * src/Commitment.hs:111-144).  Not part of the drop-in boundary.
 */
#ifndef BPPP_TEST_H
#define BPPP_TEST_H
#include "bppp.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)
#define BPPP_FE_ADD 0
#define BPPP_FE_SUB 1
#define BPPP_FE_MUL 2
#define BPPP_FE_SQR 3
#define BPPP_FE_INV 4
#define BPPP_FE_NEG 5
/* out[i] = a[i] (op) b[i] in Fq (modulus = 0: production 10x26 limbs; 2: the 8x32 code path) or Fr (modulus = 1: 8x32; 3: production
 * 10x26 limbs of csrc/fr26.hip.h, whose ops 6 and 10-14 drive the lazy limbs to their magnitude bounds); host arrays of n x 4 uint64 */
int bppp_test_fe_op(bppp_ctx *ctx, int op, int modulus, const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out);
/* out[i] = p[i] + q[i] (complete group law; op 0: mixed XYZZ+affine, op 1: XYZZ+XYZZ, op 2: 2*p[i]);
 * host arrays of n x 8 uint64 affine points */
int bppp_test_point_op(bppp_ctx *ctx, int op, const uint64_t *p, const uint64_t *q, size_t n, uint64_t *out);
/* The quad forms of csrc/ec_quad.hip.h (four lanes share one point operation) against the one-lane forms, one quad per element:
 * op 0: p[i] + q[i] (xyzz_add_quad vs xyzz_add), op 2: 2 * p[i] (xyzz_dbl_quad vs xyzz_dbl); op 1 / 3: the same with the XYZZ inputs
 * pushed to the magnitude bounds (X <= 5, Y <= 3); op 4 .. 7: ops 0 .. 3 with the quad forms on fq_mul_lone (csrc/fq26.hip.h), as the
 * bucket reduction's tail runs them.  Inputs are affine, taken to XYZZ with ZZ != 1.  out: n x 8 uint64 affine results
 * of the quad form; raw: n x 81 uint32, the quad form's 40 raw limbs (X, Y, ZZ, ZZZ), the scalar form's 40, and 1 iff all four
 * lanes of the quad held the same limbs. */
int bppp_test_point_quad(bppp_ctx *ctx, int op, const uint64_t *p, const uint64_t *q, size_t n, uint64_t *out, uint32_t *raw);
/* The pair forms of csrc/fq26.hip.h against the one-product forms on caller-built RAW limbs (n x 10 uint32 each, any magnitude <= 8):
 * kind 0: fq_mul2 (a b, c d), 1: fq_mul_sqr (a b, c^2; d is read but unused), 2: fq_sqr2 (a^2, c^2; b and d unused).  raw: n x 40 uint32, the pair
 * form's two results, then fq_mul's / fq_sqr's for the same operands. */
int bppp_test_fq_pair(bppp_ctx *ctx, int kind, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, size_t n, uint32_t *raw);
/* xyzz_add_chain / xyzz_dbl_chain (csrc/ec.hip.h) against xyzz_add / xyzz_dbl, one lane per element.  op bit 0: the left operand is
 * 3 p[i], built as a sum of three points so that ZZ != 1 (else p[i] with ZZ = 1); bit 1: the right operand is 3 q[i] likewise; bit 2:
 * double the left operand instead of adding.  out: n x 8 uint64 affine results of the chain form; raw: n x 80 uint32, the chain form's 40
 * raw limbs (X, Y, ZZ, ZZZ), then the plain form's 40. */
int bppp_test_point_chain(bppp_ctx *ctx, int op, const uint64_t *p, const uint64_t *q, size_t n, uint64_t *out, uint32_t *raw);
/* Measured ceiling of the field layer: modular multiplications per second of a kernel that does nothing but independent
 * Fq multiplications (10x26-bit limbs) at 8 wavefronts per SIMD.  bench.py quotes the MSM's multiplication rate against it. */
int bppp_test_mulmod_rate(bppp_ctx *ctx, int iters, double *mulmods_per_sec);
/* Terms of the one MSM the last bppp_rp_verify_mixed* call on this context ran (0 after an empty job): a test sees that the shared
 * bases of setups from one point stream were merged. */
int bppp_test_last_mixed_msm_terms(bppp_ctx *ctx, uint64_t *terms);
/* The scatter the last MSM of the general pipeline on this context launched: 0 = k_scatter, 2 or 4 = k_scatter_ranges with that many
 * bucket ranges per window (BPPP_SORT_RANGES; one MSM over arbitrary points with 16-bit windows only), -1 = none yet. */
int bppp_test_last_sort_ranges(bppp_ctx *ctx, int *q);
/* 1 = the ranged scatter of the last MSM of the general pipeline on this context read every chunk's digits once (k_scatter_one_read: no
 * chunk longer than the steps a lane holds in registers, and BPPP_SCATTER_ONE_READ not 0), 0 = k_scatter_ranges or k_scatter, -1 = none yet. */
int bppp_test_last_scatter_one_read(bppp_ctx *ctx, int *one_read);
/* 1 = the sort of the last MSM of the general pipeline on this context kept its per-chunk counts and prefixes as 16-bit values (a ranged
 * scatter, no chunk longer than 65535 terms, and BPPP_HIST16 not 0), 0 = as 32-bit words, -1 = none yet. */
int bppp_test_last_hist16(bppp_ctx *ctx, int *hist16);
/* How the last MSM of the general pipeline on this context accumulated its buckets: 1 = whole buckets in order of size (k_order,
 * k_acc_points_sized; BPPP_ACC_SIZED, one MSM over arbitrary points only), 0 = slices of the sorted entries (k_acc_points, k_merge),
 * -1 = none yet. */
int bppp_test_last_acc_sized(bppp_ctx *ctx, int *sized);
/* 1 = the last MSM of the general pipeline on this context accumulated on 9 x 29-bit limbs (k_acc_points_sized29; BPPP_ACC_FQ29 on a sized
 * plan), 0 = on 10 x 26, -1 = none yet. */
int bppp_test_last_acc_fq29(bppp_ctx *ctx, int *fq29);
/* csrc/fq29.hip.h on caller-built RAW limbs (n x 9 uint32 each, within the magnitude contract of the operation): op 0: a b (magnitudes with
 * product <= 7), 1: a^2 (<= 2), 2: weak_pass(sub<3>(a, b)) (a, b <= 3), 3: fq29_from_fe of the canonical 8 x 32-bit value in the first 8 words
 * of a.  raw: n x 19 uint32, the 9 limbs of the result and the 10 limbs of fq29_to_fq26(result); out: n x 8 uint32, that value canonical. */
int bppp_test_fq29_op(bppp_ctx *ctx, int op, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *raw, uint32_t *out);
/* n chains of k mixed additions (csrc/ec29.hip.h), one lane each, walked as k_acc_points_sized29 walks an item: the first point is loaded into
 * the accumulator, the others are added with xyzz29_madd.  points: n x k x 8 uint64 affine ((0, 0) = infinity), flags: n x k uint32, not 0
 * negates the point first.  out: n x 8 uint64 canonical affine sums; raw: n x 40 uint32, the sums as the kernel stores them. */
int bppp_test_madd29_chain(bppp_ctx *ctx, const uint64_t *points, const uint32_t *flags, size_t k, size_t n, uint64_t *out, uint32_t *raw);
/* fq29_mul_add2 (csrc/fq29.hip.h), xyzz29_madd_fast and xyzz29_from_two (csrc/ec29.hip.h), the routines of k_acc_points_sized29_fast, on caller-built RAW limbs
 * (uint32, 9 per field element, within each routine's magnitudes).  op 0: fq29_mul_add2(a, b, c, d), in: n x 4 elements, raw: n x 36 with the
 * result in the first 9 words;  op 1: xyzz29_madd_fast(acc, q), in: n x 6 elements X Y ZZ ZZZ x y, raw: n x 36, the limbs of X Y ZZ ZZZ;
 * op 2: xyzz29_from_two((x1, y1), (x2, y2)), in: n x 4 elements, raw as op 1. */
int bppp_test_ec29_fast_op(bppp_ctx *ctx, int op, const uint32_t *in, size_t n, uint32_t *raw);
/* The same chains over 10 x 26-bit limbs (csrc/ec.hip.h: xyzz_from_aff, aff_cneg, xyzz_madd), as k_acc_points_sized walks an item and k_acc_points a
 * run; arguments and outputs as bppp_test_madd29_chain (raw: the accumulator as stored, lazily reduced). */
int bppp_test_madd26_chain(bppp_ctx *ctx, const uint64_t *points, const uint32_t *flags, size_t k, size_t n, uint64_t *out, uint32_t *raw);
/* The stages of the LAST general-pipeline MSM on this context (any entry point that reaches msm_run_ex past the small route), read back from the
 * context's workspace, which is carved again from the plan the call stored: call these directly after the MSM, before anything else runs on the
 * context.  BPPP_ERR_ARG when no such MSM has run (or the small route ran since).
 * _layout: the plan (csrc/msm_plan.hpp) — c, W digit rows per scalar of which the first acnt are c bits wide, top (the row stored negated, -1 none),
 * M buckets per window, flat (a registered basis: one bucket set per instance), CH chunks per digit row and their length per as k_hist and the
 * scatters compute it, Q bucket ranges (0: k_scatter), one_read (k_scatter_one_read), sized / fq29 / acc_fast (the accumulation's form; acc_fast: k_acc_points_sized29_fast), L entries per lane and G
 * lanes of k_acc_points, shared_points as the call gave it; stride: uint16 per digit row; FB buckets in all; total = start[FB], the sorted entries;
 * table_stride: the rows' distance in a registered basis' table (0 otherwise).
 * _copy: one array, `bytes` must be exactly its size —
 *   DIGITS       [batch * W][stride] uint16, as stored (biased, the top row negated)
 *   NEGMASK      ceil(batch * n / 64) uint64: bit i is the sign fold of scalar i
 *   COUNT        [FB] uint32          START  [FB + 1] uint32          SORTED  [total] uint32: sign << 31 | point index
 *   BUCKETS_RAW  [FB][40] uint32, the stored XYZZ sums         BUCKETS_AFF  [FB][16] uint32: xyzz_to_aff of each, infinity as (0, 0) */
typedef struct bppp_test_msm_layout {
  int32_t c, W, acnt, top, M, flat, CH, Q, one_read, sized, fq29, L, shared_points, acc_fast;
  uint32_t stride, per;
  uint64_t batch, n, FB, G, total, table_stride;
} bppp_test_msm_layout;
enum { BPPP_TEST_MSM_DIGITS = 0, BPPP_TEST_MSM_NEGMASK = 1, BPPP_TEST_MSM_COUNT = 2, BPPP_TEST_MSM_START = 3, BPPP_TEST_MSM_SORTED = 4,
       BPPP_TEST_MSM_BUCKETS_RAW = 5, BPPP_TEST_MSM_BUCKETS_AFF = 6 };
int bppp_test_last_msm_layout(bppp_ctx *ctx, bppp_test_msm_layout *report);
int bppp_test_last_msm_copy(bppp_ctx *ctx, int what, void *out, size_t bytes);
/* The windows (digit rows per scalar) of the plan of the last MSM on this context, the small route included: 16 with 16-bit windows, where
 * the top window is stored negated instead of carrying into a 17th; 256 / c + 1 for a registered basis; -1 = none yet. */
int bppp_test_last_windows(bppp_ctx *ctx, int *windows);
/* What the last verification on this handle ran (bppp_rp_verify_batch*, _shard_device, _each*, and its group's share of
 * bppp_rp_verify_mixed*): combined MSMs (the accept check and every bisection step) and per-proof passes.  A test sees the cost of a
 * culprit search without timing it. */
int bppp_test_rp_last_verify_counts(bppp_rp *rp, uint64_t *combined_msms, uint64_t *each_passes);
/* What the last bppp_rp_verify_block* on this handle launched up to its verdict (the status passes of a rejected block are not counted): MSMs, the
 * terms of the one MSM, keys lifted (one lift per key: the signatures' stage serves the sums) and commitments square-rooted (rows * nranges: the
 * proven rows are taken from the verifier's decoder).  All zero after an empty block; a call refused with an argument error leaves them, and the
 * counts of bppp_test_rp_last_verify_counts, as they were. */
int bppp_test_rp_last_block_counts(bppp_rp *rp, uint64_t *msms, uint64_t *terms, uint64_t *key_lifts, uint64_t *coms_decoded);
/* Proofs per chunk of the per-proof pass on this handle (0 = from the row budget, the default): a test crosses a chunk boundary
 * with a small batch. */
int bppp_test_rp_set_each_chunk(bppp_rp *rp, size_t proofs);
/* The thresholds of the tally entry points on this handle, and of bppp_rp_excess_verify_*, which run the same sum stage (csrc/rptally.hip; 0
 * restores the default): the longest sum one lane walks alone
 * (default 16), the entries of one workgroup's piece of a longer sum (default 4096, at least 2: longer sums are split and their partial
 * points summed by further launches) and the entries, and sums, of one pass over the workspace (default 2^22).  A test straddles each with a
 * small job. */
int bppp_test_rp_set_tally_short_max(bppp_rp *rp, size_t entries);
int bppp_test_rp_set_tally_piece(bppp_rp *rp, size_t entries);
int bppp_test_rp_set_tally_chunk(bppp_rp *rp, size_t entries);
/* The items of one pass over the workspace in the balance calls that the tally's chunk does not plan (0 restores the default, 2^22):
 * bppp_rp_commit_batch* and bppp_rp_open_* take  max (1, items / nranges)  rows a pass, bppp_rp_excess_sign*  items  sums, bppp_rp_excess_keys* and
 * bppp_rp_excess_verify_keys_*  max (1, items / 4)  keys, bppp_rp_excess_part_*  max (1, items / 4)  sessions or parts (whole groups: a group longer
 * than that is an error).  A test takes several passes with a handful of items. */
int bppp_test_rp_set_flat_chunk(bppp_rp *rp, size_t items);
/* Cut-through on this handle (bppp_rp_cut_through*, csrc/rpcut.hip).  _force pins what a call otherwise draws or sizes itself, until it is called
 * again: mode 0 = the keyed hash, 1 = every routing hash equal, so every entry probes ONE chain of the table and every comparison of two different
 * identities is made; salt NULL = 16 fresh random bytes per call (the product's behaviour), else these 16 bytes are the key; table_bits 0 = at least
 * 2 nnz slots, else 2^table_bits slots, lifted to the smallest legal table (the power of two that holds nnz entries) where that is larger — 1 asks for
 * that smallest table.  (0, NULL, 0) restores the product's behaviour.  No output of the call may depend on any of the three.
 * _last reports what the last successful non-empty call on the handle ran: the table's slots, the groups (distinct identities among the entries)
 * and the passes of the counting sort (8 bits of 2 * groups - 1 each). */
int bppp_test_rp_cut_through_force(bppp_rp *rp, int mode, const uint8_t *salt /* NULL or [16] */, int table_bits);
int bppp_test_rp_cut_through_last(bppp_rp *rp, uint64_t *slots, uint64_t *groups, uint64_t *passes);
/* The quad walk of k_rp_excess_mulcheck alone (csrc/rpexcess.hip.h): out_i = c_i X_i in affine form, infinity as all zeros, for n instances
 * of four lanes each.  d_scalars [n][4] words (walked as the 256-bit integers they are, reduced or not), d_points_xy and d_out_xy [n][8]
 * words, all in HBM.  The real entry points derive the challenge from a hash; here a test chooses it. */
int bppp_test_rp_excess_mul(bppp_rp *rp, size_t n, const void *d_scalars, const void *d_points_xy, void *d_out_xy);
/* The joint walk of k_rp_expart_mulcheck alone (csrc/rpexpart.hip.h): out_i = b_i P_i + c_i Q_i in affine form, infinity as all zeros, for n
 * instances of four lanes each.  d_b and d_c [n][4] words (walked as the 256-bit integers they are, reduced or not), d_P_xy, d_Q_xy and d_out_xy
 * [n][8] words (infinity as all zeros), all in HBM.  P = Q, P = -Q and infinity in either place are ordinary input. */
int bppp_test_rp_excess_mul2(bppp_rp *rp, size_t n, const void *d_b, const void *d_P_xy, const void *d_c, const void *d_Q_xy, void *d_out_xy);
/* The fixed-scalar walk of bppp_rp_scan alone (csrc/rpseal.hip.h): out_i = scalar P_i in affine form, infinity as all zeros, one lane per point and
 * ONE scalar for all n of them.  scalar [4] words on the host (any 256-bit integer: reduced mod n, then split and recoded, before the launch),
 * d_points_xy and d_out_xy [n][8] words in HBM (infinity as all zeros is ordinary input). */
int bppp_test_rp_scan_mul(bppp_rp *rp, size_t n, const uint64_t scalar[4], const void *d_points_xy, void *d_out_xy);
/* The recoding that walk is driven by, on the host alone (no GPU is touched): scalar mod n = a1 + a2 lambda; out[0 .. 8] hold the two-bit digits,
 * digit i = bit i of |a1| + 2 * bit i of |a2| at bits 2 (i & 15) of word i >> 4; out[9] the number of digits, walked from the highest down;
 * out[10] the signs (bit 0: a1 < 0, bit 1: a2 < 0). */
int bppp_test_rp_scan_recode(const uint64_t scalar[4], uint32_t out[11]);
/* The multi-key walk of bppp_rp_scan_keys alone (csrc/rpscan_keys.hip.h): the per-row table, the walk of a tile of keys in one launch and the
 * batched affine conversion, without the hashes.  out[k][i] = scalars[k] P_i in affine form, infinity as all zeros.  scalars [nkeys][4] words on
 * the host (any 256-bit integers: reduced mod n, split and recoded before the launch); d_points_xy [n][8] words and d_out_xy [nkeys][n][8] words
 * in HBM (a point at infinity, all zeros, is ordinary input).  The keys go through in the tiles bppp_test_rp_scan_keys_geometry reports for
 * (rows = n, nkeys). */
int bppp_test_rp_scan_keys_mul(bppp_rp *rp, size_t nkeys, const uint64_t *scalars, size_t n, const void *d_points_xy, void *d_out_xy);
/* The recoding that walk is driven by, on the host alone: the 36 words of a key record (csrc/rpscan_keys_plan.hpp).  scalar mod n = a1 + a2 lambda,
 * each half as a width-4 signed sliding window with the half's sign folded in; position i is the byte at bits 8 (i & 3) of out[i >> 2], low nibble
 * the digit of a1, high nibble of a2; a nibble is 0 for the digit 0, else (|digit| + 1) / 2 in its low three bits and 8 for a negative digit;
 * out[33] the number of positions, walked from the highest down; out[34 .. 35] zero. */
int bppp_test_rp_scan_keys_recode(const uint64_t scalar[4], uint32_t out[36]);
/* The geometry bppp_rp_scan_keys would choose on this handle for (rows, nkeys): out[0] rows per pass, out[1] keys per tile (KT), out[2] survivors
 * per open chunk.  Host only. */
int bppp_test_rp_scan_keys_geometry(bppp_rp *rp, size_t rows, size_t nkeys, uint64_t out[3]);
/* The witness kernel of bppp_rp_prove_batch_device alone (csrc/rpwitness.hip.h): inputs in HBM as that entry point takes them
 * (d_types ignored on a binary handle, d_public_amounts NULL or CANONICAL scalars [batch][public_count][4]); its arrays copied to the
 * host: in_sc [batch][nranges][3][4] words, status [batch] (0 = a witness; the arrays of a refused proof are unspecified) and, typed:
 * dig, mul [batch][norm_len], mss [batch][lin_len - 6] as rpp_device_prove takes them; binary: dig [batch][live positions] holds the
 * bits, mul and mss are not written (may be NULL). */
int bppp_test_rp_witness_device(bppp_rp *rp, size_t batch, const void *d_amounts, const void *d_types, const void *d_blinds,
                                const void *d_public_amounts, uint64_t *in_sc, uint32_t *dig, uint32_t *mul, uint32_t *mss, uint32_t *status);
/* bppp_points_from_seed with every pass forced to `chunk` candidates (1 .. 2^20; csrc/seedpoints.hip.h): a small request crosses pass
 * and workgroup boundaries.  points_xy: host, [count][8] words. */
int bppp_test_points_from_seed_chunked(bppp_ctx *ctx, const uint8_t *seed, size_t seed_len, uint64_t first_candidate, size_t count, size_t chunk,
                                       uint64_t *points_xy, uint64_t *next_candidate);
/* The decode-and-lift step of the candidate kernel on caller-given digests ([n][32] bytes as SHA-256 writes them) — a digest that
 * decodes to p or more is out of any hash's reach: x [n][4] = decode mod p, is_point [n], points_xy [n][8] (zero where not a point). */
int bppp_test_seed_lift_digests(bppp_ctx *ctx, const uint8_t *digests, size_t n, uint64_t *x, uint32_t *is_point, uint64_t *points_xy);
/* The decode stage of the verifier alone (csrc/rpdecode.hip.h: k_rp_decode_points + k_rp_decode_scalars through rp_decode_launch, the launch
 * bppp_rp_verify_batch* makes per upload slice) on `batch` host files of the handle's coms_bytes / proof_bytes each — any bytes of
 * that length, they need not be proofs.  Everything it wrote, copied to the host (k = rounds, nrp = 4 range-proof commitments, 2 on a
 * binary handle; points as 8 words x | y, all zero = "not a point"; scalars as 4 words, canonical):
 *   resp_pts [batch][2k][8]          resp[b][t] = point nrp + t of proof file b (the argument's responses, last round first)
 *   init_pts [batch][nrp + nranges][8]   init[b] = the nrp range-proof commitments (points 0 .. nrp-1 of proof file b), then the nranges
 *                                    input commitments (commitments file b)
 *   wit_norm [batch][final_norm][4], wit_lin [batch][final_lin][4]   the proof file's scalars, norm part then linear part
 *   bad [batch]                      non-zero iff some x of proof b is not on the curve;  any_bad [1]: their OR
 * bad and any_bad are zeroed before the launch as the verifier does; the point and scalar arrays are pre-filled with 0xA5 bytes, so a
 * slot the kernels did not write shows. */
int bppp_test_rp_decode_device(bppp_rp *rp, size_t batch, const uint8_t *coms, const uint8_t *proofs, uint64_t *init_pts, uint64_t *resp_pts, uint64_t *wit_norm,
                               uint64_t *wit_lin, uint32_t *bad, uint32_t *any_bad);
/* The fixed-base comb (csrc/comb.hip.h) on a table of the test's own, so that every route of its launchers runs at small shapes.
 * bppp_test_comb_create: the table of T affine points in HBM ([T][8] words, all zero = infinity) at window_bits in [4, 18], as the product's
 * comb_create builds it; it borrows ctx (destroy the table first).  The tuning is the context's (BPPP_COMB_ROWS_MIN_MB, BPPP_COMB_ROWS_WAVES
 * when the context was created).  d_scalars: canonical scalars in HBM.  out: HOST words, uploaded before the launch and downloaded after it,
 * so a slot the kernels did not write keeps what the caller put there.
 *   _msm     comb_msm: d_scalars [ninst][nterms] over the first nterms <= T points (0 = T), rows_hint 0 any / 1 pairs / 2 dense, a scratch of
 *            exactly scratch_bytes (0: none); out [ninst][8]
 *   _groups  comb_groups: d_scalars [ninst][1 + l0 + n0], out [ninst][out_stride][8] (slot 1 + q = group q of 2^L points; slot 0 and the slots past
 *            the groups are not written)
 *   _lanes   comb_lanes: d_scalars [ninst][nterms], out [ninst][8]
 * What the launchers refuse (nterms > T, 1 + l0 + n0 > T, L outside [1, 20], a stride below 1 + the groups) comes back as their BPPP_ERR_ARG: nothing
 * was launched and out is left as it was. */
typedef struct bppp_test_comb bppp_test_comb;
int bppp_test_comb_create(bppp_ctx *ctx, const void *d_points, size_t T, int window_bits, bppp_test_comb **out);
void bppp_test_comb_destroy(bppp_test_comb *tab);
int bppp_test_comb_msm(bppp_test_comb *tab, const void *d_scalars, size_t ninst, size_t nterms, int rows_hint, size_t scratch_bytes, uint64_t *out);
int bppp_test_comb_groups(bppp_test_comb *tab, const void *d_scalars, size_t ninst, size_t l0, size_t n0, int L, size_t out_stride, uint64_t *out);
int bppp_test_comb_lanes(bppp_test_comb *tab, const void *d_scalars, size_t nterms, size_t ninst, uint64_t *out);
/* What the last comb_msm launch on this context did, the product's own calls included.  route: -1 none yet, 0 k_comb_msm (a wavefront, or
 * parts = tparts x wsplit of them, per instance; heavy_first: the even instances dispatched first), 1 / 2 k_comb_msm_packed with 8 / 16 lanes
 * per instance, 3 k_comb_msm_rows (lane = instance: chunks partial sums of clen terms per instance, k_comb_join_rows with join_lanes lanes per
 * instance), 4 the same with the instances dispatched as pairs.  Fields of the other routes are 0. */
typedef struct bppp_test_comb_report { int32_t route, heavy_first; uint32_t parts, tparts, wsplit, chunks, clen, join_lanes; } bppp_test_comb_report;
int bppp_test_last_comb_msm(bppp_ctx *ctx, bppp_test_comb_report *report);
/* What the bucket reduction of the last MSM on this context launched, the small route and the product's own calls included.  route: -1 none
 * yet, 0 the small route (the tail of k_msm_small and, with S > 1 slices, k_msm_small_join), 1 k_reduce_groups (RG lanes per window, Lw buckets
 * per lane), 2 k_reduce_marg + k_reduce_tail_quad (a .. TC: the MargGeom of csrc/msm_plan.hpp), 3 k_reduce1 + k_reduce2 (Lw buckets per lane, WPW
 * wavefronts per window).  c: window bits, W: windows left for the combine (1 for a registered basis), M = 2^(c-1) buckets per window.  combine:
 * 1 = the windows were combined in k_window_combine, 0 = on the host.  Fields of the other routes are 0. */
typedef struct bppp_test_reduce_report { int32_t route, combine, c, W, M, RG, Lw, WPW, a, LO, HI, PR, PC, SR, SC, TR, TC, S; } bppp_test_reduce_report;
int bppp_test_last_reduce(bppp_ctx *ctx, bppp_test_reduce_report *report);
/* The transcript text kernel of the last verification on this handle (bppp_rp_verify_batch*, _each*, its share of _mixed*): 0 = k_rp_text,
 * 1 = k_rp_text_lds (while the text image of a proof fits 64 KiB of LDS: up to 272 transcript points), -1 = none yet. */
int bppp_test_rp_last_text_kernel(bppp_rp *rp, int *lds);
/* The size classes of the typed-reciprocal kernels whose dynamic LDS grows with the setup.  bppp_test_rp_lds_plan asks the host functions that
 * size the launches and gate the routes (csrc/rpprove_dev.hpp, csrc/trrp.hpp); it takes dimensions, needs no context and launches nothing.
 *   kernel  BPPP_TEST_RP_K_PHASE2 / _PHASE3: the provers' k_rpp_phase2 / k_rpp_phase3 for a setup of `nranges` ranges whose widest live digit base
 *           is max_base (nsyms, batch unused).  table: the entries of the per-proof reciprocal table, the power of two at or above max_base
 *           (16 .. 1024); lanes 64; fits: lds_bytes <= 160 KiB — where either phase does not fit, a prove takes the host-algebra route.
 *           BPPP_TEST_RP_K_PUBLIC: bppp_trrp_public_device on `batch` proofs of a setup of nranges ranges and nsyms reciprocal symbols (max_base
 *           unused).  lanes per proof and lds_bytes of k_trrp_public; split: 1 = the call runs k_trrp_pre / k_trrp_pos / k_trrp_lin instead
 *           (batch > 1024, or fits = 0).
 * Above 64 KiB a launch asks for its LDS with hipFuncSetAttribute.
 * bppp_test_rp_last_prove: the last typed-reciprocal prove on the handle.  route 0 = none yet, 1 = the device algebra (lds2_bytes / lds3_bytes: the
 * dynamic LDS its phase kernels were launched with), 2 = the host-algebra route (both 0); table as above, for the handle's setup.  The report is
 * written on the handle that proves: a batch of SPLIT_MIN proofs or more runs as two halves, the second on the handle's twin, so after such a call
 * the report describes the first half only (same setup, same route and LDS); a batch run on the twin alone does not exist.  The reports say what
 * was planned and launched, not whether hipFuncSetAttribute was called: a launch above 64 KiB has been seen to run without it.
 * bppp_test_trrp_last_public / bppp_test_rp_last_public: the last bppp_trrp_public_device on these tables, resp. the last run of the same kernels
 * inside a verification or a prove on the handle.  route 0 = none yet, 1 = k_trrp_public (lanes per proof, lds_bytes), 2 = the three kernels. */
enum { BPPP_TEST_RP_K_PUBLIC = 0, BPPP_TEST_RP_K_PHASE2 = 2, BPPP_TEST_RP_K_PHASE3 = 3 };
typedef struct bppp_test_rp_lds_plan_report { uint64_t lds_bytes; uint32_t table, lanes, fits, split; } bppp_test_rp_lds_plan_report;
typedef struct bppp_test_rp_prove_report { int32_t route; uint32_t table; uint64_t lds2_bytes, lds3_bytes; } bppp_test_rp_prove_report;
typedef struct bppp_test_rp_public_report { int32_t route, lanes; uint64_t lds_bytes; } bppp_test_rp_public_report;
int bppp_test_rp_lds_plan(int kernel, size_t max_base, size_t nranges, size_t nsyms, size_t batch, bppp_test_rp_lds_plan_report *report);
int bppp_test_rp_last_prove(bppp_rp *rp, bppp_test_rp_prove_report *report);
int bppp_test_trrp_last_public(bppp_trrp *tabs, bppp_test_rp_public_report *report);
int bppp_test_rp_last_public(bppp_rp *rp, bppp_test_rp_public_report *report);
/* The provers' transcript (RppTranscript of csrc/rpp_transcript.hip) alone, in device mode whatever the batch size: begin with the `ncalls` oracle
 * calls given, no argument rounds, then call 0, 1, ... in turn.  Call c puts calls[c].points new points in front of every proof's text and draws
 * calls[c].count (1 .. 3) challenges, into slots first_slot .. of ch (first_slot + count <= 7) or, first_slot = 7 and count = 1, into es.
 * points: host words, for call 0, then call 1, ...: [batch][calls[c].points][8] affine x | y, any values below 2^256 — they are text, not checked
 * to be on the curve; the calls' points together may not exceed the handle's own transcript (nrp + nranges + 2 rounds), which sizes the text
 * buffer.  bindings: NULL or [batch][32] bytes (the tag of proof b is then oracle_tag <> bindings[b]).  challenges: host, [ncalls][batch][3][4]
 * words, the outputs of call c as read back after it (zero beyond count). */
typedef struct bppp_test_rpp_call { uint32_t points, count, first_slot; } bppp_test_rpp_call;
int bppp_test_rpp_transcript(bppp_rp *rp, size_t batch, const bppp_test_rpp_call *calls, size_t ncalls, const uint64_t *points, const uint8_t *bindings,
                             uint64_t *challenges);
/* rpp_draws: out[b][c] = hashToScalar (prefix_b <> show c), c < nd; prefixes host [batch][prefix_len] (prefix_len 0: NULL will do), out host
 * [batch][nd][4] words. */
int bppp_test_rpp_draws(bppp_ctx *ctx, const uint8_t *prefixes, size_t prefix_len, size_t batch, size_t nd, uint64_t *out);
/* Poison: every SCRATCH buffer of a context, or of a range-proof handle, filled with `byte` (0 .. 255) at its current capacity, so that the next call
 * cannot rest on what an earlier call left there (csrc/ctx.hpp: no entry point reads a workspace word that the same call has not written).  Both drain
 * the context first (ctx_drain), fill HBM with hipMemsetAsync on the context's stream and wait for it, and fill pinned host memory with memset.
 * bytes_poisoned: the bytes filled in all (0: nothing had been allocated yet).  A NULL handle or a closed context is BPPP_ERR_ARG.
 * Scratch = rewritten by every call that uses it; persistent = filled at creation or first use and read by later calls (never poisoned).
 * _ctx_ (members of bppp_ctx, csrc/ctx.hpp); it also drops last_msm_valid, so bppp_test_last_msm_layout / _copy refuse instead of copying poison:
 *   ws           scratch     the MSM's workspace, carved per call (csrc/msm.hip), and the batch inversion's (csrc/rounds.hip)
 *   ws2          scratch     what a caller that also runs an MSM assembles for it (csrc/nlbatch.hip, nl.hip, ip.hip, glv.hip, trrp.hip, seedpoints.hip, rpmixed.hip, rpblock.hip)
 *   mix          scratch     one call's MSM input and shared scalars of the multi-setup verifier and the block call, the input commitments of one bppp_rp_prove_mixed (csrc/rpmixed.hip, rpblock.hip — with the half-aggregate's tree in bppp_rp_verify_block_agg —, rpshare.hip)
 *   pinned       scratch     pinned host staging of small results and uploads (csrc/msm.hip, rounds.hip, ip.hip, capi.hip)
 *   pre_acc, pre_acc_arg     not buffers: the one-shot upload hook of bppp_msm and its argument, set and cleared within one call (csrc/msm.hip)
 * _rp_ (members of bppp_rp, csrc/rp_internal.hpp); with a twin handle (a split prove batch), the twin's buffers and the twin's own context as well, but
 * NOT the handle's own context: the caller poisons both:
 *   pwork        scratch     the provers' and the commit / open / tally / excess calls' workspace (csrc/rpprove.hip, rpprove_dev.hip, brpprove*.hip, rpcommit.hip, rptally.hip, rpexcess.hip, rpexkeys.hip, rpexpart.hip, rpexagg.hip: the half-aggregate's leaves and tree levels in front of a pass; rpcut.hip: cut-through's identities, table and sort)
 *   awork        scratch     the device-resident inner-product argument's workspace and final witness (csrc/rpprove_dev.hip hands it to ipb_prove_stream, csrc/ipb.hip)
 *   hpin         scratch     pinned staging of the batch provers (csrc/rpprove.hip, brpprove.hip)
 *   work         scratch     the verifier's per-proof arrays of one prepared batch (csrc/rp.hip: rp_verify_prepare)
 *   stage        scratch     the host files of one verification, uploaded in slices (csrc/rp.hip: rp_stage_files)
 *   ework        scratch     the per-proof verifier's rows (csrc/rpeach.hip)
 *   hstage       scratch     pinned downloads and uploads of the host oracle of one verification (csrc/rp.hip)
 *   hflag        scratch     64 pinned bytes; word 0 is copied from bad[batch] by every rp_verify_prepare (csrc/rp.hip) and read after the same call's MSM (csrc/rp.hip, rpmixed.hip, rpblock.hip)
 *   d_pub        scratch     one call's canonical public amounts (csrc/rp.hip: rp_upload_public)
 *   d_sel        scratch     the accepted / refused proofs of one status call (csrc/rpwitness.hip)
 *   d_bind       scratch     one bound call's bindings (csrc/rpbind.hip)
 *   d_bhdr       scratch     one bound call's per-proof headers (csrc/rpbind.hip: rp_bound_headers)
 *   d_comb_out   scratch     comb_out_rows points: the first-round commitments of one call of the fold route, written by comb_msm and copied out in the same call (csrc/rpprove.hip)
 *   d_basis, d_plan          persistent   the basis and the hash plan, uploaded by bppp_rp_create* (csrc/rp.hip)
 *   d_fixed, commit_basis    persistent   the window table of (g, H0, H1) and the registered [g | H | G], built at first use (csrc/rpcommit.hip, rpprove.hip)
 *   d_wit                    persistent   per-range data of the witness kernels, uploaded at the first device prove (csrc/rpwitness.hip)
 *   tabs, btabs, comb        persistent   the setup's device tables and the comb table (csrc/trrp.hip, rp.hip, comb.hip)
 *   ctx, twin, twin_ctx, pool             handles and the host oracle's workers, not buffers
 *   pre_inputs               borrowed     the caller's precomputed input commitments while bppp_rp_prove_mixed runs (csrc/rpshare.hip) */
int bppp_test_ctx_poison(bppp_ctx *ctx, int byte, uint64_t *bytes_poisoned);
int bppp_test_rp_poison(bppp_rp *rp, int byte, uint64_t *bytes_poisoned);
#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
