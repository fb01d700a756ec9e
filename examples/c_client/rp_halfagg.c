/* rp_halfagg.c — the kernels of a block kept as 33 bytes each and ONE scalar: the half-aggregate of their signatures.  Plain C99.
 *
 *   setup      the two transactions of rp_cut_through.c: tx 1 spends A into B and C with fee f1, tx 2 spends B into D with fee f2; each states its
 *              excess as a 33-byte key and signs with it
 *   check      bppp_rp_excess_verify_keys_batch accepts the two signatures: the aggregator does not evaluate their equations, so this comes first
 *   aggregate  bppp_rp_excess_halfagg turns the 2 x 65 signature bytes into BPPP_RP_EXCESS_AGG_BYTES (2) = 98: the two R rows and one scalar
 *   verify     bppp_rp_excess_halfagg_verify accepts the aggregate with no seed, and refuses it with one message changed: every key then reads
 *              MISMATCH, for an aggregate cannot name a culprit
 *   block      bppp_rp_verify_block_agg checks the block after cut-through — the sum - A + C + D against the two keys, and the aggregate in place of
 *              the signatures — as one MSM
 *
 * Build and run (tests/test_gpu_c_client_halfagg.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_halfagg.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_halfagg
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bppp.h"

static bppp_ctx *ctx = NULL;
#define CHECK(call)                                                                                       \
  do {                                                                                                    \
    int rc_ = (call);                                                                                     \
    if (rc_) { fprintf(stderr, "%s:%d %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, ctx ? bppp_last_error(ctx) : ""); return 1; } \
  } while (0)
#define EXPECT(cond)                                                                                      \
  do { if (!(cond)) { fprintf(stderr, "%s:%d expectation failed: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

#define SUB 0x80000000u

int main(void) {
  enum { A = 0, B = 1, C = 2, D = 3, O1 = 4, O2 = 5, WROWS = 6, COMS = 4, KEYS = 2, AGG = BPPP_RP_EXCESS_AGG_BYTES(KEYS) };
  static const char seed_text[] = "test points";
  static const uint64_t f1 = 500, f2 = 70;
  /* the builders' sums over their witness rows: the signing keys of the two transactions, then the summed offset */
  static const uint32_t b_start[4] = {0, 4, 7, 9};
  static const uint32_t b_entries[9] = {A | SUB, B, C, O1 | SUB, B | SUB, D, O2 | SUB, O1, O2};
  /* the block's one sum over its pool of three files: - A + C + D */
  static const uint32_t sum_start[2] = {0, 3}, entries[3] = {0u | SUB, 1u, 2u};
  static const uint32_t key_start[2] = {0, KEYS};
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp_block blk;
  bppp_rp_block_status bst;
  bppp_rp *rp = NULL;
  uint64_t amounts[WROWS][1][4], types[WROWS][1][4], blinds[WROWS][1][4];
  uint64_t b_amount[3][4], b_type[3][4], b_blind[3][4], claim_amount[4], claim_type[4], claim_offset[4];
  uint8_t vseed[32], aux[32], msgs[KEYS][32], keys[KEYS][BPPP_RP_EXCESS_KEY_BYTES], sigs[KEYS][BPPP_RP_EXCESS_SIG_BYTES], agg[AGG];
  uint8_t *coms, *pool;
  uint32_t commit_status[COMS], kstatus[KEYS], status[KEYS], sum_status[1];
  int accept = -1, b;
  FILE *ur;

  EXPECT(AGG == 98);
  CHECK(bppp_ctx_create(0, &ctx));
  memset(&range, 0, sizeof range);
  range.base = 16; range.flags = BPPP_RP_OUTPUT; range.max[1] = 1;          /* [0, 2^64) */
  CHECK(bppp_rp_create_seeded(ctx, 1, 0, &range, 1, NULL, 0, (const uint8_t *)seed_text, sizeof seed_text - 1, NULL, &rp));
  CHECK(bppp_rp_info(rp, &shp));

  memset(amounts, 0, sizeof amounts);
  memset(types, 0, sizeof types);
  amounts[A][0][0] = 1000000;
  amounts[B][0][0] = 400000; amounts[C][0][0] = 1000000 - 400000 - f1;
  amounts[D][0][0] = 400000 - f2;                                            /* the two offset rows keep amount zero */
  ur = fopen("/dev/urandom", "rb");                                          /* blindings and offsets, the signers' aux, the block call's weights, the transactions */
  EXPECT(ur && fread(blinds, 1, sizeof blinds, ur) == sizeof blinds && fread(vseed, 1, 32, ur) == 32 && fread(aux, 1, 32, ur) == 32 &&
         fread(msgs, 1, sizeof msgs, ur) == sizeof msgs);
  fclose(ur);
  for (b = 0; b < WROWS; b++) blinds[b][0][3] >>= 1;                         /* < 2^255 < n */
  coms = (uint8_t *)calloc(COMS, shp.coms_bytes);
  pool = (uint8_t *)calloc(3, shp.coms_bytes);
  EXPECT(coms != NULL && pool != NULL);
  CHECK(bppp_rp_commit_batch(rp, COMS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], commit_status, coms));
  for (b = 0; b < COMS; b++) EXPECT(commit_status[b] == BPPP_RP_WIT_OK);

  /* the builders, as in rp_cut_through.c: k_i = e_i - o_i signs and is published as a key; o_1 + o_2 is revealed */
  CHECK(bppp_rp_tally_claims(rp, WROWS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], 3, b_start, b_entries, 9, &b_amount[0][0], &b_type[0][0], &b_blind[0][0]));
  CHECK(bppp_rp_excess_keys(rp, KEYS, &b_blind[0][0], &keys[0][0], kstatus));
  CHECK(bppp_rp_excess_sign(rp, KEYS, &b_blind[0][0], &msgs[0][0], aux, &sigs[0][0], NULL, status));
  for (b = 0; b < KEYS; b++) EXPECT(kstatus[b] == BPPP_RP_EXCESS_OK && status[b] == BPPP_RP_EXCESS_OK);
  memcpy(claim_offset, b_blind[2], sizeof claim_offset);
  memset(b_blind, 0, sizeof b_blind);

  /* the signatures first: the aggregator takes them as they are */
  CHECK(bppp_rp_excess_verify_keys_batch(rp, KEYS, &keys[0][0], &msgs[0][0], &sigs[0][0], vseed, &accept, status, NULL));
  EXPECT(accept == 1 && status[0] == BPPP_RP_OPEN_OK && status[1] == BPPP_RP_OPEN_OK);
  printf("verify_keys_batch: accept\n");

  memset(agg, 0xA5, sizeof agg);
  CHECK(bppp_rp_excess_halfagg(rp, KEYS, &keys[0][0], &msgs[0][0], &sigs[0][0], agg, status));
  EXPECT(status[0] == BPPP_RP_OPEN_OK && status[1] == BPPP_RP_OPEN_OK);
  EXPECT(!memcmp(agg, sigs[0], 33) && !memcmp(agg + 33, sigs[1], 33));      /* the R rows as the signatures hold them */
  printf("halfagg: %d signature bytes became %d\n", (int)(KEYS * BPPP_RP_EXCESS_SIG_BYTES), (int)AGG);
  memset(sigs, 0, sizeof sigs);                                              /* from here on the 65-byte signatures are gone */

  accept = -1;
  CHECK(bppp_rp_excess_halfagg_verify(rp, KEYS, &keys[0][0], &msgs[0][0], agg, &accept, status, NULL));
  EXPECT(accept == 1 && status[0] == BPPP_RP_OPEN_OK && status[1] == BPPP_RP_OPEN_OK);
  printf("halfagg_verify: accept\n");

  msgs[1][7] ^= 1;                                                           /* one message changed in one bit */
  CHECK(bppp_rp_excess_halfagg_verify(rp, KEYS, &keys[0][0], &msgs[0][0], agg, &accept, status, NULL));
  EXPECT(accept == 0 && status[0] == BPPP_RP_OPEN_MISMATCH && status[1] == BPPP_RP_OPEN_MISMATCH);
  printf("one message changed: reject, MISMATCH for both keys\n");
  msgs[1][7] ^= 1;

  /* the block after cut-through: B is gone; the sum against the two keys and the aggregate in place of the signatures, one MSM */
  memcpy(pool, coms + (size_t)A * shp.coms_bytes, shp.coms_bytes);
  memcpy(pool + shp.coms_bytes, coms + (size_t)C * shp.coms_bytes, shp.coms_bytes);
  memcpy(pool + 2 * (size_t)shp.coms_bytes, coms + (size_t)D * shp.coms_bytes, shp.coms_bytes);
  claim_amount[0] = (uint64_t)0 - (f1 + f2); claim_amount[1] = claim_amount[2] = claim_amount[3] = ~(uint64_t)0;       /* minus the fees, in two's complement */
  memset(claim_type, 0, sizeof claim_type);
  memset(&blk, 0, sizeof blk);                                               /* no proofs here; sigs stays NULL and key_offset 0 */
  blk.rows = 3; blk.coms_files = pool;
  blk.nsums = 1; blk.sum_start = sum_start; blk.entries = entries; blk.nnz = 3;
  blk.claim_amounts = claim_amount; blk.claim_types = claim_type; blk.claim_offsets = claim_offset;
  blk.nkeys = KEYS; blk.key_start = key_start; blk.keys = keys; blk.msgs = msgs;
  bst.proof_status = NULL; bst.key_status = status; bst.sum_status = sum_status;
  accept = -1;
  CHECK(bppp_rp_verify_block_agg(rp, &blk, agg, vseed, &accept, &bst, NULL));
  EXPECT(accept == 1 && status[0] == BPPP_RP_OPEN_OK && status[1] == BPPP_RP_OPEN_OK && sum_status[0] == BPPP_RP_OPEN_OK);
  printf("verify_block_agg: accept\n");

  claim_amount[0] += 1;                                                      /* a fee of one less than the transactions paid */
  CHECK(bppp_rp_verify_block_agg(rp, &blk, agg, vseed, &accept, &bst, NULL));
  EXPECT(accept == 0 && status[0] == BPPP_RP_OPEN_OK && status[1] == BPPP_RP_OPEN_OK && sum_status[0] == BPPP_RP_OPEN_MISMATCH);
  printf("a fee off by one: reject, the sum MISMATCH, the aggregate OK\n");

  printf("halfagg c client ok: two kernels kept as %d bytes, checked alone and inside the block\n", (int)(KEYS * BPPP_RP_EXCESS_KEY_BYTES + AGG));
  bppp_rp_destroy(rp);
  free(coms);
  free(pool);
  bppp_ctx_destroy(ctx);
  return 0;
}
