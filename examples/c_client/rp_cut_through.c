/* rp_cut_through.c — a block checked as ONE sum after cut-through: every transaction states its excess as a 33-byte key.  Plain C99.
 *
 *   setup     the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded)
 *   tx 1      spends A into B and C with fee f1;  tx 2 spends B into D with fee f2.  Sums are outputs - inputs: the amount of a sum is minus its fee
 *   builders  each splits its blinding sum e into a revealed offset o and a signing key k = e - o (bppp_rp_tally_claims does the arithmetic: the
 *             offset is a witness row of amount zero), publishes the key k B (bppp_rp_excess_keys) and signs with k (bppp_rp_excess_sign)
 *   block     keeps - A + C + D, the summed fee and the summed offset; B, created and spent inside the block, is gone from its pool
 *   check     bppp_rp_excess_verify_keys_batch accepts the two (key, message, signature) triples with no commitment in hand, and
 *             bppp_rp_excess_sums_each reports BPPP_RP_OPEN_OK for the block's one sum against the two keys; with one key left out, with a fee off
 *             by one and with the signatures under each other's keys it is MISMATCH
 *
 * Build and run (tests/test_gpu_c_client_cut_through.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_cut_through.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_cut_through
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
  enum { A = 0, B = 1, C = 2, D = 3, O1 = 4, O2 = 5, WROWS = 6, COMS = 4, KEYS = 2 };
  static const char seed_text[] = "test points";
  static const uint64_t f1 = 500, f2 = 70;
  /* the builders' sums over their witness rows: the signing keys of the two transactions, then the summed offset */
  static const uint32_t b_start[4] = {0, 4, 7, 9};
  static const uint32_t b_entries[9] = {A | SUB, B, C, O1 | SUB, B | SUB, D, O2 | SUB, O1, O2};
  /* the block's one sum over its pool of three files: - A + C + D */
  static const uint32_t sum_start[2] = {0, 3}, entries[3] = {0u | SUB, 1u, 2u};
  static const uint32_t key_start[2] = {0, KEYS}, key_start_one[2] = {0, 1};
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  uint64_t amounts[WROWS][1][4], types[WROWS][1][4], blinds[WROWS][1][4];
  uint64_t b_amount[3][4], b_type[3][4], b_blind[3][4], claim_amount[4], claim_type[4], claim_offset[4];
  uint8_t vseed[32], aux[32], msgs[KEYS][32], keys[KEYS][BPPP_RP_EXCESS_KEY_BYTES], swapped[KEYS][BPPP_RP_EXCESS_KEY_BYTES], sigs[KEYS][BPPP_RP_EXCESS_SIG_BYTES];
  uint8_t *coms, *pool;
  uint32_t commit_status[COMS], kstatus[KEYS], status[KEYS];
  int accept = -1, b;
  FILE *ur;

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
  ur = fopen("/dev/urandom", "rb");                                          /* blindings and offsets, the signers' aux, the checker's weights, the transactions */
  EXPECT(ur && fread(blinds, 1, sizeof blinds, ur) == sizeof blinds && fread(vseed, 1, 32, ur) == 32 && fread(aux, 1, 32, ur) == 32 &&
         fread(msgs, 1, sizeof msgs, ur) == sizeof msgs);
  fclose(ur);
  for (b = 0; b < WROWS; b++) blinds[b][0][3] >>= 1;                         /* < 2^255 < n */
  coms = (uint8_t *)calloc(COMS, shp.coms_bytes);
  pool = (uint8_t *)calloc(3, shp.coms_bytes);
  EXPECT(coms != NULL && pool != NULL);
  CHECK(bppp_rp_commit_batch(rp, COMS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], commit_status, coms));
  for (b = 0; b < COMS; b++) EXPECT(commit_status[b] == BPPP_RP_WIT_OK);

  /* the builders: k_i = e_i - o_i signs and is published as a key; o_1 + o_2 is revealed */
  CHECK(bppp_rp_tally_claims(rp, WROWS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], 3, b_start, b_entries, 9, &b_amount[0][0], &b_type[0][0], &b_blind[0][0]));
  EXPECT(b_amount[0][0] == (uint64_t)0 - f1 && b_amount[1][0] == (uint64_t)0 - f2 && b_amount[0][3] == ~(uint64_t)0 && !b_amount[2][0]);
  CHECK(bppp_rp_excess_keys(rp, KEYS, &b_blind[0][0], &keys[0][0], kstatus));
  CHECK(bppp_rp_excess_sign(rp, KEYS, &b_blind[0][0], &msgs[0][0], aux, &sigs[0][0], NULL, status));
  for (b = 0; b < KEYS; b++) EXPECT(kstatus[b] == BPPP_RP_EXCESS_OK && status[b] == BPPP_RP_EXCESS_OK && keys[b][32] <= 1);
  memcpy(claim_offset, b_blind[2], sizeof claim_offset);
  memset(b_blind, 0, sizeof b_blind);
  printf("builders: two keys of %d bytes, two signatures, one summed offset\n", (int)BPPP_RP_EXCESS_KEY_BYTES);

  /* anyone: the (key, message, signature) triples, no commitment in hand */
  CHECK(bppp_rp_excess_verify_keys_batch(rp, KEYS, &keys[0][0], &msgs[0][0], &sigs[0][0], vseed, &accept, status, NULL));
  EXPECT(accept == 1 && status[0] == BPPP_RP_OPEN_OK && status[1] == BPPP_RP_OPEN_OK);
  printf("verify_keys_batch: accept\n");

  /* the block: B is gone; what is left, less the fees and the offset, is the sum of the stated keys */
  memcpy(pool, coms + (size_t)A * shp.coms_bytes, shp.coms_bytes);
  memcpy(pool + shp.coms_bytes, coms + (size_t)C * shp.coms_bytes, shp.coms_bytes);
  memcpy(pool + 2 * (size_t)shp.coms_bytes, coms + (size_t)D * shp.coms_bytes, shp.coms_bytes);
  claim_amount[0] = (uint64_t)0 - (f1 + f2); claim_amount[1] = claim_amount[2] = claim_amount[3] = ~(uint64_t)0;       /* minus the fees, in two's complement */
  memset(claim_type, 0, sizeof claim_type);
  CHECK(bppp_rp_excess_sums_each(rp, 3, pool, 1, sum_start, entries, 3, claim_amount, claim_type, claim_offset, KEYS, key_start, &keys[0][0], status, NULL));
  EXPECT(status[0] == BPPP_RP_OPEN_OK);
  printf("sums_each: OK with B cut through\n");
  CHECK(bppp_rp_excess_sums_batch(rp, 3, pool, 1, sum_start, entries, 3, claim_amount, claim_type, claim_offset, KEYS, key_start, &keys[0][0], vseed, &accept, status, NULL));
  EXPECT(accept == 1 && status[0] == BPPP_RP_OPEN_OK);
  printf("sums_batch: accept\n");

  CHECK(bppp_rp_excess_sums_each(rp, 3, pool, 1, sum_start, entries, 3, claim_amount, claim_type, claim_offset, 1, key_start_one, &keys[0][0], status, NULL));
  EXPECT(status[0] == BPPP_RP_OPEN_MISMATCH);
  printf("one key left out: MISMATCH\n");

  claim_amount[0] += 1;                                                      /* a fee of one less than the transactions paid */
  CHECK(bppp_rp_excess_sums_each(rp, 3, pool, 1, sum_start, entries, 3, claim_amount, claim_type, claim_offset, KEYS, key_start, &keys[0][0], status, NULL));
  EXPECT(status[0] == BPPP_RP_OPEN_MISMATCH);
  CHECK(bppp_rp_excess_sums_batch(rp, 3, pool, 1, sum_start, entries, 3, claim_amount, claim_type, claim_offset, KEYS, key_start, &keys[0][0], vseed, &accept, status, NULL));
  EXPECT(accept == 0 && status[0] == BPPP_RP_OPEN_MISMATCH);
  printf("a fee off by one: MISMATCH, reject\n");

  memcpy(swapped[0], keys[1], sizeof swapped[0]);
  memcpy(swapped[1], keys[0], sizeof swapped[1]);                            /* each signature under the other transaction's key */
  CHECK(bppp_rp_excess_verify_keys_each(rp, KEYS, &swapped[0][0], &msgs[0][0], &sigs[0][0], status));
  EXPECT(status[0] == BPPP_RP_OPEN_MISMATCH && status[1] == BPPP_RP_OPEN_MISMATCH);
  CHECK(bppp_rp_excess_verify_keys_batch(rp, KEYS, &swapped[0][0], &msgs[0][0], &sigs[0][0], vseed, &accept, NULL, NULL));
  EXPECT(accept == 0);
  printf("a signature under the other key: MISMATCH, reject\n");

  printf("cut-through c client ok: a block of two transactions balanced as one sum against two stated keys, the spent output never shown\n");
  bppp_rp_destroy(rp);
  free(coms);
  free(pool);
  bppp_ctx_destroy(ctx);
  return 0;
}
