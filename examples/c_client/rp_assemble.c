/* rp_assemble.c — two transactions as they arrived become one block with ONE call: bppp_rp_cut_through.  Plain C99.
 *
 * The scenario of rp_cut_through.c, with the block's hand-written pool and index arrays replaced by the call:
 *   setup     the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded)
 *   tx 1      spends A into B and C with fee f1;  tx 2 spends B and E into D with fee f2.  Sums are outputs - inputs: the amount of a sum is minus its fee
 *   received  six rows, in arrival order: A; B, C; B again, as tx 2 brings its own copy of the output it spends; D; E — and one sum per transaction
 *   builders  each splits its blinding sum into a revealed offset and a signing key, publishes the key (bppp_rp_excess_keys) and signs with it
 *   block     bppp_rp_cut_through finds B created and spent inside the set, drops both sides, puts the new outputs C and D in front of the inputs A
 *             and E, re-bases the one sum - A + C - E + D and adds up the fees and the offsets
 *   check     bppp_rp_excess_sums_each over what the call returned, with both keys in one group, is BPPP_RP_OPEN_OK; with a fee off by one, MISMATCH
 *
 * Build and run (tests/test_gpu_c_client_assemble.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_assemble.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_assemble
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
  enum { A = 0, B = 1, C = 2, D = 3, E = 4, O1 = 5, O2 = 6, WROWS = 7, COMS = 5, ROWS = 6, TXS = 2, NNZ = 6 };
  static const char seed_text[] = "test points";
  static const uint64_t f1 = 500, f2 = 70;
  /* the builders' sums over their witness rows: the signing key of each transaction is its blinding sum less its offset */
  static const uint32_t b_start[3] = {0, 4, 8};
  static const uint32_t b_entries[8] = {A | SUB, B, C, O1 | SUB, B | SUB, E | SUB, D, O2 | SUB};
  /* the job as received: which commitment lies in which of the six rows, and one sum per transaction over them */
  static const int arrived[ROWS] = {A, B, C, B, D, E};
  static const uint32_t sum_start[TXS + 1] = {0, 3, 6}, entries[NNZ] = {0u | SUB, 1u, 2u, 3u | SUB, 5u | SUB, 4u};
  static const uint32_t tx_key_start[TXS + 1] = {0, 1, 2}, key_start[2] = {0, TXS};
  uint32_t block_start[2] = {0, 0};
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  bppp_rp_cut_counts counts;
  uint64_t amounts[WROWS][1][4], types[WROWS][1][4], blinds[WROWS][1][4];
  uint64_t b_amount[TXS][4], b_type[TXS][4], b_blind[TXS][4], tx_amount[TXS][4], tx_type[TXS][4], tx_offset[TXS][4], block_claims[3][4];
  uint8_t aux[32], msgs[TXS][32], keys[TXS][BPPP_RP_EXCESS_KEY_BYTES], sigs[TXS][BPPP_RP_EXCESS_SIG_BYTES];
  uint8_t *coms, *pool, *new_pool;
  uint32_t commit_status[COMS], kstatus[TXS], status[TXS], entry_status[NNZ], row_map[ROWS], new_entries[NNZ];
  int b;
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
  amounts[E][0][0] = 250000; amounts[D][0][0] = 400000 + 250000 - f2;        /* the two offset rows keep amount zero */
  ur = fopen("/dev/urandom", "rb");                                          /* blindings and offsets, the signers' aux, the transactions */
  EXPECT(ur && fread(blinds, 1, sizeof blinds, ur) == sizeof blinds && fread(aux, 1, 32, ur) == 32 && fread(msgs, 1, sizeof msgs, ur) == sizeof msgs);
  fclose(ur);
  for (b = 0; b < WROWS; b++) blinds[b][0][3] >>= 1;                         /* < 2^255 < n */
  coms = (uint8_t *)calloc(COMS, shp.coms_bytes);
  pool = (uint8_t *)calloc(ROWS, shp.coms_bytes);
  new_pool = (uint8_t *)calloc(ROWS, shp.coms_bytes);
  EXPECT(coms != NULL && pool != NULL && new_pool != NULL);
  CHECK(bppp_rp_commit_batch(rp, COMS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], commit_status, coms));
  for (b = 0; b < COMS; b++) EXPECT(commit_status[b] == BPPP_RP_WIT_OK);

  /* the builders: k_t = e_t - o_t signs and is published as a key; o_t is revealed with the transaction */
  CHECK(bppp_rp_tally_claims(rp, WROWS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], TXS, b_start, b_entries, 8, &b_amount[0][0], &b_type[0][0], &b_blind[0][0]));
  EXPECT(b_amount[0][0] == (uint64_t)0 - f1 && b_amount[1][0] == (uint64_t)0 - f2 && b_amount[0][3] == ~(uint64_t)0);
  CHECK(bppp_rp_excess_keys(rp, TXS, &b_blind[0][0], &keys[0][0], kstatus));
  CHECK(bppp_rp_excess_sign(rp, TXS, &b_blind[0][0], &msgs[0][0], aux, &sigs[0][0], NULL, status));
  for (b = 0; b < TXS; b++) EXPECT(kstatus[b] == BPPP_RP_EXCESS_OK && status[b] == BPPP_RP_EXCESS_OK);
  memset(b_blind, 0, sizeof b_blind);
  printf("builders: two transactions, each with a key, a signature, a fee and an offset\n");

  /* the transactions as received: six rows, one sum each, the claim of each (minus its fee, no type, its offset) */
  for (b = 0; b < ROWS; b++) memcpy(pool + (size_t)b * shp.coms_bytes, coms + (size_t)arrived[b] * shp.coms_bytes, shp.coms_bytes);
  memcpy(tx_amount, b_amount, sizeof tx_amount);
  memset(tx_type, 0, sizeof tx_type);
  memcpy(tx_offset[0], blinds[O1][0], sizeof tx_offset[0]);
  memcpy(tx_offset[1], blinds[O2][0], sizeof tx_offset[1]);
  CHECK(bppp_rp_excess_sums_each(rp, ROWS, pool, TXS, sum_start, entries, NNZ, &tx_amount[0][0], &tx_type[0][0], &tx_offset[0][0], TXS, tx_key_start, &keys[0][0],
                                 status, NULL));
  EXPECT(status[0] == BPPP_RP_OPEN_OK && status[1] == BPPP_RP_OPEN_OK);
  printf("as received: each transaction balances against its own key\n");

  /* the step: one call */
  CHECK(bppp_rp_cut_through(rp, ROWS, pool, TXS, sum_start, entries, NNZ, &tx_amount[0][0], &tx_type[0][0], &tx_offset[0][0], entry_status, row_map, new_pool, new_entries,
                            &block_claims[0][0], &counts));
  EXPECT(counts.new_rows == 4 && counts.out_rows == 2 && counts.new_nnz == 4 && counts.ncut == 2 && counts.nagain == 0);
  EXPECT(entry_status[1] == BPPP_RP_CUT_SPENT && entry_status[3] == BPPP_RP_CUT_SPENT);                   /* + B of tx 1, - B of tx 2 */
  EXPECT(entry_status[0] == BPPP_RP_CUT_KEPT && entry_status[2] == BPPP_RP_CUT_KEPT && entry_status[4] == BPPP_RP_CUT_KEPT && entry_status[5] == BPPP_RP_CUT_KEPT);
  EXPECT(row_map[0] == 2 && row_map[1] == 4 && row_map[2] == 0 && row_map[3] == 5);                       /* C, D: the new outputs; then A, E */
  EXPECT(new_entries[0] == (2u | SUB) && new_entries[1] == 0u && new_entries[2] == (3u | SUB) && new_entries[3] == 1u);
  for (b = 0; b < 4; b++) EXPECT(memcmp(new_pool + (size_t)b * shp.coms_bytes, pool + (size_t)row_map[b] * shp.coms_bytes, shp.coms_bytes) == 0);
  EXPECT(block_claims[0][0] == (uint64_t)0 - (f1 + f2) && block_claims[0][3] == ~(uint64_t)0);            /* minus the fees, in two's complement */
  printf("cut_through: B is gone; %d rows (%d new outputs in front), %d entries, %d cut\n", (int)counts.new_rows, (int)counts.out_rows, (int)counts.new_nnz, (int)counts.ncut);

  /* the block: what the call returned, the keys of both transactions in one group */
  block_start[1] = (uint32_t)counts.new_nnz;
  CHECK(bppp_rp_excess_sums_each(rp, counts.new_rows, new_pool, 1, block_start, new_entries, counts.new_nnz, block_claims[0], block_claims[1], block_claims[2], TXS, key_start,
                                 &keys[0][0], status, NULL));
  EXPECT(status[0] == BPPP_RP_OPEN_OK);
  printf("sums_each over the block: OK\n");

  block_claims[0][0] += 1;                                                   /* a fee of one less than the transactions paid */
  CHECK(bppp_rp_excess_sums_each(rp, counts.new_rows, new_pool, 1, block_start, new_entries, counts.new_nnz, block_claims[0], block_claims[1], block_claims[2], TXS, key_start,
                                 &keys[0][0], status, NULL));
  EXPECT(status[0] == BPPP_RP_OPEN_MISMATCH);
  printf("a fee off by one: MISMATCH\n");

  printf("assemble c client ok: two transactions merged into a block by one call, the output spent inside it never shown\n");
  bppp_rp_destroy(rp);
  free(coms);
  free(pool);
  free(new_pool);
  bppp_ctx_destroy(ctx);
  return 0;
}
