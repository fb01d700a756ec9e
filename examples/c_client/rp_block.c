/* rp_block.c — a block validated by ONE call: range proofs, kernel signatures and the balance after cut-through in one MSM.  Plain C99.
 *
 *   setup     the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded)
 *   tx 1      spends A into B and C with fee f1;  tx 2 spends B into D with fee f2 (rp_cut_through.c's block)
 *   builders  prove the new outputs C and D in range, each proof bound to its transaction's 32-byte message (bppp_rp_prove_bound); split the
 *             blinding sum into a revealed offset and a signing key, publish the key (bppp_rp_excess_keys) and sign with it (bppp_rp_excess_sign)
 *   block     pool rows C, D (with their proofs) and A (an input); B, created and spent inside the block, is gone; one sum  C + D - A
 *   check     ONE bppp_rp_verify_block accepts.  A fee off by one, proof D under tx 1's binding and the signatures under each other's keys are
 *             each rejected, and sum_status, proof_status and key_status name the culprit
 *
 * Build and run (tests/test_gpu_c_client_block.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_block.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_block
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
  enum { A = 0, B = 1, C = 2, D = 3, O1 = 4, O2 = 5, WROWS = 6, KEYS = 2, PROOFS = 2, ROWS = 3 };
  static const char seed_text[] = "test points", prefix[] = "block c client rnd C" "block c client rnd D";
  static const uint64_t f1 = 500, f2 = 70;
  /* the builders' sums over their witness rows: the signing keys of the two transactions, then the summed offset */
  static const uint32_t b_start[4] = {0, 4, 7, 9};
  static const uint32_t b_entries[9] = {A | SUB, B, C, O1 | SUB, B | SUB, D, O2 | SUB, O1, O2};
  /* the block's one sum over its pool [C, D, A]: C + D - A */
  static const uint32_t sum_start[2] = {0, 3}, entries[3] = {0u, 1u, 2u | SUB}, key_start[2] = {0, KEYS};
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  bppp_rp_block blk;
  bppp_rp_block_status st;
  uint64_t amounts[WROWS][1][4], types[WROWS][1][4], blinds[WROWS][1][4];
  uint64_t b_amount[3][4], b_type[3][4], b_blind[3][4], claim_amount[4], claim_type[4], claim_offset[4];
  uint8_t vseed[32], aux[32], msgs[KEYS][32], keys[KEYS][BPPP_RP_EXCESS_KEY_BYTES], swapped[KEYS][BPPP_RP_EXCESS_KEY_BYTES], sigs[KEYS][BPPP_RP_EXCESS_SIG_BYTES];
  uint8_t bindings[PROOFS][BPPP_RP_BINDING_BYTES], wrong[PROOFS][BPPP_RP_BINDING_BYTES];
  uint8_t *pool, *proofs, *a_file;
  uint32_t commit_status, kstatus[KEYS], sstatus[KEYS], proof_status[PROOFS], key_status[KEYS], sum_status[1];
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
  pool = (uint8_t *)calloc(ROWS, shp.coms_bytes);
  proofs = (uint8_t *)calloc(PROOFS, shp.proof_bytes);
  a_file = pool + 2 * (size_t)shp.coms_bytes;
  EXPECT(pool != NULL && proofs != NULL);

  /* the builders: C proven under tx 1's message, D under tx 2's (rows C and D of the witness are adjacent: one call writes pool rows 0 and 1);
   * k_i = e_i - o_i signs and is published as a key; o_1 + o_2 is revealed */
  memcpy(bindings, msgs, sizeof bindings);
  CHECK(bppp_rp_prove_bound(rp, PROOFS, &amounts[C][0][0], &types[C][0][0], &blinds[C][0][0], NULL, &bindings[0][0], (const uint8_t *)prefix, (sizeof prefix - 1) / PROOFS, pool,
                            proofs, NULL));
  CHECK(bppp_rp_commit_batch(rp, 1, &amounts[A][0][0], &types[A][0][0], &blinds[A][0][0], &commit_status, a_file));
  EXPECT(commit_status == BPPP_RP_WIT_OK);
  CHECK(bppp_rp_tally_claims(rp, WROWS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], 3, b_start, b_entries, 9, &b_amount[0][0], &b_type[0][0], &b_blind[0][0]));
  CHECK(bppp_rp_excess_keys(rp, KEYS, &b_blind[0][0], &keys[0][0], kstatus));
  CHECK(bppp_rp_excess_sign(rp, KEYS, &b_blind[0][0], &msgs[0][0], aux, &sigs[0][0], NULL, sstatus));
  for (b = 0; b < KEYS; b++) EXPECT(kstatus[b] == BPPP_RP_EXCESS_OK && sstatus[b] == BPPP_RP_EXCESS_OK);
  memcpy(claim_offset, b_blind[2], sizeof claim_offset);
  memset(b_blind, 0, sizeof b_blind);
  printf("builders: two bound proofs, two keys, two signatures, one summed offset\n");

  /* the node: everything it received, in one struct and one call */
  claim_amount[0] = (uint64_t)0 - (f1 + f2); claim_amount[1] = claim_amount[2] = claim_amount[3] = ~(uint64_t)0;       /* minus the fees, in two's complement */
  memset(claim_type, 0, sizeof claim_type);
  memset(&blk, 0, sizeof blk);
  blk.rows = ROWS; blk.coms_files = pool;
  blk.nproofs = PROOFS; blk.proof_files = proofs; blk.bindings = bindings;
  blk.nsums = 1; blk.sum_start = sum_start; blk.entries = entries; blk.nnz = 3;
  blk.claim_amounts = claim_amount; blk.claim_types = claim_type; blk.claim_offsets = claim_offset;
  blk.nkeys = KEYS; blk.key_start = key_start; blk.keys = keys; blk.msgs = msgs; blk.sigs = sigs;
  st.proof_status = proof_status; st.key_status = key_status; st.sum_status = sum_status;
  CHECK(bppp_rp_verify_block(rp, &blk, vseed, &accept, &st, NULL));
  EXPECT(accept == 1 && proof_status[0] == BPPP_RP_VALID && proof_status[1] == BPPP_RP_VALID && key_status[0] == BPPP_RP_OPEN_OK && key_status[1] == BPPP_RP_OPEN_OK &&
         sum_status[0] == BPPP_RP_OPEN_OK);
  printf("verify_block: accept\n");

  claim_amount[0] += 1;                                                      /* a fee of one less than the transactions paid */
  CHECK(bppp_rp_verify_block(rp, &blk, vseed, &accept, &st, NULL));
  EXPECT(accept == 0 && sum_status[0] == BPPP_RP_OPEN_MISMATCH && proof_status[0] == BPPP_RP_VALID && proof_status[1] == BPPP_RP_VALID &&
         key_status[0] == BPPP_RP_OPEN_OK && key_status[1] == BPPP_RP_OPEN_OK);
  printf("a fee off by one: reject, sum_status MISMATCH\n");
  claim_amount[0] -= 1;

  memcpy(wrong, bindings, sizeof wrong);
  memcpy(wrong[1], bindings[0], sizeof wrong[1]);                            /* D's proof presented as part of tx 1 */
  blk.bindings = wrong;
  CHECK(bppp_rp_verify_block(rp, &blk, vseed, &accept, &st, NULL));
  EXPECT(accept == 0 && proof_status[0] == BPPP_RP_VALID && proof_status[1] == BPPP_RP_INVALID && sum_status[0] == BPPP_RP_OPEN_OK &&
         key_status[0] == BPPP_RP_OPEN_OK && key_status[1] == BPPP_RP_OPEN_OK);
  printf("a proof under the other binding: reject, proof_status INVALID\n");
  blk.bindings = bindings;

  memcpy(swapped[0], keys[1], sizeof swapped[0]);
  memcpy(swapped[1], keys[0], sizeof swapped[1]);                            /* each signature under the other transaction's key: the sum still balances */
  blk.keys = swapped;
  CHECK(bppp_rp_verify_block(rp, &blk, vseed, &accept, &st, NULL));
  EXPECT(accept == 0 && key_status[0] == BPPP_RP_OPEN_MISMATCH && key_status[1] == BPPP_RP_OPEN_MISMATCH && sum_status[0] == BPPP_RP_OPEN_OK &&
         proof_status[0] == BPPP_RP_VALID && proof_status[1] == BPPP_RP_VALID);
  printf("a signature under the other key: reject, key_status MISMATCH\n");
  blk.keys = keys;

  CHECK(bppp_rp_verify_block(rp, &blk, vseed, &accept, NULL, NULL));
  EXPECT(accept == 1);
  printf("block c client ok: two transactions, the spent output never shown, validated by one call and one MSM\n");
  bppp_rp_destroy(rp);
  free(pool);
  free(proofs);
  bppp_ctx_destroy(ctx);
  return 0;
}
