/* rp_excess.c — a PUBLIC validator's balance check: the excess blinding is never revealed, its owner signs with it.  Plain C99.
 *
 *   setup    the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded): a
 *            shape whose proofs say nothing about balance
 *   pool     four commitments files (bppp_rp_commit_batch): two inputs, two outputs; inputs - outputs = the fee
 *   builder  bppp_rp_tally_claims over its witnesses for the one sum  + in0 + in1 - out0 - out1 : the amount is the public fee, the blinding
 *            e stays with the builder, who signs the transaction's 32 bytes with it (bppp_rp_excess_sign)
 *   check    the validator has the files, the fee, the message and the 65-byte signature: bppp_rp_excess_verify_each reports BPPP_RP_OPEN_OK
 *            and bppp_rp_excess_verify_batch accepts; the same signature under another message is refused, and so is an output off by one
 *
 * Build and run (tests/test_gpu_c_client_excess.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_excess.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_excess
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

int main(void) {
  enum { ROWS = 4, NNZ = 4 };
  static const char seed_text[] = "test points";
  static const uint64_t fee = 500;
  static const uint32_t sum_start[2] = {0, NNZ};
  static const uint32_t entries[NNZ] = {0u, 1u, 2u | 0x80000000u, 3u | 0x80000000u};      /* + in0 + in1 - out0 - out1 */
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  uint64_t amounts[ROWS][1][4], types[ROWS][1][4], blinds[ROWS][1][4];
  uint64_t claim_amount[4], claim_type[4], claim_blind[4], excess_signed[8], excess_seen[8];
  uint8_t vseed[32], aux[32], msg[32], other_msg[32], sig[BPPP_RP_EXCESS_SIG_BYTES], *coms;
  uint32_t commit_status[ROWS], status[1];
  int accept = -1, b;
  FILE *ur;

  CHECK(bppp_ctx_create(0, &ctx));
  memset(&range, 0, sizeof range);
  range.base = 16; range.flags = BPPP_RP_OUTPUT; range.max[1] = 1;          /* [0, 2^64) */
  CHECK(bppp_rp_create_seeded(ctx, 1, 0, &range, 1, NULL, 0, (const uint8_t *)seed_text, sizeof seed_text - 1, NULL, &rp));
  CHECK(bppp_rp_info(rp, &shp));

  memset(amounts, 0, sizeof amounts);
  memset(types, 0, sizeof types);
  memset(blinds, 0, sizeof blinds);
  amounts[0][0][0] = 700000; amounts[1][0][0] = 300500;                      /* inputs */
  amounts[2][0][0] = 600000; amounts[3][0][0] = 400000;                      /* outputs: 500 less, the fee */
  ur = fopen("/dev/urandom", "rb");                                          /* blindings, the signer's aux, the checker's weights, the transaction */
  EXPECT(ur && fread(blinds, 1, sizeof blinds, ur) == sizeof blinds && fread(vseed, 1, 32, ur) == 32 && fread(aux, 1, 32, ur) == 32 && fread(msg, 1, 32, ur) == 32);
  fclose(ur);
  for (b = 0; b < ROWS; b++) blinds[b][0][3] >>= 1;                          /* < 2^255 < n */
  coms = (uint8_t *)calloc(ROWS, shp.coms_bytes);
  EXPECT(coms != NULL);
  CHECK(bppp_rp_commit_batch(rp, ROWS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], commit_status, coms));
  for (b = 0; b < ROWS; b++) EXPECT(commit_status[b] == BPPP_RP_WIT_OK);

  /* the builder: the claim of the sum from its witnesses; the blinding sum signs and is not passed on */
  CHECK(bppp_rp_tally_claims(rp, ROWS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], 1, sum_start, entries, NNZ, claim_amount, claim_type, claim_blind));
  EXPECT(claim_amount[0] == fee && !claim_amount[1] && !claim_amount[2] && !claim_amount[3]);
  CHECK(bppp_rp_excess_sign(rp, 1, claim_blind, msg, aux, sig, excess_signed, status));
  EXPECT(status[0] == BPPP_RP_EXCESS_OK && sig[32] <= 1);
  memset(claim_blind, 0, sizeof claim_blind);
  printf("claim: amount %llu = the fee, signed with the excess blinding\n", (unsigned long long)claim_amount[0]);

  /* the validator: the files, the public fee, the message and the signature — no witness, no blinding */
  claim_amount[0] = fee;
  CHECK(bppp_rp_excess_verify_each(rp, ROWS, coms, 1, sum_start, entries, NNZ, claim_amount, claim_type, msg, sig, status, excess_seen));
  EXPECT(status[0] == BPPP_RP_OPEN_OK && memcmp(excess_seen, excess_signed, sizeof excess_seen) == 0);
  printf("excess_verify_each: OK\n");
  CHECK(bppp_rp_excess_verify_batch(rp, ROWS, coms, 1, sum_start, entries, NNZ, claim_amount, claim_type, msg, sig, vseed, &accept, status, NULL));
  EXPECT(accept == 1 && status[0] == BPPP_RP_OPEN_OK);
  printf("excess_verify_batch: accept\n");

  memcpy(other_msg, msg, 32);
  other_msg[0] ^= 1;                                                         /* the signature does not carry over to another transaction */
  CHECK(bppp_rp_excess_verify_each(rp, ROWS, coms, 1, sum_start, entries, NNZ, claim_amount, claim_type, other_msg, sig, status, NULL));
  EXPECT(status[0] == BPPP_RP_OPEN_MISMATCH);
  CHECK(bppp_rp_excess_verify_batch(rp, ROWS, coms, 1, sum_start, entries, NNZ, claim_amount, claim_type, other_msg, sig, vseed, &accept, status, NULL));
  EXPECT(accept == 0 && status[0] == BPPP_RP_OPEN_MISMATCH);
  printf("another message: MISMATCH, reject\n");

  amounts[3][0][0] += 1;                                                     /* an output that takes one more than the inputs leave */
  CHECK(bppp_rp_commit_batch(rp, ROWS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], commit_status, coms));
  CHECK(bppp_rp_excess_verify_each(rp, ROWS, coms, 1, sum_start, entries, NNZ, claim_amount, claim_type, msg, sig, status, NULL));
  EXPECT(status[0] == BPPP_RP_OPEN_MISMATCH);
  CHECK(bppp_rp_excess_verify_batch(rp, ROWS, coms, 1, sum_start, entries, NNZ, claim_amount, claim_type, msg, sig, vseed, &accept, status, NULL));
  EXPECT(accept == 0 && status[0] == BPPP_RP_OPEN_MISMATCH);
  printf("an output off by one: MISMATCH, reject\n");

  printf("excess c client ok: 2 inputs - 2 outputs - fee balanced under a %d-byte signature, the blinding sum never shown\n", (int)BPPP_RP_EXCESS_SIG_BYTES);
  bppp_rp_destroy(rp);
  free(coms);
  bppp_ctx_destroy(ctx);
  return 0;
}
