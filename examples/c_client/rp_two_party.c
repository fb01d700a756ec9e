/* rp_two_party.c — a sender and a receiver sign ONE transaction together; neither learns the other's blindings.  Plain C99.
 *
 *   setup     the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded)
 *   tx        the sender spends I into the receiver's output Out and its own change Ch with fee f.  The sender knows the blindings of I and Ch, the
 *             receiver that of Out: e_sender = bl (Ch) - bl (I), e_receiver = bl (Out), and nobody holds their sum
 *   round 1   each party states its key e_i B (bppp_rp_excess_keys) and its public nonce (bppp_rp_excess_part_nonces), under aux of its own
 *   sender    aggregates the two nonces and the two keys (bppp_rp_excess_part_aggregate) and hands the aggregates to the receiver
 *   round 2   each party signs its part (bppp_rp_excess_part_sign); the sender adds the partials up (bppp_rp_excess_part_combine)
 *   check     the 65 bytes are an ordinary excess signature: bppp_rp_excess_verify_keys_each reports OK under the aggregated key, and
 *             bppp_rp_excess_verify_each reports OK against the pool - I + Ch + Out with the fee as the public claim
 *   blame     with the receiver's partial altered by one the combined signature is MISMATCH, and bppp_rp_excess_part_verify names the
 *             receiver's part alone
 *
 * Build and run (tests/test_gpu_c_client_two_party.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_two_party.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_two_party
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
  enum { I = 0, CH = 1, OUT = 2, COMS = 3, SENDER = 0, RECEIVER = 1, PARTIES = 2 };
  static const char seed_text[] = "test points";
  static const uint64_t fee = 500;
  /* what each party can add up on its own: the sender - I + Ch, the receiver Out */
  static const uint32_t p_start[3] = {0, 2, 3}, p_entries[3] = {I | SUB, CH, OUT};
  /* the transaction as a checker sees it: one sum over the pool of three files */
  static const uint32_t sum_start[2] = {0, 3}, entries[3] = {I | SUB, CH, OUT};
  static const uint32_t part_start[2] = {0, PARTIES};
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  uint64_t amounts[COMS][1][4], types[COMS][1][4], blinds[COMS][1][4];
  uint64_t p_amount[PARTIES][4], p_type[PARTIES][4], e[PARTIES][4], claim_amount[4], claim_type[4];
  uint8_t aux[PARTIES][32], msg[32];
  uint8_t keys[PARTIES][BPPP_RP_EXCESS_KEY_BYTES], pubnonces[PARTIES][BPPP_RP_EXCESS_PUBNONCE_BYTES], partials[PARTIES][BPPP_RP_EXCESS_PARTIAL_BYTES];
  uint8_t agg_nonce[BPPP_RP_EXCESS_PUBNONCE_BYTES], agg_key[BPPP_RP_EXCESS_KEY_BYTES], agg_key2[BPPP_RP_EXCESS_KEY_BYTES], sig[BPPP_RP_EXCESS_SIG_BYTES];
  uint8_t *coms;
  uint32_t commit_status[COMS], kstatus[PARTIES], status[PARTIES], sum_status[1];
  int b;
  FILE *ur;

  CHECK(bppp_ctx_create(0, &ctx));
  memset(&range, 0, sizeof range);
  range.base = 16; range.flags = BPPP_RP_OUTPUT; range.max[1] = 1;          /* [0, 2^64) */
  CHECK(bppp_rp_create_seeded(ctx, 1, 0, &range, 1, NULL, 0, (const uint8_t *)seed_text, sizeof seed_text - 1, NULL, &rp));
  CHECK(bppp_rp_info(rp, &shp));

  memset(amounts, 0, sizeof amounts);
  memset(types, 0, sizeof types);
  amounts[I][0][0] = 1000000;
  amounts[OUT][0][0] = 600000; amounts[CH][0][0] = 1000000 - 600000 - fee;
  ur = fopen("/dev/urandom", "rb");                                          /* the blindings, FRESH aux for each party and session, the transaction */
  EXPECT(ur && fread(blinds, 1, sizeof blinds, ur) == sizeof blinds && fread(aux, 1, sizeof aux, ur) == sizeof aux && fread(msg, 1, 32, ur) == 32);
  fclose(ur);
  for (b = 0; b < COMS; b++) blinds[b][0][3] >>= 1;                          /* < 2^255 < n */
  coms = (uint8_t *)calloc(COMS, shp.coms_bytes);
  EXPECT(coms != NULL);
  CHECK(bppp_rp_commit_batch(rp, COMS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], commit_status, coms));
  for (b = 0; b < COMS; b++) EXPECT(commit_status[b] == BPPP_RP_WIT_OK);
  /* here the two blinding parts come out of one call for brevity; each party adds up its own rows and never shows the result */
  CHECK(bppp_rp_tally_claims(rp, COMS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], PARTIES, p_start, p_entries, 3, &p_amount[0][0], &p_type[0][0], &e[0][0]));

  /* round 1: each party on its own, with its own aux */
  CHECK(bppp_rp_excess_keys(rp, PARTIES, &e[0][0], &keys[0][0], kstatus));
  for (b = 0; b < PARTIES; b++) {
    CHECK(bppp_rp_excess_part_nonces(rp, 1, e[b], msg, aux[b], pubnonces[b], status));
    EXPECT(kstatus[b] == BPPP_RP_EXCESS_OK && status[0] == BPPP_RP_EXCESS_OK);
  }
  printf("round 1: two keys of %d bytes, two public nonces of %d bytes\n", (int)BPPP_RP_EXCESS_KEY_BYTES, (int)BPPP_RP_EXCESS_PUBNONCE_BYTES);

  /* the sender aggregates; no secret is needed */
  CHECK(bppp_rp_excess_part_aggregate(rp, 1, PARTIES, part_start, &pubnonces[0][0], &keys[0][0], agg_nonce, agg_key, sum_status));
  EXPECT(sum_status[0] == BPPP_RP_EXCESS_OK);
  printf("aggregate: OK\n");

  /* round 2: each party signs its part under the same aux as in round 1, once */
  for (b = 0; b < PARTIES; b++) {
    CHECK(bppp_rp_excess_part_sign(rp, 1, e[b], msg, aux[b], agg_nonce, agg_key, partials[b], status));
    EXPECT(status[0] == BPPP_RP_EXCESS_OK);
  }
  memset(e, 0, sizeof e);
  CHECK(bppp_rp_excess_part_combine(rp, 1, PARTIES, part_start, &pubnonces[0][0], &keys[0][0], &partials[0][0], msg, sig, agg_key2, sum_status));
  EXPECT(sum_status[0] == BPPP_RP_EXCESS_OK && memcmp(agg_key, agg_key2, sizeof agg_key) == 0);
  printf("round 2: two partials of %d bytes combined into one signature of %d bytes\n", (int)BPPP_RP_EXCESS_PARTIAL_BYTES, (int)BPPP_RP_EXCESS_SIG_BYTES);

  /* anyone: the signature under the aggregated key, and against the pool with the fee as the public claim */
  CHECK(bppp_rp_excess_verify_keys_each(rp, 1, agg_key, msg, sig, status));
  EXPECT(status[0] == BPPP_RP_OPEN_OK);
  printf("verify_keys_each: OK under the aggregated key\n");
  claim_amount[0] = (uint64_t)0 - fee; claim_amount[1] = claim_amount[2] = claim_amount[3] = ~(uint64_t)0;       /* minus the fee, in two's complement */
  memset(claim_type, 0, sizeof claim_type);
  CHECK(bppp_rp_excess_verify_each(rp, COMS, coms, 1, sum_start, entries, 3, claim_amount, claim_type, msg, sig, status, NULL));
  EXPECT(status[0] == BPPP_RP_OPEN_OK);
  printf("verify_each: OK against the pool with the fee\n");

  /* the receiver's partial altered by one: the signature fails, and the partial check says whose part it was */
  partials[RECEIVER][7] ^= 1;
  CHECK(bppp_rp_excess_part_combine(rp, 1, PARTIES, part_start, &pubnonces[0][0], &keys[0][0], &partials[0][0], msg, sig, NULL, sum_status));
  EXPECT(sum_status[0] == BPPP_RP_EXCESS_OK);
  CHECK(bppp_rp_excess_verify_keys_each(rp, 1, agg_key, msg, sig, status));
  EXPECT(status[0] == BPPP_RP_OPEN_MISMATCH);
  CHECK(bppp_rp_excess_part_verify(rp, 1, PARTIES, part_start, &pubnonces[0][0], &keys[0][0], &partials[0][0], msg, status, sum_status));
  EXPECT(sum_status[0] == BPPP_RP_EXCESS_OK && status[SENDER] == BPPP_RP_OPEN_OK && status[RECEIVER] == BPPP_RP_OPEN_MISMATCH);
  printf("a partial altered by one: MISMATCH, part_verify names the receiver alone\n");

  printf("two-party c client ok: one signature from two parties who never shared a blinding\n");
  bppp_rp_destroy(rp);
  free(coms);
  bppp_ctx_destroy(ctx);
  return 0;
}
