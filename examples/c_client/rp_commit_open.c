/* rp_commit_open.c — commitments before a proof exists, and checking their openings, from plain C99.
 *
 *   setup    the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded)
 *   commit   bppp_rp_commit_batch: the commitments files of two rows — what a receiver hands a sender, before any transaction
 *   open     bppp_rp_open_each and bppp_rp_open_batch accept the true (amount, type, blinding); with one amount changed
 *            the first reports BPPP_RP_OPEN_MISMATCH at that commitment and the second rejects with the same verdicts
 *   prove    bppp_rp_prove_batch on the same rows writes the same commitments files, byte for byte
 *
 * Build and run (tests/test_gpu_c_client_commit_open.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_commit_open.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_commit_open
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
  enum { B = 2, PLEN = 16 };
  static const char seed_text[] = "test points";
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  uint64_t amounts[B][1][4], types[B][1][4], blinds[B][1][4];
  uint8_t prefix[B * PLEN], vseed[32], *coms, *proved_coms, *proofs;
  uint32_t commit_status[B], open_status[B];
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
  amounts[0][0][0] = 1000000;
  amounts[1][0][0] = 0x0123456789ABCDEFull;
  ur = fopen("/dev/urandom", "rb");                                          /* blindings and the checker's weights: fresh randomness */
  EXPECT(ur && fread(blinds, 1, sizeof blinds, ur) == sizeof blinds && fread(vseed, 1, 32, ur) == 32);
  fclose(ur);
  for (b = 0; b < B; b++) {
    char tmp[32];
    blinds[b][0][3] >>= 1;                                                   /* < 2^255 < n */
    snprintf(tmp, sizeof tmp, "commit   %07d", b);
    memcpy(prefix + b * PLEN, tmp, PLEN);
  }
  coms = (uint8_t *)calloc(B, shp.coms_bytes);
  proved_coms = (uint8_t *)calloc(B, shp.coms_bytes);
  proofs = (uint8_t *)calloc(B, shp.proof_bytes);
  EXPECT(coms && proved_coms && proofs);

  CHECK(bppp_rp_commit_batch(rp, B, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], commit_status, coms));
  EXPECT(commit_status[0] == BPPP_RP_WIT_OK && commit_status[1] == BPPP_RP_WIT_OK);

  CHECK(bppp_rp_open_each(rp, B, coms, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], open_status));
  EXPECT(open_status[0] == BPPP_RP_OPEN_OK && open_status[1] == BPPP_RP_OPEN_OK);
  CHECK(bppp_rp_open_batch(rp, B, coms, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], vseed, &accept, open_status, NULL));
  EXPECT(accept == 1 && open_status[0] == BPPP_RP_OPEN_OK && open_status[1] == BPPP_RP_OPEN_OK);

  amounts[1][0][0] ^= 1;                                                     /* a claim that is off by one */
  CHECK(bppp_rp_open_each(rp, B, coms, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], open_status));
  EXPECT(open_status[0] == BPPP_RP_OPEN_OK && open_status[1] == BPPP_RP_OPEN_MISMATCH);
  CHECK(bppp_rp_open_batch(rp, B, coms, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], vseed, &accept, open_status, NULL));
  EXPECT(accept == 0 && open_status[0] == BPPP_RP_OPEN_OK && open_status[1] == BPPP_RP_OPEN_MISMATCH);
  amounts[1][0][0] ^= 1;

  CHECK(bppp_rp_prove_batch(rp, B, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], prefix, PLEN, proved_coms, proofs));
  EXPECT(memcmp(coms, proved_coms, B * shp.coms_bytes) == 0);

  printf("commit / open c client ok: %d commitments files of %zu bytes committed, opened, refused when off by one, and equal to the prover's\n", (int)B,
         shp.coms_bytes);
  bppp_rp_destroy(rp);
  free(coms); free(proved_coms); free(proofs);
  bppp_ctx_destroy(ctx);
  return 0;
}
