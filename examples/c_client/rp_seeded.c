/* rp_seeded.c — a setup named as the reference's schemas name it, by its "basisSeed", from plain C99.
 *
 *   basis   bppp_rp_create_seeded derives h : g : hs ++ gs from the string "test points" on the GPU (getPoints, app/Main.hs:68-72) — the
 *           seed of every example the reference ships, so these proofs belong to a schema anybody can reproduce
 *   prove   two proofs of the examples/64bit schema (one 64-bit value, base 16, an output; inner-product argument, the CLI's default)
 *   verify  bppp_rp_verify_batch on the two files
 *   print   the first point of the stream (h), from bppp_points_from_seed, as "basis[0] <x> <y>" in hexadecimal
 *
 * Build and run (tests/test_gpu_c_client_seeded.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_seeded.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_seeded
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
  const uint8_t *seed = (const uint8_t *)seed_text;
  const size_t seed_len = sizeof seed_text - 1;
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  uint64_t amounts[B][1][4], types[B][1][4], blinds[B][1][4], first[8], next = 0, x0[4];
  uint8_t prefix[B * PLEN], vseed[32], *coms, *proofs;
  uint32_t status[B];
  int accept = -1, b, k;
  FILE *ur;

  CHECK(bppp_ctx_create(0, &ctx));
  memset(&range, 0, sizeof range);
  range.base = 16; range.flags = BPPP_RP_OUTPUT; range.max[1] = 1;          /* [0, 2^64) */
  CHECK(bppp_rp_create_seeded(ctx, 1, 0, &range, 1, NULL, 0, seed, seed_len, NULL, &rp));
  CHECK(bppp_rp_info(rp, &shp));

  memset(amounts, 0, sizeof amounts);
  memset(types, 0, sizeof types);
  memset(blinds, 0, sizeof blinds);
  amounts[0][0][0] = 0x0123456789ABCDEFull;
  amounts[1][0][0] = ~0ull;                                                  /* the range's upper end */
  ur = fopen("/dev/urandom", "rb");                                          /* blindings and the verifier's weights: fresh randomness */
  EXPECT(ur && fread(blinds, 1, sizeof blinds, ur) == sizeof blinds && fread(vseed, 1, 32, ur) == 32);
  fclose(ur);
  for (b = 0; b < B; b++) {
    char tmp[32];
    blinds[b][0][3] >>= 1;                                                   /* < 2^255 < n */
    snprintf(tmp, sizeof tmp, "seeded   %07d", b);
    memcpy(prefix + b * PLEN, tmp, PLEN);
  }
  coms = (uint8_t *)calloc(B, shp.coms_bytes);
  proofs = (uint8_t *)calloc(B, shp.proof_bytes);
  EXPECT(coms && proofs);
  CHECK(bppp_rp_prove_batch(rp, B, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], prefix, PLEN, coms, proofs));
  CHECK(bppp_rp_verify_batch(rp, B, coms, proofs, vseed, &accept, status, NULL, NULL));
  EXPECT(accept == 1 && status[0] == BPPP_RP_VALID && status[1] == BPPP_RP_VALID);

  CHECK(bppp_points_from_seed(ctx, seed, seed_len, 0, 1, first, &next));
  CHECK(bppp_seed_candidate_x(seed, seed_len, next - 1, x0));                /* the accepted candidate's x is the point's */
  EXPECT(memcmp(x0, first, 32) == 0);
  printf("basis[0] ");
  for (k = 3; k >= 0; k--) printf("%016llx", (unsigned long long)first[k]);
  printf(" ");
  for (k = 7; k >= 4; k--) printf("%016llx", (unsigned long long)first[k]);
  printf("\n");
  printf("seeded c client ok: %d proofs over the basis of \"%s\" (%zu + %zu bytes each) proved and verified\n", (int)B, seed_text, shp.coms_bytes,
         shp.proof_bytes);
  bppp_rp_destroy(rp);
  free(coms); free(proofs);
  bppp_ctx_destroy(ctx);
  return 0;
}
