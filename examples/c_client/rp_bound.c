/* rp_bound.c — range proofs tied to their transactions (per-proof transcript bindings), from plain C99.
 *
 *   setup    the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded)
 *   prove    bppp_rp_prove_bound: two transactions on ONE handle, each proof under its own 32-byte binding (here two fixed byte patterns; a
 *            service takes SHA-256 of the transaction's public data: fee, recipients, memo, chain id)
 *   verify   bppp_rp_verify_bound accepts the proofs with their bindings; with the two bindings swapped — each proof lifted into the other
 *            transaction — both are refused; and so is every proof by the unbound verifier (bindings == NULL)
 *
 * Build and run (tests/test_gpu_c_client_bound.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_bound.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_bound
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
  uint8_t prefix[B * PLEN], vseed[32], bindings[B][BPPP_RP_BINDING_BYTES], swapped[B][BPPP_RP_BINDING_BYTES], *coms, *proofs;
  uint32_t status[B];
  int accept = -1, b, i;
  FILE *ur;

  CHECK(bppp_ctx_create(0, &ctx));
  memset(&range, 0, sizeof range);
  range.base = 16; range.flags = BPPP_RP_OUTPUT; range.max[1] = 1;          /* [0, 2^64) */
  CHECK(bppp_rp_create_seeded(ctx, 0, 0, &range, 1, NULL, 0, (const uint8_t *)seed_text, sizeof seed_text - 1, "rp_bound example", &rp));
  CHECK(bppp_rp_info(rp, &shp));

  memset(amounts, 0, sizeof amounts);
  memset(types, 0, sizeof types);
  memset(blinds, 0, sizeof blinds);
  amounts[0][0][0] = 1000000;
  amounts[1][0][0] = 0x0123456789ABCDEFull;
  ur = fopen("/dev/urandom", "rb");                                          /* blindings, prover randomness and the verifier's weights: fresh */
  EXPECT(ur && fread(blinds, 1, sizeof blinds, ur) == sizeof blinds && fread(prefix, 1, sizeof prefix, ur) == sizeof prefix && fread(vseed, 1, 32, ur) == 32);
  fclose(ur);
  for (b = 0; b < B; b++) {
    blinds[b][0][3] >>= 1;                                                   /* < 2^255 < n */
    for (i = 0; i < BPPP_RP_BINDING_BYTES; i++) bindings[b][i] = (uint8_t)(b ? 0xFF - i : i);      /* raw bytes: 0x00 and 0xFF are ordinary values */
  }
  memcpy(swapped[0], bindings[1], BPPP_RP_BINDING_BYTES);
  memcpy(swapped[1], bindings[0], BPPP_RP_BINDING_BYTES);
  coms = (uint8_t *)calloc(B, shp.coms_bytes);
  proofs = (uint8_t *)calloc(B, shp.proof_bytes);
  EXPECT(coms && proofs);

  CHECK(bppp_rp_prove_bound(rp, B, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], NULL, &bindings[0][0], prefix, PLEN, coms, proofs, NULL));

  CHECK(bppp_rp_verify_bound(rp, B, coms, proofs, NULL, &bindings[0][0], vseed, &accept, status, NULL, NULL));
  printf("own bindings:     accept %d, statuses %u %u\n", accept, (unsigned)status[0], (unsigned)status[1]);
  EXPECT(accept == 1 && status[0] == BPPP_RP_VALID && status[1] == BPPP_RP_VALID);

  CHECK(bppp_rp_verify_bound(rp, B, coms, proofs, NULL, &swapped[0][0], vseed, &accept, status, NULL, NULL));
  printf("swapped bindings: accept %d, statuses %u %u\n", accept, (unsigned)status[0], (unsigned)status[1]);
  EXPECT(accept == 0 && status[0] == BPPP_RP_INVALID && status[1] == BPPP_RP_INVALID);

  CHECK(bppp_rp_verify_bound(rp, B, coms, proofs, NULL, NULL, vseed, &accept, status, NULL, NULL));
  printf("no bindings:      accept %d, statuses %u %u\n", accept, (unsigned)status[0], (unsigned)status[1]);
  EXPECT(accept == 0 && status[0] == BPPP_RP_INVALID && status[1] == BPPP_RP_INVALID);

  printf("bound c client ok: %d proofs of %zu bytes accepted under their own bindings, refused under each other's and without one\n", (int)B, shp.proof_bytes);
  bppp_rp_destroy(rp);
  free(coms); free(proofs);
  bppp_ctx_destroy(ctx);
  return 0;
}
