/* rp_one_sided.c — a one-sided receive from plain C99: outputs sealed to a view key, and the scan that finds them again.
 *
 *   setup    the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded)
 *   keys     bppp_rp_excess_keys: the view key A = a B of the wallet's view secret a, and the key of somebody else
 *   seal     bppp_rp_seal: two outputs to A and one to the other key; each comes back with the blinding to commit with
 *   prove    bppp_rp_prove_batch with those blindings, bppp_rp_verify_batch accepts: nothing changes for the prover
 *   scan     bppp_rp_scan under a over four rows: the two, the foreign one, and the first again with one memo bit flipped; the verdicts and the
 *            recovered amounts are printed, and the recovered blindings open the commitments (bppp_rp_open_each)
 *
 * The secrets are fixed numbers so that the run prints the same lines every time: a wallet derives a and every r from its seed or draws them.
 * Build and run (tests/test_gpu_c_client_one_sided.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_one_sided.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_one_sided
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
  enum { B = 3, ROWS = 4, PLEN = 16, SEAL = BPPP_RP_SEAL_BYTES(1) };
  static const char seed_text[] = "test points";
  static const char *names[4] = {"foreign", "owned", "bad hint", "tag only"};
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  uint64_t secrets[2][4] = {{0x1122334455667788ull, 0x99AABBCCDDEEFF00ull, 0x0F1E2D3C4B5A6978ull, 0x0123456789ABCDEFull},     /* a: the wallet's view secret */
                            {0x0807060504030201ull, 0x100F0E0D0C0B0A09ull, 0x1817161514131211ull, 0x201F1E1D1C1B1A19ull}};    /* somebody else's */
  uint64_t eph[B][4], amounts[B][1][4], types[B][1][4], blinds[B][1][4];
  uint64_t got_amounts[ROWS][1][4], got_blinds[ROWS][1][4];
  uint8_t keys[2][BPPP_RP_EXCESS_KEY_BYTES], view_keys[B][BPPP_RP_EXCESS_KEY_BYTES], seals[B][SEAL], scan_seals[ROWS][SEAL];
  uint8_t prefix[B * PLEN], vseed[32], *coms, *proofs, *scan_coms;
  uint32_t seal_status[B], scan_status[ROWS], open_status[2];
  size_t nowned = 0;
  int accept = -1, b, k;

  CHECK(bppp_ctx_create(0, &ctx));
  memset(&range, 0, sizeof range);
  range.base = 16; range.flags = BPPP_RP_OUTPUT; range.max[1] = 1;          /* [0, 2^64) */
  CHECK(bppp_rp_create_seeded(ctx, 1, 0, &range, 1, NULL, 0, (const uint8_t *)seed_text, sizeof seed_text - 1, NULL, &rp));
  CHECK(bppp_rp_info(rp, &shp));

  CHECK(bppp_rp_excess_keys(rp, 2, &secrets[0][0], &keys[0][0], NULL));     /* A = a B, as 33 bytes */
  memcpy(view_keys[0], keys[0], sizeof keys[0]);
  memcpy(view_keys[1], keys[0], sizeof keys[0]);
  memcpy(view_keys[2], keys[1], sizeof keys[1]);

  memset(amounts, 0, sizeof amounts);
  memset(types, 0, sizeof types);
  amounts[0][0][0] = 1000000;
  amounts[1][0][0] = 0x0123456789ABCDEFull;
  amounts[2][0][0] = 42;
  for (b = 0; b < B; b++) {
    char tmp[32];
    for (k = 0; k < 4; k++) eph[b][k] = 0x0101010101010101ull * (uint64_t)(16 * b + k + 1);      /* r_b: below 2^255 < n, not zero */
    snprintf(tmp, sizeof tmp, "one-sided%07d", b);
    memcpy(prefix + b * PLEN, tmp, PLEN);
  }
  memset(vseed, 7, sizeof vseed);
  coms = (uint8_t *)calloc(B, shp.coms_bytes);
  proofs = (uint8_t *)calloc(B, shp.proof_bytes);
  scan_coms = (uint8_t *)calloc(ROWS, shp.coms_bytes);
  EXPECT(coms && proofs && scan_coms);

  CHECK(bppp_rp_seal(rp, B, &view_keys[0][0], &eph[0][0], &amounts[0][0][0], &types[0][0][0], &seals[0][0], &blinds[0][0][0], seal_status));
  for (b = 0; b < B; b++) EXPECT(seal_status[b] == BPPP_RP_SEAL_OK);

  /* the sender proves with the blindings the seal derived: the prover sees nothing new */
  CHECK(bppp_rp_prove_batch(rp, B, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], prefix, PLEN, coms, proofs));
  CHECK(bppp_rp_verify_batch(rp, B, coms, proofs, vseed, &accept, NULL, NULL, NULL));
  EXPECT(accept == 1);

  /* the receiver, later and with nothing but a: rows 0 and 1 are its own, row 2 is not, row 3 is row 0 with a damaged memo */
  memcpy(scan_coms, coms, B * shp.coms_bytes);
  memcpy(scan_coms + 3 * shp.coms_bytes, coms, shp.coms_bytes);
  memcpy(scan_seals, seals, sizeof seals);
  memcpy(scan_seals[3], seals[0], SEAL);
  scan_seals[3][34 + 31] ^= 1;
  CHECK(bppp_rp_scan(rp, secrets[0], ROWS, scan_coms, &scan_seals[0][0], scan_status, &got_amounts[0][0][0], NULL, &got_blinds[0][0][0], &nowned));
  for (b = 0; b < ROWS; b++) {
    EXPECT(scan_status[b] < 4);
    if (scan_status[b] == BPPP_RP_SCAN_OWNED) printf("row %d: owned, amount %llu\n", b, (unsigned long long)got_amounts[b][0][0]);
    else printf("row %d: %s\n", b, names[scan_status[b]]);
  }
  EXPECT(nowned == 2 && scan_status[0] == BPPP_RP_SCAN_OWNED && scan_status[1] == BPPP_RP_SCAN_OWNED);
  EXPECT(scan_status[2] == BPPP_RP_SCAN_FOREIGN && scan_status[3] == BPPP_RP_SCAN_TAG_ONLY);
  EXPECT(memcmp(got_amounts, amounts, 2 * sizeof amounts[0]) == 0 && memcmp(got_blinds, blinds, 2 * sizeof blinds[0]) == 0);
  for (k = 0; k < 4; k++) EXPECT(!got_amounts[2][0][k] && !got_blinds[2][0][k] && !got_amounts[3][0][k] && !got_blinds[3][0][k]);
  CHECK(bppp_rp_open_each(rp, 2, scan_coms, &got_amounts[0][0][0], &types[0][0][0], &got_blinds[0][0][0], open_status));
  EXPECT(open_status[0] == BPPP_RP_OPEN_OK && open_status[1] == BPPP_RP_OPEN_OK);

  printf("one-sided c client ok: %d outputs sealed in %d bytes each and proved; %zu of %d scanned rows owned, their openings recovered\n", (int)B, (int)SEAL, nowned,
         (int)ROWS);
  bppp_rp_destroy(rp);
  free(coms); free(proofs); free(scan_coms);
  bppp_ctx_destroy(ctx);
  return 0;
}
