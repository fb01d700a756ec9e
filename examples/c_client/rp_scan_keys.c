/* rp_scan_keys.c — a scanning service from plain C99: one output set tested against the view secrets of several accounts in ONE call.
 *
 *   setup    the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded)
 *   keys     bppp_rp_excess_keys: the view keys of three accounts, and the key of somebody the service does not serve
 *   seal     bppp_rp_seal: eight outputs — two to account 0, two to account 1, none to account 2, four to the stranger — committed with the
 *            blindings the seal derived (bppp_rp_commit_batch)
 *   scan     bppp_rp_scan_keys under the three secrets: the hit list (key, row, amount) in (row, key) order, the per-row verdicts, and the recovered
 *            blindings open the commitments (bppp_rp_open_each)
 *   again    one more output is sealed to account 2 and the nine rows are scanned once more: the new hit is found
 *
 * The secrets are fixed numbers so that the run prints the same lines every time: a service holds its accounts' secrets and senders draw every r.
 * Build and run (tests/test_gpu_c_client_scan_keys.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_scan_keys.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_scan_keys
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
  enum { ACCOUNTS = 3, ROWS = 9, FIRST = 8, CAP = 8, SEAL = BPPP_RP_SEAL_BYTES(1) };
  static const char seed_text[] = "test points";
  static const char *names[4] = {"foreign", "owned", "bad hint", "tag only"};
  static const int recipient[ROWS] = {3, 0, 3, 1, 0, 3, 1, 3, 2};              /* 3: the stranger; row 8 arrives later */
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  uint64_t secrets[4][4] = {{0x1122334455667788ull, 0x99AABBCCDDEEFF00ull, 0x0F1E2D3C4B5A6978ull, 0x0123456789ABCDEFull},     /* accounts 0, 1, 2 */
                            {0x0807060504030201ull, 0x100F0E0D0C0B0A09ull, 0x1817161514131211ull, 0x201F1E1D1C1B1A19ull},
                            {0x2222222222222223ull, 0x3333333333333335ull, 0x5555555555555557ull, 0x0777777777777777ull},
                            {0x0102030405060708ull, 0x1112131415161718ull, 0x2122232425262728ull, 0x3132333435363738ull}};    /* the stranger */
  uint64_t eph[ROWS][4], amounts[ROWS][1][4], types[ROWS][1][4], blinds[ROWS][1][4];
  uint64_t got_amounts[CAP][1][4], got_blinds[CAP][1][4], hit_types[CAP][1][4];
  uint8_t keys[4][BPPP_RP_EXCESS_KEY_BYTES], view_keys[ROWS][BPPP_RP_EXCESS_KEY_BYTES], seals[ROWS][SEAL], *coms, *hit_coms;
  uint32_t seal_status[ROWS], row_status[ROWS], hit_key[CAP], hit_row[CAP], open_status[CAP];
  size_t nhits = 0, h;
  uint64_t ntag_only = 0;
  int b, k, pass;

  CHECK(bppp_ctx_create(0, &ctx));
  memset(&range, 0, sizeof range);
  range.base = 16; range.flags = BPPP_RP_OUTPUT; range.max[1] = 1;          /* [0, 2^64) */
  CHECK(bppp_rp_create_seeded(ctx, 1, 0, &range, 1, NULL, 0, (const uint8_t *)seed_text, sizeof seed_text - 1, NULL, &rp));
  CHECK(bppp_rp_info(rp, &shp));
  CHECK(bppp_rp_excess_keys(rp, 4, &secrets[0][0], &keys[0][0], NULL));

  memset(amounts, 0, sizeof amounts);
  memset(types, 0, sizeof types);
  memset(hit_types, 0, sizeof hit_types);
  for (b = 0; b < ROWS; b++) {
    memcpy(view_keys[b], keys[recipient[b]], sizeof keys[0]);
    amounts[b][0][0] = 1000 * (uint64_t)(b + 1);
    for (k = 0; k < 4; k++) eph[b][k] = 0x0101010101010101ull * (uint64_t)(16 * b + k + 1);      /* r_b: below 2^255 < n, not zero */
  }
  coms = (uint8_t *)calloc(ROWS, shp.coms_bytes);
  hit_coms = (uint8_t *)calloc(CAP, shp.coms_bytes);
  EXPECT(coms && hit_coms);
  CHECK(bppp_rp_seal(rp, ROWS, &view_keys[0][0], &eph[0][0], &amounts[0][0][0], &types[0][0][0], &seals[0][0], &blinds[0][0][0], seal_status));
  for (b = 0; b < ROWS; b++) EXPECT(seal_status[b] == BPPP_RP_SEAL_OK);
  CHECK(bppp_rp_commit_batch(rp, ROWS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], NULL, coms));

  /* the service, with the three secrets and nothing else: first the eight outputs of the block, then the nine after one more arrived */
  for (pass = 0; pass < 2; pass++) {
    const size_t rows = pass ? ROWS : FIRST, want = pass ? 5 : 4;
    CHECK(bppp_rp_scan_keys(rp, ACCOUNTS, &secrets[0][0], rows, coms, &seals[0][0], row_status, CAP, hit_key, hit_row, &got_amounts[0][0][0], NULL, &got_blinds[0][0][0], &nhits,
                            &ntag_only));
    EXPECT(nhits == want && nhits <= CAP);
    printf("scan of %zu rows under %d keys: %zu hits\n", rows, (int)ACCOUNTS, nhits);
    for (h = 0; h < nhits; h++) {
      EXPECT(hit_row[h] < rows && hit_key[h] == (uint32_t)recipient[hit_row[h]] && (h == 0 || hit_row[h - 1] < hit_row[h]));
      EXPECT(memcmp(got_amounts[h], amounts[hit_row[h]], sizeof amounts[0]) == 0 && memcmp(got_blinds[h], blinds[hit_row[h]], sizeof blinds[0]) == 0);
      memcpy(hit_coms + h * shp.coms_bytes, coms + hit_row[h] * shp.coms_bytes, shp.coms_bytes);
      printf("  hit %zu: account %u owns row %u, amount %llu\n", h, (unsigned)hit_key[h], (unsigned)hit_row[h], (unsigned long long)got_amounts[h][0][0]);
    }
    for (h = nhits; h < CAP; h++) for (k = 0; k < 4; k++) EXPECT(!hit_key[h] && !hit_row[h] && !got_amounts[h][0][k] && !got_blinds[h][0][k]);
    for (b = 0; b < (int)rows; b++) {
      EXPECT(row_status[b] < 4);
      /* a stranger's row is foreign, or, one time in 256 per key, tag only */
      EXPECT(recipient[b] == 3 ? row_status[b] == BPPP_RP_SCAN_FOREIGN || row_status[b] == BPPP_RP_SCAN_TAG_ONLY : row_status[b] == BPPP_RP_SCAN_OWNED);
      printf("  row %d: %s\n", b, names[row_status[b]]);
    }
    CHECK(bppp_rp_open_each(rp, nhits, hit_coms, &got_amounts[0][0][0], &hit_types[0][0][0], &got_blinds[0][0][0], open_status));
    for (h = 0; h < nhits; h++) EXPECT(open_status[h] == BPPP_RP_OPEN_OK);
  }
  EXPECT(hit_key[4] == 2 && hit_row[4] == 8);

  printf("scan-keys c client ok: %d rows under %d keys in one call, %zu hits, their openings recovered\n", (int)ROWS, (int)ACCOUNTS, nhits);
  bppp_rp_destroy(rp);
  free(coms); free(hit_coms);
  bppp_ctx_destroy(ctx);
  return 0;
}
