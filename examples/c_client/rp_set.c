/* rp_set.c — what a block header commits to, from plain C99: the output set as 32 bytes, a membership path, and its check by someone who holds
 * the 32 bytes alone.
 *
 *   setup    the examples/64bit schema (one 64-bit value, base 16, an output) over the basis of "test points" (bppp_rp_create_seeded)
 *   outputs  bppp_rp_commit_batch: six outputs, their commitments files the rows of the set
 *   set      bppp_rp_set_create (every node kept) and a second set that keeps its peaks alone; the files appended in two calls, four rows then two:
 *            the roots agree after each, and a third set restored from the peaks in between reaches the same root
 *   path     bppp_rp_set_paths: the path of output 2; bppp_rp_set_verify_paths accepts it under the root
 *   refused  the same path under the root before the second append (that root speaks of four rows), and with one byte of the row changed
 *
 * Build and run (tests/test_gpu_c_client_set.py does this under -m gpu):
 *   gcc -std=c99 -O2 -Iinclude examples/c_client/rp_set.c -Lbulletproofspp_amd/lib -lbppp_hip -Wl,-rpath,$PWD/bulletproofspp_amd/lib -o rp_set
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

static void print_hex(const char *what, const uint8_t *b, size_t n) {
  size_t i;
  printf("%s", what);
  for (i = 0; i < n; i++) printf("%02x", b[i]);
  printf("\n");
}

int main(void) {
  enum { ROWS = 6, FIRST = 4 };
  static const char seed_text[] = "test points";
  bppp_rp_range range;
  bppp_rp_shape shp;
  bppp_rp *rp = NULL;
  bppp_rp_set *full = NULL, *frontier = NULL, *restored = NULL;
  uint64_t amounts[ROWS][1][4], types[ROWS][1][4], blinds[ROWS][1][4], n = 0, idx = 2;
  uint8_t *coms, *row, root4[32], root6[32], other[32], peaks[64 * 32], path[64 * 32];
  uint32_t status = 9;
  size_t rb, npeaks = 0, store = 0, pb;
  int b, k, accept = -1;

  CHECK(bppp_ctx_create(0, &ctx));
  memset(&range, 0, sizeof range);
  range.base = 16; range.flags = BPPP_RP_OUTPUT; range.max[1] = 1;          /* [0, 2^64) */
  CHECK(bppp_rp_create_seeded(ctx, 1, 0, &range, 1, NULL, 0, (const uint8_t *)seed_text, sizeof seed_text - 1, NULL, &rp));
  CHECK(bppp_rp_info(rp, &shp));
  rb = shp.coms_bytes;
  memset(amounts, 0, sizeof amounts);
  memset(types, 0, sizeof types);
  for (b = 0; b < ROWS; b++) {
    amounts[b][0][0] = 1000 * (uint64_t)(b + 1);
    for (k = 0; k < 4; k++) blinds[b][0][k] = 0x0101010101010101ull * (uint64_t)(16 * b + k + 1);
  }
  coms = (uint8_t *)calloc(ROWS, rb);
  row = (uint8_t *)calloc(1, rb);
  EXPECT(coms && row);
  CHECK(bppp_rp_commit_batch(rp, ROWS, &amounts[0][0][0], &types[0][0][0], &blinds[0][0][0], NULL, coms));

  /* the first four outputs: a full store and a frontier agree */
  CHECK(bppp_rp_set_create(rp, rb, 1, &full));
  CHECK(bppp_rp_set_create(rp, rb, 0, &frontier));
  CHECK(bppp_rp_set_append(full, FIRST, coms));
  CHECK(bppp_rp_set_append(frontier, FIRST, coms));
  CHECK(bppp_rp_set_root(full, root4));
  CHECK(bppp_rp_set_root(frontier, other));
  EXPECT(memcmp(root4, other, 32) == 0);
  CHECK(bppp_rp_set_info(frontier, &n, NULL, &npeaks, NULL));
  EXPECT(n == FIRST && npeaks == 1);
  CHECK(bppp_rp_set_peaks(frontier, peaks));
  CHECK(bppp_rp_set_restore(rp, rb, n, peaks, &restored));
  printf("rows of %zu bytes\n", rb);
  print_hex("root after 4 rows: ", root4, 32);

  /* two more: every set reaches the same root, however it got there */
  CHECK(bppp_rp_set_append(full, ROWS - FIRST, coms + FIRST * rb));
  CHECK(bppp_rp_set_append(frontier, ROWS - FIRST, coms + FIRST * rb));
  CHECK(bppp_rp_set_append(restored, ROWS - FIRST, coms + FIRST * rb));
  CHECK(bppp_rp_set_root(full, root6));
  CHECK(bppp_rp_set_root(frontier, other));
  EXPECT(memcmp(root6, other, 32) == 0);
  CHECK(bppp_rp_set_root(restored, other));
  EXPECT(memcmp(root6, other, 32) == 0 && memcmp(root6, root4, 32) != 0);
  CHECK(bppp_rp_set_info(full, &n, NULL, &npeaks, &store));
  EXPECT(n == ROWS && npeaks == 2 && store >= 64 * ROWS - 64);
  print_hex("root after 6 rows: ", root6, 32);

  /* a path for output 2, checked by a holder of the root alone */
  pb = bppp_rp_set_path_bytes(n);
  EXPECT(pb == 3 * 32);
  CHECK(bppp_rp_set_paths(full, 1, &idx, path));
  CHECK(bppp_rp_set_verify_paths(rp, rb, n, root6, 1, &idx, coms + idx * rb, path, &status, &accept));
  EXPECT(accept == 1 && status == BPPP_RP_SET_OK);
  printf("path of row 2 among 6: %zu bytes, accepted\n", pb);
  /* the frontier-only set has no nodes to serve a path from */
  EXPECT(bppp_rp_set_paths(frontier, 1, &idx, path) == BPPP_ERR_ARG);

  /* the root before the second append speaks of four rows: the same path is refused there (with n = 6 the roots differ; with n = 4 the path's third hash
   * would have to be zero padding), and so is a row with one byte changed */
  CHECK(bppp_rp_set_verify_paths(rp, rb, n, root4, 1, &idx, coms + idx * rb, path, &status, &accept));
  EXPECT(accept == 0 && status == BPPP_RP_SET_MISMATCH);
  CHECK(bppp_rp_set_verify_paths(rp, rb, FIRST, root4, 1, &idx, coms + idx * rb, path, &status, &accept));
  EXPECT(accept == 0 && status != BPPP_RP_SET_OK);
  printf("the same path under the root of 4 rows: refused\n");
  memcpy(row, coms + idx * rb, rb);
  row[rb - 1] ^= 1;
  CHECK(bppp_rp_set_verify_paths(rp, rb, n, root6, 1, &idx, row, path, &status, &accept));
  EXPECT(accept == 0 && status == BPPP_RP_SET_MISMATCH);
  printf("a row with one byte changed: refused\n");

  printf("set c client ok: %d rows in two appends, one root from three sets, a path accepted and twice refused\n", (int)ROWS);
  bppp_rp_set_destroy(full); bppp_rp_set_destroy(frontier); bppp_rp_set_destroy(restored);
  bppp_rp_destroy(rp);
  free(coms); free(row);
  bppp_ctx_destroy(ctx);
  return 0;
}
