/*
 * index_blocks.c — what a node holds is a pool, not a chain: index it on the GPU.
 *
 * The reference keeps every block it has seen, of every rival and every fork,
 * in map<string,Block> node_blocks, in the order they arrived, and walks it by
 * previous_block_hash (sanity_test, verify_chain_indexes, look_for_block:
 * node.cpp:40-148).  This example makes such a pool: at every height three
 * rivals mine on the current tip (one pow_mine_batch call; node.cpp:292-299 for
 * the templates), all three sealed blocks are kept and the one that needed the
 * fewest trials becomes the next tip.  The pool is shuffled, pow_index_blocks
 * finds every block's parent, audits the chain under every block and picks the
 * winning tip, and the chain under that tip, followed along parent[], goes
 * through pow_verify_chain once more.
 *
 *   cc -std=c11 -I include examples/index_blocks.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o index_blocks && ./index_blocks [heights] [difficulty] [pool-dump]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pow_gpu.h"

#define RIVALS 3

#define CHECK(x)                                                                   \
  do {                                                                             \
    int rc_ = (x);                                                                 \
    if (rc_ < 0) {                                                                 \
      fprintf(stderr, "%s failed (%d): %s\n", #x, rc_, pow_last_error());          \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

int main(int argc, char** argv) {
  const int heights = argc > 1 ? atoi(argv[1]) : 10;
  const unsigned diff = argc > 2 ? (unsigned)atoi(argv[2]) : 9;
  const char* dump = argc > 3 ? argv[3] : NULL;
  if (heights < 1 || heights > 1000) return fprintf(stderr, "1 to 1000 heights\n"), 2;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));
  CHECK(pow_warmup(ctx));

  const size_t n = 1 + (size_t)RIVALS * (size_t)heights;
  pow_block* pool = calloc(n, sizeof(pow_block));
  const uint64_t window = diff + 7 < 32 ? 1ull << (diff + 7) : 1ull << 32;
  const uint64_t t0 = 1700000000ull;

  /* the root: an empty previous_block_hash, sealed like any block so that it has a name */
  pow_block tmpl[RIVALS];
  uint64_t ctr[RIVALS];
  size_t solved = 0;
  memset(tmpl, 0, sizeof tmpl);
  tmpl[0].difficulty = diff;
  tmpl[0].created_at = t0;
  CHECK(pow_mine_batch(ctx, tmpl, 1, diff, 0, window, NULL, 0, &pool[0], ctr, &solved, NULL));
  if (solved != 1) return fprintf(stderr, "the root's window held no solution\n"), 1;

  size_t tip = 0;
  for (int h = 0; h < heights; ++h) {
    for (int r = 0; r < RIVALS; ++r) { /* node.cpp:292-299 */
      tmpl[r] = pool[tip];
      tmpl[r].index = pool[tip].index + 1;
      tmpl[r].node_owner_number = (uint32_t)r;
      tmpl[r].difficulty = diff;
      tmpl[r].created_at = t0 + 1 + (uint64_t)(RIVALS * h + r);
      memcpy(tmpl[r].previous_block_hash, pool[tip].block_hash, POW_HASH_SIZE);
    }
    pow_block* out = &pool[1 + RIVALS * (size_t)h];
    CHECK(pow_mine_batch(ctx, tmpl, RIVALS, diff, 0, window, NULL, 0, out, ctr, &solved, NULL));
    if (solved != RIVALS) return fprintf(stderr, "height %d: a rival's window held no solution\n", h + 1), 1;
    int won = 0;
    for (int r = 1; r < RIVALS; ++r)
      if (ctr[r] < ctr[won]) won = r;
    tip = 1 + RIVALS * (size_t)h + (size_t)won;
  }

  /* the order of arrival is anybody's: Fisher-Yates with a fixed generator */
  uint32_t lcg = 2463534242u;
  for (size_t i = n - 1; i > 0; --i) {
    lcg = lcg * 1664525u + 1013904223u;
    const size_t j = (size_t)(lcg >> 8) % (i + 1);
    const pow_block t = pool[i];
    pool[i] = pool[j];
    pool[j] = t;
  }
  if (dump) {
    FILE* f = fopen(dump, "wb");
    if (!f || fwrite(pool, sizeof(pow_block), n, f) != n || fclose(f) != 0) return fprintf(stderr, "cannot write %s\n", dump), 1;
  }

  uint8_t* status = calloc(n, 1);
  uint32_t* parent = calloc(n, sizeof(uint32_t));
  uint32_t* depth = calloc(n, sizeof(uint32_t));
  uint32_t* n_bad = calloc(n, sizeof(uint32_t));
  size_t best = SIZE_MAX;
  const int rc = pow_index_blocks(ctx, pool, n, diff, status, parent, depth, n_bad, &best);
  CHECK(rc);
  pow_stats st;
  CHECK(pow_get_stats(ctx, &st));
  size_t roots = 0, tips = 0;
  uint8_t* has_child = calloc(n, 1);
  for (size_t i = 0; i < n; ++i) {
    roots += parent[i] == POW_POOL_ROOT;
    if (parent[i] < n) has_child[parent[i]] = 1;
  }
  for (size_t i = 0; i < n; ++i) tips += !has_child[i];
  free(has_child);
  printf("pool of %zu blocks: %zu root, %zu tips, %s; %u launches, %.3f ms on the GPU\n", n, roots, tips,
         rc == 1 ? "no block flagged" : "some blocks flagged", st.launches, st.kernel_ms);
  if (rc != 1 || best == SIZE_MAX) return fprintf(stderr, "the pool this example mined must be sound\n"), 1;

  /* the best chain, tip first, along parent[] */
  const size_t len = depth[best];
  pow_block* chain = calloc(len, sizeof(pow_block));
  size_t at = best;
  for (size_t k = 0; k < len; ++k) {
    chain[k] = pool[at];
    printf("block %u at %zu owner %u nonce %.9s hash %s\n", pool[at].index, at, pool[at].node_owner_number, pool[at].nonce,
           pool[at].block_hash);
    at = parent[at];
  }
  if (at != POW_POOL_ROOT || pool[best].index != (uint32_t)heights) return fprintf(stderr, "the best chain is not the race's\n"), 1;

  size_t first_bad = 0, bad = 0;
  const int ok = pow_verify_chain(ctx, chain, len, diff, NULL, &first_bad, &bad);
  CHECK(ok);
  if (ok != 1) return fprintf(stderr, "%zu flagged blocks, the first at %zu\n", bad, first_bad), 1;
  printf("best chain of %zu blocks at difficulty %u: valid\n", len, diff);
  free(chain);
  free(n_bad);
  free(depth);
  free(parent);
  free(status);
  free(pool);
  pow_destroy(ctx);
  return 0;
}
