/*
 * pool_fork.c — a node's reorg: where do the old best chain and the new one part?
 *
 * When a block arrives and the best tip moves to a block that does not stand
 * on the old best, the node has to roll back the blocks of its old chain down
 * to the fork point and apply the blocks of the new one from there
 * (verificar_y_migrar_cadena, node.cpp:150-191, with find_block and
 * look_for_block, node.cpp:131-148).  This example mines a race of three
 * rivals: the first mines its chain on a root, the second forks off the
 * first's second block, the third off the second's second block, and each
 * keeps to its own fork.  Their blocks arrive one by one in a mixed order and
 * go into a pow_pool.  Whenever best moves to a block that is not a child of
 * the old best, one pow_pool_fork_points call says where the two chains part
 * and how far back that is on either side, and two pow_pool_chain calls list
 * the blocks to roll back and to apply.  No parent array comes down and no
 * walk runs on the host.
 *
 *   cc -std=c11 -I include examples/pool_fork.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o pool_fork && ./pool_fork [heights] [difficulty] [pool-dump]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pow_gpu.h"

#define RIVALS 3
#define FORK_AT 2 /* a rival forks off the block of this height of the rival before it */

#define CHECK(x)                                                                   \
  do {                                                                             \
    int rc_ = (x);                                                                 \
    if (rc_ < 0) {                                                                 \
      fprintf(stderr, "%s failed (%d): %s\n", #x, rc_, pow_last_error());          \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

int main(int argc, char** argv) {
  const int heights = argc > 1 ? atoi(argv[1]) : 6;
  const unsigned diff = argc > 2 ? (unsigned)atoi(argv[2]) : 9;
  const char* dump = argc > 3 ? argv[3] : NULL;
  if (heights < FORK_AT || heights > 1000) return fprintf(stderr, "%d to 1000 heights\n", FORK_AT), 2;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));
  CHECK(pow_warmup(ctx));

  const size_t n = 1 + (size_t)RIVALS * (size_t)heights;
  pow_block* mined = calloc(n, sizeof(pow_block));  /* the root, then every rival's chain */
  pow_block* blocks = calloc(n, sizeof(pow_block)); /* in the order of arrival */
  uint32_t* walk = calloc(n, sizeof(uint32_t));
  const uint64_t window = diff + 7 < 32 ? 1ull << (diff + 7) : 1ull << 32;
  const uint64_t t0 = 1700000000ull;

  pow_block tmpl;
  uint64_t ctr = 0;
  size_t solved = 0;
  memset(&tmpl, 0, sizeof tmpl);
  tmpl.difficulty = diff;
  tmpl.created_at = t0;
  CHECK(pow_mine_batch(ctx, &tmpl, 1, diff, 0, window, NULL, 0, &mined[0], &ctr, &solved, NULL));
  if (solved != 1) return fprintf(stderr, "the root's window held no solution\n"), 1;
  for (int r = 0; r < RIVALS; ++r) {
    const pow_block* on = r == 0 ? &mined[0] : &mined[1 + (size_t)(r - 1) * heights + (FORK_AT - 1)];
    for (int h = 0; h < heights; ++h) {
      pow_block* out = &mined[1 + (size_t)r * heights + h];
      tmpl = *on;
      tmpl.index = on->index + 1;
      tmpl.node_owner_number = (uint32_t)r;
      tmpl.difficulty = diff;
      tmpl.created_at = t0 + 1 + (uint64_t)(r * heights + h);
      memcpy(tmpl.previous_block_hash, on->block_hash, POW_HASH_SIZE);
      CHECK(pow_mine_batch(ctx, &tmpl, 1, diff, 0, window, NULL, 0, out, &ctr, &solved, NULL));
      if (solved != 1) return fprintf(stderr, "rival %d, height %d: the window held no solution\n", r, h + 1), 1;
      on = out;
    }
  }

  /* the order of arrival: a rival's blocks in their order, the rivals by turns of a fixed generator; a rival
   * starts once the block it forks off has arrived, so no block is an orphan */
  int next[RIVALS] = {0};
  uint32_t lcg = 2718281828u;
  blocks[0] = mined[0];
  for (size_t i = 1; i < n;) {
    lcg = lcg * 1664525u + 1013904223u;
    const int r = (int)((lcg >> 8) % RIVALS);
    if (next[r] == heights || (r > 0 && next[r - 1] < FORK_AT)) continue;
    blocks[i++] = mined[1 + (size_t)r * heights + next[r]++];
  }
  if (dump) { /* the pool as it is fed */
    FILE* f = fopen(dump, "wb");
    if (!f || fwrite(blocks, sizeof(pow_block), n, f) != n || fclose(f) != 0) return fprintf(stderr, "cannot write %s\n", dump), 1;
  }

  pow_pool* pool = NULL;
  CHECK(pow_pool_open(ctx, diff, 0, &pool));
  pow_pool_info info;
  pow_stats st;
  uint32_t best = POW_POOL_NONE;
  unsigned reorgs = 0;
  for (size_t i = 0; i < n; ++i) {
    CHECK(pow_pool_add(pool, &blocks[i], 1, &info));
    if (info.n_flagged || info.best == POW_POOL_NONE) return fprintf(stderr, "the pool this example mined must be sound\n"), 1;
    const uint32_t old = best;
    best = info.best;
    if (best == old || old == POW_POOL_NONE) continue;
    uint32_t parent = 0;
    CHECK(pow_pool_read(pool, best, 1, NULL, &parent, NULL, NULL));
    if (parent == old) continue; /* the chain grew by its next block: nothing to roll back */
    uint32_t at = 0, back_old = 0, back_new = 0;
    size_t len = 0;
    CHECK(pow_pool_fork_points(pool, &old, &best, 1, &at, &back_old, &back_new));
    CHECK(pow_get_stats(ctx, &st));
    printf("add %zu: best %u -> %u: fork point %d, %u back, %u forward; %u launches\n", i, old, best,
           at == POW_POOL_NONE ? -1 : (int)at, back_old, back_new, st.launches);
    CHECK(pow_pool_chain(pool, old, back_old, walk, &len)); /* tip first: the order to undo them in */
    CHECK(pow_get_stats(ctx, &st));
    if (len != back_old) return fprintf(stderr, "the old chain is %zu blocks above the fork point, not %u\n", len, back_old), 1;
    printf("  roll back");
    for (size_t k = 0; k < len; ++k) printf(" %u", walk[k]);
    printf("; %u launches\n", st.launches);
    CHECK(pow_pool_chain(pool, best, back_new, walk, &len));
    CHECK(pow_get_stats(ctx, &st));
    if (len != back_new) return fprintf(stderr, "the new chain is %zu blocks above the fork point, not %u\n", len, back_new), 1;
    printf("  apply");
    for (size_t k = len; k > 0; --k) printf(" %u", walk[k - 1]); /* the fork point's child first */
    printf("; %u launches\n", st.launches);
    ++reorgs;
  }
  pow_pool_lift_info lift;
  CHECK(pow_pool_lift_get_info(pool, &lift));
  printf("pool of %zu blocks fed one by one at difficulty %u: %u reorgs; best %u at index %u; table of %u rows, %llu bytes\n",
         n, diff, reorgs, info.best, info.best_index, lift.rows, (unsigned long long)lift.bytes);
  pow_pool_close(pool);
  free(walk);
  free(blocks);
  free(mined);
  pow_destroy(ctx);
  return 0;
}
