/*
 * pool_above.c — looking up the tree: the live tips, what stands on a block,
 * and forgetting a block with everything built on it.
 *
 * Three rivals mine as in pool_fork.c: the first on a root, the second forks
 * off the first's second block, the third off the second's second block.  All
 * their blocks go into a pow_pool.  pow_pool_tips lists the fork tips (every
 * rank's last_block_in_chain is one); pow_pool_subtrees says for each rival's
 * first block how many blocks were built on it, how high (its confirmations)
 * and which tip above it wins; then the node rules the second rival's first
 * block out (say its created_at was outside valid_new_block's window) and
 * pow_pool_drop removes it with the whole of the second and third rivals'
 * chains that stand on it.  No parent array comes down and no walk runs on the
 * host.
 *
 *   cc -std=c11 -I include examples/pool_above.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o pool_above && ./pool_above [heights] [difficulty] [pool-dump]
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
  pow_block* blocks = calloc(n, sizeof(pow_block)); /* the root, then every rival's chain */
  uint32_t* map = calloc(n, sizeof(uint32_t));
  uint32_t* tips = calloc(n, sizeof(uint32_t));
  const uint64_t window = diff + 7 < 32 ? 1ull << (diff + 7) : 1ull << 32;
  const uint64_t t0 = 1700000000ull;

  pow_block tmpl;
  uint64_t ctr = 0;
  size_t solved = 0;
  memset(&tmpl, 0, sizeof tmpl);
  tmpl.difficulty = diff;
  tmpl.created_at = t0;
  CHECK(pow_mine_batch(ctx, &tmpl, 1, diff, 0, window, NULL, 0, &blocks[0], &ctr, &solved, NULL));
  if (solved != 1) return fprintf(stderr, "the root's window held no solution\n"), 1;
  for (int r = 0; r < RIVALS; ++r) {
    const pow_block* on = r == 0 ? &blocks[0] : &blocks[1 + (size_t)(r - 1) * heights + (FORK_AT - 1)];
    for (int h = 0; h < heights; ++h) {
      pow_block* out = &blocks[1 + (size_t)r * heights + h];
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
  if (dump) { /* the pool as it is fed */
    FILE* f = fopen(dump, "wb");
    if (!f || fwrite(blocks, sizeof(pow_block), n, f) != n || fclose(f) != 0) return fprintf(stderr, "cannot write %s\n", dump), 1;
  }

  pow_pool* pool = NULL;
  pow_pool_info info;
  pow_stats st;
  CHECK(pow_pool_open(ctx, diff, 0, &pool));
  CHECK(pow_pool_add(pool, blocks, n, &info));
  if (info.n_flagged || info.best == POW_POOL_NONE) return fprintf(stderr, "the pool this example mined must be sound\n"), 1;

  size_t n_tips = 0;
  CHECK(pow_pool_tips(pool, POW_TIPS_SOUND_ONLY, tips, n, &n_tips));
  CHECK(pow_get_stats(ctx, &st));
  printf("%zu sound tips:", n_tips);
  for (size_t k = 0; k < n_tips; ++k) printf(" %u", tips[k]);
  printf("; %u launches\n", st.launches);

  uint32_t roots[RIVALS], size[RIVALS], height[RIVALS], best[RIVALS], best_index[RIVALS];
  for (int r = 0; r < RIVALS; ++r) roots[r] = 1u + (uint32_t)(r * heights); /* each rival's first block */
  CHECK(pow_pool_subtrees(pool, roots, RIVALS, size, height, best, best_index, NULL, NULL));
  CHECK(pow_get_stats(ctx, &st));
  for (int r = 0; r < RIVALS; ++r)
    printf("rival %d's first block %u: %u blocks on it, %u confirmations, best tip above it %d at index %u\n", r, roots[r],
           size[r], height[r], best[r] == POW_POOL_NONE ? -1 : (int)best[r], best_index[r]);
  printf("subtrees: %u launches\n", st.launches);

  const uint32_t out = roots[1]; /* ruled out: the second rival's first block */
  const int rc = pow_pool_drop(pool, &out, 1, map, &info);
  CHECK(rc);
  CHECK(pow_get_stats(ctx, &st));
  size_t gone = 0;
  for (size_t i = 0; i < n; ++i) gone += map[i] == POW_POOL_NONE;
  printf("dropped block %u and what stood on it: %zu blocks gone, size %u flagged %u best %d index %u capacity %u; %u launches\n",
         out, gone, info.size, info.n_flagged, info.best == POW_POOL_NONE ? -1 : (int)info.best, info.best_index,
         info.capacity, st.launches);
  CHECK(pow_pool_tips(pool, 0, tips, n, &n_tips));
  printf("%zu tips left:", n_tips);
  for (size_t k = 0; k < n_tips; ++k) printf(" %u", tips[k]);
  printf("\npool of %zu blocks at difficulty %u: %u left, sound %d\n", n, diff, info.size, rc);
  pow_pool_close(pool);
  free(tips);
  free(map);
  free(blocks);
  pow_destroy(ctx);
  return 0;
}
