/*
 * pool_prune.c — a node that keeps its pool open forgets the forks that lost.
 *
 * The reference never migrates to a fork more than VALIDATION_BLOCKS (5)
 * behind the tip (verificar_y_migrar_cadena), yet node_blocks keeps every
 * loser for ever.  This example mines the forked pool of
 * examples/index_blocks.c (three rivals on the current tip at every height,
 * all three kept: two of every three blocks are losers), shuffles it and feeds
 * it to a pow_pool.  It asks which blocks lie on the chain under the winning
 * tip (pow_pool_mark), then prunes: every sound block within five heights of
 * the tip is a seed, and everything that is not on a walk from a seed goes
 * (pow_pool_prune).  The host's own struct array is compacted with the map the
 * prune returns, and the next block is mined on the tip and added: the pool
 * goes on as if it had only ever held the survivors.
 *
 *   cc -std=c11 -I include examples/pool_prune.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o pool_prune && ./pool_prune [heights] [difficulty] [pool-dump]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pow_gpu.h"

#define RIVALS 3
#define VALIDATION_BLOCKS 5

#define CHECK(x)                                                                   \
  do {                                                                             \
    int rc_ = (x);                                                                 \
    if (rc_ < 0) {                                                                 \
      fprintf(stderr, "%s failed (%d): %s\n", #x, rc_, pow_last_error());          \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

static void print_info(const char* what, const pow_pool_info* info, const pow_stats* st) {
  printf("%s: size %u flagged %u best %d index %u rehashed %u capacity %u slots %u; %u launches\n", what, info->size,
         info->n_flagged, info->best == POW_POOL_NONE ? -1 : (int)info->best, info->best_index, info->rehashed,
         info->capacity, info->slots, st->launches);
}

int main(int argc, char** argv) {
  const int heights = argc > 1 ? atoi(argv[1]) : 10;
  const unsigned diff = argc > 2 ? (unsigned)atoi(argv[2]) : 9;
  const char* dump = argc > 3 ? argv[3] : NULL;
  if (heights < 1 || heights > 1000) return fprintf(stderr, "1 to 1000 heights\n"), 2;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));
  CHECK(pow_warmup(ctx));

  const size_t n = 1 + (size_t)RIVALS * (size_t)heights;
  pow_block* blocks = calloc(n + 1, sizeof(pow_block)); /* and the block mined after the prune */
  const uint64_t window = diff + 7 < 32 ? 1ull << (diff + 7) : 1ull << 32;
  const uint64_t t0 = 1700000000ull;

  /* the root, then three rivals per height on the current tip (node.cpp:292-299) */
  pow_block tmpl[RIVALS];
  uint64_t ctr[RIVALS];
  size_t solved = 0;
  memset(tmpl, 0, sizeof tmpl);
  tmpl[0].difficulty = diff;
  tmpl[0].created_at = t0;
  CHECK(pow_mine_batch(ctx, tmpl, 1, diff, 0, window, NULL, 0, &blocks[0], ctr, &solved, NULL));
  if (solved != 1) return fprintf(stderr, "the root's window held no solution\n"), 1;
  size_t tip = 0;
  for (int h = 0; h < heights; ++h) {
    for (int r = 0; r < RIVALS; ++r) {
      tmpl[r] = blocks[tip];
      tmpl[r].index = blocks[tip].index + 1;
      tmpl[r].node_owner_number = (uint32_t)r;
      tmpl[r].difficulty = diff;
      tmpl[r].created_at = t0 + 1 + (uint64_t)(RIVALS * h + r);
      memcpy(tmpl[r].previous_block_hash, blocks[tip].block_hash, POW_HASH_SIZE);
    }
    pow_block* out = &blocks[1 + RIVALS * (size_t)h];
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
    const pow_block t = blocks[i];
    blocks[i] = blocks[j];
    blocks[j] = t;
  }

  if (dump) { /* the pool as it is fed */
    FILE* f = fopen(dump, "wb");
    if (!f || fwrite(blocks, sizeof(pow_block), n, f) != n || fclose(f) != 0) return fprintf(stderr, "cannot write %s\n", dump), 1;
  }

  pow_pool* pool = NULL;
  CHECK(pow_pool_open(ctx, diff, 0, &pool));
  pow_pool_info info;
  pow_stats st;
  CHECK(pow_pool_add(pool, blocks, n, &info));
  CHECK(pow_get_stats(ctx, &st));
  print_info("fed", &info, &st);
  if (info.n_flagged || info.best == POW_POOL_NONE || info.best_index != (uint32_t)heights)
    return fprintf(stderr, "the pool this example mined must be sound\n"), 1;

  /* look_for_block over the winning chain without a host walk: which blocks lie under the tip? */
  uint8_t* on = calloc(n, 1);
  uint32_t* map = calloc(n, sizeof(uint32_t));
  size_t n_on = 0;
  const uint32_t best_before = info.best;
  CHECK(pow_pool_mark(pool, &best_before, 1, 0, 0, on, &n_on));
  CHECK(pow_get_stats(ctx, &st));
  printf("chain under block %u: %zu blocks; %u launches\n", best_before, n_on, st.launches);
  if (n_on != (size_t)heights + 1 || !on[best_before]) return fprintf(stderr, "the winning chain has one block per height\n"), 1;

  /* forget what can no longer win: keep the chains of every sound block within five heights of the tip */
  const uint32_t min_index = info.best_index > VALIDATION_BLOCKS ? info.best_index - VALIDATION_BLOCKS : 0;
  const int rc = pow_pool_prune(pool, NULL, 0, min_index, POW_KEEP_BY_INDEX | POW_KEEP_SOUND_ONLY, map, &info);
  CHECK(rc);
  CHECK(pow_get_stats(ctx, &st));
  printf("pruned from index %u: ", min_index);
  print_info("kept", &info, &st);
  if (rc != 1 || map[best_before] != info.best) return fprintf(stderr, "the tip must survive the prune\n"), 1;

  /* the host's structs follow the map; survivors keep their order */
  size_t kept = 0;
  for (size_t i = 0; i < n; ++i)
    if (map[i] != POW_POOL_NONE) {
      if (map[i] != kept) return fprintf(stderr, "the map is not in order at %zu\n", i), 1;
      blocks[kept++] = blocks[i];
    }
  if (kept != info.size) return fprintf(stderr, "the map keeps %zu blocks, the pool %u\n", kept, info.size), 1;

  /* the next block on the tip, at its new position */
  tip = info.best;
  tmpl[0] = blocks[tip];
  tmpl[0].index = blocks[tip].index + 1;
  tmpl[0].node_owner_number = 0;
  tmpl[0].created_at = t0 + 1 + (uint64_t)(RIVALS * heights);
  memcpy(tmpl[0].previous_block_hash, blocks[tip].block_hash, POW_HASH_SIZE);
  CHECK(pow_mine_batch(ctx, tmpl, 1, diff, 0, window, NULL, 0, &blocks[kept], ctr, &solved, NULL));
  if (solved != 1) return fprintf(stderr, "the next block's window held no solution\n"), 1;
  if (dump) { /* ... and the block that came after the prune */
    FILE* f = fopen(dump, "ab");
    if (!f || fwrite(&blocks[kept], sizeof(pow_block), 1, f) != 1 || fclose(f) != 0) return fprintf(stderr, "cannot write %s\n", dump), 1;
  }
  CHECK(pow_pool_add(pool, &blocks[kept], 1, &info));
  CHECK(pow_get_stats(ctx, &st));
  print_info("next block", &info, &st);
  uint32_t parent = 0, depth = 0, at = POW_POOL_NONE;
  CHECK(pow_pool_read(pool, kept, 1, NULL, &parent, &depth, NULL));
  CHECK(pow_pool_find(pool, blocks[kept].block_hash, 1, &at));
  printf("block %u at %u owner %u nonce %.9s hash %s parent %u depth %u\n", blocks[kept].index, at,
         blocks[kept].node_owner_number, blocks[kept].nonce, blocks[kept].block_hash, parent, depth);
  if (info.best != kept || at != kept || parent != tip || depth != (uint32_t)heights + 2 || info.n_flagged)
    return fprintf(stderr, "the next block must stand on the tip\n"), 1;
  printf("pool of %zu blocks pruned to %zu and fed again at difficulty %u\n", n, kept, diff);
  pow_pool_close(pool);
  free(map);
  free(on);
  free(blocks);
  pow_destroy(ctx);
  return 0;
}
