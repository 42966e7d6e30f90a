/*
 * pool_stream.c — a node's pool grows one block at a time: keep its index on the GPU.
 *
 * node_blocks (node.cpp:21) takes a block whenever one arrives (node.cpp:199,
 * 319), and after each arrival the node asks again which blocks hang
 * together and which tip wins (node.cpp:100-148, 204-253).  This example
 * mines the forked pool of examples/index_blocks.c (three rivals on the
 * current tip at every height, all three kept), shuffles it and feeds it to a
 * pow_pool block by block: a block whose parent has not arrived is an orphan
 * until it does, and the add that brings the parent adopts it and ranks the
 * pool again.  One line per add; at the end the pool's state is compared with
 * one pow_index_blocks call over the same blocks, and the winning chain is
 * walked on the host along parent[].
 *
 *   cc -std=c11 -I include examples/pool_stream.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o pool_stream && ./pool_stream [heights] [difficulty] [pool-dump]
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
  pow_block* blocks = calloc(n, sizeof(pow_block));
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
  if (dump) {
    FILE* f = fopen(dump, "wb");
    if (!f || fwrite(blocks, sizeof(pow_block), n, f) != n || fclose(f) != 0) return fprintf(stderr, "cannot write %s\n", dump), 1;
  }

  /* block by block, as they arrive */
  pow_pool* pool = NULL;
  CHECK(pow_pool_open(ctx, diff, 0, &pool));
  pow_pool_info info;
  pow_stats st;
  unsigned reranks = 0;
  for (size_t i = 0; i < n; ++i) {
    const int rc = pow_pool_add(pool, &blocks[i], 1, &info);
    CHECK(rc);
    CHECK(pow_get_stats(ctx, &st));
    reranks += info.reranked;
    printf("add %zu: size %u flagged %u best %d index %u adopted %u reranked %u rehashed %u capacity %u slots %u; %u launches\n",
           i, info.size, info.n_flagged, info.best == POW_POOL_NONE ? -1 : (int)info.best, info.best_index, info.adopted,
           info.reranked, info.rehashed, info.capacity, info.slots, st.launches);
    if ((rc == 1) != (info.n_flagged == 0)) return fprintf(stderr, "add %zu: the return value and the info disagree\n", i), 1;
  }

  /* the same answer as one pow_index_blocks call over everything */
  uint8_t* status = calloc(2 * n, 1);
  uint32_t* words = calloc(6 * n, sizeof(uint32_t));
  uint32_t *parent = words, *depth = words + 2 * n, *n_bad = words + 4 * n;
  size_t best = SIZE_MAX;
  CHECK(pow_pool_read(pool, 0, n, status, parent, depth, n_bad));
  const int rc = pow_index_blocks(ctx, blocks, n, diff, status + n, parent + n, depth + n, n_bad + n, &best);
  CHECK(rc);
  const int same = memcmp(status, status + n, n) == 0 && memcmp(parent, parent + n, 4 * n) == 0 &&
                   memcmp(depth, depth + n, 4 * n) == 0 && memcmp(n_bad, n_bad + n, 4 * n) == 0 &&
                   (best == SIZE_MAX ? info.best == POW_POOL_NONE : info.best == best) && (rc == 1) == (info.n_flagged == 0);
  printf("pool of %zu blocks fed one by one: %u adds ranked it again; %s one pow_index_blocks call\n", n, reranks,
         same ? "equal to" : "DIFFERS from");
  if (!same || rc != 1 || info.best == POW_POOL_NONE) return fprintf(stderr, "the pool this example mined must be sound\n"), 1;

  /* node_blocks.find, then the walk on the host: read parent and follow it */
  uint32_t at = POW_POOL_NONE;
  CHECK(pow_pool_find(pool, blocks[info.best].block_hash, 1, &at));
  if (at != info.best) return fprintf(stderr, "the best block's name finds %u\n", at), 1;
  const size_t len = depth[at];
  for (size_t k = 0; k < len; ++k) {
    printf("block %u at %u owner %u nonce %.9s hash %s\n", blocks[at].index, at, blocks[at].node_owner_number,
           blocks[at].nonce, blocks[at].block_hash);
    at = parent[at];
  }
  if (at != POW_POOL_ROOT || info.best_index != (uint32_t)heights) return fprintf(stderr, "the best chain is not the race's\n"), 1;
  printf("best chain of %zu blocks at difficulty %u\n", len, diff);
  pow_pool_close(pool);
  free(words);
  free(status);
  free(blocks);
  pow_destroy(ctx);
  return 0;
}
