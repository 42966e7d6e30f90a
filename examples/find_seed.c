/*
 * find_seed.c — recover the seed of a reference rank from the blocks it mined,
 * in plain C over include/pow_gpu.h.
 *
 * The reference seeds its nonces with time(NULL) + mpi_rank (node.cpp:386) and
 * keeps the seed nowhere.  A block carries what is left of it: its nonce, one
 * of the seed's stream, and created_at, which bounds the seed.  This example
 * mines three blocks with pow_mine_rand from a seed (mine_rand.c's loop),
 * forgets the seed, and asks pow_find_seed which seeds within an hour before the
 * first block's created_at drew those three nonces, and at which trials.
 *
 *   cc -std=c11 -I include examples/find_seed.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o find_seed && ./find_seed [seconds before created_at] [difficulty]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pow_gpu.h"

#define CHECK(x)                                                                   \
  do {                                                                             \
    int rc_ = (x);                                                                 \
    if (rc_ < 0) {                                                                 \
      fprintf(stderr, "%s failed (%d): %s\n", #x, rc_, pow_last_error());          \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

#define BLOCKS 3

int main(int argc, char** argv) {
  const uint64_t t0 = 1700000000ull;
  const uint32_t rank = 2;
  const uint32_t before = argc > 1 ? (uint32_t)strtoul(argv[1], NULL, 0) : 1234u;
  const unsigned diff = argc > 2 ? (unsigned)atoi(argv[2]) : 9;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));

  /* ---- the rank: started `before` seconds ahead of its first block ---- */
  pow_block chain[BLOCKS + 1];
  memset(chain, 0, sizeof chain);
  chain[0].difficulty = diff;
  chain[0].created_at = t0;
  uint64_t trials[BLOCKS + 1] = {0};
  {
    const uint32_t seed = (uint32_t)(t0 - before) + rank;  /* srand(time(NULL) + mpi_rank) */
    uint64_t at = 0;
    for (int i = 1; i <= BLOCKS; ++i) {
      pow_block tmpl = chain[i - 1];
      tmpl.index += 1;
      tmpl.node_owner_number = rank;
      tmpl.difficulty = diff;
      tmpl.created_at = t0 + 17ull * (uint64_t)(i - 1);
      memcpy(tmpl.previous_block_hash, tmpl.block_hash, POW_HASH_SIZE);
      int rc = pow_mine_rand(ctx, &tmpl, seed, at, 1ull << 32, diff, NULL, 0, &chain[i], &trials[i], NULL);
      CHECK(rc);
      if (rc != 1) return fprintf(stderr, "no solution for block %d in 2^32 trials\n", i), 1;
      at = trials[i] + 1;
    }
    printf("mined %d blocks with seed %u\n", BLOCKS, seed);
  }  /* ... and the seed is gone */

  /* ---- the auditor: the blocks alone ---- */
  char nonces[BLOCKS][POW_NONCE_SIZE];
  for (int i = 1; i <= BLOCKS; ++i) memcpy(nonces[i - 1], chain[i].nonce, POW_NONCE_SIZE);
  const uint32_t n_seeds = 3600u + rank + 1u;  /* started within the hour before its first block */
  const uint32_t first = (uint32_t)(chain[1].created_at - 3600u);
  pow_seed_match m[16];
  size_t n = 0;
  uint64_t pairs = 0;
  int rc = pow_find_seed(ctx, &nonces[0][0], BLOCKS, first, n_seeds, 0, 1ull << 20, NULL, 0, m, 16, &n, &pairs);
  CHECK(rc);
  pow_stats st;
  CHECK(pow_get_stats(ctx, &st));
  printf("searched %llu (seed, trial) pairs in %.3f ms of kernel time, %u launches: %zu matches\n",
         (unsigned long long)pairs, st.kernel_ms, st.launches, n);
  if (n != BLOCKS) return fprintf(stderr, "expected one match per block\n"), 1;
  for (size_t i = 0; i < n; ++i) {
    printf("block %u nonce %.9s: seed %u trial %llu\n", m[i].target + 1, nonces[m[i].target], m[i].seed,
           (unsigned long long)m[i].trial);
    if (m[i].seed != m[0].seed || m[i].trial != trials[m[i].target + 1])
      return fprintf(stderr, "not the trial the block was mined at\n"), 1;
  }
  printf("recovered seed %u: rank %u started %u s before its first block\n", m[0].seed, rank,
         (uint32_t)(chain[1].created_at + rank) - m[0].seed);
  pow_destroy(ctx);
  return 0;
}
