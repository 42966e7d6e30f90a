/*
 * mine_rand.c — replay a solo rank of the reference from its seed, in plain C
 * over include/pow_gpu.h.
 *
 * The reference draws every nonce with gen_random_nonce (block.cpp:61-72),
 * 9 x rand() % 62, after srand(time(NULL) + mpi_rank) (node.cpp:386), tests
 * its trials in order and stops at the first that solves (node.cpp:285-318);
 * the stream of rand() runs on from block to block.  pow_mine_rand returns the
 * LOWEST solving trial of that very stream, so the loop below mines the blocks
 * the reference mines with this seed, at the trials it mines them: refresh the
 * template on the tip, mine from where the stream stands, go on at the trial
 * after the one found.  created_at is pinned (the reference takes the clock),
 * so that a seed always gives the same chain.
 *
 *   cc -std=c11 -I include examples/mine_rand.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o mine_rand && ./mine_rand [seed] [blocks] [difficulty]
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

int main(int argc, char** argv) {
  const uint32_t seed = argc > 1 ? (uint32_t)strtoul(argv[1], NULL, 0) : 1u;
  const int blocks = argc > 2 ? atoi(argv[2]) : 10;
  const unsigned diff = argc > 3 ? (unsigned)atoi(argv[3]) : 9;
  const uint32_t rank = 0;
  const uint64_t t0 = 1700000000ull;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));

  pow_block* chain = calloc((size_t)blocks + 1, sizeof(pow_block));
  chain[0].difficulty = diff;  /* genesis: index 0, block_hash all zero */
  chain[0].created_at = t0;
  uint64_t at = 0;             /* the stream's next trial: gen_random_nonce calls so far */
  for (int i = 1; i <= blocks; ++i) {
    pow_block tmpl = chain[i - 1];             /* node.cpp:292 */
    tmpl.index += 1;                           /* node.cpp:295-299 */
    tmpl.node_owner_number = rank;
    tmpl.difficulty = diff;
    tmpl.created_at = t0 + 17ull * (uint64_t)(i - 1);
    memcpy(tmpl.previous_block_hash, tmpl.block_hash, POW_HASH_SIZE);
    uint64_t found = 0;
    int rc = pow_mine_rand(ctx, &tmpl, seed, at, 1ull << 32, diff, NULL, 0, &chain[i], &found, NULL);
    CHECK(rc);
    if (rc != 1) {
      fprintf(stderr, "no solution for block %d in 2^32 trials\n", i);
      return 1;
    }
    /* the nonce is the stream's own at that trial */
    char nonce[POW_NONCE_SIZE];
    CHECK(pow_rand_nonces(seed, found, 1, nonce));
    if (memcmp(nonce, chain[i].nonce, POW_NONCE_SIZE) != 0) return fprintf(stderr, "nonce mismatch at %d\n", i), 1;
    printf("block %d trial %llu nonce %.9s hash %s\n", i, (unsigned long long)found, chain[i].nonce,
           chain[i].block_hash);
    at = found + 1;                            /* where the reference's stream stands now */
  }
  /* receiver-side validation of the whole chain */
  for (int i = 1; i <= blocks; ++i) {
    char hex[65];
    CHECK(pow_hash_block(ctx, &chain[i], NULL, hex));
    if (strcmp(hex, chain[i].block_hash) != 0) return fprintf(stderr, "hash mismatch at %d\n", i), 1;
    if (memcmp(chain[i].previous_block_hash, chain[i - 1].block_hash, POW_HASH_SIZE) != 0)
      return fprintf(stderr, "broken link at %d\n", i), 1;
    if (!pow_solves_problem(hex, diff)) return fprintf(stderr, "difficulty not met at %d\n", i), 1;
  }
  printf("chain of %d blocks at difficulty %u: valid\n", blocks, diff);
  printf("seed %u: the rank drew %llu trials\n", seed, (unsigned long long)at);
  free(chain);
  pow_destroy(ctx);
  return 0;
}
