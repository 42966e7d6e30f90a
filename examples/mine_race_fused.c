/*
 * mine_race_fused.c — the reference's N competing ranks on one GPU, one call for the whole race.
 *
 * What mine_race.c does with one pow_mine_batch call and a host step per
 * block, pow_mine_race does in one call: at every height each miner refreshes
 * its own template on the current tip (node.cpp:292-299), the miner that needs
 * the fewest trials wins (the lowest solving counter, ties to the lowest
 * position), and its block is the next tip.  No loser is searched past the
 * winner's counter.  pow_verify_chain then audits the result, with the genesis
 * block (node.cpp:361-372: its hash zeroed) as the oldest block's parent.
 *
 *   cc -std=c11 -I include examples/mine_race_fused.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o mine_race_fused && ./mine_race_fused [miners] [blocks] [difficulty]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

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
  const int miners = argc > 1 ? atoi(argv[1]) : 10;
  const int blocks = argc > 2 ? atoi(argv[2]) : 10;
  const unsigned diff = argc > 3 ? (unsigned)atoi(argv[3]) : 9;
  if (miners < 1 || blocks < 1) return fprintf(stderr, "miners and blocks must be at least 1\n"), 2;
  if (miners > POW_RACE_MAX_RIVALS) return fprintf(stderr, "at most %d miners\n", POW_RACE_MAX_RIVALS), 2;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));
  CHECK(pow_warmup(ctx));

  /* chain[0 .. blocks-1]: the winners, tip first; chain[blocks]: the genesis block */
  pow_block* chain = calloc((size_t)blocks + 1, sizeof(pow_block));
  uint32_t* owners = calloc((size_t)miners, sizeof(uint32_t));
  uint32_t* winners = calloc((size_t)blocks, sizeof(uint32_t));
  uint64_t* ctrs = calloc((size_t)blocks, sizeof(uint64_t));
  pow_block* genesis = &chain[blocks];
  genesis->difficulty = diff; /* index 0, block_hash all zero */
  genesis->created_at = (uint64_t)time(NULL);
  for (int m = 0; m < miners; ++m) owners[m] = (uint32_t)m;

  /* a window near what a height needs keeps the batches long and the watchdog tight (pow_gpu.h) */
  const uint64_t window = diff + 7 < 32 ? 1ull << (diff + 7) : 1ull << 32;
  size_t mined = 0;
  uint64_t trials = 0;
  const int rc_race = pow_mine_race(ctx, genesis, (size_t)blocks, diff, owners, (size_t)miners, NULL, 0, window, NULL, 0,
                                    chain, winners, ctrs, &mined, &trials);
  CHECK(rc_race);
  if (rc_race != 1) return fprintf(stderr, "block %zu: no miner's window held a solution\n", mined + 1), 1;
  pow_stats st;
  CHECK(pow_get_stats(ctx, &st));
  for (int k = 0; k < blocks; ++k) {
    const pow_block* b = &chain[blocks - 1 - k];
    printf("block %u miner %u after %llu trials nonce %.9s hash %s\n", b->index, winners[blocks - 1 - k],
           (unsigned long long)ctrs[blocks - 1 - k] + 1, b->nonce, b->block_hash);
  }
  printf("%d miners, %llu trials, %.3f ms on the GPU\n", miners, (unsigned long long)trials, st.kernel_ms);

  /* the audit: every stored hash, every proof of work, every link and index */
  size_t first_bad = 0, n_bad = 0;
  int rc = pow_verify_chain(ctx, chain, (size_t)blocks, diff, NULL, &first_bad, &n_bad);
  CHECK(rc);
  if (rc != 1) return fprintf(stderr, "%zu flagged blocks, the first at %zu\n", n_bad, first_bad), 1;
  if (memcmp(chain[blocks - 1].previous_block_hash, genesis->block_hash, POW_HASH_SIZE) != 0 ||
      chain[blocks - 1].index != genesis->index + 1)
    return fprintf(stderr, "the oldest block is no child of the genesis block\n"), 1;
  printf("chain of %d blocks at difficulty %u: valid\n", blocks, diff);
  free(ctrs);
  free(winners);
  free(owners);
  free(chain);
  pow_destroy(ctx);
  return 0;
}
