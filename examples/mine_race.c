/*
 * mine_race.c — the reference's N competing ranks on one GPU, one call per block.
 *
 * Every rank of the reference refreshes its own template on the current tip
 * (node.cpp:292-299: the tip copied, index + 1, its own node_owner_number,
 * created_at, the tip's block_hash as previous_block_hash) and mines it.  Here
 * one pow_mine_batch call mines all the miners' templates of a block at once;
 * the winner is the miner that needed the fewest trials (the lowest solving
 * counter, ties to the lowest owner), and its block becomes the next tip.
 * pow_verify_chain then audits the result, with the genesis block
 * (node.cpp:361-372: its hash zeroed) as the oldest block's parent.
 *
 *   cc -std=c11 -I include examples/mine_race.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o mine_race && ./mine_race [miners] [blocks] [difficulty]
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
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));
  CHECK(pow_warmup(ctx));

  /* chain[0 .. blocks-1]: the winners, tip first; chain[blocks]: the genesis block */
  pow_block* chain = calloc((size_t)blocks + 1, sizeof(pow_block));
  pow_block* tmpls = calloc((size_t)miners, sizeof(pow_block));
  uint64_t* ctrs = calloc((size_t)miners, sizeof(uint64_t));
  pow_block* genesis = &chain[blocks];
  genesis->difficulty = diff; /* index 0, block_hash all zero */
  genesis->created_at = (uint64_t)time(NULL);

  /* a window near what a template needs keeps all the miners in one launch (pow_gpu.h) */
  const uint64_t window = diff + 7 < 32 ? 1ull << (diff + 7) : 1ull << 32;
  uint64_t trials = 0;
  double gpu_ms = 0;
  for (int k = 0; k < blocks; ++k) {
    const pow_block* tip = &chain[blocks - k];
    const uint64_t now = (uint64_t)time(NULL);
    for (int m = 0; m < miners; ++m) { /* node.cpp:292-299 */
      tmpls[m] = *tip;
      tmpls[m].index = tip->index + 1;
      tmpls[m].node_owner_number = (uint32_t)m;
      tmpls[m].difficulty = diff;
      tmpls[m].created_at = now;
      memcpy(tmpls[m].previous_block_hash, tip->block_hash, POW_HASH_SIZE);
    }
    size_t solved = 0;
    uint64_t hashes = 0;
    CHECK(pow_mine_batch(ctx, tmpls, (size_t)miners, diff, 0, window, NULL, 0, tmpls, ctrs, &solved, &hashes));
    if (solved == 0) return fprintf(stderr, "block %d: no miner's window held a solution\n", k + 1), 1;
    int win = -1;
    for (int m = 0; m < miners; ++m)
      if (ctrs[m] != UINT64_MAX && (win < 0 || ctrs[m] < ctrs[win])) win = m;
    chain[blocks - 1 - k] = tmpls[win];
    pow_stats st;
    CHECK(pow_get_stats(ctx, &st));
    trials += hashes;
    gpu_ms += st.kernel_ms;
    printf("block %u miner %d after %llu trials nonce %.9s hash %s\n", tmpls[win].index, win,
           (unsigned long long)ctrs[win] + 1, tmpls[win].nonce, tmpls[win].block_hash);
  }
  printf("%d miners, %llu trials, %.3f ms on the GPU\n", miners, (unsigned long long)trials, gpu_ms);

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
  free(tmpls);
  free(chain);
  pow_destroy(ctx);
  return 0;
}
