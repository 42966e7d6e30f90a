/*
 * mine_chain_fused.c — the loop of mine_chain.c as one call.
 *
 * pow_mine_chain mines `blocks` linked blocks on top of a genesis block whose
 * hash is zeroed (node.cpp:361-372): the template refresh (node.cpp:292-299),
 * the search for the lowest solving counter and the strcpy of the hex
 * (node.cpp:318) all happen on the GPU, block after block.  pow_verify_chain
 * then audits the result, with the genesis block as the oldest block's parent.
 *
 *   cc -std=c11 -I include examples/mine_chain_fused.c -L mpi_blockchain_amd -lpow_gpu \
 *      -Wl,-rpath,$PWD/mpi_blockchain_amd -o mine_chain_fused && ./mine_chain_fused [blocks] [difficulty]
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
  const int blocks = argc > 1 ? atoi(argv[1]) : 10;
  const unsigned diff = argc > 2 ? (unsigned)atoi(argv[2]) : 9;
  if (blocks < 1) return fprintf(stderr, "blocks must be at least 1\n"), 2;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));
  CHECK(pow_warmup(ctx));

  /* chain[0 .. blocks-1]: the mined blocks, tip first; chain[blocks]: the genesis block */
  pow_block* chain = calloc((size_t)blocks + 1, sizeof(pow_block));
  pow_block* genesis = &chain[blocks];
  genesis->difficulty = diff; /* index 0, block_hash all zero */
  genesis->created_at = (uint64_t)time(NULL);

  size_t mined = 0;
  uint64_t hashes = 0;
  int rc = pow_mine_chain(ctx, genesis, (size_t)blocks, diff, 0, NULL, 0, 1ull << 32, NULL, 0, chain, &mined, &hashes);
  CHECK(rc);
  if (rc != 1) return fprintf(stderr, "stopped after %zu of %d blocks\n", mined, blocks), 1;
  pow_stats st;
  CHECK(pow_get_stats(ctx, &st));
  for (int i = blocks - 1; i >= 0; --i)
    printf("block %u nonce %.9s hash %s\n", chain[i].index, chain[i].nonce, chain[i].block_hash);
  printf("%llu trials, %u launches, %.3f ms on the GPU\n", (unsigned long long)hashes, st.launches, st.kernel_ms);

  /* the audit: every stored hash, every proof of work, every link and index.
   * The genesis block is only the parent here: its zeroed hash is no digest. */
  size_t first_bad = 0, n_bad = 0;
  rc = pow_verify_chain(ctx, chain, (size_t)blocks, diff, NULL, &first_bad, &n_bad);
  CHECK(rc);
  if (rc != 1) return fprintf(stderr, "%zu flagged blocks, the first at %zu\n", n_bad, first_bad), 1;
  if (memcmp(chain[blocks - 1].previous_block_hash, genesis->block_hash, POW_HASH_SIZE) != 0 ||
      chain[blocks - 1].index != genesis->index + 1)
    return fprintf(stderr, "the oldest block is no child of the genesis block\n"), 1;
  printf("chain of %d blocks at difficulty %u: valid\n", blocks, diff);
  free(chain);
  pow_destroy(ctx);
  return 0;
}
