/*
 * mine_chain_bench.c — wall time of mining n linked blocks, per call, from C.
 *
 *   mine_chain_bench chain <d> <n> <calls>   one pow_mine_chain call per sample
 *   mine_chain_bench loop  <d> <n> <calls>   the loop of examples/mine_chain.c per sample:
 *                                            refresh on the host, pow_mine, next block
 *
 * Both mine the same chain (genesis parent, created_at = 1700000000 + k, the
 * window [0, 2^32), lowest counter) and print the tip's hash so a caller can
 * check that.  After pow_warmup and one discarded sample, `calls` samples go
 * out as one JSON line: wall ms, kernel ms and launches of each.  Which path
 * pow_mine_chain takes is the library's business (the test library reads
 * POW_CHAIN_FUSED_MAX); tools/mine_chain_bench.py drives this program.
 */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "pow_gpu.h"

#define CHECK(x)                                                          \
  do {                                                                    \
    int rc_ = (x);                                                        \
    if (rc_ < 0) {                                                        \
      fprintf(stderr, "%s failed (%d): %s\n", #x, rc_, pow_last_error()); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

static double now_ms(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec * 1e3 + (double)t.tv_nsec * 1e-6;
}

int main(int argc, char** argv) {
  if (argc != 5) return fprintf(stderr, "usage: mine_chain_bench chain|loop <d> <n> <calls>\n"), 2;
  const int loop = strcmp(argv[1], "loop") == 0;
  const unsigned d = (unsigned)atoi(argv[2]);
  const size_t n = (size_t)atol(argv[3]);
  const int calls = atoi(argv[4]);
  if (n < 1 || calls < 1) return 2;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));
  CHECK(pow_warmup(ctx));
  pow_block genesis;
  memset(&genesis, 0, sizeof genesis);
  genesis.difficulty = 9;
  genesis.created_at = 1699999990u;
  uint64_t* created = malloc(n * sizeof *created);
  pow_block* out = calloc(n, sizeof *out);
  double* ms = malloc((size_t)calls * sizeof *ms);
  double* kms = malloc((size_t)calls * sizeof *kms);
  unsigned* launches = malloc((size_t)calls * sizeof *launches);
  for (size_t k = 0; k < n; ++k) created[k] = 1700000000u + k;
  for (int c = -1; c < calls; ++c) { /* c = -1: discarded */
    double k_ms = 0;
    unsigned nl = 0;
    const double t0 = now_ms();
    if (!loop) {
      size_t mined = 0;
      int rc = pow_mine_chain(ctx, &genesis, n, d, 0, created, 0, 1ull << 32, NULL, 0, out, &mined, NULL);
      CHECK(rc);
      if (rc != 1) return fprintf(stderr, "stopped after %zu blocks\n", mined), 1;
    } else {
      pow_block last = genesis;
      for (size_t k = 0; k < n; ++k) {
        pow_block tmpl = last; /* node.cpp:292-299 */
        tmpl.index += 1;
        tmpl.node_owner_number = 0;
        tmpl.difficulty = d;
        tmpl.created_at = created[k];
        memcpy(tmpl.previous_block_hash, last.block_hash, POW_HASH_SIZE);
        int rc = pow_mine(ctx, &tmpl, 0, 1ull << 32, d, NULL, 0, &out[n - 1 - k], NULL, NULL);
        CHECK(rc);
        if (rc != 1) return fprintf(stderr, "no solution for block %zu\n", k), 1;
        last = out[n - 1 - k];
        pow_stats s;
        pow_get_stats(ctx, &s); /* in the timed region on purpose: cheap, and the loop's caller wants it too */
        k_ms += s.kernel_ms;
        nl += s.launches;
      }
    }
    const double t1 = now_ms();
    if (!loop) {
      pow_stats s;
      CHECK(pow_get_stats(ctx, &s));
      k_ms = s.kernel_ms;
      nl = s.launches;
    }
    if (c >= 0) {
      ms[c] = t1 - t0;
      kms[c] = k_ms;
      launches[c] = nl;
    }
  }
  size_t bad = 0;
  int ok = pow_verify_chain(ctx, out, n, d, NULL, NULL, &bad);
  CHECK(ok);
  printf("{\"mode\": \"%s\", \"d\": %u, \"n\": %zu, \"valid\": %d, \"tip\": \"%.64s\", \"ms\": [", argv[1], d, n, ok,
         out[0].block_hash);
  for (int c = 0; c < calls; ++c) printf("%s%.4f", c ? ", " : "", ms[c]);
  printf("], \"kernel_ms\": [");
  for (int c = 0; c < calls; ++c) printf("%s%.4f", c ? ", " : "", kms[c]);
  printf("], \"launches\": [");
  for (int c = 0; c < calls; ++c) printf("%s%u", c ? ", " : "", launches[c]);
  printf("]}\n");
  pow_destroy(ctx);
  return 0;
}
