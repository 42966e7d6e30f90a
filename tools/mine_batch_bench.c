/*
 * mine_batch_bench.c — wall time of mining n independent templates, per call, from C.
 *
 *   mine_batch_bench batch <d> <window_log2> <calls> <n>...   one pow_mine_batch call per sample
 *   mine_batch_bench loop  <d> <window_log2> <calls> <n>...   the loop around pow_mine per sample:
 *                                                             what a caller had before pow_mine_batch
 *
 * Both mine the same templates: one parent, template i with index 1, owner i,
 * created_at = 1700000000 + i, the window [0, 2^window_log2), lowest counter.
 * For every n, after pow_warmup and one discarded sample, `calls` samples go
 * out as one JSON line: wall ms, kernel ms and launches of each, and a
 * checksum (FNV-1a) over every output byte and counter so a caller can compare
 * the two ways across processes.  `batch` also mines every template once more
 * through pow_mine, outside the timed region, and compares all 552 bytes and
 * the counter of each with what the batch call gave ("equal").  Which path
 * pow_mine_batch takes is the library's business (the test library reads
 * POW_BATCH_FUSED_MAX); tools/mine_batch_bench.py drives this program.
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

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

int main(int argc, char** argv) {
  if (argc < 6) return fprintf(stderr, "usage: mine_batch_bench batch|loop <d> <window_log2> <calls> <n>...\n"), 2;
  const int loop = strcmp(argv[1], "loop") == 0;
  const unsigned d = (unsigned)atoi(argv[2]);
  const unsigned wlog = (unsigned)atoi(argv[3]);
  const int calls = atoi(argv[4]);
  if (wlog > 32 || calls < 1) return 2;
  const uint64_t window = 1ull << wlog;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));
  CHECK(pow_warmup(ctx));
  double* ms = malloc((size_t)calls * sizeof *ms);
  double* kms = malloc((size_t)calls * sizeof *kms);
  unsigned* launches = malloc((size_t)calls * sizeof *launches);
  for (int a = 5; a < argc; ++a) {
    const size_t n = (size_t)atol(argv[a]);
    if (n < 1) return 2;
    pow_block* tmpls = calloc(n, sizeof *tmpls);
    pow_block* out = calloc(n, sizeof *out);
    uint64_t* ctrs = calloc(n, sizeof *ctrs);
    for (size_t i = 0; i < n; ++i) { /* node.cpp:292-299 on one parent */
      tmpls[i].index = 1;
      tmpls[i].node_owner_number = (uint32_t)i;
      tmpls[i].difficulty = d;
      tmpls[i].created_at = 1700000000u + i;
      memcpy(tmpls[i].previous_block_hash, "00c3a1f0e2d4b5968778695a4b3c2d1e0ff1e2d3c4b5a69788796a5b4c3d2e1f", 64);
    }
    for (int c = -1; c < calls; ++c) { /* c = -1: discarded */
      double k_ms = 0;
      unsigned nl = 0;
      const double t0 = now_ms();
      if (!loop) {
        size_t solved = 0;
        int rc = pow_mine_batch(ctx, tmpls, n, d, 0, window, NULL, 0, out, ctrs, &solved, NULL);
        CHECK(rc);
        if (rc != 1) return fprintf(stderr, "%zu of %zu templates solved\n", solved, n), 1;
      } else {
        for (size_t i = 0; i < n; ++i) {
          int rc = pow_mine(ctx, &tmpls[i], 0, window, d, NULL, 0, &out[i], &ctrs[i], NULL);
          CHECK(rc);
          if (rc != 1) return fprintf(stderr, "no solution for template %zu\n", i), 1;
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
    int equal = -1; /* loop: nothing to compare with */
    if (!loop) {
      equal = 1;
      for (size_t i = 0; i < n; ++i) {
        pow_block one;
        uint64_t ctr = 0;
        int rc = pow_mine(ctx, &tmpls[i], 0, window, d, NULL, 0, &one, &ctr, NULL);
        CHECK(rc);
        if (rc != 1 || ctr != ctrs[i] || memcmp(&one, &out[i], sizeof one) != 0) equal = 0;
      }
    }
    uint64_t sum = fnv(14695981039346656037ull, out, n * sizeof *out);
    sum = fnv(sum, ctrs, n * sizeof *ctrs);
    printf("{\"mode\": \"%s\", \"d\": %u, \"window_log2\": %u, \"n\": %zu, \"equal\": %d, \"checksum\": \"%016llx\", \"ms\": [",
           argv[1], d, wlog, n, equal, (unsigned long long)sum);
    for (int c = 0; c < calls; ++c) printf("%s%.4f", c ? ", " : "", ms[c]);
    printf("], \"kernel_ms\": [");
    for (int c = 0; c < calls; ++c) printf("%s%.4f", c ? ", " : "", kms[c]);
    printf("], \"launches\": [");
    for (int c = 0; c < calls; ++c) printf("%s%u", c ? ", " : "", launches[c]);
    printf("]}\n");
    fflush(stdout);
    free(ctrs);
    free(out);
    free(tmpls);
  }
  pow_destroy(ctx);
  return 0;
}
