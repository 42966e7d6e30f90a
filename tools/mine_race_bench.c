/*
 * mine_race_bench.c — wall time of a race of R rival miners over n heights, per call, from C.
 *
 *   mine_race_bench race  <d> <window_log2> <calls> <heights> <R>...   one pow_mine_race call per sample
 *   mine_race_bench batch <d> <window_log2> <calls> <heights> <R>...   the loop of examples/mine_race.c per sample:
 *                                                                      per height a host refresh of R templates,
 *                                                                      one pow_mine_batch call, the lowest
 *                                                                      (counter, position), the next height
 *
 * Both run the same race: the genesis block of examples/mine_race.c with
 * created_at 1699999990 as parent, rival r with owner r, created_at =
 * 1700000000 + 17 k + r at height k, the window [0, 2^window_log2).  For every
 * R, after pow_warmup and one discarded sample, `calls` samples go out as one
 * JSON line: wall ms, kernel ms, launches and trials of each, and a checksum
 * (FNV-1a) over every output byte, winner and counter so a caller can compare
 * the ways across processes.  Which path pow_mine_race takes is the library's
 * business (the test library reads POW_RACE_FUSED_MAX);
 * tools/mine_race_bench.py drives this program.
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
  if (argc < 7) return fprintf(stderr, "usage: mine_race_bench race|batch <d> <window_log2> <calls> <heights> <R>...\n"), 2;
  const int by_batch = strcmp(argv[1], "batch") == 0;
  const unsigned d = (unsigned)atoi(argv[2]);
  const unsigned wlog = (unsigned)atoi(argv[3]);
  const int calls = atoi(argv[4]);
  const size_t n = (size_t)atol(argv[5]);
  if (wlog > 32 || calls < 1 || n < 1) return 2;
  const uint64_t window = 1ull << wlog;
  pow_ctx* ctx = NULL;
  CHECK(pow_init(0, &ctx));
  CHECK(pow_warmup(ctx));
  double* ms = malloc((size_t)calls * sizeof *ms);
  double* kms = malloc((size_t)calls * sizeof *kms);
  unsigned* launches = malloc((size_t)calls * sizeof *launches);
  unsigned long long* trials = malloc((size_t)calls * sizeof *trials);
  pow_block genesis;
  memset(&genesis, 0, sizeof genesis);
  genesis.difficulty = d; /* index 0, block_hash all zero */
  genesis.created_at = 1699999990u;
  for (int a = 6; a < argc; ++a) {
    const size_t R = (size_t)atol(argv[a]);
    if (R < 1 || R > POW_RACE_MAX_RIVALS) return 2;
    uint32_t* owners = calloc(R, sizeof *owners);
    uint64_t* created = calloc(n * R, sizeof *created);
    pow_block* out = calloc(n, sizeof *out);
    pow_block* tmpls = calloc(R, sizeof *tmpls);
    uint64_t* tctr = calloc(R, sizeof *tctr);
    uint32_t* winners = calloc(n, sizeof *winners);
    uint64_t* ctrs = calloc(n, sizeof *ctrs);
    for (size_t r = 0; r < R; ++r) owners[r] = (uint32_t)r;
    for (size_t k = 0; k < n; ++k)
      for (size_t r = 0; r < R; ++r) created[k * R + r] = 1700000000u + 17 * k + r;
    for (int c = -1; c < calls; ++c) { /* c = -1: discarded */
      double k_ms = 0;
      unsigned nl = 0;
      uint64_t nt = 0;
      const double t0 = now_ms();
      if (!by_batch) {
        size_t mined = 0;
        int rc = pow_mine_race(ctx, &genesis, n, d, owners, R, created, 0, window, NULL, 0, out, winners, ctrs, &mined, &nt);
        CHECK(rc);
        if (rc != 1) return fprintf(stderr, "%zu of %zu heights mined\n", mined, n), 1;
        pow_stats s;
        CHECK(pow_get_stats(ctx, &s));
        k_ms = s.kernel_ms;
        nl = s.launches;
      } else {
        for (size_t k = 0; k < n; ++k) {
          const pow_block* tip = k ? &out[n - k] : &genesis;
          for (size_t r = 0; r < R; ++r) { /* node.cpp:292-299 */
            tmpls[r] = *tip;
            tmpls[r].index = tip->index + 1;
            tmpls[r].node_owner_number = owners[r];
            tmpls[r].difficulty = d;
            tmpls[r].created_at = created[k * R + r];
            memcpy(tmpls[r].previous_block_hash, tip->block_hash, POW_HASH_SIZE);
          }
          size_t solved = 0;
          uint64_t hashes = 0;
          CHECK(pow_mine_batch(ctx, tmpls, R, d, 0, window, NULL, 0, tmpls, tctr, &solved, &hashes));
          if (solved == 0) return fprintf(stderr, "height %zu: no window held a solution\n", k), 1;
          size_t win = R;
          for (size_t r = 0; r < R; ++r)
            if (tctr[r] != UINT64_MAX && (win == R || tctr[r] < tctr[win])) win = r;
          out[n - 1 - k] = tmpls[win];
          winners[n - 1 - k] = (uint32_t)win;
          ctrs[n - 1 - k] = tctr[win];
          pow_stats s;
          pow_get_stats(ctx, &s); /* in the timed region on purpose: cheap, and examples/mine_race.c reads it too */
          k_ms += s.kernel_ms;
          nl += s.launches;
          nt += hashes;
        }
      }
      const double t1 = now_ms();
      if (c >= 0) {
        ms[c] = t1 - t0;
        kms[c] = k_ms;
        launches[c] = nl;
        trials[c] = nt;
      }
    }
    /* outside the timed region: the audit of what the last sample mined */
    size_t first_bad = 0, n_bad = 0;
    int valid = pow_verify_chain(ctx, out, n, d, NULL, &first_bad, &n_bad);
    CHECK(valid);
    uint64_t sum = fnv(14695981039346656037ull, out, n * sizeof *out);
    sum = fnv(sum, winners, n * sizeof *winners);
    sum = fnv(sum, ctrs, n * sizeof *ctrs);
    uint64_t solo = 0; /* the trials the race itself needs: every pair up to each winner's */
    for (size_t k = 0; k < n; ++k) solo += ctrs[k] * R + winners[k] + 1;
    printf("{\"mode\": \"%s\", \"d\": %u, \"window_log2\": %u, \"heights\": %zu, \"rivals\": %zu, \"valid\": %d, "
           "\"checksum\": \"%016llx\", \"pairs_needed\": %llu, \"ms\": [",
           argv[1], d, wlog, n, R, valid, (unsigned long long)sum, (unsigned long long)solo);
    for (int c = 0; c < calls; ++c) printf("%s%.4f", c ? ", " : "", ms[c]);
    printf("], \"kernel_ms\": [");
    for (int c = 0; c < calls; ++c) printf("%s%.4f", c ? ", " : "", kms[c]);
    printf("], \"launches\": [");
    for (int c = 0; c < calls; ++c) printf("%s%u", c ? ", " : "", launches[c]);
    printf("], \"trials\": [");
    for (int c = 0; c < calls; ++c) printf("%s%llu", c ? ", " : "", trials[c]);
    printf("]}\n");
    fflush(stdout);
    free(ctrs);
    free(winners);
    free(tctr);
    free(tmpls);
    free(out);
    free(created);
    free(owners);
  }
  pow_destroy(ctx);
  return 0;
}
