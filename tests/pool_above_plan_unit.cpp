// The per-lane test of the pool's descendant queries (K14) on the CPU:
// pow_above_member (csrc/pow_above_dev.h) over K13's table
// (csrc/pow_lift_dev.h), the code the subtree kernel of pow_pool_above.hip
// runs.  Linked with pow_host.cpp alone and run under AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_pool_above_host.py.  On every shape
// the table is built level by level with pow_lift_entry and every (block, root)
// pair, or every pair of a sample where that is too many, is held against a
// plain walk from the block:
//   a. flat chains of exactly 2^k and 2^k + 1 blocks, k = 0 .. 10, in order and
//      shuffled (the depth differences cross every table level, and
//      depth == 2^levels);
//   b. a two-arm tree: a trunk and two arms from its tip;
//   c. an orphan chain (its walk ends at POW_POOL_NONE) beside a rooted one;
//   d. depth[i] < depth[r]: the answer is no from the two depths alone; the
//      view has no parent array and no table there, so a read of either is a
//      null dereference.  This guards the early exit only, not an answer: on a
//      forest the jump could not reach r anyway (it stays on i's own walk), so
//      without the depth test every other case here still passes;
//   e. a root equal to the block, on every shape;
//   f. random forests with several roots and orphans.
// Every array is allocated at exactly its size, so ASan sees a read past it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "pow_above_dev.h"
#include "pow_gpu.h"
#include "pow_host.h"
#include "pow_lift_dev.h"

namespace {

long checks = 0, failed = 0;

#define CHECK(cond, ...)                \
  do {                                  \
    ++checks;                           \
    if (!(cond)) {                      \
      if (++failed <= 20) {             \
        printf("FAILED %s: ", #cond);   \
        printf(__VA_ARGS__);            \
        printf("\n");                   \
      }                                 \
    }                                   \
  } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t below) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((rng_state >> 33) % below);
}

struct Words {
  std::unique_ptr<uint32_t[]> p;
  explicit Words(size_t n) : p(n ? new uint32_t[n] : nullptr) {}
  uint32_t* get() const { return p.get(); }
};

// A forest with its depths by plain walks and its table as K13a makes it.
struct Forest {
  uint32_t n, rows;
  Words parent, depth, up;
  explicit Forest(const std::vector<uint32_t>& par)
      : n((uint32_t)par.size()), rows(pow_pool_lift_rows(n)), parent(n), depth(n), up((size_t)n * rows) {
    std::copy(par.begin(), par.end(), parent.get());
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t d = 0;
      for (uint32_t x = i; x < n; x = parent.get()[x]) ++d;
      depth.get()[i] = d;
    }
    for (uint32_t j = 1; j <= rows; ++j) {
      const uint32_t* const prev = j > 1u ? up.get() + (size_t)(j - 2u) * n : parent.get();
      for (uint32_t i = 0; i < n; ++i) up.get()[(size_t)(j - 1u) * n + i] = pow_lift_entry(prev, n, i);
    }
  }
  PowLiftView view() const { return PowLiftView{parent.get(), depth.get(), up.get(), n, n, pow_pool_rounds(n)}; }
  bool walks_past(uint32_t i, uint32_t r) const {
    for (uint32_t x = i; x < n; x = parent.get()[x])
      if (x == r) return true;
    return false;
  }
};

// Node `name[i]` stands where node i of `par` stood.
std::vector<uint32_t> renamed(const std::vector<uint32_t>& par, bool shuffle) {
  const uint32_t n = (uint32_t)par.size();
  std::vector<uint32_t> name(n), out(n);
  for (uint32_t i = 0; i < n; ++i) name[i] = i;
  if (shuffle)
    for (uint32_t i = n; i > 1; --i) std::swap(name[i - 1], name[rnd(i)]);
  for (uint32_t i = 0; i < n; ++i) out[name[i]] = par[i] < n ? name[par[i]] : par[i];
  return out;
}

// Every pair up to `all` nodes, else `sample` random pairs and every (i, i).
void check_forest(const char* what, const std::vector<uint32_t>& par, uint32_t all = 300, uint32_t sample = 200000) {
  const Forest f(par);
  const PowLiftView v = f.view();
  const uint32_t n = f.n;
  uint32_t members = 0;
  auto one = [&](uint32_t i, uint32_t r) {
    const bool got = pow_above_member(v, i, r), want = f.walks_past(i, r);
    members += got;
    CHECK(got == want, "%s: n %u block %u root %u: %d, the walk says %d", what, n, i, r, (int)got, (int)want);
  };
  for (uint32_t i = 0; i < n; ++i) one(i, i);
  CHECK(members == n, "%s: a root is a member of its own subtree", what);
  if (n <= all) {
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t r = 0; r < n; ++r) one(i, r);
  } else {
    for (uint32_t s = 0; s < sample; ++s) one(rnd(n), rnd(n));
  }
}

std::vector<uint32_t> chain_of(uint32_t n, uint32_t end) {
  std::vector<uint32_t> par(n);
  for (uint32_t i = 0; i < n; ++i) par[i] = i ? i - 1 : end;
  return par;
}

}  // namespace

int main() {
  // a. chains of 2^k and 2^k + 1
  for (uint32_t k = 0; k <= 10; ++k)
    for (uint32_t extra = 0; extra <= 1; ++extra)
      for (int shuffle = 0; shuffle <= 1; ++shuffle) {
        const uint32_t n = (1u << k) + extra;
        const std::vector<uint32_t> par = renamed(chain_of(n, POW_POOL_ROOT), shuffle != 0);
        check_forest("chain", par);
        const Forest f(par);
        const PowLiftView v = f.view();
        uint32_t tip = 0, root = 0;
        for (uint32_t i = 0; i < n; ++i) {
          if (f.depth.get()[i] == n) tip = i;
          if (f.depth.get()[i] == 1u) root = i;
        }
        uint32_t size = 0;
        for (uint32_t i = 0; i < n; ++i) size += pow_above_member(v, i, root);
        CHECK(size == n, "chain of %u: everything stands on the root (%u)", n, size);
        CHECK(pow_above_member(v, tip, root) && (n == 1u || !pow_above_member(v, root, tip)), "chain of %u: tip and root", n);
      }
  // b. two arms from a trunk's tip
  for (int shuffle = 0; shuffle <= 1; ++shuffle) {
    const uint32_t trunk = 70, arm_a = 130, arm_b = 57;
    std::vector<uint32_t> par = chain_of(trunk, POW_POOL_ROOT);
    for (uint32_t i = 0; i < arm_a; ++i) par.push_back(i ? (uint32_t)par.size() - 1u : trunk - 1u);
    for (uint32_t i = 0; i < arm_b; ++i) par.push_back(i ? (uint32_t)par.size() - 1u : trunk - 1u);
    check_forest("two arms", renamed(par, shuffle != 0));
    if (!shuffle) {
      const Forest f(par);
      const PowLiftView v = f.view();
      uint32_t on_a = 0, on_tip = 0;
      for (uint32_t i = 0; i < f.n; ++i) on_a += pow_above_member(v, i, trunk), on_tip += pow_above_member(v, i, trunk - 1u);
      CHECK(on_a == arm_a && on_tip == 1u + arm_a + arm_b, "two arms: %u on the first arm, %u on the trunk's tip", on_a, on_tip);
      CHECK(!pow_above_member(v, trunk + arm_a, trunk), "two arms: the second arm's first block is not on the first arm");
    }
  }
  // c. an orphan chain beside a rooted one
  for (int shuffle = 0; shuffle <= 1; ++shuffle) {
    std::vector<uint32_t> par = chain_of(33, POW_POOL_NONE);
    for (uint32_t i = 0; i < 65; ++i) par.push_back(i ? (uint32_t)par.size() - 1u : POW_POOL_ROOT);
    check_forest("orphans", renamed(par, shuffle != 0));
  }
  // d. depth[i] < depth[r]: decided by the two depths; nothing else exists to be read (the early exit, not an answer)
  {
    const uint32_t depth[4] = {1, 2, 3, 7};
    const PowLiftView v{nullptr, depth, nullptr, 4, 4, 2};
    for (uint32_t i = 0; i < 4; ++i)
      for (uint32_t r = i + 1; r < 4; ++r) CHECK(!pow_above_member(v, i, r), "block %u is not as deep as root %u", i, r);
  }
  // f. random forests
  for (uint32_t n : {1u, 2u, 3u, 64u, 65u, 255u, 256u, 257u, 1000u, 5000u}) {
    std::vector<uint32_t> par(n);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t dice = rnd(100);
      if (i == 0 || dice < 3) par[i] = POW_POOL_ROOT;
      else if (dice < 6) par[i] = POW_POOL_NONE;
      else if (dice < 70) par[i] = i - 1;
      else par[i] = rnd(i);
    }
    check_forest("forest", renamed(par, true));
  }
  printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
