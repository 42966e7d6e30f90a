// The host plan and the per-lane walks of the pool's ancestry queries (K13) on
// the CPU: pow_pool_lift_rows, _bytes and _launches (csrc/pow_host.cpp) and the
// functions of csrc/pow_lift_dev.h, the code the kernels of pow_pool_lift.hip
// run.  Linked with pow_host.cpp alone and run under AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_pool_lift_host.py.
//   a. rows, bytes and launches against hand-computed cases;
//   b. the table of a forest built level by level (the stale case), then
//      ancestor and fork point against plain walks;
//   c. the same forest fed in batches of 1, 256 and 257 blocks and the table
//      extended as the plan says it would be (the one-workgroup form level by
//      level with a hand-off array, the wide form row by row, then the new
//      rows over all blocks): the launches counted equal the plan's, the table
//      equals the one built from nothing, and the queries are checked again;
//   d. flat chains of exactly 64 and 65 blocks;
//   e. the pool's full depth against closed forms, since plain walks are
//      quadratic there: lists of exactly 2^k and 2^k + 1 nodes for k = 7 .. 20
//      (depth == 2^levels), a shuffled list of 2^20 with every row entry and
//      every step count from its tip, four two-arm shapes of about 2^20 nodes,
//      and the batches (2^19 - 100, 2^19 + 100) and (2^20 - 256, 2^20) through
//      the batch model of c.
// Every array is allocated at exactly its size, so ASan sees a read past it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

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

// Heap arrays of exactly n words (n = 0: a one-word array that nobody may read is avoided too).
struct Words {
  std::unique_ptr<uint32_t[]> p;
  explicit Words(size_t n) : p(n ? new uint32_t[n] : nullptr) {}
  uint32_t* get() const { return p.get(); }
};

struct Forest {
  uint32_t n;
  Words parent, depth;
  explicit Forest(uint32_t n_) : n(n_), parent(n_), depth(n_) {}
  void rank() {  // depth by plain walks
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t d = 0;
      for (uint32_t x = i; x < n; x = parent.get()[x]) ++d;
      depth.get()[i] = d;
    }
  }
};

// parent[i] < i or an end, long chains likely; then every batch [cut[b], cut[b+1]) is shuffled inside itself.
Forest random_forest(const std::vector<uint32_t>& cut) {
  const uint32_t n = cut.back();
  std::vector<uint32_t> par(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t dice = rnd(100);
    if (i == 0 || dice < 3) par[i] = POW_POOL_ROOT;
    else if (dice < 6) par[i] = POW_POOL_NONE;
    else if (dice < 80) par[i] = i - 1;
    else par[i] = rnd(i);
  }
  std::vector<uint32_t> name(n);
  for (uint32_t i = 0; i < n; ++i) name[i] = i;
  for (size_t b = 0; b + 1 < cut.size(); ++b)
    for (uint32_t i = cut[b + 1]; i > cut[b] + 1; --i) std::swap(name[i - 1], name[cut[b] + rnd(i - cut[b])]);
  Forest f(n);
  for (uint32_t i = 0; i < n; ++i) f.parent.get()[name[i]] = par[i] < n ? name[par[i]] : par[i];
  f.rank();
  return f;
}

struct Table {
  uint32_t cap, covered = 0;
  Words up;
  explicit Table(uint32_t cap_) : cap(cap_), up((size_t)cap_ * pow_pool_lift_rows(cap_)) {}
  uint32_t* row(uint32_t j) const { return up.get() + (size_t)(j - 1) * cap; }
  const uint32_t* level(const uint32_t* parent, uint32_t j) const { return j ? row(j) : parent; }
};

// What a query call does to the table for a pool of `size`; returns the launches.
uint32_t bring_up(Table& t, const uint32_t* parent, uint32_t size, bool stale) {
  const uint32_t covered = stale ? 0 : t.covered, m = size - covered;
  const uint32_t have = stale ? 0 : pow_pool_lift_rows(covered), rows = pow_pool_lift_rows(size);
  uint32_t launches = 0;
  if (m && have) {
    if (m <= POW_POOL_LIFT_SMALL) {  // K13b: levels in order, a lane's previous level handed on through an array
      ++launches;
      std::vector<uint32_t> mine(m), hand(m);
      for (uint32_t k = 0; k < m; ++k) mine[k] = parent[covered + k];
      for (uint32_t j = 1; j <= have; ++j) {
        hand = mine;
        for (uint32_t k = 0; k < m; ++k) {
          if (mine[k] < size) mine[k] = mine[k] >= covered ? hand[mine[k] - covered] : t.level(parent, j - 1)[mine[k]];
          t.row(j)[covered + k] = mine[k];
        }
      }
    } else {
      for (uint32_t j = 1; j <= have; ++j, ++launches)
        for (uint32_t i = covered; i < size; ++i) t.row(j)[i] = pow_lift_entry(t.level(parent, j - 1), size, i);
    }
  }
  for (uint32_t j = have + 1; j <= rows; ++j, ++launches)
    for (uint32_t i = 0; i < size; ++i) t.row(j)[i] = pow_lift_entry(t.level(parent, j - 1), size, i);
  t.covered = size;
  return launches;
}

uint32_t walk(const uint32_t* parent, uint32_t n, uint32_t pos, uint32_t steps) {
  for (uint32_t s = 0; s < steps && pos < n; ++s) pos = parent[pos];
  return pos;
}

// The first block on a's walk that is on b's: by plain walks and a mark per block.
uint32_t plain_fork(const Forest& f, uint32_t a, uint32_t b, uint32_t* back_a, uint32_t* back_b) {
  std::vector<uint32_t> at_b(f.n, 0xFFFFFFFFu);
  uint32_t s = 0;
  for (uint32_t x = b; x < f.n; x = f.parent.get()[x]) at_b[x] = s++;
  s = 0;
  for (uint32_t x = a; x < f.n; x = f.parent.get()[x], ++s)
    if (at_b[x] != 0xFFFFFFFFu) {
      *back_a = s, *back_b = at_b[x];
      return x;
    }
  *back_a = f.depth.get()[a], *back_b = f.depth.get()[b];
  return POW_POOL_NONE;
}

// The first `size` blocks of f (closed under parent by construction) as a forest with arrays of exactly `size`.
Forest prefix(const Forest& f, uint32_t size) {
  Forest g(size);
  for (uint32_t i = 0; i < size; ++i) g.parent.get()[i] = f.parent.get()[i], g.depth.get()[i] = f.depth.get()[i];
  return g;
}

void check_queries(const Forest& f, const Table& t, uint32_t pairs, const char* what) {
  const uint32_t n = f.n;
  const PowLiftView v{f.parent.get(), f.depth.get(), t.up.get(), t.cap, n, pow_pool_rounds(n)};
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t d = f.depth.get()[i];
    const uint32_t steps[] = {0u, d - 1u, d, d + 1u, 0xFFFFFFFFu, rnd(d + 2u), 1u, 2u, d / 2u};
    for (uint32_t s : steps) {
      const uint32_t got = pow_lift_ancestor(v, i, s), want = walk(f.parent.get(), n, i, s);
      CHECK(got == want, "%s: ancestor(%u, %u) of %u blocks = %u, the walk gives %u", what, i, s, n, got, want);
    }
  }
  for (uint32_t q = 0; q < pairs; ++q) {
    const uint32_t a = q < n ? q : rnd(n), b = q < n ? (q * 7u + 3u) % n : rnd(n);
    uint32_t ba = 7, bb = 7, wa = 0, wb = 0;
    const uint32_t got = pow_lift_fork(v, a, b, &ba, &bb), want = plain_fork(f, a, b, &wa, &wb);
    CHECK(got == want && ba == wa && bb == wb, "%s: fork(%u, %u) of %u blocks = %u (%u, %u), the walks give %u (%u, %u)",
          what, a, b, n, got, ba, bb, want, wa, wb);
  }
  for (uint32_t i = 0; i < n && i < 300; ++i) {  // a == b, and a block against its parent
    uint32_t ba = 7, bb = 7;
    CHECK(pow_lift_fork(v, i, i, &ba, &bb) == i && ba == 0 && bb == 0, "%s: fork(%u, %u)", what, i, i);
    const uint32_t p = f.parent.get()[i];
    if (p < n) CHECK(pow_lift_fork(v, i, p, &ba, &bb) == p && ba == 1 && bb == 0, "%s: fork(%u, parent %u)", what, i, p);
  }
}

void plan_by_hand() {
  const struct { uint32_t n, rows; } rows[] = {{0, 0}, {1, 0}, {2, 0}, {3, 1}, {4, 1}, {5, 2}, {64, 5}, {65, 6}, {1u << 20, 19}};
  for (const auto& r : rows) CHECK(pow_pool_lift_rows(r.n) == r.rows, "rows(%u) = %u", r.n, pow_pool_lift_rows(r.n));
  const struct { uint32_t cap; uint64_t bytes; } bytes[] = {{0, 0}, {1, 0}, {2, 0}, {3, 12}, {4, 16}, {5, 40}, {64, 1280},
                                                            {65, 1560}, {1u << 20, 79691776ull}};
  for (const auto& b : bytes)
    CHECK(pow_pool_lift_bytes(b.cap) == b.bytes, "bytes(%u) = %llu", b.cap, (unsigned long long)pow_pool_lift_bytes(b.cap));
  const struct { uint32_t covered, size; bool stale; uint32_t launches; } plan[] = {
      {0, 0, true, 0}, {0, 1, true, 0}, {0, 2, true, 0}, {0, 3, true, 1}, {0, 4, true, 1}, {0, 5, true, 2},
      {0, 64, true, 5}, {0, 65, true, 6}, {0, 1u << 20, true, 19}, {40, 64, true, 5},  // stale: whatever it covered
      {1, 1, false, 0}, {64, 64, false, 0}, {1u << 20, 1u << 20, false, 0},           // up to date
      {1, 2, false, 0}, {2, 3, false, 1}, {3, 4, false, 1}, {4, 5, false, 2},          // m = 1
      {63, 64, false, 1}, {64, 65, false, 2}, {65, 66, false, 1}, {(1u << 20) - 1, 1u << 20, false, 1},
      {600, 856, false, 1}, {600, 857, false, 9},                                      // m = 256, 257: 9 rows
      {300, 556, false, 2}, {300, 557, false, 9},                                      // ... past 512: 8 rows and a new one
      {1, 257, false, 8}, {2, 258, false, 8}, {1000, 1257, false, 10}, {64, 320, false, 4}};
  for (const auto& c : plan)
    CHECK(pow_pool_lift_launches(c.covered, c.size, c.stale) == c.launches, "launches(%u, %u, %d) = %u, by hand %u",
          c.covered, c.size, (int)c.stale, pow_pool_lift_launches(c.covered, c.size, c.stale), c.launches);
  CHECK(POW_LIFT_MAX_LEVELS == pow_pool_rounds(POW_POOL_MAX_BLOCKS) && POW_LIFT_NONE == POW_POOL_NONE, "the header's constants");
}

void forest_in_batches(const std::vector<uint32_t>& cut, uint32_t pairs) {
  const Forest f = random_forest(cut);
  const uint32_t n = f.n;
  Table whole(n);
  CHECK(bring_up(whole, f.parent.get(), n, true) == pow_pool_lift_launches(0, n, true), "stale launches of %u", n);
  check_queries(f, whole, pairs, "built from nothing");
  Table fed(n);
  for (size_t b = 0; b + 1 < cut.size(); ++b) {
    const uint32_t size = cut[b + 1];
    const Forest g = prefix(f, size);  // arrays of exactly `size`: what the pool holds after this batch
    const bool stale = fed.covered == 0;
    const uint32_t want = pow_pool_lift_launches(fed.covered, size, stale);
    const uint32_t got = bring_up(fed, g.parent.get(), size, stale);
    CHECK(got == want, "batch to %u blocks: %u launches, the plan says %u", size, got, want);
    Table fresh(n);
    bring_up(fresh, g.parent.get(), size, true);
    for (uint32_t j = 1; j <= pow_pool_lift_rows(size); ++j)
      for (uint32_t i = 0; i < size; ++i)
        CHECK(fed.row(j)[i] == fresh.row(j)[i], "after the batch to %u: row %u of block %u is %u, from nothing %u", size, j, i,
              fed.row(j)[i], fresh.row(j)[i]);
    check_queries(g, fed, size <= 8 ? 64 : pairs / 4, "fed in batches");
  }
}

void flat_chain(uint32_t n) {
  Forest f(n);
  for (uint32_t i = 0; i < n; ++i) f.parent.get()[i] = i ? i - 1 : POW_POOL_ROOT;
  f.rank();
  Table t(n);
  bring_up(t, f.parent.get(), n, true);
  const PowLiftView v{f.parent.get(), f.depth.get(), t.up.get(), t.cap, n, pow_pool_rounds(n)};
  CHECK(f.depth.get()[n - 1] == n, "depth of the tip");
  CHECK(pow_lift_ancestor(v, n - 1, n - 1) == 0, "chain of %u: the root", n);
  CHECK(pow_lift_ancestor(v, n - 1, n) == POW_POOL_ROOT, "chain of %u: the end", n);
  CHECK(pow_lift_ancestor(v, n - 1, 0xFFFFFFFFu) == POW_POOL_ROOT, "chain of %u: the end from afar", n);
  check_queries(f, t, n * n, "flat chain");
}

// ---- the pool's full depth: up to POW_POOL_MAX_BLOCKS nodes, against closed forms (plain walks are quadratic here) ----

// One list whose node at height h is order[h - 1] and whose last parent is
// `end`.  The first `covered` heights take the positions below `covered`, the
// rest those behind, each shuffled among themselves: the prefix is closed.
struct List {
  Forest f;
  std::vector<uint32_t> order;
  uint32_t end;
};

void shuffle(std::vector<uint32_t>& v, uint32_t lo, uint32_t hi) {
  for (uint32_t i = hi; i > lo + 1; --i) std::swap(v[i - 1], v[lo + rnd(i - lo)]);
}

List shuffled_list(uint32_t n, uint32_t covered, uint32_t end) {
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  shuffle(order, 0, covered);
  shuffle(order, covered, n);
  Forest f(n);
  for (uint32_t h = 0; h < n; ++h) f.parent.get()[order[h]] = h ? order[h - 1] : end, f.depth.get()[order[h]] = h + 1;
  return List{std::move(f), std::move(order), end};
}

// The step counts where a level's bit comes or goes, around a walk of d blocks.
std::vector<uint32_t> seam_steps(uint32_t d) {
  std::vector<uint32_t> s = {0u, d - 2u, d - 1u, d, d + 1u, 0xFFFFFFFFu, 0xFFFFFFFEu};
  for (uint32_t j = 0; j <= 20; ++j)
    for (uint32_t x : {(1u << j) - 1u, 1u << j, (1u << j) + 1u}) s.push_back(x);
  return s;
}

void check_list_rows(const List& l, const Table& t, const char* what) {
  const uint32_t n = l.f.n;
  for (uint32_t j = 1; j <= pow_pool_lift_rows(n); ++j)
    for (uint32_t h = 0; h < n; ++h) {
      const uint32_t want = h >= (1u << j) ? l.order[h - (1u << j)] : l.end, got = t.row(j)[l.order[h]];
      CHECK(got == want, "%s of %u: row %u at height %u is %u, by the order %u", what, n, j, h + 1, got, want);
    }
}

// every_step: every step count from the tip, else the seams only; from `sample`
// random heights the seams; `pairs` fork points.
void check_list_queries(const List& l, const Table& t, bool every_step, uint32_t sample, uint32_t pairs, const char* what) {
  const uint32_t n = l.f.n;
  const PowLiftView v{l.f.parent.get(), l.f.depth.get(), t.up.get(), t.cap, n, pow_pool_rounds(n)};
  auto ancestor = [&](uint32_t h, uint32_t s) {  // from the node at height h + 1
    const uint32_t got = pow_lift_ancestor(v, l.order[h], s), want = s <= h ? l.order[h - s] : l.end;
    CHECK(got == want, "%s of %u: ancestor(height %u, %u) = %u, by the order %u", what, n, h + 1, s, got, want);
  };
  if (every_step)
    for (uint32_t s = 0; s <= n + 1u; ++s) ancestor(n - 1u, s);
  for (uint32_t s : seam_steps(n)) ancestor(n - 1u, s);
  for (uint32_t q = 0; q < sample; ++q) {
    const uint32_t h = q < 3 ? q % n : rnd(n);
    for (uint32_t s : seam_steps(h + 1u)) ancestor(h, s);
  }
  for (uint32_t q = 0; q < pairs; ++q) {
    const uint32_t ha = q == 0 ? n - 1u : rnd(n), hb = q < 2 ? 0u : q % 97u == 0 ? ha : rnd(n), lo = std::min(ha, hb);
    uint32_t ba = 7, bb = 7;
    const uint32_t got = pow_lift_fork(v, l.order[ha], l.order[hb], &ba, &bb);
    CHECK(got == l.order[lo] && ba == ha - lo && bb == hb - lo, "%s of %u: fork(heights %u, %u) = %u (%u, %u)", what, n, ha + 1,
          hb + 1, got, ba, bb);
  }
}

// A list of exactly n nodes: depth == 2^levels when n is a power of two.
void deep_chain(uint32_t n) {
  const List l = shuffled_list(n, 0, n & 2u ? POW_POOL_NONE : POW_POOL_ROOT);
  Table t(n);
  CHECK(bring_up(t, l.f.parent.get(), n, true) == pow_pool_lift_rows(n), "launches of %u", n);
  const PowLiftView v{l.f.parent.get(), l.f.depth.get(), t.up.get(), t.cap, n, pow_pool_rounds(n)};
  const uint32_t tip = l.order[n - 1];
  CHECK(l.f.depth.get()[tip] == n, "depth of the tip");
  CHECK(pow_lift_ancestor(v, tip, n - 1) == l.order[0], "list of %u: the root", n);
  CHECK(pow_lift_ancestor(v, tip, n) == l.end, "list of %u: the end", n);
  CHECK(pow_lift_ancestor(v, tip, 0xFFFFFFFFu) == l.end, "list of %u: the end from afar", n);
  check_list_queries(l, t, false, 200, 2000, "list");
}

void deep_list(uint32_t n) {
  const List l = shuffled_list(n, 0, POW_POOL_ROOT);
  Table t(n);
  bring_up(t, l.f.parent.get(), n, true);
  check_list_rows(l, t, "list");
  check_list_queries(l, t, true, 2000, 200000, "every step");
}

// A list over the first `covered` positions, its table as a pool of that size
// had it, then the rest as one batch: the launches, every entry against the
// table made from nothing and against the closed form, then the queries.
void deep_extension(uint32_t covered, uint32_t n) {
  const List l = shuffled_list(n, covered, POW_POOL_ROOT);
  Table fed(n);
  {
    const Forest g = prefix(l.f, covered);  // arrays of exactly `covered`
    bring_up(fed, g.parent.get(), covered, true);
  }
  const uint32_t got = bring_up(fed, l.f.parent.get(), n, false), want = pow_pool_lift_launches(covered, n, false);
  CHECK(got == want, "from %u to %u blocks: %u launches, the plan says %u", covered, n, got, want);
  Table fresh(n);
  bring_up(fresh, l.f.parent.get(), n, true);
  for (uint32_t j = 1; j <= pow_pool_lift_rows(n); ++j)
    for (uint32_t i = 0; i < n; ++i)
      CHECK(fed.row(j)[i] == fresh.row(j)[i], "from %u to %u: row %u of block %u is %u, from nothing %u", covered, n, j, i,
            fed.row(j)[i], fresh.row(j)[i]);
  check_list_rows(l, fed, "extended");
  check_list_queries(l, fed, false, 500, 20000, "extended");
}

// Two lists that share a trunk, positions shuffled: the fork point of a pair is
// the lower node if both lie on one line, else the trunk's top.
void deep_arms(uint32_t trunk, uint32_t arm_a, uint32_t arm_b, uint32_t pairs) {
  const uint32_t n = trunk + arm_a + arm_b;
  std::vector<uint32_t> perm(n);
  for (uint32_t i = 0; i < n; ++i) perm[i] = i;
  shuffle(perm, 0, n);
  Forest f(n);
  std::vector<uint8_t> side(n, 0);
  for (uint32_t h = 0; h < trunk + arm_a; ++h) {  // line A: the trunk, then arm A
    f.parent.get()[perm[h]] = h ? perm[h - 1] : POW_POOL_ROOT, f.depth.get()[perm[h]] = h + 1;
    if (h >= trunk) side[perm[h]] = 1;
  }
  for (uint32_t k = 0; k < arm_b; ++k) {
    const uint32_t i = perm[trunk + arm_a + k];
    f.parent.get()[i] = k ? perm[trunk + arm_a + k - 1] : perm[trunk - 1], f.depth.get()[i] = trunk + k + 1, side[i] = 2;
  }
  Table t(n);
  bring_up(t, f.parent.get(), n, true);
  const PowLiftView v{f.parent.get(), f.depth.get(), t.up.get(), t.cap, n, pow_pool_rounds(n)};
  const uint32_t top = perm[trunk - 1];
  auto fork = [&](uint32_t a, uint32_t b) {
    const uint32_t da = f.depth.get()[a], db = f.depth.get()[b];
    const bool across = side[a] && side[b] && side[a] != side[b];
    const uint32_t at = across ? top : da <= db ? a : b, to = across ? trunk : std::min(da, db);
    uint32_t ba = 7, bb = 7;
    const uint32_t got = pow_lift_fork(v, a, b, &ba, &bb);
    CHECK(got == at && ba == da - to && bb == db - to, "arms %u + %u, %u: fork(%u, %u) = %u (%u, %u), closed form %u (%u, %u)", trunk,
          arm_a, arm_b, a, b, got, ba, bb, at, da - to, db - to);
  };
  auto node_a = [&](uint32_t h) { return perm[trunk + h - 1]; };          // arm A at height h (1 .. arm_a) above the trunk
  auto node_b = [&](uint32_t h) { return perm[trunk + arm_a + h - 1]; };  // arm B
  std::vector<uint32_t> ha, hb;
  for (uint32_t s : seam_steps(arm_a))
    if (s >= 1 && s <= arm_a) ha.push_back(s);
  for (uint32_t s : seam_steps(arm_b))
    if (s >= 1 && s <= arm_b) hb.push_back(s);
  for (uint32_t x : ha)
    for (uint32_t y : hb) fork(node_a(x), node_b(y)), fork(node_b(y), node_a(x));
  for (uint32_t s : seam_steps(trunk))
    if (s >= 1 && s <= trunk) {  // one line: against the trunk
      fork(node_a(arm_a), perm[s - 1]), fork(perm[s - 1], node_b(arm_b)), fork(perm[s - 1], perm[s - 1]);
      if (s > 1) fork(perm[s - 1], perm[s - 2]), fork(perm[s - 2], perm[s - 1]);
    }
  for (uint32_t q = 0; q < pairs; ++q) fork(rnd(n), rnd(n));
  for (uint32_t i = 0; i < n; i += 1 + n / 5000) {  // a == b, and a block against its parent
    fork(i, i);
    if (f.parent.get()[i] < n) fork(i, f.parent.get()[i]), fork(f.parent.get()[i], i);
  }
}

}  // namespace

int main() {
  plan_by_hand();
  for (uint32_t k = 7; k <= 20; ++k) {
    deep_chain(1u << k);
    if (k < 20) deep_chain((1u << k) + 1u);  // 2^20 + 1 is past POW_POOL_MAX_BLOCKS
  }
  deep_list(1u << 20);
  deep_arms(1u << 19, 1u << 18, (1u << 18) - 1u, 50000);
  deep_arms(1u, 1u << 19, (1u << 19) - 2u, 50000);
  deep_arms((1u << 19) + 1u, 1u, (1u << 19) - 2u, 50000);
  deep_arms((1u << 20) - 2u, 1u, 1u, 50000);
  deep_extension((1u << 19) - 100u, (1u << 19) + 100u);
  deep_extension((1u << 20) - 256u, 1u << 20);
  for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 64u, 65u}) flat_chain(n);
  forest_in_batches({0, 1, 2, 3, 4, 5, 261, 518, 519, 775, 1032, 1033}, 4000);  // + 1, + 256, + 257, across 512 and 1,024
  forest_in_batches({0, 300, 556, 813}, 4000);                                  // the GPU test's seam
  forest_in_batches({0, 64, 65, 128, 129}, 2000);
  for (int k = 0; k < 20; ++k) forest_in_batches({0, 1 + rnd(40), 50 + rnd(300), 400 + rnd(300)}, 1000);
  printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
