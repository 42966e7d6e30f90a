// The CPU side of tools/index_blocks_bench.py, as a small shared library
// (g++ -O2 -shared): pools to measure on, and the two baselines' host work.
//
//   pool_make        a forked pool at difficulty 0 (any nonce solves): a trunk
//                    of half the blocks on one root, the rest as `branches`
//                    chains that all fork from the trunk's tip.
//   pool_make_race   the published shape as a pool: at every height `rivals`
//                    blocks on the block of rival 0 of the height below, on a
//                    root.  Every loser is a tip: the forks a race leaves.
//   pool_ref_audit   what the reference does with such a pool, in our words:
//                    node_blocks as std::map<std::string, Block> keyed on the
//                    stored text, then the walk of sanity_test by
//                    previous_block_hash from every tip (a block nobody names),
//                    with block_to_hash, the work test, the link and the index
//                    per block; the sound tip of the highest index wins.
//   pool_extract     today's way's host part: the same map and tips, and every
//                    tip's chain copied out tip first, back to back, ready for
//                    one pow_verify_chains call.
//   pool_walk_fork,  tools/pool_lift_bench.py's baselines: the fork point of two
//   pool_walk_chain  blocks and the chain under a tip by plain walks along a
//                    host copy of parent[] and depth[].
//
// SHA-256 is written out here (FIPS 180-4) so that the library needs nothing
// but the C++ runtime.
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "pow_gpu.h"

namespace {

const uint32_t K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

void compress(uint32_t h[8], const uint8_t* p) {
  uint32_t w[64];
  for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
  for (int i = 16; i < 64; ++i) {
    const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
    const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
    w[i] = w[i - 16] + s0 + w[i - 7] + s1;
  }
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7];
  for (int i = 0; i < 64; ++i) {
    const uint32_t t1 = k + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
    const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    k = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
  }
  h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += k;
}

// block_to_hash: the 270-byte message (the low byte of index, owner,
// difficulty and created_at, the nonce, previous_block_hash), its digest's
// lowercase hex.  Returns the digest's leading zero bits.
unsigned block_to_hash(const pow_block& b, char hex[65]) {
  uint8_t m[320] = {0};
  m[0] = (uint8_t)b.index, m[1] = (uint8_t)b.node_owner_number, m[2] = (uint8_t)b.difficulty, m[3] = (uint8_t)b.created_at;
  memcpy(m + 4, b.nonce, POW_NONCE_SIZE);
  memcpy(m + 4 + POW_NONCE_SIZE, b.previous_block_hash, POW_HASH_SIZE);
  m[POW_MSG_BYTES] = 0x80;
  m[318] = (uint8_t)((POW_MSG_BYTES * 8) >> 8), m[319] = (uint8_t)(POW_MSG_BYTES * 8);
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  for (int c = 0; c < 5; ++c) compress(h, m + 64 * c);
  unsigned zeros = 0;
  bool counting = true;
  for (int i = 0; i < 8; ++i) {
    for (int n = 7; n >= 0; --n) hex[8 * i + 7 - n] = "0123456789abcdef"[(h[i] >> (4 * n)) & 15];
    if (counting) {
      zeros += h[i] ? (unsigned)__builtin_clz(h[i]) : 32u;
      counting = h[i] == 0;
    }
  }
  hex[64] = 0;
  return zeros;
}

void seal_child(pow_block& b, const pow_block* parent, uint32_t index, uint32_t owner) {
  memset(&b, 0, sizeof b);
  b.index = index;
  b.node_owner_number = owner;
  b.created_at = 1700000000ull + index;
  memcpy(b.nonce, "aaaaaaaaa", POW_NONCE_SIZE);
  if (parent) memcpy(b.previous_block_hash, parent->block_hash, POW_HASH_SIZE);
  block_to_hash(b, b.block_hash);
}

std::string text(const char* field) { return std::string(field, strnlen(field, POW_HASH_SIZE)); }

// The tips of a pool: the blocks whose stored text nobody carries as previous_block_hash.
template <class Map>
std::vector<const pow_block*> tips_of(const Map& blocks) {
  std::set<std::string> named;
  for (const auto& kv : blocks) named.insert(text(kv.second.previous_block_hash));
  std::vector<const pow_block*> tips;
  for (const auto& kv : blocks)
    if (!named.count(kv.first)) tips.push_back(&kv.second);
  return tips;
}

}  // namespace

extern "C" {

void pool_make(pow_block* out, size_t n, size_t branches) {
  const size_t trunk = branches && n > 2 * branches ? n / 2 : n;
  for (size_t k = 0; k < trunk; ++k) seal_child(out[k], k ? &out[k - 1] : nullptr, (uint32_t)k, 0);
  size_t at = trunk;
  for (size_t b = 0; b < branches && at < n; ++b) {
    const size_t len = (n - at) / (branches - b);
    for (size_t k = 0; k < len; ++k, ++at)
      seal_child(out[at], k ? &out[at - 1] : &out[trunk - 1], (uint32_t)(trunk + k), (uint32_t)(b + 1));
  }
}

// heights x rivals + 1 blocks.
void pool_make_race(pow_block* out, size_t heights, size_t rivals) {
  seal_child(out[0], nullptr, 0, 0);
  const pow_block* tip = &out[0];
  for (size_t h = 0; h < heights; ++h) {
    for (size_t r = 0; r < rivals; ++r) seal_child(out[1 + h * rivals + r], tip, (uint32_t)(h + 1), (uint32_t)r);
    tip = &out[1 + h * rivals];
  }
}

// Returns the number of sound tips; *best = the pool position of the winning one (SIZE_MAX: none).
size_t pool_ref_audit(const pow_block* pool, size_t n, unsigned diff, size_t* n_tips, size_t* best, uint64_t* hashed) {
  std::map<std::string, pow_block> node_blocks;
  for (size_t i = 0; i < n; ++i) node_blocks.insert({text(pool[i].block_hash), pool[i]});
  const std::vector<const pow_block*> tips = tips_of(node_blocks);
  size_t sound = 0;
  uint64_t count = 0;
  const pow_block* win = nullptr;
  for (const pow_block* tip : tips) {
    const pow_block* cur = tip;
    bool ok = true;
    while (ok) {
      char hex[65];
      ++count;
      ok = block_to_hash(*cur, hex) >= diff && text(cur->block_hash) == hex;
      if (!ok || cur->previous_block_hash[0] == 0) break;
      const auto it = node_blocks.find(text(cur->previous_block_hash));
      ok = it != node_blocks.end() && cur->index - 1u == it->second.index;
      if (ok) cur = &it->second;
    }
    if (ok) {
      ++sound;
      if (!win || tip->index > win->index) win = tip;
    }
  }
  *n_tips = tips.size();
  *hashed = count;
  *best = SIZE_MAX;
  if (win)
    for (size_t i = 0; i < n; ++i)
      if (memcmp(&pool[i], win, sizeof(pow_block)) == 0) {
        *best = i;
        break;
      }
  return sound;
}

// ---- tools/pool_add_bench.py: a pool that is fed ----

// m blocks in a chain on `parent` (owner tells them from the pool's own).
void pool_extend(const pow_block* parent, pow_block* out, size_t m, uint32_t owner) {
  for (size_t k = 0; k < m; ++k) seal_child(out[k], k ? &out[k - 1] : parent, parent->index + 1 + (uint32_t)k, owner);
}

// The reference's node_blocks, kept between arrivals.
void* pool_ref_new(const pow_block* pool, size_t n) {
  auto* blocks = new std::map<std::string, pow_block>;
  for (size_t i = 0; i < n; ++i) blocks->insert({text(pool[i].block_hash), pool[i]});
  return blocks;
}

void pool_ref_free(void* handle) { delete (std::map<std::string, pow_block>*)handle; }

// What an arrival costs the reference, in our words: the m blocks into
// node_blocks (node.cpp:199, 319), then the sanity_test walk from the last of
// them (node.cpp:100-148) with block_to_hash, the work test, the link and the
// index per block.  Returns 1 if the walk is sound down to a root; *blocks_walked
// counts it.  The blocks are taken out again behind the caller's clock
// (pool_ref_drop), so that every repetition meets the same pool.
int pool_ref_add(void* handle, const pow_block* add, size_t m, unsigned diff, uint64_t* blocks_walked) {
  auto& node_blocks = *(std::map<std::string, pow_block>*)handle;
  for (size_t i = 0; i < m; ++i) node_blocks.insert({text(add[i].block_hash), add[i]});
  const pow_block* cur = &node_blocks.find(text(add[m - 1].block_hash))->second;
  uint64_t count = 0;
  bool ok = true;
  while (ok) {
    char hex[65];
    ++count;
    ok = block_to_hash(*cur, hex) >= diff && text(cur->block_hash) == hex;
    if (!ok || cur->previous_block_hash[0] == 0) break;
    const auto it = node_blocks.find(text(cur->previous_block_hash));
    ok = it != node_blocks.end() && cur->index - 1u == it->second.index;
    if (ok) cur = &it->second;
  }
  *blocks_walked = count;
  return ok ? 1 : 0;
}

void pool_ref_drop(void* handle, const pow_block* add, size_t m) {
  auto& node_blocks = *(std::map<std::string, pow_block>*)handle;
  for (size_t i = 0; i < m; ++i) node_blocks.erase(text(add[i].block_hash));
}

// ---- tools/pool_lift_bench.py: the walks a host does along a copy of parent[] ----

// The fork point of a and b by plain walks, as a node without the device's
// table finds it: the deeper side steps down to the other's depth, then both
// step together until they meet.  parent, depth: n entries as pow_pool_read
// gives them.  Returns the block (0xFFFFFFFE: none) and the steps on either side.
uint32_t pool_walk_fork(const uint32_t* parent, const uint32_t* depth, size_t n, uint32_t a, uint32_t b, uint32_t* back_a,
                        uint32_t* back_b) {
  uint32_t x = a, y = b, sa = 0, sb = 0, da = depth[a], db = depth[b];
  for (; da > db && x < n; --da, ++sa) x = parent[x];
  for (; db > da && y < n; --db, ++sb) y = parent[y];
  while (x < n && y < n && x != y) x = parent[x], y = parent[y], ++sa, ++sb;
  const bool met = x < n && x == y;
  *back_a = met ? sa : depth[a];
  *back_b = met ? sb : depth[b];
  return met ? x : 0xFFFFFFFEu;
}

// The walk from tip, at most max_len blocks, tip first; returns its length.
size_t pool_walk_chain(const uint32_t* parent, size_t n, uint32_t tip, size_t max_len, uint32_t* out) {
  size_t len = 0;
  for (uint32_t x = tip; x < n && len < max_len; x = parent[x]) out[len++] = x;
  return len;
}

// Returns the blocks written (at most cap; more were needed if it returns cap + 1).
size_t pool_extract(const pow_block* pool, size_t n, pow_block* out, size_t cap, uint32_t* lengths, size_t* n_chains) {
  std::map<std::string, pow_block> blocks;
  for (size_t i = 0; i < n; ++i) blocks.insert({text(pool[i].block_hash), pool[i]});
  const std::vector<const pow_block*> tips = tips_of(blocks);
  size_t at = 0, c = 0;
  for (const pow_block* tip : tips) {
    const size_t first = at;
    for (const pow_block* cur = tip; cur;) {
      if (at == cap) return cap + 1;
      out[at++] = *cur;
      const auto it = cur->previous_block_hash[0] ? blocks.find(text(cur->previous_block_hash)) : blocks.end();
      cur = it == blocks.end() ? nullptr : &it->second;
    }
    lengths[c++] = (uint32_t)(at - first);
  }
  *n_chains = c;
  return at;
}

}  // extern "C"
