/*
 * pow_gpu.h — C ABI of the MI355X (gfx950) proof-of-work miner.
 *
 * Drop-in for the mining hot path of MPI_blockchain (reference at
 * /root/reference): the inner loop of proof_of_work (node.cpp:292-308),
 *     gen_random_nonce (block.cpp:61-72)
 *  -> block_to_hash    (block.cpp:74-88, picosha2::hash256_hex_string)
 *  -> solves_problem   (block.cpp:91-96)
 * moves behind these entry points.  Everything else (node.cpp's MPI protocol,
 * the success tail node.cpp:311-327) stays host C/C++.
 *
 * The reference has no FFI for this path; its de-facto boundary is the
 * free-function set declared in block.h:27-30 and called from the pthread
 * entry `void* proof_of_work(void*)` (node.h:15).  Each entry point below says
 * which of those it replaces.
 *
 * Conventions
 *   - Plain C: pointers and sizes only, no exceptions across the ABI.
 *   - Return codes: >= 0 success (meaning per function), < 0 error, one of
 *     POW_E* below (HIP failures are reported as POW_EHIP; pow_last_error()
 *     gives the text).
 *   - A pow_ctx is bound to one GPU and is NOT thread-safe: exactly one
 *     thread (that rank's mining thread) drives it.  The only cross-thread
 *     inputs are the cancel word passed to pow_mine, which any thread may
 *     bump, and pow_cancel (one other thread).
 *   - The caller owns every pow_block and output array; the library owns the
 *     device buffers, the HIP stream and the per-template constants.
 *
 * Counter nonces.  The reference draws 9 chars with rand()%62 (block.cpp:61-72).
 * The GPU path replaces the RNG by a deterministic counter: counter c maps to
 * the 9 base-62 digits of c, most significant first, through the reference's
 * alphabet (0-25 -> 'a'..'z', 26-51 -> 'A'..'Z', 52-61 -> '0'..'9'), followed
 * by NUL.  The counter space is [0, 62^9).  Any nonce the reference can draw
 * is reachable, with the same probability of solving per trial.
 */
#ifndef POW_GPU_H
#define POW_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POW_HASH_SIZE 256  /* block.h:4 HASH_SIZE  */
#define POW_NONCE_SIZE 10  /* block.h:5 NONCE_SIZE */
#define POW_MSG_BYTES 270  /* 4 header bytes + nonce[10] + prev[256] (block.cpp:79-88) */
#define POW_COUNTER_LIMIT 13537086546263552ULL /* 62^9 */

/* Byte-identical to the reference's `struct Block` (block.h:17-25) on LP64:
 * sizeof 552; offsets index 0, node_owner_number 4, difficulty 8,
 * created_at 16, nonce 24, previous_block_hash 34, block_hash 290.
 * A reference Block* may be passed wherever a pow_block* is expected. */
typedef struct pow_block {
  uint32_t index;
  uint32_t node_owner_number;
  uint32_t difficulty;
  uint64_t created_at; /* `unsigned long int` in block.h:21 */
  char nonce[POW_NONCE_SIZE];
  char previous_block_hash[POW_HASH_SIZE];
  char block_hash[POW_HASH_SIZE];
} pow_block;

typedef struct pow_ctx pow_ctx;

enum {
  POW_OK = 0,
  POW_EINVAL = -1,    /* bad argument (null pointer, range past 62^9, d > 256, ...) */
  POW_ENOSPC = -2,    /* pow_sweep: more solutions than `cap` */
  POW_EHIP = -3,      /* a HIP runtime call failed; see pow_last_error() */
  POW_ENODEV = -4,    /* no such GPU */
  POW_ECOMM = -5,     /* RCCL unavailable or a collective failed (pow_group_*) */
};

/* Per-call statistics of the last pow_mine / pow_sweep / pow_hash_blocks / pow_verify_chain[s]. */
typedef struct pow_stats {
  double kernel_ms;      /* sum of kernel durations on the ctx stream: HIP events around the
                            sweep/mine kernels; the latency kernel (first sub-round of
                            pow_mine[_any] at d <= 21) times itself with the GPU's realtime
                            counter, from workgroup 0's start to the last workgroup's exit */
  uint32_t launches;     /* kernels launched by the call */
  uint64_t hashes;       /* trials issued to the GPU (incl. edge lanes masked out); pow_find_seed:
                            (seed, trial) pairs issued, no SHA-256 runs */
} pow_stats;

/* ---- context --------------------------------------------------------- */
/* Number of visible GPUs (HIP devices). */
int pow_device_count(int* n);
int pow_init(int device, pow_ctx** out);
void pow_destroy(pow_ctx* ctx);
/* Launch every kernel once with empty work so the code objects are loaded and
 * the first real call pays no start-up cost (HIP loads them lazily). */
int pow_warmup(pow_ctx* ctx);
const char* pow_last_error(void);
int pow_get_stats(const pow_ctx* ctx, pow_stats* out);
/* How the context launches its latency-bound kernels (the one-block hash of
 * pow_hash_block and the first sub-round of pow_mine[_any]):
 * POW_LAUNCH_HIP = hipLaunchKernel on the context's stream, the shipped
 * library's only path; POW_LAUNCH_DIRECT = AQL packets into the process's
 * shared per-device queue (no barrier bit; the test library with POW_AQL=1,
 * for the dispatch A/B and the ordering tests).  Same kernels, same results.
 * Every host wait on a launch is bounded (watchdog): a launch that has not
 * published its result by its deadline (10 s for the latency launches,
 * 10 s + 2 ns per counter for a throughput launch) fails the call with
 * POW_EHIP and a diagnostic in pow_last_error(); the context must then not be
 * reused.  < 0 = error. */
enum { POW_LAUNCH_HIP = 0, POW_LAUNCH_DIRECT = 1 };
int pow_launch_path(const pow_ctx* ctx);
/* Device properties the roofline uses: CU count and peak engine clock (kHz). */
int pow_device_info(const pow_ctx* ctx, int* cu_count, int* clock_khz, char* name, size_t name_cap);
/* The ctx's GPU as "domain:bus:device.function" (hipDeviceGetPCIBusId): the
 * N > 1 bench's check that its ranks run on N distinct devices (partitions of
 * one GPU differ in the function). */
int pow_device_pci_bus_id(const pow_ctx* ctx, char* out, size_t cap);

/* ---- host helpers (no GPU work) ---------------------------------------- */
/* Counter -> nonce[10] (9 base-62 chars MSB first + NUL).
 * Replaces gen_random_nonce (block.cpp:61-72) with a deterministic mapping.
 * Returns POW_EINVAL if ctr >= 62^9. */
int pow_nonce_from_counter(uint64_t ctr, char nonce[POW_NONCE_SIZE]);
/* Exact 270-byte message the reference hashes (block_to_str, block.cpp:79-88):
 * low byte of index, owner, difficulty, created_at; nonce[0..9]; prev[0..255]. */
int pow_block_to_bytes(const pow_block* b, uint8_t out[POW_MSG_BYTES]);
/* solves_problem (block.cpp:91-96) with a run-time difficulty: the first
 * `diff_bits` binary digits of the 64-char hex digest are all '0'. */
int pow_solves_problem(const char* hex, unsigned diff_bits);
/* The reference's OWN nonces: what its gen_random_nonce (block.cpp:61-72, 9 x
 * rand() % 62 over a-z, A-Z, 0-9, then NUL) returns at calls trial_start ..
 * trial_start + n - 1 (the first call of a process is trial 0) after
 * srand(seed); the reference seeds with time(NULL) + mpi_rank (node.cpp:386).
 * This is glibc's TYPE_3 generator, the one the reference was built and
 * measured with: r[i] = r[i-31] + r[i-3] over 2^32, seeded by the 16807
 * Lehmer step (seed 0 counts as 1), draw k = r[k + 344] >> 1.  The library
 * restates it and jumps to trial_start by a polynomial power; it never calls
 * rand() or srand(), keeps no process-global state and is thread-safe.
 * nonces: n x POW_NONCE_SIZE bytes.  POW_EINVAL: trial_start + n >
 * POW_RAND_TRIAL_LIMIT, or null nonces with n > 0.  No GPU work. */
#define POW_RAND_TRIAL_LIMIT (1ULL << 56)
int pow_rand_nonces(uint32_t seed, uint64_t trial_start, size_t n, char* nonces);

/* ---- GPU entry points -------------------------------------------------- */
/* block_to_hash (block.cpp:74-77) for a batch of blocks on the GPU.
 * digests: n*32 bytes (may be NULL); hex: n*65 chars, 64 lowercase hex + NUL
 * each (may be NULL).  Returns POW_OK. */
int pow_hash_blocks(pow_ctx* ctx, const pow_block* blocks, size_t n,
                    uint8_t* digests, char* hex);
/* Single-block form of the above (validation of a received block: valid_new_block,
 * block.cpp:13-25).  One block (also pow_hash_blocks with n = 1) takes the
 * low-latency path: the message travels as a kernel argument and the digest comes
 * back through mapped host memory, no copies (~24 us per call on an MI355X). */
int pow_hash_block(pow_ctx* ctx, const pow_block* b, uint8_t digest[32], char hex[65]);

/* "Is this chain valid?": one fused pass on the GPU over a chain of n blocks,
 * tip first, as on the wire (send_blockchain, node.cpp:334-359) and in the
 * <rank>.out dumps: chain[i + 1] is the parent of chain[i].  n counts real
 * blocks: the caller trims the reference's padding after a block whose
 * previous_block_hash is empty.  The raw structs are copied to the GPU as they
 * are (no per-block host work) and no digests come back.  The reference checks
 * less: check_first hashes only chain[0] of a migrated chain (node.cpp:111-115)
 * and neither valid_new_block (block.cpp:13-25) nor check_chain
 * (node.cpp:117-125) calls solves_problem.  status[i] (n bytes, may be NULL)
 * is the OR of the flags of block i, each evaluated on its own:
 *   POW_V_HASH   the lowercase hex of SHA-256 over block_to_str(chain[i])
 *                differs from block_hash as a C string: the first 64 bytes
 *                must be equal and block_hash[64] must be NUL;
 *   POW_V_WORK   the COMPUTED digest (never the stored text) has fewer than
 *                diff_bits leading zero bits (0..256, as pow_solves_problem);
 *   POW_V_LINK   i < n - 1 and previous_block_hash of i differs from
 *                block_hash of i + 1, as the reference's (string) casts
 *                compare them: C strings cut at the first NUL, at most 256
 *                bytes (bytes after the NUL are hashed, but not linked);
 *   POW_V_INDEX  i < n - 1 and chain[i].index - 1 != chain[i + 1].index in
 *                uint32_t arithmetic (index 0 over 0xFFFFFFFF passes).
 * The last block gets no link or index check.  The time window of
 * valid_new_block (created_at within VALIDATION_MINUTES) is the caller's
 * business: it depends on the caller's clock, not on the chain.
 * Returns 1 if every block passes, 0 if any flag is set; then *first_bad (may
 * be NULL) = the lowest flagged index, n if none, and *n_bad (may be NULL) =
 * the number of flagged blocks.  n = 0 returns 1.  POW_EINVAL for diff_bits >
 * 256, n > 2^24, a null ctx or a null chain with n > 0.  n above 2^16 runs in
 * tiles of 2^16 blocks (36 MB of device memory however long the chain).
 * pow_get_stats: kernel_ms, launches (one per tile), hashes = n.
 * Cost (MI355X, profiles/verify_chain/README.md): a call takes ~50 us up to
 * 16 blocks and 78 us at 200 (kernel 23-36 us), 0.72 ms at 2^16 and 11.5 ms
 * at 2^20 blocks, where it is the copy of the structs.  The reference's own
 * block_to_hash loop at -O2 takes 2.9 us per block on the same box, so the
 * call is slower than the CPU below the crossover, measured between 16 blocks
 * (0.93x the loop's speed) and 32 (1.33x); at 5 blocks it takes 3.3x the
 * loop's time, at 2^16 and above 1/266 of it. */
enum { POW_V_HASH = 1, POW_V_WORK = 2, POW_V_LINK = 4, POW_V_INDEX = 8 };
int pow_verify_chain(pow_ctx* ctx, const pow_block* chain, size_t n, unsigned diff_bits,
                     uint8_t* status /* n bytes, may be NULL */,
                     size_t* first_bad /* may be NULL */, size_t* n_bad /* may be NULL */);

/* "Which of these chains are valid, and which one wins?": pow_verify_chain's
 * audit of n_chains independent chains in one call, one launch per tile of
 * 2^16 blocks however many chains it holds.  `blocks` holds the chains back to
 * back, each tip first as pow_verify_chain takes it: chain c is the
 * lengths[c] blocks from position lengths[0] + ... + lengths[c - 1].  A length
 * of 0 is allowed anywhere.  The raw structs go up as they are; the host work
 * is per chain (n_chains + 1 offsets up, two words per chain down), never per
 * block.
 * status[g] (sum of lengths bytes, may be NULL), g the position in `blocks`,
 * is exactly what pow_verify_chain gives that block when called on its chain
 * alone (POW_V_HASH, POW_V_WORK, POW_V_LINK, POW_V_INDEX): the last block of
 * every chain gets no link or index check, and what follows it in the buffer,
 * another chain's tip, is not looked at.  first_bad[c] (n_chains entries, may
 * be NULL) = the lowest flagged index within chain c, lengths[c] if none;
 * n_bad[c] (n_chains entries, may be NULL) = the flagged blocks of chain c.
 * *best (may be NULL) = the fork choice: among the chains with lengths[c] > 0
 * and n_bad[c] == 0, the one whose tip (its first block) has the greatest
 * index in plain uint32_t comparison, height being what the reference
 * migrates on (node.cpp:249); ties go to the lowest c, as the reference keeps
 * what it saw first and moves only to a strictly higher index; SIZE_MAX if no
 * chain qualifies.
 * Returns 1 if no block of any chain is flagged, 0 otherwise.  n_chains = 0,
 * or all lengths 0, returns 1 with *best = SIZE_MAX.  POW_EINVAL, checked in
 * this order before the context is touched and with nothing written: diff_bits
 * > 256; n_chains > POW_VERIFY_MAX_CHAINS; the sum of lengths above 2^24; a
 * null ctx, null lengths with n_chains > 0, or null blocks with a non-zero sum.
 * Device memory: pow_verify_chain's 36 MB, and 12 bytes per chain (at most
 * 4 MB of offsets and 8 MB of verdicts) with a pinned host twin of the same
 * size, which only grow.
 * pow_get_stats: kernel_ms, launches (one per tile), hashes = the sum of
 * lengths.  pow_warmup does not launch this call's kernel.
 * Cost (MI355X, profiles/verify_chains/README.md; chains x length, valid
 * chains, against the loop of pow_verify_chain calls over the same chains and
 * against the reference's block_to_hash loop at -O2 over as many blocks on
 * the same box's CPU): 2 x 5: 72 us against 98 us and 29 us, so the call
 * gains half a launch boundary on the loop and is still 2.5x slower than the
 * CPU; 16 x 5: 98 us against 788 us and 229 us; 64 x 5: 105 us (1.6 us per
 * chain; kernel 37 us) against 3.14 ms (49 us per chain) and 0.91 ms;
 * 1,024 x 5: 154 us against 50.4 ms and 14.9 ms; 64 x 200: 227 us against
 * 4.95 ms and 37.4 ms; 2^14 x 5: 1.02 ms (kernel 80 us, the rest is the copy
 * of 45 MB of structs) against 810 ms and 238 ms.  64 x 5 costs more than one
 * pow_verify_chain call of 200 blocks (77 us): the offsets' copy and the two
 * resets are three more operations on the stream in front of the launch. */
#define POW_VERIFY_MAX_CHAINS (1u << 20)
int pow_verify_chains(pow_ctx* ctx, const pow_block* blocks, const uint32_t* lengths, size_t n_chains,
                      unsigned diff_bits,
                      uint8_t* status     /* sum(lengths) bytes, may be NULL */,
                      uint32_t* first_bad /* n_chains, may be NULL */,
                      uint32_t* n_bad     /* n_chains, may be NULL */,
                      size_t* best        /* may be NULL */);

/* "Which blocks of this pool hang together, which chains are sound, and which
 * tip wins?": the block tree of a pool of n raw structs in ANY order, as a
 * node holds them in map<string,Block> node_blocks (blocks of every rival and
 * fork, in the order they arrived), with the audit of pow_verify_chain for
 * the chain under every block at once.  It replaces the walks by
 * previous_block_hash of sanity_test, verify_chain_indexes, look_for_block and
 * find_block (node.cpp:40-148).  The structs go up as they are, in
 * pow_verify_chain's tiles of 2^16; there is no per-block host work.
 * Names.  A block has a name exactly when it is not flagged POW_V_HASH (its
 * stored text is the 64 lowercase hex characters of its computed digest and
 * block_hash[64] is NUL); its name is then that digest.  A block flagged
 * POW_V_HASH is nobody's parent, so a forged block that copies an honest
 * block's stored text cannot shadow it.  This differs from pow_verify_chain,
 * where a child whose previous_block_hash equals the stored text of a
 * POW_V_HASH parent gets no link flag: there the order says who the parent is,
 * here only the name does.  Of several blocks with one digest (the same block
 * received twice, or blocks that differ only in bytes that are not hashed:
 * the high bytes of index, owner and created_at, and the padding) the one at
 * the lowest pool position is the parent, as std::map::insert keeps what came
 * first; the others find their own parent like anyone else and have no child.
 * A block's parent.  previous_block_hash is read as the reference's (string)
 * cast reads it: cut at the first NUL, at most 256 bytes (bytes after the NUL
 * are hashed, but not linked).  The empty string: POW_POOL_ROOT.  Exactly 64
 * characters of 0-9a-f, then NUL: the named block of that digest, or
 * POW_POOL_NONE if the pool holds none.  Anything else (63 characters, 64 and
 * no NUL behind them, an uppercase digit, a field without a NUL):
 * POW_POOL_NONE, since no name can equal it.
 * status[i] (n bytes, may be NULL): POW_V_HASH and POW_V_WORK exactly as
 * pow_verify_chain gives them; POW_V_LINK: the parent is POW_POOL_NONE;
 * POW_V_INDEX: the parent is a block and index - 1 != its index in uint32_t
 * arithmetic (index 0 over 0xFFFFFFFF passes).  A root gets neither.
 * parent[i] (n entries, may be NULL): a pool position, POW_POOL_ROOT or
 * POW_POOL_NONE.  depth[i] (may be NULL): the blocks on the walk from i along
 * parent to its end, i included; n_bad[i] (may be NULL): the flagged blocks on
 * that walk.  The chain under tip i is sound exactly when n_bad[i] == 0 (it
 * then ends at a root: an orphan end carries POW_V_LINK): the reference's
 * sanity_test plus hash and work, for every possible tip.  A walk that does
 * not end (a cycle of names, which needs a SHA-256 cycle) gives every block on
 * or above it depth 0, n_bad 0xFFFFFFFF and POW_V_LINK.
 * *best (may be NULL): among the blocks with n_bad == 0 the one with the
 * greatest index in plain uint32_t comparison, pow_verify_chains' fork choice
 * for the same reason; ties go to the lowest pool position; SIZE_MAX if no
 * block qualifies.
 * Returns 1 if no block is flagged, 0 otherwise; n = 0 returns 1 with *best =
 * SIZE_MAX.  POW_EINVAL, checked in this order before the context is touched
 * and with nothing written: diff_bits > 256; n > POW_POOL_MAX_BLOCKS; a null
 * ctx, or a null pool with n > 0.  POW_EHIP if the table overflowed, which a
 * table of at least 2 n slots cannot.
 * Device memory: pow_verify_chain's 36 MB, and 98 bytes per block (two
 * digests, index, parent and the ranking's six words) plus a table of 4-byte
 * slots, the lowest power of two that is at least 2 n (8 to 16 bytes per
 * block): 111 MB at 2^20 blocks.  It only grows.
 * Known limit: the table is open-addressed from a slot the digest's last word
 * names.  An adversary who grinds many blocks onto one start slot makes the
 * probes long (and the call slow), never wrong or unbounded: a probe ends
 * after one pass of the table.
 * pow_get_stats: kernel_ms, launches (one per tile, insert, join, one per
 * round of ceil(log2 n) rounds of pointer jumping, fork choice), hashes = n.
 * pow_warmup does not launch this call's kernels.
 * Cost (MI355X, profiles/index_blocks/README.md; medians of 9 calls on
 * shuffled sound pools at d = 0, against the reference's way at -O2 on one
 * CPU thread of the same box, a std::map keyed on the stored text and the
 * sanity_test walk from every tip with block_to_hash per block, and against
 * extracting every tip's chain on the host for one pow_verify_chains call):
 * the call is slower than both below a few dozen blocks: 5 blocks in one
 * chain take 99 us (7 launches, kernels 44 us) against 6 us and 65 us, 16
 * blocks 102 us against 18 us and 68 us.  The published shape as a pool (3
 * rivals x 10 heights on a root: 31 blocks, 21 tips): 117 us against 138 us
 * and 115 us, the crossover.  200 blocks with 8 tips: 137 us against 0.91 ms
 * and 0.24 ms; 4,096: 0.21 ms against 22.7 ms and 5.7 ms; 2^16: 0.89 ms
 * (kernels 0.17 ms) against 555 ms and 286 ms; 2^20: 12.6 ms (39 launches,
 * kernels 1.8 ms; the rest is the copy of 579 MB of structs) against 18.9 s
 * and 14.9 s. */
#define POW_POOL_MAX_BLOCKS (1u << 20)
#define POW_POOL_ROOT 0xFFFFFFFFu /* previous_block_hash is the empty string */
#define POW_POOL_NONE 0xFFFFFFFEu /* names a parent the pool does not hold */
int pow_index_blocks(pow_ctx* ctx, const pow_block* pool, size_t n, unsigned diff_bits,
                     uint8_t* status  /* n, may be NULL */,
                     uint32_t* parent /* n, may be NULL */,
                     uint32_t* depth  /* n, may be NULL */,
                     uint32_t* n_bad  /* n, may be NULL */,
                     size_t* best     /* may be NULL */);

/* A pool that stays on the device and is fed: pow_index_blocks' answers kept
 * current while blocks arrive, as node_blocks grows one block at a time
 * (node.cpp:199, 319) or by a migrated run (node.cpp:174-179).  A pow_pool
 * keeps pow_index_blocks' 98 bytes per block and its table resident; the raw
 * structs are not kept on the device, the host owns them as before.
 * The contract.  A block's position is the order of its arrival.  After any
 * sequence of adds, status, parent, depth, n_bad (pow_pool_read), best
 * (pow_pool_info) and the value pow_pool_add returned are byte for byte what
 * pow_index_blocks gives on the concatenation of everything added, in that
 * order, at the pool's diff_bits.  Every rule of pow_index_blocks above
 * carries over unchanged: names are computed digests; a POW_V_HASH block is
 * nobody's parent; of several blocks with one digest the lowest position is
 * the parent; how previous_block_hash is read; the flags; the fork choice and
 * its tie rule.  A cycle of names needs a SHA-256 cycle and cannot be built
 * through this interface; what the pool gives on one is not specified.
 * How an add runs (N blocks before it, m with it).  The new structs go up and
 * are audited in pow_verify_chain's tiles of 2^16, as pow_index_blocks does
 * it.  The new named blocks go into the table; if N + m exceeds half its slots
 * the table is rebuilt from all N + m blocks with at least 2 (N + m) slots
 * instead (info: rehashed).  One launch over N + m lanes joins the new blocks
 * and lets every old block that is an orphan so far (parent POW_POOL_NONE, a
 * previous_block_hash that can name somebody) look its parent up again;
 * nothing else about an old block can change, since a new twin has a higher
 * position and never takes a name over.  ceil(log2 m) rounds rank the new
 * blocks among themselves; a walk that reaches an old block takes over that
 * block's depth and n_bad.  The new blocks alone feed the resident fork
 * choice and flagged count.  The host waits once per tile of the audit, as
 * pow_index_blocks does, then once for all the rest.  If no old orphan found
 * its parent (info: adopted == 0, the common case) the add is done.  Otherwise
 * everything above an adopted orphan is stale, and the whole pool is ranked
 * again on the device, behind one more bounded wait (info: reranked).  An add
 * of one block waits twice, three times when it re-ranks.
 * Cost.  Host work, uploads and downloads of an add are O(m), never O(N):
 * there is no per-block host loop and no copy of earlier structs.  Launches
 * (pow_get_stats; hashes = m): ceil(m / 2^16) + 3 + ceil(log2 m), what
 * pow_index_blocks takes on the m blocks alone, 4 for one block; a re-rank
 * adds 3 + ceil(log2(N + m)).  The arrays grow by doubling, device to device,
 * never past POW_POOL_MAX_BLOCKS blocks, which bounds the blocks a pool holds at
 * a time; only pow_pool_prune makes them fewer.
 * pow_warmup does not launch this call's kernels.
 * Device memory: 98 bytes per block of the capacity and 4 per slot, the
 * context's tile staging buffer (pow_verify_chain's) apart; while an add grows
 * the arrays or the table, the ones it leaves stand beside the new until it
 * returns.
 * Measured (MI355X, profiles/pool_stream/README.md; medians of 9 adds into
 * shuffled sound pools of N blocks at d = 0, against pow_index_blocks over
 * the N + 1 blocks and against the reference's way at -O2 on one CPU thread of
 * the same box, a std::map insert and the sanity_test walk from the new tip):
 * the add of one block does not grow with N: 98 us at N = 31, 101 us at 200,
 * 102 us at 4,096, 105 us at 2^16, 106 us at 2^20 - 1 (4 launches, kernels
 * 39 to 41 us: four launch boundaries), against 0.138, 0.156, 0.220, 0.908
 * and 12.5 ms for pow_index_blocks.  The add is slower than the reference's
 * map below a few hundred blocks: 98 us against 18 us at 31 blocks, even at
 * 200 (101 against 110 us); then 2.4 ms at 4,096, 48 ms at 2^16 and 1.28 s at
 * 2^20 for the reference, whose walk hashes the whole chain again.  An add
 * that re-ranks: 0.17 ms at 31 blocks (13 launches), 0.20 ms at 4,096, 0.23 ms
 * at 2^16, 1.19 ms at 2^20 (27 launches, kernels 1.10 ms).  A run of 5 blocks:
 * 0.11 ms at every size (7 launches).  Device memory at 2^20 blocks: 111.1 MB.
 * Walks.  Walking a chain in order (send_blockchain, log_chain), a block's
 * ancestor and the fork point of two chains run on the device:
 * pow_pool_chain, pow_pool_ancestors, pow_pool_fork_points below.  So do
 * which blocks lie under a tip, and dropping the forks that lost:
 * pow_pool_mark, pow_pool_prune below; and the live tips, what stands on a
 * block, and dropping a block with all that stands on it: pow_pool_tips,
 * pow_pool_subtrees, pow_pool_drop below.
 * Lifetime and threads.  A pool is driven by its context's one thread.
 * Several pools may live on one context; pow_index_blocks and the verify calls
 * may be used between adds (they share the tile staging buffer and do not
 * disturb a pool).  Every pool is closed before pow_destroy: pow_destroy of a
 * context with open pools frees nothing, keeps the context usable and leaves
 * its reason in pow_last_error; close the pools and call it again.  A context bound
 * to a stop board refuses pow_pool_open, _add, _read, _find, _mark and _prune (POW_EINVAL).
 *
 * pow_pool_open: an empty pool at diff_bits.  reserve is a hint: the blocks
 * the arrays are sized for at once; 0 = 64 blocks.  POW_EINVAL, in this order
 * before the context is touched: diff_bits > 256; reserve >
 * POW_POOL_MAX_BLOCKS; a null ctx or out.
 * pow_pool_add: returns 1 if no block of the whole pool is flagged, 0
 * otherwise; *info (may be NULL) as pow_pool_get_info.  m = 0 changes nothing.
 * POW_EINVAL, in this order before the context is touched and with nothing
 * written or added: a null pool; null blocks with m > 0; an add that would
 * pass POW_POOL_MAX_BLOCKS.  An add that fails with POW_EHIP leaves the pool
 * unusable: every later call on it but pow_pool_close returns POW_EHIP at
 * once, as on a wedged context.
 * pow_pool_get_info: the pool after its last add; no GPU work.
 * pow_pool_read: blocks first .. first + count - 1 of the four per-block
 * results (each may be NULL).  POW_EINVAL: a null pool; a range past size.
 * pow_pool_find: node_blocks.find (node.cpp:83, 105) for k names of 64
 * characters each (no NUL between them).  64 characters of 0-9a-f give the
 * named block of that digest, the lowest position among twins, or
 * POW_POOL_NONE; anything else gives POW_POOL_NONE, and so does the stored
 * text of a POW_V_HASH block.  One launch.  POW_EINVAL: a null pool; null names
 * or pos with k > 0; k > POW_POOL_MAX_BLOCKS. */
typedef struct pow_pool pow_pool;
typedef struct pow_pool_info {
  uint32_t size;        /* blocks held */
  uint32_t n_flagged;   /* blocks with a non-zero status */
  uint32_t best;        /* fork choice: a position, POW_POOL_NONE if no block has n_bad == 0 */
  uint32_t best_index;  /* its index field (0 if none) */
  uint32_t adopted;     /* last add: earlier blocks that were POW_POOL_NONE and whose parent came with it */
  uint32_t reranked;    /* last add: 1 if it re-ranked the whole pool */
  uint32_t rehashed;    /* last add: 1 if it rebuilt the table */
  uint32_t capacity, slots;
} pow_pool_info;
int pow_pool_open(pow_ctx* ctx, unsigned diff_bits, size_t reserve, pow_pool** out);
void pow_pool_close(pow_pool* p);
int pow_pool_add(pow_pool* p, const pow_block* blocks, size_t m, pow_pool_info* info /* may be NULL */);
int pow_pool_get_info(const pow_pool* p, pow_pool_info* info);
int pow_pool_read(pow_pool* p, size_t first, size_t count, uint8_t* status, uint32_t* parent, uint32_t* depth,
                  uint32_t* n_bad);
int pow_pool_find(pow_pool* p, const char* names /* k x 64 */, size_t k, uint32_t* pos /* k */);

/* "Which blocks lie on the chains under these tips?", and "forget every fork
 * that lost": look_for_block and find_block over a migrated chain
 * (node.cpp:131-148) without a host walk, and the way for a pool to shrink.
 * The reference never migrates to a fork more than VALIDATION_BLOCKS behind the
 * tip (verificar_y_migrar_cadena) and yet keeps every loser for ever.  Both are
 * one computation on what the pool holds already (parent, depth, n_bad, the
 * digests): mark every ancestor of a set of seed blocks, then, for the prune,
 * compact the resident arrays onto the marked blocks.  Nothing is hashed again
 * and no struct goes up.
 * Seeds.  Every position in tips[] (duplicates allowed).  With
 * POW_KEEP_BY_INDEX also every block with index >= min_index, in plain uint32_t
 * comparison; without that flag min_index is ignored.  With POW_KEEP_SOUND_ONLY
 * as well an index seed must also have n_bad == 0; explicit tips are seeds
 * whatever their flags.  The marked set is every seed and every block on the
 * walk from a seed along parent, to the walk's end (a root or POW_POOL_NONE).
 * pow_pool_mark: on[i] (size bytes, may be NULL) is 1 for a marked block and 0
 * otherwise, *n_on (may be NULL) the count of marked blocks; the pool's answers
 * do not change.  Returns POW_OK.
 * pow_pool_prune: the pool afterwards holds exactly the marked blocks, in
 * their old order.  map[i] (the size BEFORE the call, may be NULL) is block i's
 * new position, or POW_POOL_NONE if it was dropped; the caller compacts its own
 * struct array with it.  Returns 1 if no block that is left is flagged, 0
 * otherwise; *info (may be NULL) as pow_pool_get_info.
 * The prune's contract.  After a prune status, parent, depth, n_bad, best,
 * n_flagged and pow_pool_find are byte for byte what pow_index_blocks gives on
 * the surviving structs in that order, at the pool's diff_bits; and after any
 * later adds, on the survivors followed by everything added since.  Why: the
 * marked set is closed under parent, so every survivor keeps its whole walk,
 * its depth and n_bad stand and only positions are renamed.  A parent is the
 * lowest twin of its name, and order is kept, so it stays the lowest.  A
 * dropped lower twin of a kept block names nobody that is kept (a child of that
 * name would have marked it).  A block that later names a dropped block is an
 * orphan (POW_V_LINK), as it would be in that pow_index_blocks call.  A block
 * on a cycle of names stays unspecified, as above.
 * Info after a prune that dropped something: size, n_flagged, best,
 * best_index, capacity and slots describe the pool as it now is; adopted 0,
 * reranked 0, rehashed 1.  Nothing marked: the pool is empty, best
 * POW_POOL_NONE.  Everything marked: nothing is touched, map is the identity,
 * adopted, reranked and rehashed are 0.  On an empty pool neither call does
 * GPU work.
 * How they run.  One bounded wait: the tips go up, every block starts a walk
 * at its parent and the seeds are marked (K12a), ceil(log2 size) rounds of
 * pointer jumping carry the marks down every walk (K12b), the marks are
 * counted per 256 blocks and scanned (K12c, K12d); the marks and the total
 * come down.  A prune that keeps some blocks and drops some then allocates
 * arrays at the lowest power of two that holds the survivors and is at least
 * pow_pool_open's first capacity, and a table to match (slots >= 2 size still
 * holds), and behind one more bounded wait gathers the survivors' entries into
 * them (K12e), renames the parents and redoes the fork choice and the flagged
 * count (K12f) and fills the table (K10b).  It is the one call that gives
 * device memory back; the arrays it leaves stand beside the new until it
 * returns.  The scratch is arrays the pool has anyway.
 * Cost.  Launches (pow_get_stats; hashes = 0): 3 + ceil(log2 size) for a mark,
 * 6 + ceil(log2 size) for a prune that drops and keeps.  No host loop runs
 * over the pool's blocks, only the check of the tips.  pow_warmup does not
 * launch these kernels.
 * Measured (MI355X, profiles/pool_prune/README.md; medians of 9 calls on
 * shuffled sound pools in the published shape at d = 0, three rivals per
 * height, the winning tip as the one seed, so two thirds of N blocks go;
 * against pow_pool_close, pow_pool_open and one pow_pool_add of the survivors
 * in the same process, what the library took before): mark / prune / that
 * path: 89 / 153 / 366 us at N = 31 (8 and 11 launches), 99 / 172 / 394 us at
 * 199, 110 / 191 / 437 us at 4,096, 0.14 / 0.45 / 0.91 ms at 2^16, 0.36 /
 * 1.00 / 7.3 ms at 2^20 - 3 (23 and 26 launches, kernels 0.22 and 0.34 ms).
 * The prune was expected to be the slower one below some hundreds of blocks,
 * being 6 + ceil(log2 N) launch boundaries; against that whole path it is not,
 * at any size measured.  Against the pow_pool_add of the survivors alone, into
 * a pool that is already open, it has not been measured; by the add's own
 * figures above (about 0.1 ms for a small batch) that add would be the faster
 * one for pools of some hundreds of blocks.  Device memory at 2^20 - 3 blocks:
 * 111.1 MB before, 55.6 MB after (capacity 2^20 to 2^19).  A pool opened with
 * a reserve below pow_pool_open's first capacity grows to it (31 to 64).
 * POW_EINVAL, in this order before the context is touched and with nothing
 * written: a null pool; flag bits other than the two; n_tips >
 * POW_POOL_MAX_TIPS; null tips with n_tips > 0; a tip at or past size.  Then as
 * every pool call: POW_EHIP on a pool that is unusable, POW_EINVAL on a context
 * bound to a stop board.  A prune that fails with POW_EHIP leaves the pool
 * unusable, as a failed add does. */
enum { POW_KEEP_BY_INDEX = 1, POW_KEEP_SOUND_ONLY = 2 };
#define POW_POOL_MAX_TIPS (1u << 16)
int pow_pool_mark(pow_pool* p, const uint32_t* tips, size_t n_tips, uint32_t min_index, unsigned flags,
                  uint8_t* on /* size bytes, may be NULL */, size_t* n_on /* may be NULL */);
int pow_pool_prune(pow_pool* p, const uint32_t* tips, size_t n_tips, uint32_t min_index, unsigned flags,
                   uint32_t* map /* the size BEFORE the call, may be NULL */, pow_pool_info* info /* may be NULL */);

/* "Where do the old best chain and the new one part?", "is this block on my
 * chain?", "give me the blocks under this one, in order": look_for_block and
 * find_block (node.cpp:131-148), the migration rule of
 * verificar_y_migrar_cadena (node.cpp:150-191) and the walks of
 * send_blockchain and log_chain (node.cpp:40-58, 334-359), answered on the
 * device from the pool's own parent and depth, as pow_pool_read returns them.
 * Nothing is hashed, no struct goes up and no host walk runs.
 * pow_pool_ancestors: out[q] is the block steps[q] steps along parent from
 * pos[q]; 0 steps give pos[q] itself.  If steps[q] >= depth[pos[q]], out[q] is
 * the walk's end, the parent value of the walk's last block: POW_POOL_ROOT or
 * POW_POOL_NONE.  Any uint32_t is a valid step count.
 * pow_pool_fork_points: at[q] is the first block on the walk from a[q] that
 * also lies on the walk from b[q]: a[q] itself when it is on b[q]'s walk (so
 * a == b gives a), POW_POOL_NONE when the walks share no block (different
 * roots, two orphan ends: an end is not a block).  back_a[q], back_b[q] (each
 * may be NULL) are the steps from a[q] and b[q] to at[q], or with no shared
 * block depth[a[q]] and depth[b[q]], the whole of both walks.  back_a == 0 is
 * look_for_block; with a = a received chain's tip and b = the node's own tip,
 * back_a is what find_block returns (its index == 1 clause stays with the
 * caller).  A twin is a block like any other, with its own parent: the fork
 * point of a block and its twin is their common parent.
 * pow_pool_chain: *len = min(max_len, depth[tip]); out[j] is the block j steps
 * under tip for j < *len, POW_POOL_NONE for *len <= j < min(max_len, size);
 * nothing past that is touched.  One query launch, lane j answering (tip, j).
 * A cycle of names: what the calls return is unspecified, as everywhere in
 * the pool, but they return and read nothing outside the arrays: every loop has
 * a constant bound and every position read is compared with size before use.
 * How they run.  A binary-lifting table on the device.  Level 0 is the pool's
 * parent array; row j >= 1 holds for every block the block 2^j steps under it,
 * or the walk's end marker.  A pool of n blocks has max(ceil(log2 n) - 1, 0)
 * rows.  The table is allocated by the first query call that needs it, at the
 * pool's capacity at that moment: 4 x capacity x rows(capacity) bytes, 79.7 MB
 * at a capacity of 2^20 (19 rows), beside the pool's 111.1 MB.  A pool that is
 * never queried pays nothing.  It is brought up to date lazily, inside the next
 * query call; pow_pool_add and pow_pool_prune launch nothing for it.  Up to
 * date: no table launch.  Stale (never built, an add that re-ranked, a prune
 * that dropped blocks, a capacity that outgrew the table's: then it is
 * allocated again at the pool's capacity, not copied): one launch per row over
 * all blocks.  Otherwise, for the m new blocks, the rows that exist: one launch
 * of one workgroup when m <= 256, else one launch per row over m lanes; then
 * one launch over all blocks for every row that is new because size passed a
 * power of two.  A prune that drops something frees the table; an add that
 * re-ranks keeps the allocation.
 * Cost.  One bounded wait per call: the arguments up, the table's launches, one
 * query launch, the results down.  Launches (pow_get_stats; hashes = 0): the
 * table's plus one, so 2 for a query after a one-block add at every pool size,
 * 3 when the size has just passed a power of two, 1 when nothing was added.  A
 * lane does at most about 3 ceil(log2 size) dependent 4-byte reads.  The one
 * host loop is the check of the positions, over the queries and never over the
 * pool's blocks.  pow_warmup does not launch these kernels.  k == 0 (and
 * max_len == 0) returns POW_OK with no GPU work and no table work.
 * Measured (MI355X, profiles/pool_lift/README.md; medians of 9 calls on
 * shuffled pools at d = 0: a trunk of half the blocks and eight chains forking
 * from its tip; a and b two of those tips, N / 16 steps from their fork point;
 * against pow_pool_read of parent and depth for the whole pool and a plain
 * walk on the host, which is what a caller did before, and against that walk
 * alone on arrays the host already holds): one pair with the table up to date
 * takes 31 us at N = 31, 30 us at 4,096, 32 us at 2^16 and at 2^20 - 16 (1
 * launch, kernel 7 to 10 us); after a one-block add 44, 43, 40 and 45 us (2
 * launches); 4,096 pairs 56 to 63 us; pow_pool_chain of 5 blocks 27 us at every
 * size, of the whole walk 27 us (17 blocks) to 0.29 ms (589,815 blocks, which
 * the host walk takes 5.8 ms for).  The first query of a filled pool, with the
 * table's allocation and every row: 84 us at 31 blocks (5 launches), 0.10 ms at
 * 4,096, 0.13 ms at 2^16, 0.32 ms at 2^20 - 16 (20 launches, kernels 0.19 ms).
 * Read and walk: 44, 41, 69 us and 2.9 ms.  So the query after an add ties with
 * reading the pool down up to a few thousand blocks (43 against 41 us at
 * 4,096), is 1.7x faster at 2^16 and 65x at 2^20 - 16.  Against a host that
 * keeps its own copy of the tree and walks it (3 us up to 4,096 blocks, 14 us
 * at 2^16, 0.65 ms at 2^20 - 16) the device query is slower up to 2^16 and
 * 20x faster at 2^20 - 16: one pair is one launch and one bounded wait.  What
 * that copy costs to keep current is not in its figure.  A block-major layout
 * of the table was not tried.
 * POW_EINVAL, in this order before the context is touched and with nothing
 * written: a null pool; a null required array with k > 0 (for the chain call:
 * null len, or null out with min(max_len, size) > 0); k > POW_POOL_MAX_BLOCKS;
 * a position at or past size.  Then as every pool call: POW_EHIP on a pool
 * that is unusable, POW_EINVAL on a context bound to a stop board.  The queries
 * return POW_OK.
 * pow_pool_lift_get_info: the table as the next query call will find it; no
 * GPU work.  POW_EINVAL: a null pool or out. */
int pow_pool_ancestors(pow_pool* p, const uint32_t* pos, const uint32_t* steps, size_t k, uint32_t* out /* k */);
int pow_pool_fork_points(pow_pool* p, const uint32_t* a, const uint32_t* b, size_t k, uint32_t* at /* k */,
                         uint32_t* back_a /* k, may be NULL */, uint32_t* back_b /* k, may be NULL */);
int pow_pool_chain(pow_pool* p, uint32_t tip, size_t max_len, uint32_t* out /* min(max_len, size) */, size_t* len);
typedef struct pow_pool_lift_info {
  uint32_t covered;   /* blocks the table covers (0: none, or stale) */
  uint32_t rows;      /* rows in use */
  uint32_t capacity;  /* blocks a row has room for (0: not allocated) */
  uint32_t rebuilt;   /* last query call: 1 if it made the table from nothing */
  uint32_t extended;  /* last query call: blocks it extended the table by */
  uint64_t bytes;     /* device memory the table holds */
} pow_pool_lift_info;
int pow_pool_lift_get_info(const pow_pool* p, pow_pool_lift_info* out);

/* "Which blocks are the live fork tips?", "what has been built on this block?"
 * and "forget this block and everything built on it": the questions that look
 * up the tree.  Every rank's last_block_in_chain is a tip (node.cpp:249); the
 * blocks over a block are its confirmations and hold the tip a node that has
 * committed to it should mine on; and valid_new_block's time window
 * (node.cpp:199) is the caller's business, so a caller that rules a block out
 * later needs a way to remove it, which pow_pool_prune (ancestors of seeds)
 * cannot express.  All three are defined over what pow_pool_read returns, and
 * answered on the device from it.  Nothing is hashed and no struct goes up.
 * pow_pool_tips: block i is a tip when no block j has parent[j] == i.  A twin
 * that is not the lowest of its name, and a POW_V_HASH block, have no name a
 * child could find, so they are tips.  With POW_TIPS_SOUND_ONLY a tip must also
 * have n_bad[i] == 0.  out takes the tips ascending by position; *n_tips is
 * their total, also when it exceeds cap: then POW_ENOSPC is returned and out
 * holds the first cap of them, as pow_find_seed does it.  Only out[0 ..
 * min(cap, total)) is written.  Otherwise POW_OK.  An empty pool: 0 tips, no
 * GPU work.
 * pow_pool_subtrees: block i is a member of root r's subtree when r lies on
 * the walk from i along parent; r itself is a member.  Per root q (every output
 * k entries, each may be NULL): size[q] the members; height[q] the greatest
 * depth[i] - depth[roots[q]] among them, 0 for a leaf; best[q], best_index[q]
 * pow_index_blocks' fork choice among the members: of those with n_bad == 0 the
 * greatest index, ties to the lowest position; POW_POOL_NONE and 0 if there is
 * none.  on[i] (size bytes, may be NULL) is 1 when i is a member of any root's
 * subtree and 0 otherwise, *n_on (may be NULL) the count of those.  Duplicate
 * and nested roots are allowed.  The pool's answers do not change.  Returns
 * POW_OK.  k == 0: no GPU work and no table work; on is all 0, *n_on 0.
 * pow_pool_drop: the pool afterwards holds exactly the blocks that are in no
 * root's subtree, in their old order.  map, info and the return value are
 * pow_pool_prune's, and so is the contract: status, parent, depth, n_bad, best,
 * n_flagged and pow_pool_find are byte for byte what pow_index_blocks gives on
 * the surviving structs in that order, and after later adds on the survivors
 * followed by everything added since.  Why: the complement of a union of
 * subtrees is closed under parent (if i's parent were a member of r's subtree,
 * r would lie on the parent's walk and so on i's), so every survivor keeps its
 * whole walk, and the prune's argument applies from there.  For twins it needs
 * one thing more: a dropped lower twin of a kept block names nobody that is
 * kept, because a child of that name has the lower twin as its parent and is
 * dropped with it.  A block that later names a dropped block is an orphan, as
 * in that pow_index_blocks call.  Nothing dropped (k == 0, the only way: a
 * root goes with its subtree): the pool is untouched, map is the identity,
 * no GPU work and no table work.  Every block dropped: an empty pool, best
 * POW_POOL_NONE.  A drop that drops something frees K13's table, as a prune
 * does.
 * How they run.  One bounded wait per call, and a second for a drop that
 * keeps some blocks.  Tips: a byte per block is zeroed,
 * every block sets its parent's (K14a), every block turns its own into "is a
 * tip and passes the filter" (K14b), the bytes are counted per 256 blocks and
 * scanned (K12c, K12d) and the marked positions gathered into a list (K14c);
 * the total and min(cap, size) entries come down into pinned memory.  Subtrees:
 * K13's table is brought up to date inside the call exactly as a K13 query
 * does it (allocated by the first call that needs it), then one launch of
 * ceil(size / 256) x k workgroups (K14d): lane (i, q) compares the two depths
 * and, if i is not higher than the root, jumps depth[i] - depth[root] steps and
 * compares what it finds with the root; the members are counted and their
 * height and key reduced per wave, one atomic per wave and result.  With on or
 * n_on the members also set a byte, and K12c and K12d count those.  Drop: the
 * same launch clears the members' bytes in marks preset to 1, K12c and K12d
 * count what is kept; then exactly what a prune does behind a mark that
 * drops something: an empty pool, or behind one more bounded wait new arrays,
 * K12e, K12f and K10b.  The scratch is K12's.
 * Cost.  Launches (pow_get_stats; hashes = 0), with T the table's launches as
 * under pow_pool_ancestors (0 when it is up to date, 1 after an add of at most
 * 256 blocks that passed no power of two, max(ceil(log2 size) - 1, 0) when it
 * is stale): tips 5; subtrees T + 1, and T + 3 with on or n_on; drop T + 3,
 * and T + 6 when it keeps some blocks; drop with k == 0: none.  The one host
 * loop is the check of the roots (and the identity map of a drop with k == 0).
 * The tips' list comes down as min(cap, size) entries, since the total is not
 * known before the wait: with cap = size at 2^20 blocks that copy (4 MB) is
 * most of the call, so pass the cap that is needed.  pow_warmup does not launch
 * these kernels.
 * Measured (MI355X, profiles/pool_above/README.md; medians of 9 calls on
 * shuffled pools at d = 0: a trunk of half the blocks and eight chains forking
 * from its tip; the root asked for is the first block of a chain that lost,
 * N / 16 blocks; against pow_pool_read of parent, depth and n_bad for the
 * whole pool and numpy on the host, which is what a caller did before): tips
 * with cap = N (kernels 0.03 ms at 2^20 - 16, the rest the list's copy)
 * 60 us at N = 31, 57 us at 4,096, 75 us at 2^16, 0.15 ms at 2^20 - 16, against
 * 40 us, 48 us, 0.15 ms and 2.2 ms for read and numpy: slower up to a few
 * thousand blocks, 14x faster at 2^20 - 16.  One root with the table up to
 * date 31, 34, 67 us and 0.59 ms (1 launch, kernel 0.57 ms: half a million
 * lanes each jump up to 19 dependent reads through an 80 MB table); after a
 * one-block add 50, 48, 88 us and 0.62 ms (2 launches), against 73 us, 0.21,
 * 3.3 and 93 ms for read and numpy doubling: faster at every size measured.
 * 64 roots, among them the pool's root: 33 us, 47 us, 0.55 ms and 12.1 ms; the
 * launch grows with k x the members' jumps.  Drop (6 launches, the table up to
 * date before and freed by it): 0.15, 0.16, 0.61 and 2.6 ms, against
 * pow_pool_prune handed the seven tips of what stays (11 to 26 launches, no
 * table to free): 0.15, 0.19, 0.44 and 1.2 ms.  So where the caller already
 * knows the tips of everything it wants to keep, the prune is the faster way
 * to say it from 2^16 blocks on; the drop is for the caller who knows the one
 * block it wants gone.
 * POW_EINVAL, in this order before the context is touched and with nothing
 * written: a null pool; flag bits other than POW_TIPS_SOUND_ONLY; k >
 * POW_POOL_MAX_ROOTS; null roots with k > 0 (for the tips: a null n_tips, or a
 * null out with cap > 0); a root at or past size.  Then as every pool call:
 * POW_EHIP on a pool that is unusable, POW_EINVAL on a context bound to a stop
 * board.  A drop that fails with POW_EHIP leaves the pool unusable, as a failed
 * prune does. */
enum { POW_TIPS_SOUND_ONLY = 1 };
#define POW_POOL_MAX_ROOTS 64
int pow_pool_tips(pow_pool* p, unsigned flags, uint32_t* out, size_t cap, size_t* n_tips);
int pow_pool_subtrees(pow_pool* p, const uint32_t* roots, size_t k, uint32_t* size, uint32_t* height, uint32_t* best,
                      uint32_t* best_index /* k each, may be NULL */, uint8_t* on /* size bytes, may be NULL */,
                      size_t* n_on /* may be NULL */);
int pow_pool_drop(pow_pool* p, const uint32_t* roots, size_t k, uint32_t* map /* the size BEFORE the call, may be NULL */,
                  pow_pool_info* info /* may be NULL */);

/* Mining round: replaces node.cpp:302-308 (nonce -> hash -> test) for every
 * counter in [ctr_start, ctr_start + ctr_count).  The header fields and the
 * 256-byte previous_block_hash are taken from `tmpl` as they are (the caller
 * does the template refresh of node.cpp:292-299).
 *   diff_bits     leading zero BITS required (T3), 0..256.
 *   cancel_word   optional; polled between GPU sub-rounds; if it differs from
 *                 `epoch` the call stops early and returns 0.
 * On success returns 1 and fills *out = *tmpl with out->nonce = the nonce of
 * the LOWEST solving counter in range and out->block_hash = its 64-char hex
 * digest + NUL (strcpy semantics of node.cpp:318: bytes 65..255 keep tmpl's);
 * *found_ctr = that counter.  Returns 0 if the range holds no solution or the
 * call was cancelled.  *hashes_done (optional) = trials issued.
 * pow_mine and pow_mine_any return as soon as the GPU has published the
 * result; the ctx's stream may still be retiring the launch's last
 * workgroup for a few microseconds (nothing it does then touches the result,
 * the cancel word or a board, so unbinding or closing a board right away is
 * safe).  The next launch on the ctx and pow_destroy are ordered behind it. */
int pow_mine(pow_ctx* ctx, const pow_block* tmpl, uint64_t ctr_start, uint64_t ctr_count,
             unsigned diff_bits, const volatile uint32_t* cancel_word, uint32_t epoch,
             pow_block* out, uint64_t* found_ctr, uint64_t* hashes_done);

/* Mine n blocks on top of *parent, each the child of the one before: the loop
 * of proof_of_work (node.cpp:285-327) for one solo miner, without a host step
 * between two blocks.  The producing counterpart of pow_verify_chain.
 * Block k (mining order, k = 0..n-1) is what the host sequence gives: with
 * `last` = *parent for k = 0, else block k - 1, the template is `last` copied
 * whole (all 552 bytes, padding included), then index = last.index + 1
 * (uint32_t wrap), node_owner_number = owner, difficulty = diff_bits,
 * created_at = created_at[k] (created_at NULL: time(NULL), read once at entry,
 * for every block) and previous_block_hash = all 256 bytes of last.block_hash
 * (node.cpp:299, trap T5; the parent's block_hash may be any 256 bytes).  The
 * block is the result of pow_mine on that template over [ctr_start, ctr_start
 * + ctr_count): the LOWEST solving counter, nonce = its 9 base-62 characters +
 * NUL, block_hash = 64 hex + NUL with bytes 65..255 kept from the template
 * (node.cpp:318).  Every block searches the same counter window.
 * Blocks are written tip first, as pow_verify_chain and the wire expect: block
 * k goes to out[n - 1 - k].  After the call out + (n - *n_mined) is a
 * tip-first chain of *n_mined blocks whose oldest block is a child of *parent;
 * the entries below it are not touched.
 * Returns 1 if all n blocks were mined; 0 if it stopped early, because a
 * block's window held no solution or because the cancel word (optional)
 * differs from `epoch`; *n_mined (may be NULL) then says how far it got.
 * n = 0 returns 1.  POW_EINVAL for diff_bits > 256, ctr_count == 0 or > 2^32,
 * ctr_start + ctr_count > 62^9, n > 2^24, a null ctx, a null parent or out
 * with n > 0 (all checked before the context is touched), and for a context
 * bound to a stop board: boards and pow_cancel's in-flight path are not part
 * of this call.
 * Up to d = POW_CHAIN_FUSED_MAX_D (csrc/pow_ctx.h; never above 32) the blocks
 * run fused: one launch per block, each reading the block the launch before it
 * sealed from device memory, queued in batches of about 2^26 expected trials
 * (1..64 blocks) with one bounded wait (10 s + 2 ns per counter of the batch's
 * windows) and one copy back per batch.  The cancel word is read at entry and
 * between batches, so a cancel takes up to one batch, a handful of
 * milliseconds.  Above that difficulty the call runs the host loop itself:
 * the refresh, then pow_mine with the same window and cancel word, block by
 * block.  Both give the same bytes.
 * *hashes_done (may be NULL) = trials issued.  pow_get_stats: launches,
 * kernel_ms (fused: events around each batch) and hashes.
 * pow_warmup does not launch this call's kernel (nor pow_verify_chain's): the
 * first fused call of a process also loads its code object.
 * Cost (MI355X): profiles/mine_chain/README.md. */
int pow_mine_chain(pow_ctx* ctx, const pow_block* parent, size_t n, unsigned diff_bits,
                   uint32_t owner, const uint64_t* created_at /* n entries, or NULL */,
                   uint64_t ctr_start, uint64_t ctr_count,
                   const volatile uint32_t* cancel_word, uint32_t epoch,
                   pow_block* out /* n blocks */, size_t* n_mined, uint64_t* hashes_done);

/* Mine n independent templates in one call: the reference's own workload, N
 * ranks each on its own template over the same parent (node.cpp:292-302), and
 * every other caller that holds many templates at once (a difficulty ladder,
 * the candidates after a fork, a simulated network on one GPU).
 * For every i < n the call gives exactly what pow_mine(ctx, &tmpls[i],
 * ctr_start, ctr_count, diff_bits, ...) gives; the templates share the window
 * and the difficulty, and one window without a solution stops nothing else.
 *   solved:   out[i] = tmpls[i] copied whole (552 bytes, padding included)
 *             with nonce = the 9 base-62 characters + NUL of the LOWEST
 *             solving counter of [ctr_start, ctr_start + ctr_count) and
 *             block_hash[0..64] = the 64 hex characters + NUL of the digest
 *             the GPU computed (bytes 65..255 stay the template's,
 *             node.cpp:318); found_ctr[i] = that counter.
 *   unsolved, or unreached (the call was cancelled before the template's
 *             launch): out[i] is not touched, found_ctr[i] = UINT64_MAX.
 * found_ctr (may be NULL): all n entries are written on every return >= 0.
 * out == tmpls (exactly the same array: sealing in place) is allowed; any
 * other overlap is not.
 * Returns 1 if all n were solved; 0 if some window held no solution or the
 * cancel word (optional; read at entry and between launches) differs from
 * `epoch`; *n_solved (may be NULL) says how many were solved.  n = 0 returns 1.
 * POW_EINVAL, checked in this order before the context is touched and with
 * nothing written: diff_bits > 256; ctr_count == 0 or > 2^32; ctr_start +
 * ctr_count > 62^9; n > 2^24; a null ctx, or null tmpls or out with n > 0; a
 * context bound to a stop board (boards and pow_cancel's in-flight path are
 * not part of this call).
 * Paths (all give the same bytes): n == 1 is pow_mine itself.  Above d =
 * POW_BATCH_FUSED_MAX_D (csrc/pow_ctx.h; never above 32) the call runs the
 * host loop itself: pow_mine template by template with the same cancel word.
 * Otherwise the templates run fused, in tiles: per tile one copy up of the raw
 * structs, ONE launch whose grid holds every template of the tile (256 lanes
 * per workgroup; per template lanes for four times the expected 2^d trials,
 * lowered to twice and then once while the launch's workgroups exceed one per
 * CU, and at most one workgroup per CU per template), one copy back of 48 bytes per
 * template and one bounded wait (10 s + 2 ns per counter of the tile's
 * windows); the host seals the blocks from the GPU's digests.  A tile is the
 * largest number of templates for which expected trials stay at or below
 * 2^26 (the cancel latency, a handful of milliseconds), workgroups at or
 * below 2^16, tile x ctr_count at or below 2^38 (so the watchdog stays a real
 * bound: 550 s at worst) and the tile at or below 2^14.  A 2^32 window
 * therefore gives tiles of 64 templates: a caller who wants large tiles passes
 * a window near what it needs, e.g. 2^(d + 7) counters.
 * Device memory: 12.7 MB, made at the first fused call, however large n is.
 * *hashes_done (may be NULL) = trials issued.  pow_get_stats: launches,
 * kernel_ms (fused: events around each launch) and hashes.
 * pow_warmup does not launch this call's kernel (nor pow_verify_chain's or
 * pow_mine_chain's): the first fused call of a process also loads its code
 * object and makes the buffers.
 * Cost (MI355X, profiles/mine_batch/README.md; medians of 9 calls, per
 * template, against the loop around pow_mine from C): 64 templates take 1.20 us
 * each at d = 9 (the loop: 35.7), 4.03 at d = 13 (34.7), 37.1 at d = 17 (51.9),
 * 97.7 at d = 19 (113.1), 346 at d = 21 (500) and 1,082 at d = 23 (3,035);
 * 1,024 templates at d = 9 take 0.36 us each over a 2^16 window (one launch)
 * and 1.28 over 2^32 (tiles of 64).  Two templates save one launch at d = 9
 * (26.9 against 39.8 us each) and nothing at d = 19 (135 against 132).
 * Nothing above d = 23 was measured. */
int pow_mine_batch(pow_ctx* ctx, const pow_block* tmpls, size_t n, unsigned diff_bits,
                   uint64_t ctr_start, uint64_t ctr_count,
                   const volatile uint32_t* cancel_word, uint32_t epoch,
                   pow_block* out /* n */, uint64_t* found_ctr /* n, may be NULL */,
                   size_t* n_solved /* may be NULL */, uint64_t* hashes_done /* may be NULL */);

/* Run the reference's race in one call: n_rivals miners each refresh their own
 * template on the current tip (node.cpp:292-302), the first to solve wins the
 * height, and its block is the tip of the next.  n heights on top of *parent.
 * Templates.  With `last` = *parent for height k = 0, else the winning block of
 * height k - 1, rival r's template at height k is `last` refreshed exactly as
 * pow_mine_chain does it: copied whole (all 552 bytes, padding included), index
 * = last.index + 1 (uint32_t wrap), node_owner_number = owners[r], difficulty =
 * diff_bits, created_at = created_at[k * n_rivals + r] (height-major;
 * created_at NULL: time(NULL), read once at entry, for every rival and height)
 * and previous_block_hash = all 256 bytes of last.block_hash (trap T5).
 * Winner.  Let c_r be what pow_mine gives rival r on its template over
 * [ctr_start, ctr_start + ctr_count): its LOWEST solving counter.  The winner
 * of the height is the rival with the lowest (c_r, r): the fewest trials, ties
 * in the counter to the lowest POSITION in owners[] (not the lowest owner
 * number).  Ties are real: only the low byte of node_owner_number and of
 * created_at is hashed, so owners 5 and 261 with equal created_at have
 * identical digests at every counter.
 * Outputs, tip first as pow_mine_chain's: the winner's sealed block goes to
 * out[n - 1 - k], with the bytes pow_mine gives on the winning template (nonce
 * = the 9 base-62 characters + NUL of c_r, block_hash = 64 hex + NUL, bytes
 * 65..255 of block_hash the template's, node.cpp:318); winners[n - 1 - k] (may
 * be NULL) = the winner's position r; found_ctr[n - 1 - k] (may be NULL) = its
 * absolute counter c_r.  After the call out + (n - *n_mined) is a tip-first
 * chain of *n_mined blocks whose oldest block is a child of *parent.
 * Returns 1 if all n heights were mined; 0 if it stopped early, because at some
 * height no rival's window held a solution or because the cancel word
 * (optional; read at entry and between batches) differs from `epoch`; *n_mined
 * (may be NULL) then says how far it got, as pow_mine_chain sets it, and the
 * entries of out, winners and found_ctr below that are not touched.  n = 0
 * returns 1.
 * POW_EINVAL, checked in this order before the context is touched and with
 * nothing written: diff_bits > 256; ctr_count == 0 or > 2^32; ctr_start +
 * ctr_count > 62^9; n > 2^24; n_rivals == 0 or > POW_RACE_MAX_RIVALS; a null
 * ctx, or a null parent, out or owners with n > 0; a context bound to a stop
 * board (boards and pow_cancel's in-flight path are not part of this call).
 * Paths (all give the same bytes).  n_rivals == 1 is pow_mine_chain itself.
 * Above d = POW_RACE_FUSED_MAX_D (csrc/pow_ctx.h; never above 32) the call runs
 * the host loop: per height it walks the rivals in position order, refresh and
 * then pow_mine with the same cancel word; every rival after the first hit
 * searches only [ctr_start, best counter so far), since a later position loses
 * a tie, and an empty remainder is skipped.  Otherwise the heights run fused:
 * ONE launch per height whose grid holds every rival (256 lanes per workgroup;
 * lanes for four times the expected 2^d trials split evenly over the rivals,
 * each rival at least one workgroup and at most its share of one per CU, so
 * the grid is at most max(n_rivals, CUs) workgroups).  All rivals of a launch
 * share one minimum of (counter, position), and a lane stops once its next pair
 * lies above it: a height costs about the trials of ONE solo block, not
 * n_rivals times that, and every pair below the answer is always tested.
 * Launches are queued in batches as pow_mine_chain's, about 2^26 expected
 * trials and at most 64 launches, the largest batch for which batch x n_rivals
 * x ctr_count stays at or below 2^38 (never below one height); per batch one
 * copy up of the parent, one of the owners and created_at, one copy back and
 * one bounded wait: 10 s + 2 ns per (counter, rival) pair of the batch, which
 * is 560 s at worst for a batch of several heights and 2,209 s for the one
 * height of 256 rivals over a 2^32 window.  A caller who wants a tighter bound
 * passes a window near what it needs, e.g. 2^(d + 7) counters.
 * Device memory: about 180 KB, made at the first fused call.
 * *hashes_done (may be NULL) = trials issued.  pow_get_stats: launches (fused:
 * one per height), kernel_ms (fused: events around each batch) and hashes.
 * pow_warmup does not launch this call's kernel (nor pow_verify_chain's,
 * pow_mine_chain's or pow_mine_batch's): the first fused call of a process
 * also loads its code object and makes the buffers.
 * Cost (MI355X, profiles/mine_race/README.md; medians of 9 calls of 8 heights,
 * per height, window 2^(d + 7)): fused, 3 and 64 rivals: 36 and 36 us at d = 9,
 * 40 and 40 at d = 13, 46 and 58 at d = 17, 133 and 135 at d = 19, 320 and 353
 * at d = 21, 1,100 and 2,237 at d = 23 (that race needed twice the pairs).  From
 * d = 19 the trials are within 13% of the (counter, rival) pairs the race needs;
 * at d <= 13 a height is one launch boundary and costs no less than 36 us.  The
 * host loop measured 74 us to 7.1 ms with 3 rivals and 1.3 to 103 ms with 64
 * (one launch per rival): it is slower than the loop of examples/mine_race.c
 * around pow_mine_batch at d <= 13 and at d = 23, faster only between.  The
 * fused path won at every measured d; nothing above d = 23 was measured. */
#define POW_RACE_MAX_RIVALS 256
int pow_mine_race(pow_ctx* ctx, const pow_block* parent, size_t n, unsigned diff_bits,
                  const uint32_t* owners, size_t n_rivals,
                  const uint64_t* created_at /* n * n_rivals, height-major, or NULL */,
                  uint64_t ctr_start, uint64_t ctr_count,
                  const volatile uint32_t* cancel_word, uint32_t epoch,
                  pow_block* out /* n, tip first */,
                  uint32_t* winners /* n, may be NULL */, uint64_t* found_ctr /* n, may be NULL */,
                  size_t* n_mined, uint64_t* hashes_done);

/* pow_mine with the reference's own nonces in place of the counter nonces:
 * "with seed S, which block does the reference mine, and after how many
 * trials?"  The call looks at trials [trial_start, trial_start + trial_count)
 * of the stream of srand(seed) (pow_rand_nonces above) on *tmpl.
 * Returns 1 with the LOWEST solving trial in *found_trial (may be NULL): *out =
 * *tmpl copied whole, nonce = that trial's nonce, block_hash[0..64] = the 64 hex
 * characters + NUL of the digest the GPU computed; bytes 65..255 of block_hash
 * stay the template's (node.cpp:318).  The reference tests its trials in order
 * and stops at the first that solves, so found_trial + 1 is where its stream
 * stands afterwards, also when a rival's block made it change template
 * mid-stream (the stream runs on across templates, node.cpp:285-302): a caller
 * replays a reference rank by calling again from found_trial + 1 on the next
 * template (examples/mine_rand.c).
 * Returns 0, with out not touched, if the window holds no solution or the
 * cancel word (optional; read at entry and between launches) differs from
 * `epoch`.
 * POW_EINVAL, checked in this order before the context is touched and with
 * nothing written: diff_bits > 32 (the kernel tests H0 <= threshold as
 * pow_mine_chain's does, and a 2^32 window at d > 32 more likely than not holds
 * nothing); trial_count == 0 or > 2^32; trial_start + trial_count >
 * POW_RAND_TRIAL_LIMIT; a null ctx, tmpl or out; a context bound to a stop
 * board.
 * The window runs in launches of at most 2^26 trials (the cancel latency, a
 * handful of milliseconds), in ascending order; the first launch with a hit
 * ends the call.  Per launch: one copy up (the control words, the generator's
 * state at the launch's first trial and the template), one copy back of 64
 * bytes and one bounded wait (10 s + 2 ns per trial).  In a launch lane g of G
 * walks runs of T consecutive trials of the stream, its 31-word generator state
 * in LDS; it starts from the launch's state moved by two polynomials of tables
 * that depend on T alone (made on the host at the first call with that T, 63
 * KB), and jumps from run to run by a third.  The grid is pow_mine_chain's
 * (lanes for four times the expected 2^d trials, at most one workgroup per CU);
 * T = 1 while that grid covers them, else the power of two at which one pass
 * does (at most 1,024).  All lanes share the lowest solving trial so far and
 * stop above it: every trial below the answer is tested.  The host seals the
 * block from the GPU's record and checks the nine characters the GPU hashed
 * against pow_rand_nonces: a difference fails the call with POW_EHIP.
 * *hashes_done (may be NULL) = trials issued.  pow_get_stats: launches,
 * kernel_ms (events around each launch) and hashes.  pow_warmup does not
 * launch this call's kernel: the first call of a process also loads its code
 * object and makes the buffers.
 * Cost (MI355X, profiles/mine_rand/README.md; medians of 9 passes over the same
 * templates, against pow_mine with counter nonces in the same process): SLOWER
 * than pow_mine at every d measured: 83.6 us per call at d = 9 (pow_mine:
 * 35.3), 87.2 at d = 13 (36.5), 150.5 at d = 17 (51.8), 409 at d = 19 (144),
 * 1,411 at d = 21 (452) and 5,508 at d = 23 (2,987).  A 2^30 window without a
 * solution at d = 32 runs at 6.27 G trials/s (pow_mine: 9.09).  The call is for
 * reproducing or auditing a reference run, not for throughput. */
int pow_mine_rand(pow_ctx* ctx, const pow_block* tmpl, uint32_t seed,
                  uint64_t trial_start, uint64_t trial_count, unsigned diff_bits,
                  const volatile uint32_t* cancel_word, uint32_t epoch,
                  pow_block* out, uint64_t* found_trial /* may be NULL */,
                  uint64_t* hashes_done /* may be NULL */);

/* The inverse of pow_rand_nonces: which srand() seed, at which trial, drew these
 * nonces?  The reference seeds with time(NULL) + mpi_rank and records the seed
 * nowhere, so an audit of a captured chain (pow_mine_rand above) starts here:
 * a block's created_at bounds the seeds, its nonce is the target.
 * The call returns EVERY (seed position p, trial t, target k) with p < n_seeds,
 * seed = seed_first + p in uint32_t arithmetic (a window may wrap through 2^32),
 * t in [trial_start, trial_start + trial_count), and the nine characters of
 * pow_rand_nonces(seed, t, 1) equal to the first nine bytes of nonces[k]
 * (nonces: n_targets x POW_NONCE_SIZE bytes; byte 9 of each is not read).  The
 * search is exhaustive: no early exit.  out is sorted ascending by (p, t, k);
 * *n_found = the number of matches, also when it exceeds cap, in which case
 * POW_ENOSPC is returned and out holds the first cap matches in that order (the
 * host keeps every match of the call before it sorts; out may be NULL when cap
 * == 0).  Seeds 0 and 1 have the same stream (srand(0) is srand(1)): a window
 * that holds both reports both, a real tie and not an error.
 * Returns 1 if at least one match was found; 0, with *n_found = 0 and out not
 * touched, if none was or if the cancel word (optional; read at entry and
 * between launches) differs from `epoch`.
 * POW_EINVAL, checked in this order before the context is touched and with
 * nothing written: n_targets == 0 or > POW_SEED_MAX_TARGETS; n_seeds == 0 or >
 * POW_SEED_MAX_SEEDS; trial_count == 0 or > 2^32; trial_start + trial_count >
 * POW_RAND_TRIAL_LIMIT; a null ctx, nonces or n_found, or a null out with cap >
 * 0; a target with one of its nine characters outside a-z, A-Z, 0-9 (it cannot
 * match: refused rather than answered with nothing); a context bound to a stop
 * board.
 * The request runs in launches of at most 2^30 (seed, trial) pairs and at most
 * 2^26 trials per seed, tiles of seeds outermost.  In a launch every seed has up
 * to 256 workgroups; each seeds its generator on the device (no per-seed host
 * work or copy), moves it to the launch's first trial by one polynomial from the
 * host, and its lanes walk runs of T = 31 x 2^j consecutive trials with the
 * 31-word state in registers: no SHA-256 runs.  Two 62 x 62-bit tables, on a
 * target's first two characters and on its next two, stand in front of the
 * compare.  Per launch: one copy up (1.8 KB), one copy back (12 KB: a
 * counter and up to 1,024 matches; a
 * launch that counts more fails the call with POW_EHIP rather than return a
 * subset; 64 targets that all occur in it are 128 at the most) and one bounded
 * wait (10 s + 2 ns per pair).  The host checks every match against
 * pow_rand_nonces: a difference fails the call with POW_EHIP.
 * *pairs_done (may be NULL) = (seed, trial) pairs issued.  pow_get_stats:
 * launches, kernel_ms (events around each launch) and hashes, which for this
 * call counts (seed, trial) pairs: no hash is computed.  pow_warmup does not
 * launch this call's kernel: the first call of a process also loads its code
 * object and makes the buffers.
 * Cost (MI355X, profiles/find_seed/README.md; medians of 9 calls, kernel time,
 * one target / 64 targets): one seed x 2^20 trials 18 / 31 us (59 / 83 us per
 * call), x 2^32 trials 12.0 / 28.4 ms (360 / 151 G pairs/s: one seed has at most
 * table B's 256 workgroups, one per CU); 64 seeds x 2^32 trials 221 / 385 ms;
 * 4,096 seeds x 2^20 trials 3.2 / 5.7 ms, x 2^32 trials 14.1 / 24.7 s (1,244 /
 * 713 G pairs/s sustained, about 200 and 110 times pow_mine_rand's 6.27 G
 * trials/s).  A launch of 2^30 pairs takes 0.9 / 1.5 ms, against the 10.7 ms of
 * pow_mine_rand's full launch in the same process: the cancel latency.  The
 * reference's own srand + gen_random_nonce loop does 10.9 / 9.4 M pairs/s on one
 * core of the same box: 18 days for what the last row does in 14 s. */
#define POW_SEED_MAX_SEEDS (1u << 20)
#define POW_SEED_MAX_TARGETS 64
typedef struct pow_seed_match {
  uint32_t seed;   /* the srand() argument */
  uint32_t target; /* index into nonces[] */
  uint64_t trial;  /* absolute trial: pow_rand_nonces(seed, trial, 1) gives nonces[target] */
} pow_seed_match;
int pow_find_seed(pow_ctx* ctx, const char* nonces /* n_targets x POW_NONCE_SIZE */, size_t n_targets,
                  uint32_t seed_first, uint32_t n_seeds, uint64_t trial_start, uint64_t trial_count,
                  const volatile uint32_t* cancel_word, uint32_t epoch, pow_seed_match* out, size_t cap,
                  size_t* n_found, uint64_t* pairs_done /* may be NULL */);

/* In-flight cancellation (the reference re-checks its chain only after a
 * trial, node.cpp:315).  Publishes `epoch`, the caller's current value of the
 * cancel word, to the GPU: a pow_mine / pow_mine_any launch of this ctx whose
 * `epoch` argument differs stops at its next poll (one inner step, ~60 us)
 * instead of at its sub-round boundary (up to ~0.13 s), and the call returns 0.
 * Call it after bumping the cancel word, with its new value, from one thread
 * at a time.  It is a store into host memory the GPU reads (no HIP call), so
 * the thread driving the ctx may be inside pow_mine meanwhile.  The first
 * call arms the GPU-side check for the ctx.  Returns POW_OK. */
int pow_cancel(pow_ctx* ctx, uint32_t epoch);

/* Lowest-latency form of pow_mine: returns (1) SOME solving counter of the
 * range — the first one the GPU finds; every wave stops at its next step —
 * instead of the lowest.  Same arguments, outputs and return codes.  Not
 * deterministic (like the reference's rand() nonces, node.cpp:302); use it
 * where only time-to-block matters (the protocol node, the difficulty ladder). */
int pow_mine_any(pow_ctx* ctx, const pow_block* tmpl, uint64_t ctr_start, uint64_t ctr_count,
                 unsigned diff_bits, const volatile uint32_t* cancel_word, uint32_t epoch,
                 pow_block* out, uint64_t* found_ctr, uint64_t* hashes_done);

/* Deterministic parity / throughput mode: every solving counter of
 * [ctr_start, ctr_start + ctr_count) (ctr_count <= 2^32), written to out_ctrs
 * as (counter - ctr_start), ascending.  *n_found = number of solutions
 * (also when it exceeds cap, in which case POW_ENOSPC is returned and the
 * first `cap` entries are an unspecified subset).  out_ctrs may be NULL when
 * cap == 0 (count only).  cap <= 2^31 - 1 (the list is sorted on the device;
 * POW_EINVAL above).  Returns POW_OK. */
int pow_sweep(pow_ctx* ctx, const pow_block* tmpl, uint64_t ctr_start, uint64_t ctr_count,
              unsigned diff_bits, uint32_t* out_ctrs, size_t cap, size_t* n_found);

/* Sweep variant that leaves the (unsorted) solution list on the device and
 * returns only the count and the lowest solving counter (UINT64_MAX if none):
 * the shape a sharded multi-GPU round needs (the 8-byte min goes to an RCCL
 * all-reduce).  dev_out may be NULL (count + min only). */
int pow_sweep_device(pow_ctx* ctx, const pow_block* tmpl, uint64_t ctr_start, uint64_t ctr_count,
                     unsigned diff_bits, uint32_t* dev_out, size_t cap, size_t* n_found,
                     uint64_t* min_ctr);

/* Device memory on the ctx's GPU (for pow_sweep_device's dev_out). */
int pow_dev_alloc(pow_ctx* ctx, size_t bytes, void** out);
int pow_dev_free(pow_ctx* ctx, void* p);
/* Copy `bytes` from a device pointer to host memory (synchronous). */
int pow_dev_read(pow_ctx* ctx, const void* dev, void* host, size_t bytes);

/* ---- cross-GPU stop board (one node) ------------------------------------ */
/* The reference's ranks hear of a rival's block only through MPI, between
 * trials (node.cpp:315, 404).  When several GPUs search ONE template together
 * (pow_group_*, BASELINE config 4), the finder must stop the others inside
 * their running launches: a collective only runs between kernels.  A board is
 * a page of host memory every GPU of the node maps, one 64-bit slot per rank.
 * A context bound to slot s of a board, for the search tagged `tag`:
 *   - stores every hit of its pow_mine / pow_mine_any launches into slot s,
 *     from the kernel itself (system-scope store over PCIe);
 *   - stops, within one inner step, as soon as another slot holds a solution
 *     of the same tag that makes its remaining counters moot: in
 *     pow_mine_any any peer solution; in pow_mine a peer solution below the
 *     counters it would still compute (the lowest-counter result stays exact:
 *     counters below the peer's are always finished).
 * Such a call then returns 0 (the peer's result wins the caller's
 * reduction).  In pow_mine that includes a call that found a solution while a
 * peer already holds a lower one: the call's own counter is then not the
 * search's answer, and not necessarily the lowest of its own range (its waves
 * above the peer's counter may have stopped), so it is not reported.  A 1 from
 * a bound pow_mine is the lowest solution of its range; the search's answer is
 * the minimum over the ranks' results (pow_group_* reduce it for you).
 * pow_group_* use a board automatically; these entry points are for callers
 * that drive several contexts themselves. */
#define POW_BOARD_MAX_SLOTS 64
#define POW_BOARD_MAX_TAG 1023
typedef struct pow_board pow_board;
/* name NULL: memory private to this process (contexts of one process, one
 * host thread per GPU).  name "/x": POSIX shared memory shared by every
 * process of the node that opens the same name (one process per GPU); it is
 * created zeroed if absent.  nslots 1..64.  Opening, posting and peeking
 * need no GPU; the first pow_board_bind maps the page for the GPUs. */
int pow_board_open(const char* name, int nslots, pow_board** out);
/* Remove a named board's name (processes that opened it keep their mapping). */
int pow_board_unlink(const char* name);
/* Unbind every context from the board first. */
void pow_board_close(pow_board* b);
/* Bind ctx to `slot` for the search tagged `tag` (1..1023; use a new tag per
 * search so stale slots are ignored) and mark the slot "nothing found yet";
 * b = NULL unbinds.  The ctx's launches watch and feed the board until
 * unbound. */
int pow_board_bind(pow_ctx* ctx, pow_board* b, int slot, uint32_t tag);
/* Host-side view: publish `ctr` in `slot` for `tag`; lowest counter any other
 * slot holds for `tag` (UINT64_MAX = none). */
int pow_board_post(pow_board* b, int slot, uint32_t tag, uint64_t ctr);
int pow_board_peek(const pow_board* b, int except_slot, uint32_t tag, uint64_t* min_ctr);

/* ---- sharded search over several GPUs (RCCL) --------------------------- */
/* One template mined cooperatively by `nranks` GPUs, one pow_ctx each (one
 * process or host thread per GPU).  The reference has no such mode: its ranks
 * compete, each on its own template (node.cpp:302, 386).  These calls are
 * collective: every rank makes them with the same arguments.  RCCL is loaded
 * on first use (dlopen); without it they return POW_ECOMM. */
#define POW_GROUP_ID_BYTES 128 /* sizeof(ncclUniqueId) */
enum { POW_REDUCE_MIN = 0, POW_REDUCE_MAX = 1, POW_REDUCE_SUM = 2 };
typedef struct pow_group pow_group;

/* Rank `rank`'s contiguous static shard of [start, start + count): shards of
 * ranks 0..nranks-1 are consecutive and differ in size by at most one. */
void pow_group_partition(uint64_t start, uint64_t count, int rank, int nranks,
                         uint64_t* shard_start, uint64_t* shard_count);
/* Rank 0 makes the id; the caller hands it to every rank (MPI_Bcast, a file,
 * torch.distributed ...) before pow_group_init. */
int pow_group_unique_id(uint8_t id[POW_GROUP_ID_BYTES]);
/* Joins the RCCL communicator on ctx's GPU; returns once all ranks joined.
 * Bounded: the communicator is made non-blocking (ncclCommInitRankConfig,
 * config.blocking = 0) and polled (ncclCommGetAsyncError) until every rank
 * joined or 60 s passed; then it is aborted (ncclCommAbort) and POW_ECOMM
 * names the rank, nranks, device and elapsed time.  (The reference's ranks
 * block in MPI_Recv with no bound, node.cpp:155-161.) */
int pow_group_init(pow_ctx* ctx, int nranks, int rank, const uint8_t id[POW_GROUP_ID_BYTES],
                   pow_group** out);
/* pow_group_init with the caller's deadline for every rank to join (ms, > 0). */
int pow_group_init_within(pow_ctx* ctx, int nranks, int rank, const uint8_t id[POW_GROUP_ID_BYTES],
                          unsigned timeout_ms, pow_group** out);
/* The same group over a reduction the caller supplies instead of RCCL: the
 * rounds, the stop board and the {counter, go, ok} consensus of
 * pow_group_mine[_any] are unchanged, only the one all-reduce per round goes
 * through `reduce`.  For ranks that already share a transport (MPI_Allreduce
 * in an MPI job, torch.distributed gloo), and for several ranks on ONE GPU,
 * which RCCL refuses (the multi-process GPU tests).  RCCL stays the
 * collective of one process per GPU (pow_group_init).
 *   reduce(user, vals, n, op): in place over every rank's n <= 8 words with
 *       op = POW_REDUCE_*, collective (every rank calls it in the same order);
 *       returns 0 on success.  Called from the thread that calls pow_group_*.
 *   board_name: "/name" opens that node-local stop board (the same name on
 *       every rank; fresh per group; unlinked once every rank has joined), or
 *       NULL for none.
 *   ctx may be NULL: the group then carries only pow_group_allreduce_u64.
 * Collective: the first reduction (a barrier that also checks nranks) runs
 * inside this call. */
typedef int (*pow_group_reduce_fn)(void* user, uint64_t* vals, size_t n, int op);
int pow_group_init_custom(pow_ctx* ctx, int nranks, int rank, pow_group_reduce_fn reduce, void* user,
                          const char* board_name, pow_group** out);
void pow_group_destroy(pow_group* g);
/* The group as its transport sees it: *comm_count = the ranks in RCCL's
 * communicator (ncclCommCount) and *comm_device = its HIP device
 * (ncclCommCuDevice); for a custom group, nranks (every rank joined) and the
 * ctx's device (-1 without one).  Either pointer may be NULL.  The scaling
 * bench records both per rank to show that N distinct GPUs took part. */
int pow_group_info(const pow_group* g, int* comm_count, int* comm_device);
/* The file of the RCCL library pow_group_* use (loaded at the first call of
 * any pow_group_* that needs RCCL; no GPU work): the copy another library of
 * the process had already loaded (torch's librccl.so) if there is one, else
 * librccl.so.1 from the library search path.  POW_ECOMM if RCCL cannot be
 * loaded. */
int pow_group_rccl_path(char* path, size_t cap);
/* In-place all-reduce of n <= 8 uint64 words (POW_REDUCE_*), on ctx's stream.
 * A collective that fails or passes its deadline leaves the group broken:
 * every later collective of it returns POW_ECOMM at once (destroy it). */
int pow_group_allreduce_u64(pow_group* g, uint64_t* vals, size_t n, int op);
/* What this rank did in the group's last pow_group_mine[_any] call (no GPU
 * work, no collective): the N > 1 bench's record of whether the stop board
 * worked (a missing board shows as peers that run out their shards: a large
 * spread between the finder's and the last peer's mine_end_ns). */
typedef struct pow_group_search_info {
  int board_open;        /* the group has the node's stop board (pow_group_init opened it) */
  int board_bound;       /* the last search ran with this rank's context bound to it */
  uint32_t rounds;       /* rounds of the last search (one all-reduce each) */
  int local_found;       /* this rank's own launch found a solution in the last round */
  uint64_t mine_end_ns;  /* CLOCK_MONOTONIC when that launch returned (0: none ran) */
  double mine_ms;        /* wall ms in this rank's own launches, all rounds */
  double allreduce_ms;   /* wall ms in the rounds' all-reduces, waiting for peers included */
} pow_group_search_info;
int pow_group_last_search(const pow_group* g, pow_group_search_info* out);
/* On one node the ranks also share a stop board (named after the id, opened
 * by pow_group_init): a rank's hit stops the other GPUs inside their running
 * launches, not only at the round's all-reduce.
 * pow_mine over all ranks: rounds of `round_size` counters (0 = adaptive:
 * ~4x the expected trials first, then 4x larger up to 2^30 per rank), each
 * split into static shards; each rank mines the lowest solving
 * counter of its shard, then one 24-byte ncclAllReduce(ncclMin) per round
 * picks the winner, spreads cancellation (any rank whose cancel word moved
 * stops every rank: returns 0) and failures (every rank returns < 0).  On 1 the
 * result equals pow_mine's over the whole range on one GPU, on every rank:
 * *out / *found_ctr as pow_mine; *hashes_done = this rank's trials. */
int pow_group_mine(pow_group* g, const pow_block* tmpl, uint64_t ctr_start, uint64_t ctr_count,
                   uint64_t round_size, unsigned diff_bits, const volatile uint32_t* cancel_word,
                   uint32_t epoch, pow_block* out, uint64_t* found_ctr, uint64_t* hashes_done);
/* pow_mine_any over all ranks (time-to-block: the first solution any GPU
 * finds ends the search on every GPU).  Rounds of `round_size` counters (0 =
 * 2^32 per rank), static shards; the first hit stops the node's other GPUs
 * through the board, and one 24-byte all-reduce(min) per round agrees on the
 * winner: the lowest counter among the solutions the ranks found.  Same
 * outputs and return codes as pow_group_mine, the same result on every rank. */
int pow_group_mine_any(pow_group* g, const pow_block* tmpl, uint64_t ctr_start, uint64_t ctr_count,
                       uint64_t round_size, unsigned diff_bits, const volatile uint32_t* cancel_word,
                       uint32_t epoch, pow_block* out, uint64_t* found_ctr, uint64_t* hashes_done);

#ifdef __cplusplus
}
#endif

#endif /* POW_GPU_H */
