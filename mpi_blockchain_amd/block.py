"""The reference's Block model (block.h / block.cpp) over the native library.

Same names and meaning as the reference's free functions (block.h:27-34), so a
caller of the reference finds them here:

=========================  ====================================================
reference                  here
=========================  ====================================================
``struct Block``           :class:`Block` (ctypes, byte-identical, 552 B)
``block_to_str``           :func:`block_to_str` (270 bytes, traps T1/T2)
``block_to_hash``          :meth:`mpi_blockchain_amd.miner.GpuMiner.block_to_hash`
                           (GPU; needs a device context)
``solves_problem``         :func:`solves_problem` (run-time difficulty)
``gen_random_nonce``       :func:`gen_random_nonce` (same alphabet, seeded RNG) and
                           :func:`nonce_from_counter` (the GPU path's counter map)
``check_chain`` and more   :func:`verify_chain` (host statement of what
                           ``pow_verify_chain`` checks on the GPU:
                           :meth:`mpi_blockchain_amd.miner.GpuMiner.verify_chain`)
a pool in any order       :func:`index_blocks` and :func:`chain_from` (host statement of
                           ``pow_index_blocks``: the block tree of ``node_blocks``, every
                           chain in it audited, and the fork choice:
                           :meth:`mpi_blockchain_amd.miner.GpuMiner.index_blocks`)
a pool that is fed        :class:`BlockPool` (host statement of ``pow_pool``: the same answers kept
                           current while blocks arrive:
                           :meth:`mpi_blockchain_amd.miner.GpuMiner.open_pool`)
the same, many chains     :func:`verify_chains` and :func:`best_chain` (host statement of
                           ``pow_verify_chains``' verdicts and fork choice:
                           :meth:`mpi_blockchain_amd.miner.GpuMiner.verify_chains`)
``proof_of_work``, solo    :func:`mine_chain` (host statement of the blocks
                           ``pow_mine_chain`` mines on the GPU:
                           :meth:`mpi_blockchain_amd.miner.GpuMiner.mine_chain`)
``proof_of_work``, N       :func:`mine_batch` (host statement of what
ranks on one parent        ``pow_mine_batch`` mines on the GPU for many templates:
                           :meth:`mpi_blockchain_amd.miner.GpuMiner.mine_batch`)
=============================================================================
"""
from __future__ import annotations

import ctypes
import hashlib
import random
import time

from ._lib import HASH_SIZE, MSG_BYTES, NONCE_SIZE, POOL_NONE, POOL_ROOT, Block, check, load

# block.h:4-9, node.h:7-10
DEFAULT_DIFFICULTY = 9
BLOCKS_TO_MINE = 10
VALIDATION_MINUTES = 1
VALIDATION_BLOCKS = 5
TAG_NEW_BLOCK = 10
TAG_CHAIN_HASH = 21
TAG_CHAIN_RESPONSE = 22
MAX_BLOCKS = 200

ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"

__all__ = ["Block", "make_block", "block_to_str", "solves_problem", "nonce_from_counter",
           "gen_random_nonce", "field", "set_field", "verify_chain", "verify_chains", "best_chain", "index_blocks", "BlockPool", "prune_structs", "chain_from", "POOL_ROOT", "POOL_NONE", "mine_chain", "mine_batch", "V_HASH", "V_WORK", "V_LINK", "V_INDEX", "DEFAULT_DIFFICULTY", "BLOCKS_TO_MINE",
           "VALIDATION_MINUTES", "VALIDATION_BLOCKS", "HASH_SIZE", "NONCE_SIZE", "MSG_BYTES"]


def field(b: Block, name: str) -> bytes:
    """Raw bytes of a char[] field (ctypes' attribute access stops at NUL)."""
    f = getattr(Block, name)
    return ctypes.string_at(ctypes.addressof(b) + f.offset, f.size)


def set_field(b: Block, name: str, data: bytes) -> None:
    f = getattr(Block, name)
    data = bytes(data)[: f.size].ljust(f.size, b"\0")
    ctypes.memmove(ctypes.addressof(b) + f.offset, data, f.size)


def make_block(index: int = 0, owner: int = 0, difficulty: int = DEFAULT_DIFFICULTY, created_at: int = 0,
               prev: bytes = b"", nonce: bytes = b"", block_hash: bytes = b"") -> Block:
    b = Block()
    b.index = index & 0xFFFFFFFF
    b.node_owner_number = owner & 0xFFFFFFFF
    b.difficulty = difficulty & 0xFFFFFFFF
    b.created_at = created_at & 0xFFFFFFFFFFFFFFFF
    set_field(b, "previous_block_hash", prev)
    set_field(b, "nonce", nonce)
    set_field(b, "block_hash", block_hash)
    return b


def block_to_str(b: Block) -> bytes:
    """block.cpp:79-88: the exact 270-byte message the reference hashes."""
    out = ctypes.create_string_buffer(MSG_BYTES)
    check(load().pow_block_to_bytes(ctypes.byref(b), out))
    return out.raw


def solves_problem(hex_digest: str | bytes, difficulty: int = DEFAULT_DIFFICULTY) -> bool:
    """block.cpp:91-96 with the difficulty (leading zero BITS) as an argument."""
    if isinstance(hex_digest, str):
        hex_digest = hex_digest.encode()
    return bool(load().pow_solves_problem(hex_digest, difficulty))


def nonce_from_counter(ctr: int) -> bytes:
    """Counter -> nonce[10]: 9 base-62 chars (MSB first, alphabet of
    block.cpp:61-72) + NUL."""
    out = ctypes.create_string_buffer(NONCE_SIZE)
    check(load().pow_nonce_from_counter(ctr, out))
    return out.raw


def gen_random_nonce(rng: random.Random | None = None) -> bytes:
    """block.cpp:61-72 with a Python RNG in place of glibc rand()."""
    rng = rng or random
    return "".join(ALPHABET[rng.randrange(62)] for _ in range(NONCE_SIZE - 1)).encode() + b"\0"


# pow_verify_chain's status flags (include/pow_gpu.h POW_V_*)
V_HASH, V_WORK, V_LINK, V_INDEX = 1, 2, 4, 8


def _c_string(raw: bytes) -> bytes:
    """A char[] field as the reference's (string) cast reads it: cut at the
    first NUL, at most the whole field."""
    return raw.split(b"\0", 1)[0]


def verify_chain(blocks, difficulty: int = DEFAULT_DIFFICULTY) -> list[int]:
    """The status byte of every block of a chain, tip first (``blocks[i + 1]``
    is the parent of ``blocks[i]``): what ``pow_verify_chain`` computes on the
    GPU, stated on the host with hashlib.  Flags, each on its own:

    * ``V_HASH``  the hex of SHA-256 over ``block_to_str(b)`` is not ``block_hash`` as a C
      string (64 equal bytes, then NUL);
    * ``V_WORK``  the computed digest has fewer than `difficulty` leading zero bits (0..256);
    * ``V_LINK``  ``previous_block_hash`` is not the parent's ``block_hash``, both as C strings;
    * ``V_INDEX`` ``index - 1`` is not the parent's index, in 32-bit arithmetic.

    The last block has no parent in the chain: no link or index check."""
    if not 0 <= difficulty <= 256:
        raise ValueError(f"difficulty {difficulty} not in 0..256")
    n = len(blocks)
    stored = [field(b, "block_hash") for b in blocks]
    status = []
    for i, b in enumerate(blocks):
        digest = hashlib.sha256(block_to_str(b)).digest()
        flags = 0
        if stored[i][:64] != digest.hex().encode() or stored[i][64] != 0:
            flags |= V_HASH
        if 256 - int.from_bytes(digest, "big").bit_length() < difficulty:
            flags |= V_WORK
        if i < n - 1:
            if _c_string(field(b, "previous_block_hash")) != _c_string(stored[i + 1]):
                flags |= V_LINK
            if (b.index - 1) & 0xFFFFFFFF != blocks[i + 1].index:
                flags |= V_INDEX
        status.append(flags)
    return status


def verify_chains(chains, difficulty: int = DEFAULT_DIFFICULTY) -> list[list[int]]:
    """The status bytes of every chain of `chains`, each audited on its own:
    what ``pow_verify_chains`` computes on the GPU in one call.  A chain's
    last block never links to what follows it in the batch."""
    return [verify_chain(c, difficulty) for c in chains]


def best_chain(chains, statuses) -> int | None:
    """``pow_verify_chains``' fork choice, stated on the host: among the chains
    that are not empty and have no flagged block (``statuses[c]`` all zero),
    the position of the one whose tip, its first block, has the greatest
    ``index`` as a plain unsigned 32-bit number; the lowest position on a tie
    (the reference keeps what it saw first and moves only to a strictly higher
    index, node.cpp:249); None if no chain qualifies."""
    best = None
    for c, (chain, status) in enumerate(zip(chains, statuses)):
        if len(chain) == 0 or any(status):
            continue
        if best is None or chain[0].index > chains[best][0].index:
            best = c
    return best


def index_blocks(pool, difficulty: int = DEFAULT_DIFFICULTY):
    """``(status, parent, depth, n_bad, best)`` of a pool of blocks in any
    order: what ``pow_index_blocks`` computes on the GPU, stated on the host
    with hashlib and a dict.

    A block that is not flagged ``V_HASH`` has a name, its digest's hex; of
    several blocks with one name the lowest position keeps it (a dict's
    ``setdefault``, as ``std::map::insert``).  A block's parent is
    ``POOL_ROOT`` if its ``previous_block_hash`` as a C string is empty, the
    block of that name if there is one, ``POOL_NONE`` otherwise.  ``V_HASH``
    and ``V_WORK`` are :func:`verify_chain`'s; ``V_LINK``: the parent is
    ``POOL_NONE``; ``V_INDEX``: the parent is a block and ``index - 1`` is not
    its index in 32 bits.  ``depth[i]`` counts the blocks on the walk from i
    along ``parent``, i included, ``n_bad[i]`` the flagged ones among them.
    ``best`` is the block with ``n_bad == 0`` and the greatest index, the
    lowest position on a tie; None if there is none."""
    if not 0 <= difficulty <= 256:
        raise ValueError(f"difficulty {difficulty} not in 0..256")
    n = len(pool)
    status, names = [], {}
    for i, b in enumerate(pool):
        digest = hashlib.sha256(block_to_str(b)).digest()
        stored = field(b, "block_hash")
        flags = 0
        if stored[:64] != digest.hex().encode() or stored[64] != 0:
            flags |= V_HASH
        else:
            names.setdefault(digest.hex().encode(), i)
        if 256 - int.from_bytes(digest, "big").bit_length() < difficulty:
            flags |= V_WORK
        status.append(flags)
    parent = []
    for i, b in enumerate(pool):
        prev = _c_string(field(b, "previous_block_hash"))
        p = POOL_ROOT if prev == b"" else names.get(prev, POOL_NONE)
        if p == POOL_NONE:
            status[i] |= V_LINK
        elif p != POOL_ROOT and (b.index - 1) & 0xFFFFFFFF != pool[p].index:
            status[i] |= V_INDEX
        parent.append(p)
    depth, n_bad = [None] * n, [None] * n
    for i in range(n):
        walk = []
        j = i
        while j < n and depth[j] is None:  # names are digests: a walk cannot come back to itself
            walk.append(j)
            j = parent[j]
        d, f = (depth[j], n_bad[j]) if j < n else (0, 0)
        for k in reversed(walk):
            d, f = d + 1, f + (1 if status[k] else 0)
            depth[k], n_bad[k] = d, f
    best = None
    for i in range(n):
        if n_bad[i] == 0 and (best is None or pool[i].index > pool[best].index):
            best = i
    return status, parent, depth, n_bad, best


class BlockPool:
    """A pool that is fed: the host statement of ``pow_pool`` (``pow_pool_open``,
    ``pow_pool_add``, ``pow_pool_find``, ``pow_pool_mark``, ``pow_pool_prune``, the ancestry queries), incremental in its own right with a
    dict of names and a dict of waiting orphans.  After any sequence of
    :meth:`add` calls ``status``, ``parent``, ``depth``, ``n_bad``, ``best`` and
    ``ok`` are what :func:`index_blocks` gives on everything added so far, in
    the order of arrival.  ``adopted`` counts the last add's earlier blocks that
    were ``POOL_NONE`` and whose parent came with it."""

    def __init__(self, difficulty: int = DEFAULT_DIFFICULTY):
        if not 0 <= difficulty <= 256:
            raise ValueError(f"difficulty {difficulty} not in 0..256")
        self.difficulty = difficulty
        self.index, self.status, self.parent, self.depth, self.n_bad = [], [], [], [], []
        self.best, self.adopted, self.n_flagged = None, 0, 0
        self._names, self._waiting, self._children = {}, {}, {}
        self._name = []  # per block: its name, None for a V_HASH block (prune hands a dropped twin's name on)

    def __len__(self) -> int:
        return len(self.status)

    @property
    def ok(self) -> bool:
        return self.n_flagged == 0

    def results(self):
        """``(status, parent, depth, n_bad, best)``, as :func:`index_blocks` returns them."""
        return self.status, self.parent, self.depth, self.n_bad, self.best

    def find(self, name: bytes) -> int:
        """The named block of that text (the lowest position among twins), or ``POOL_NONE``."""
        return self._names.get(bytes(name), POOL_NONE)

    def _join(self, i: int, p: int) -> None:
        """Block i's parent is p: the link and index flags against it."""
        s = self.status[i] & (V_HASH | V_WORK)
        if p == POOL_NONE:
            s |= V_LINK
        elif p != POOL_ROOT:
            if (self.index[i] - 1) & 0xFFFFFFFF != self.index[p]:
                s |= V_INDEX
            self._children.setdefault(p, []).append(i)
        self.n_flagged += bool(s) - bool(self.status[i])
        self.status[i], self.parent[i] = s, p

    def _rank(self, i: int) -> None:
        """depth and n_bad of block i, of what it stands on if that is open,
        and of everything that stands on it; a sound block feeds ``best``."""
        todo = [i]
        while todo:
            j = todo.pop()
            p = self.parent[j]
            if p < len(self) and self.depth[p] is None:  # a new block under a new block: that one first
                todo += [j, p]
                continue
            d, f = (self.depth[p], self.n_bad[p]) if p < len(self) else (0, 0)
            self.depth[j], self.n_bad[j] = d + 1, f + bool(self.status[j])
            if self.n_bad[j] == 0 and (self.best is None or self.index[j] > self.index[self.best]
                                       or (self.index[j] == self.index[self.best] and j < self.best)):
                self.best = j
            todo += [c for c in self._children.get(j, ()) if self.depth[c] != self.depth[j] + 1
                     or self.n_bad[c] != self.n_bad[j] + bool(self.status[c])]

    def add(self, blocks) -> bool:
        base, new_names = len(self), []
        for i, b in enumerate(blocks, base):
            digest = hashlib.sha256(block_to_str(b)).digest()
            stored = field(b, "block_hash")
            flags = 0
            if stored[:64] != digest.hex().encode() or stored[64] != 0:
                flags |= V_HASH
            elif self._names.setdefault(digest.hex().encode(), i) == i:
                new_names.append(digest.hex().encode())
            self._name.append(None if flags & V_HASH else digest.hex().encode())
            if 256 - int.from_bytes(digest, "big").bit_length() < self.difficulty:
                flags |= V_WORK
            self.index.append(b.index)
            self.status.append(flags)
            self.n_flagged += bool(flags)
            self.parent.append(None)
            self.depth.append(None)
            self.n_bad.append(None)
        for i, b in enumerate(blocks, base):
            prev = _c_string(field(b, "previous_block_hash"))
            p = POOL_ROOT if prev == b"" else self._names.get(prev, POOL_NONE)
            if p == POOL_NONE:
                self._waiting.setdefault(prev, []).append(i)
            self._join(i, p)
        old = []
        for name in new_names:
            for i in self._waiting.pop(name, ()):  # all of them old: the new blocks were joined with every name in place
                self._join(i, self._names[name])
                old.append(i)
        self.adopted = len(old)
        for i in range(base, len(self)):
            if self.depth[i] is None:
                self._rank(i)
        for i in old:
            self._rank(i)
        return self.ok

    def mark(self, tips=(), min_index: int | None = None, sound_only: bool = False) -> list[int]:
        """The host statement of ``pow_pool_mark``: per block 1 if it is a
        seed or lies on the walk from a seed along ``parent``, else 0.  The
        seeds are the positions in `tips` and, unless `min_index` is None,
        every block with ``index >= min_index`` (`sound_only`: and ``n_bad ==
        0``; the tips are seeds whatever their flags)."""
        n = len(self)
        tips = [int(t) for t in tips]
        if any(not 0 <= t < n for t in tips):
            raise ValueError("a tip past the pool")
        seeds = list(tips)
        if min_index is not None:
            seeds += [i for i in range(n) if self.index[i] >= min_index and not (sound_only and self.n_bad[i])]
        on = [0] * n
        for i in seeds:
            while i < n and not on[i]:  # a marked block's walk is marked already
                on[i] = 1
                i = self.parent[i]
        return on

    def prune(self, tips=(), min_index: int | None = None, sound_only: bool = False) -> list[int]:
        """The host statement of ``pow_pool_prune``: the pool keeps exactly
        what :meth:`mark` marks, in its order, and every later :meth:`add` goes
        on from there.  Returns the map: per block of the pool before the call
        its new position, or ``POOL_NONE`` if it was dropped.  The marked set
        is closed under ``parent``, so status, depth and n_bad stand; parents,
        names, waiting orphans and children move to the new positions, and a
        name whose lowest twin was dropped goes to the lowest twin kept."""
        on = self.mark(tips, min_index, sound_only)
        new, kept = [], 0
        for m in on:
            new.append(kept if m else POOL_NONE)
            kept += m
        self.adopted = 0
        if kept == len(on):
            return new
        keep = [i for i, m in enumerate(on) if m]
        self.parent = [new[p] if p < len(on) else p for p in (self.parent[i] for i in keep)]
        self.index, self.status, self.depth, self.n_bad, self._name = (
            [a[i] for i in keep] for a in (self.index, self.status, self.depth, self.n_bad, self._name))
        self._names = {}
        for j, name in enumerate(self._name):
            if name is not None:
                self._names.setdefault(name, j)
        self._waiting = {prev: [new[i] for i in who if on[i]] for prev, who in self._waiting.items()}
        self._waiting = {prev: who for prev, who in self._waiting.items() if who}
        self._children = {new[p]: [new[c] for c in cs if on[c]] for p, cs in self._children.items() if on[p]}
        self.n_flagged = sum(1 for s in self.status if s)
        self.best = None
        for j in range(kept):
            if self.n_bad[j] == 0 and (self.best is None or self.index[j] > self.index[self.best]):
                self.best = j
        return new

    def _at(self, *pos) -> None:
        if any(not 0 <= int(i) < len(self) for i in pos):
            raise ValueError("a position past the pool")

    def ancestor(self, pos: int, steps: int) -> int:
        """The host statement of ``pow_pool_ancestors``, as a plain walk: the
        block `steps` steps along ``parent`` from `pos`, or the walk's end
        (``POOL_ROOT`` or ``POOL_NONE``) if the walk is shorter."""
        self._at(pos)
        i = int(pos)
        for _ in range(min(int(steps), self.depth[i])):
            i = self.parent[i]
        return i

    def fork_point(self, a: int, b: int):
        """The host statement of ``pow_pool_fork_points``: ``(at, back_a,
        back_b)``.  `at` is the first block on the walk from `a` that also lies
        on the walk from `b`, or ``POOL_NONE``; the backs are the steps from `a`
        and `b` to it, or with no shared block the two depths."""
        self._at(a, b)
        steps_b, i, s = {}, int(b), 0
        while i < len(self):
            steps_b[i] = s
            i, s = self.parent[i], s + 1
        i, s = int(a), 0
        while i < len(self):
            if i in steps_b:
                return i, s, steps_b[i]
            i, s = self.parent[i], s + 1
        return POOL_NONE, self.depth[int(a)], self.depth[int(b)]

    def chain(self, tip: int, max_len: int | None = None) -> list[int]:
        """The host statement of ``pow_pool_chain``: `tip`, its parent and so
        on, at most `max_len` positions (all of the walk by default)."""
        self._at(tip)
        walk, i = [], int(tip)
        while i < len(self) and (max_len is None or len(walk) < max_len):
            walk.append(i)
            i = self.parent[i]
        return walk

    def tips(self, sound_only: bool = False) -> list[int]:
        """The host statement of ``pow_pool_tips``: the positions no block has
        as its ``parent``, ascending (`sound_only`: and ``n_bad == 0``)."""
        named = set(self.parent)
        return [i for i in range(len(self)) if i not in named and not (sound_only and self.n_bad[i])]

    def _members(self, root: int) -> list[int]:
        """The blocks whose walk along ``parent`` passes `root`, itself included, ascending."""
        n = len(self)
        state = [None] * n  # per block: is `root` on its walk
        state[root] = True
        for i in range(n):
            walk = []
            while i < n and state[i] is None:
                walk.append(i)
                i = self.parent[i]
            for j in walk:
                state[j] = i < n and state[i]
        return [i for i in range(n) if state[i]]

    def subtrees(self, roots):
        """The host statement of ``pow_pool_subtrees``, as plain walks:
        ``(size, height, best, best_index, on)``, the first four one entry per
        root, `on` per block 1 if it is a member of any root's subtree.  A
        root's members are the blocks whose walk passes it; ``best`` is the
        fork choice among them (``POOL_NONE`` and index 0 if none is sound)."""
        roots = [int(r) for r in roots]
        self._at(*roots)
        size, height, best, best_index, on = [], [], [], [], [0] * len(self)
        for r in roots:
            members = self._members(r)
            pick = None
            for i in members:
                on[i] = 1
                if self.n_bad[i] == 0 and (pick is None or self.index[i] > self.index[pick]):
                    pick = i
            size.append(len(members))
            height.append(max(self.depth[i] for i in members) - self.depth[r])
            best.append(POOL_NONE if pick is None else pick)
            best_index.append(0 if pick is None else self.index[pick])
        return size, height, best, best_index, on

    def drop(self, roots) -> list[int]:
        """The host statement of ``pow_pool_drop``: the pool loses every member
        of every root's subtree and keeps the rest in its order; returns the
        map as :meth:`prune` does.  What is kept is closed under ``parent``
        and is exactly what its own tips mark, so the prune does the rest."""
        on = self.subtrees(roots)[4]
        keep = [i for i in range(len(self)) if not on[i]]
        if len(keep) == len(self):
            self.adopted = 0
            return list(range(len(self)))
        return self.prune(tips=keep)


def prune_structs(blocks, new):
    """The survivors of a prune in their order: the blocks whose entry in
    `new` (``BlockPool.prune``'s or ``GpuPool.prune``'s map) is a position."""
    if len(blocks) != len(new):
        raise ValueError("one map entry per block")
    return [b for b, j in zip(blocks, new) if j != POOL_NONE]


def chain_from(pool, parent, i: int):
    """The chain under block i of a pool as a ctypes ``Block`` array, tip
    first, ready for :func:`verify_chain`: i, its parent, and so on along
    `parent` (``index_blocks``' second result) to the walk's end."""
    walk = []
    while i < len(pool):
        walk.append(i)
        i = parent[i]
    arr = (Block * len(walk))()
    for k, j in enumerate(walk):
        ctypes.memmove(ctypes.byref(arr, k * ctypes.sizeof(Block)), ctypes.addressof(pool[j]), ctypes.sizeof(Block))
    return arr


def mine_chain(parent: Block, n: int, difficulty: int = DEFAULT_DIFFICULTY, owner: int = 0, created_at=None,
               ctr_start: int = 0, ctr_count: int = 1 << 32) -> list[Block]:
    """The blocks ``pow_mine_chain`` produces, stated on the host with hashlib:
    `n` blocks on top of `parent`, each the child of the one before, returned
    tip first (``result[i + 1]`` is the parent of ``result[i]``).

    Block k's template is the block before it copied whole (node.cpp:292-299),
    then ``index + 1`` in 32 bits, `owner`, `difficulty`, ``created_at[k]`` (one
    ``time.time()`` for every block if `created_at` is None) and all 256 bytes
    of the parent's ``block_hash`` as ``previous_block_hash``.  It is sealed
    with the lowest counter of ``[ctr_start, ctr_start + ctr_count)`` whose
    digest has `difficulty` leading zero bits: its nonce, and the digest's hex
    + NUL over the first 65 bytes of ``block_hash`` (node.cpp:318).  Mining
    stops at the first block whose window holds no solution, so the result may
    be shorter than `n`."""
    if not 0 <= difficulty <= 256:
        raise ValueError(f"difficulty {difficulty} not in 0..256")
    if created_at is None:
        created_at = [int(time.time())] * n
    chain: list[Block] = []
    last = parent
    for k in range(n):
        b = Block()
        ctypes.memmove(ctypes.addressof(b), ctypes.addressof(last), ctypes.sizeof(Block))  # padding included
        b.index = (last.index + 1) & 0xFFFFFFFF
        b.node_owner_number = owner & 0xFFFFFFFF
        b.difficulty = difficulty & 0xFFFFFFFF
        b.created_at = created_at[k] & 0xFFFFFFFFFFFFFFFF
        set_field(b, "previous_block_hash", field(last, "block_hash"))
        msg = bytearray(block_to_str(b))
        for ctr in range(ctr_start, ctr_start + ctr_count):
            nonce = nonce_from_counter(ctr)
            msg[4:4 + NONCE_SIZE] = nonce
            digest = hashlib.sha256(msg).digest()
            if 256 - int.from_bytes(digest, "big").bit_length() >= difficulty:
                break
        else:
            break
        set_field(b, "nonce", nonce)
        ctypes.memmove(ctypes.addressof(b) + Block.block_hash.offset, digest.hex().encode() + b"\0", 65)
        chain.insert(0, b)
        last = b
    return chain


def mine_batch(tmpls, difficulty: int = DEFAULT_DIFFICULTY, ctr_start: int = 0,
               ctr_count: int = 1 << 32) -> list[tuple[Block | None, int | None]]:
    """What ``pow_mine_batch`` produces, stated on the host with hashlib: for
    every template of `tmpls`, on its own, ``(block, counter)`` with the lowest
    counter of ``[ctr_start, ctr_start + ctr_count)`` whose digest has
    `difficulty` leading zero bits, or ``(None, None)`` if the window holds
    none (the other templates are mined all the same).

    The block is the template copied whole (padding included) with the
    counter's nonce (9 base-62 characters + NUL) and the digest's hex + NUL
    over the first 65 bytes of ``block_hash`` (node.cpp:318: the bytes behind
    them stay the template's).  The nonce is made here, in Python, from the
    alphabet of block.cpp:61-72."""
    if not 0 <= difficulty <= 256:
        raise ValueError(f"difficulty {difficulty} not in 0..256")
    if ctr_start < 0 or ctr_count < 0 or ctr_start + ctr_count > 62 ** 9:
        raise ValueError("counter range past 62^9")
    limit = 1 << (256 - difficulty)  # a digest solves iff it is below
    abc = ALPHABET.encode()
    results: list[tuple[Block | None, int | None]] = []
    for t in tmpls:
        msg = bytearray(block_to_str(t))
        msg[4 + NONCE_SIZE - 1] = 0
        found = None
        c, idx = ctr_start, [0] * 9  # the counter's base-62 digits, most significant first
        for i in range(8, -1, -1):
            c, idx[i] = divmod(c, 62)
        digits = bytearray(abc[k] for k in idx)
        for ctr in range(ctr_start, ctr_start + ctr_count):
            if ctr != ctr_start:  # + 1 with carry
                i = 8
                while idx[i] == 61:
                    idx[i], digits[i] = 0, abc[0]
                    i -= 1
                idx[i] += 1
                digits[i] = abc[idx[i]]
            msg[4:13] = digits
            digest = hashlib.sha256(msg).digest()
            if int.from_bytes(digest, "big") < limit:
                found = ctr
                break
        if found is None:
            results.append((None, None))
            continue
        b = Block()
        ctypes.memmove(ctypes.addressof(b), ctypes.addressof(t), ctypes.sizeof(Block))  # padding included
        set_field(b, "nonce", bytes(digits) + b"\0")
        ctypes.memmove(ctypes.addressof(b) + Block.block_hash.offset, digest.hex().encode() + b"\0", 65)
        results.append((b, found))
    return results


def mine_race(parent: Block, n: int, difficulty: int = DEFAULT_DIFFICULTY, owners=(0,), created_at=None,
              ctr_start: int = 0, ctr_count: int = 1 << 32) -> tuple[list[Block], list[int], list[int]]:
    """What ``pow_mine_race`` produces, stated on the host with hashlib:
    ``(blocks, winners, counters)`` of a race of ``len(owners)`` rival miners
    over `n` heights on top of `parent`, all three tip first (entry ``i + 1``
    is the height below entry ``i``).

    At every height rival r's template is the block before it (`parent`, then
    the winner of the height below) copied whole (node.cpp:292-299), then
    ``index + 1`` in 32 bits, ``owners[r]``, `difficulty`,
    ``created_at[k * len(owners) + r]`` for height k in mining order (one
    ``time.time()`` for every rival and height if `created_at` is None) and all
    256 bytes of the parent's ``block_hash`` as ``previous_block_hash``.  The
    pairs (counter, r) are tried in ascending order over ``[ctr_start, ctr_start
    + ctr_count)``: the first whose digest has `difficulty` leading zero bits
    wins the height, so the winner needed the fewest trials and a tie in the
    counter goes to the lowest position in `owners`.  Its block is sealed with
    its nonce and the digest's hex + NUL over the first 65 bytes of
    ``block_hash`` (node.cpp:318).  The race stops at the first height at which
    no rival's window holds a solution, so the result may be shorter than `n`."""
    if not 0 <= difficulty <= 256:
        raise ValueError(f"difficulty {difficulty} not in 0..256")
    if ctr_start < 0 or ctr_count < 0 or ctr_start + ctr_count > 62 ** 9:
        raise ValueError("counter range past 62^9")
    R = len(owners)
    if not 1 <= R <= 256:
        raise ValueError(f"{R} rivals not in 1..256")
    if created_at is None:
        created_at = [int(time.time())] * (n * R)
    if len(created_at) != n * R:
        raise ValueError(f"created_at has {len(created_at)} entries for {n} heights of {R} rivals")
    limit = 1 << (256 - difficulty)  # a digest solves iff it is below
    blocks: list[Block] = []
    winners: list[int] = []
    counters: list[int] = []
    last = parent
    for k in range(n):
        tmpls, msgs = [], []
        for r in range(R):
            b = Block()
            ctypes.memmove(ctypes.addressof(b), ctypes.addressof(last), ctypes.sizeof(Block))  # padding included
            b.index = (last.index + 1) & 0xFFFFFFFF
            b.node_owner_number = owners[r] & 0xFFFFFFFF
            b.difficulty = difficulty & 0xFFFFFFFF
            b.created_at = created_at[k * R + r] & 0xFFFFFFFFFFFFFFFF
            set_field(b, "previous_block_hash", field(last, "block_hash"))
            tmpls.append(b)
            msgs.append(bytearray(block_to_str(b)))
        won = None
        for ctr in range(ctr_start, ctr_start + ctr_count):
            nonce = nonce_from_counter(ctr)
            for r in range(R):
                msgs[r][4:4 + NONCE_SIZE] = nonce
                digest = hashlib.sha256(msgs[r]).digest()
                if int.from_bytes(digest, "big") < limit:
                    won = r
                    break
            if won is not None:
                break
        if won is None:
            break
        b = tmpls[won]
        set_field(b, "nonce", nonce)
        ctypes.memmove(ctypes.addressof(b) + Block.block_hash.offset, digest.hex().encode() + b"\0", 65)
        blocks.insert(0, b)
        winners.insert(0, won)
        counters.insert(0, ctr)
        last = b
    return blocks, winners, counters
