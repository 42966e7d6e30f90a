"""The reference's nonce stream, restated in pure Python for the tests of
pow_rand_nonces and pow_mine_rand: glibc's TYPE_3 rand() (seeding, walk and the
polynomial jump), gen_random_nonce's mapping (block.cpp:61-72) and a
brute-force miner over hashlib and the 270-byte message.  Independent of the
library: it shares no code with csrc/pow_host.cpp."""
import hashlib

ALPHABET = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
M32 = 0xFFFFFFFF
DEG = 31
TRIAL_LIMIT = 1 << 56


def seed_words(seed: int) -> list:
    """r[0..343] of srand(seed): draw k is r[k + 344] >> 1."""
    seed &= M32
    r = [seed or 1]
    for _ in range(1, 31):
        w = r[-1] - (1 << 32) if r[-1] & 0x80000000 else r[-1]  # (int32)
        hi = abs(w) // 127773 * (1 if w >= 0 else -1)            # C division: toward zero
        lo = w - hi * 127773
        v = 16807 * lo - 2836 * hi
        if v < 0:
            v += 2147483647
        r.append(v & M32)
    for i in range(31, 34):
        r.append(r[i - 31])
    for i in range(34, 344):
        r.append((r[i - 31] + r[i - 3]) & M32)
    return r


class Stream:
    """The stream of srand(seed), standing at a draw: `s` holds the last 31 words."""

    def __init__(self, seed: int, draw: int = 0):
        self.s = seed_words(seed)[-DEG:]
        if draw:
            self.s = apply_poly(x_power(draw), self.s)

    def rand(self) -> int:
        v = (self.s[0] + self.s[28]) & M32
        self.s = self.s[1:] + [v]
        return v >> 1

    def nonce(self) -> bytes:
        return bytes(ALPHABET[self.rand() % 62] for _ in range(9)) + b"\0"


def poly_mul(a: list, b: list) -> list:
    """a * b mod (x^31 - x^28 - 1), coefficients mod 2^32."""
    t = [0] * (2 * DEG - 1)
    for i, ai in enumerate(a):
        if ai:
            for j, bj in enumerate(b):
                t[i + j] += ai * bj
    for k in range(2 * DEG - 2, DEG - 1, -1):
        t[k - 3] += t[k]
        t[k - 31] += t[k]
    return [v & M32 for v in t[:DEG]]


def x_power(n: int) -> list:
    c = [1] + [0] * (DEG - 1)
    sq = [0, 1] + [0] * (DEG - 2)
    while n:
        if n & 1:
            c = poly_mul(c, sq)
        sq = poly_mul(sq, sq)
        n >>= 1
    return c


def apply_poly(c: list, s: list) -> list:
    e = list(s)
    for k in range(DEG, 2 * DEG - 1):
        e.append((e[k - 31] + e[k - 3]) & M32)
    return [sum(c[i] * e[i + j] for i in range(DEG)) & M32 for j in range(DEG)]


def nonces(seed: int, start: int, n: int) -> list:
    """gen_random_nonce's results at calls start .. start + n - 1 after srand(seed)."""
    st = Stream(seed, 9 * start)
    return [st.nonce() for _ in range(n)]


def message(block_bytes: bytes, nonce10: bytes) -> bytes:
    """block_to_str (block.cpp:79-88) of the raw 552-byte struct with `nonce10`."""
    b = block_bytes
    return bytes([b[0], b[4], b[8], b[16]]) + nonce10 + b[34:290]


def solves(digest: bytes, d: int) -> bool:
    return d == 0 or int.from_bytes(digest, "big") >> (256 - d) == 0


def mine(block_bytes: bytes, seed: int, start: int, count: int, d: int, want: int = 1) -> list:
    """The first `want` solving trials of [start, start + count), in order, as
    (trial, nonce10, hex digest)."""
    st = Stream(seed, 9 * start)
    head, tail = bytes([block_bytes[0], block_bytes[4], block_bytes[8], block_bytes[16]]), block_bytes[34:290]
    out = []
    for t in range(start, start + count):
        n = st.nonce()
        dg = hashlib.sha256(head + n + tail).digest()
        if solves(dg, d):
            out.append((t, n, dg.hex()))
            if len(out) == want:
                break
    return out


def seal(block_bytes: bytes, nonce10: bytes, hexd: str) -> bytes:
    """The success tail of node.cpp:311-318 on a refreshed template."""
    b = bytearray(block_bytes)
    b[24:34] = nonce10
    b[290:355] = hexd.encode() + b"\0"
    return bytes(b)
