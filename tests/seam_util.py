"""Shared pieces of the 32-bit difficulty seam tests: the recorded witnesses
(tests/golden/lz_witnesses.json), their hashlib references and the synthetic
digests with a chosen number of leading zero bits.  Nothing here calls the code
under test: every expected value is hashlib's or Python's bit_length."""
import functools
import hashlib
import json
import os
import random

from oracle.oracle import py_block_to_str, py_nonce_from_counter

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BEFORE, WINDOW = 1000, 2048   # a witness's window: [counter - BEFORE, counter - BEFORE + WINDOW)
SEAM_D = range(29, 36)
# which witness solves which difficulty (leading zeros 33, 32, 31)
SOLVES = {"S2": 33, "S1": 32, "S0": 31}


@functools.lru_cache(maxsize=None)
def witnesses() -> dict:
    with open(os.path.join(GOLDEN, "lz_witnesses.json")) as f:
        return json.load(f)


def seam_rows() -> list:
    rows = witnesses()["seam"]
    assert {r["template"]: r["leading_zeros"] for r in rows} == SOLVES
    return rows


def lz_of(digest: bytes) -> int:
    return 256 - int.from_bytes(digest, "big").bit_length()


def digest_of(t: dict, ctr: int) -> bytes:
    """hashlib over block_to_str (block.cpp:79-88, restated in Python) of the
    golden.json template `t` with counter `ctr`'s nonce."""
    return hashlib.sha256(py_block_to_str(t["index"], t["node_owner_number"], t["difficulty"], t["created_at"],
                                          py_nonce_from_counter(ctr),
                                          bytes.fromhex(t["previous_block_hash_hex"]))).digest()


_tables: dict = {}


def lz_table(t: dict, lo: int, hi: int) -> dict:
    """counter -> hashlib's leading zero bits over [lo, hi), computed once per counter."""
    tab = _tables.setdefault(t["name"], {})
    for c in range(lo, hi):
        if c not in tab:
            tab[c] = lz_of(digest_of(t, c))
    return tab


def want_list(t: dict, start: int, count: int, d: int) -> list:
    """Ascending (counter - start) of hashlib's solutions of [start, start + count) at d bits."""
    tab = lz_table(t, start, start + count)
    return [c - start for c in range(start, start + count) if tab[c] >= d]


def synthetic_digests() -> list:
    """(leading zero bits, 256-bit value): for every k in 0..256 the smallest
    and the largest digest with exactly k leading zero bits (k = 256: zero)."""
    out = []
    for k in range(257):
        if k == 256:
            out.append((256, 0))
            continue
        out.append((k, 1 << (255 - k)))
        out.append((k, (1 << (256 - k)) - 1))
    return out


def word_digests(seed: int = 32) -> list:
    """256-bit values that walk every word of the count: all ones, zero, for
    every word i the value with the words below i zero, word i = 1 and every
    later word 0xFFFFFFFF, and 1,000 random ones behind 0..8 zero words."""
    rng = random.Random(seed)
    out = [(1 << 256) - 1, 0]
    for i in range(8):
        low = 32 * (7 - i)
        out.append((1 << low) | ((1 << low) - 1))
    for _ in range(1000):
        zero_words = rng.randrange(9)
        out.append(rng.getrandbits(256) >> (32 * zero_words) if zero_words < 8 else 0)
    return out
