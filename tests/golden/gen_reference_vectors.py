#!/usr/bin/env python3
"""Records what the REFERENCE's own build (oracle/_ref, made by `make -C oracle
ref` where the reference's sources are present) gives for the fixed inputs of
the tests that compare against it, so that those tests also run where the
reference build is absent:

  reference_vectors.json
    agreement     the 200 (template, counter) cases of
                  tests/test_oracle.py::test_reference_build_agrees: the
                  reference's block_to_str (hex), block_to_hash and
                  solves_problem, and its sweep of S2 over [0, 2^14);
    random_nonces 100 gen_random_nonce() results after srand(1);
    log_chain     ref_log_chain's dump (rank 5) of the synthetic chains of
                  tests/test_node_host.py::test_chain_dump_matches_reference.

    python tests/golden/gen_reference_vectors.py      # needs oracle/_ref

The tests regenerate their inputs the same way (agreement_cases, and
test_node_host._chain) and, where oracle/_ref exists, also check that the live
reference still gives what is recorded here.
"""
import ctypes
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle.oracle import OBlock, RefLib, make_oblock, py_nonce_from_counter  # noqa: E402

LOG_CHAIN_SIZES = (1, 10, 37)
LOG_CHAIN_RANK = 5


def template_oblock(t) -> OBlock:
    return make_oblock(t["index"], t["node_owner_number"], t["difficulty"], t["created_at"],
                       bytes.fromhex(t["previous_block_hash_hex"]))


def agreement_cases(templates: dict):
    """The (template name, counter) sequence of test_reference_build_agrees."""
    rng = random.Random(11)
    names = list(templates)
    for _ in range(200):
        name = rng.choice(names)
        yield name, rng.randrange(62 ** 9)


def main():
    from helpers import reference_dump
    from test_node_host import _chain

    with open(os.path.join(HERE, "golden.json")) as f:
        templates = {t["name"]: t for t in json.load(f)["templates"]}
    R = RefLib("O2")
    cases = []
    for name, counter in agreement_cases(templates):
        b = template_oblock(templates[name])
        ctypes.memmove(ctypes.addressof(b) + OBlock.nonce.offset, py_nonce_from_counter(counter), 10)
        hx = R.block_to_hash(b)
        cases.append({"template": name, "counter": counter, "str_hex": R.block_to_str(b).hex(), "hash": hx,
                      "solves_d9": bool(R.solves_problem(hx))})
    got, n = R.sweep(template_oblock(templates["S2"]), 0, 1 << 14)
    R.L.ref_srand(1)
    nonces = [bytes(R.gen_random_nonce()).hex() for _ in range(100)]
    dumps = {str(n_): reference_dump(_chain(n_, random.Random(n_)), LOG_CHAIN_RANK).decode("latin-1")
             for n_ in LOG_CHAIN_SIZES}
    out = {"generator": "tests/golden/gen_reference_vectors.py",
           "reference": "oracle/_ref/libref_O2.so and oracle/_ref/ref_log_chain (the reference's own sources)",
           "agreement": {"cases": cases, "sweep_S2_2p14": {"count": int(n), "counters": [int(c) for c in got[:n]]}},
           "random_nonces": {"srand": 1, "nonces_hex": nonces},
           "log_chain": {"rank": LOG_CHAIN_RANK, "dumps_latin1": dumps}}
    with open(os.path.join(HERE, "reference_vectors.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote reference_vectors.json:", len(cases), "cases,", n, "sweep solutions,", len(nonces), "nonces,",
          {k: len(v) for k, v in dumps.items()}, "dump bytes")


if __name__ == "__main__":
    main()
