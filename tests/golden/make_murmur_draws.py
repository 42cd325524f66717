#!/usr/bin/env python3
"""Generates tests/golden/murmur_draws.json: the reference hash of every random draw of
tests/test_formats_cpu.py::test_murmur_matches_reference_build_when_present (seed 7, 20 draws per length),
so that test checks the same words against the reference's answers when oracle/_ref is not built.

Needs oracle/_ref/libref_hash.so (`make -C oracle ref` with the reference tree at REF, see oracle/Makefile).
The vectors (inputs + outputs, data only) travel; the reference does not.
"""
import ctypes as C
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = list(range(1, 18)) + [32, 64, 256]
DRAWS = 20


def draws():
    r = np.random.default_rng(7)
    for n in LENGTHS:
        for _ in range(DRAWS):
            yield r.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


if __name__ == "__main__":
    lib = C.CDLL(os.path.join(HERE, "..", "..", "oracle", "_ref", "libref_hash.so"))
    lib.ref_hash_u32s.restype = C.c_uint64
    lib.ref_hash_u32s.argtypes = [C.c_void_p, C.c_ulong]
    vectors = [{"words": w.tolist(), "hash": "%016x" % lib.ref_hash_u32s(w.ctypes.data, w.size)} for w in draws()]
    with open(os.path.join(HERE, "murmur_draws.json"), "w") as f:
        json.dump({"about": "MurmurHash64A(seed 0) of u32 words, computed by the reference's hash_utils.hpp "
                            "(oracle/_ref/libref_hash.so); see make_murmur_draws.py", "vectors": vectors},
                  f, separators=(",", ":"))
    print("wrote", len(vectors), "vectors")
