"""Key sets for the kbtree tests: klib's kbtree of chains (t = 5) as mem_chain drives it -- chain i
with key pos[i] inserted in turn, kb_lower(pos[i]) asked before each insertion, the in-order
traversal at the end.  The tree's shape only matters when keys tie, so besides distinct keys the
sets hold ties everywhere.  The oracle's answers (oracle/bwa_pe.c afo_debug_kbtree) are computed
once per case and shared by the CPU test (tests/test_oracle.py) and the GPU test
(tests/test_gpu_genome.py), which runs the device template on both of its stores.

store 0: the S2 store (32-bit keys, at most 32 chains; the first root split comes with key 10);
store 1: the genome store (64-bit keys; 700 keys pass its 96 LDS nodes, 1,100 its 1,024 LDS keys,
3,000 give three tree levels)."""
import ctypes
import functools

import numpy as np

import oracle

SIZES = {0: (1, 9, 10, 11, 19, 32), 1: (10, 100, 700, 1100, 3000)}
KINDS = ("distinct", "ascending", "descending", "three_values", "all_equal")


def keys(store, kind, n):
    hi = 2_000_000_000 if store == 0 else 6_000_000_000
    rng = np.random.default_rng([store, KINDS.index(kind), n])
    if kind == "three_values":
        return rng.choice(rng.choice(hi, 3, replace=False), n).astype(np.int64)
    if kind == "all_equal":
        return np.full(n, int(rng.integers(hi)), np.int64)
    k = rng.choice(hi, n, replace=False).astype(np.int64)
    return np.sort(k) if kind == "ascending" else np.sort(k)[::-1].copy() if kind == "descending" else k


def cases():
    return [(s, kind, n) for s in (0, 1) for kind in KINDS for n in SIZES[s]]


@functools.lru_cache(maxsize=None)
def oracle_answer(store, kind, n):
    """(rc, lower, order) of the oracle for the case; the arrays are read-only."""
    pos = keys(store, kind, n)
    lower = np.full(n, -9, np.int32)
    order = np.full(n, -9, np.int32)
    f = oracle.lib().afo_debug_kbtree
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    rc = f(pos.ctypes.data, n, lower.ctypes.data, order.ctypes.data)
    lower.setflags(write=False)
    order.setflags(write=False)
    return rc, lower, order
