"""Cases and expected values shared by tests/test_fr_reduce_host.py (CPU) and tests/test_gpu_fr_reduce.py: the operands of
`snarkvm_hip_fr_reduce` / `snarkvm_hip_fr_support` and what every result is compared with, bit for bit.

Expected values do not come from the library: `oracle.fr_op("to_bigint")` turns the elements into Python ints, the sum (of products) is
taken mod r in Python, and `oracle.fr_op("from_bigint")` gives the memory form back.  Support triples come from numpy on the host copy.
"""
import ctypes

import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib
from tests import util
from tests.helpers import lincomb as lc

R = pyref.R_MOD
SUM, DOT = 0, 1
GUARD = 0x5A5A5A5A5A5A5A5A
rnd, special, raw = lc.rnd, lc.special, lc.raw

def to_ints(v):
    """(n, 4) memory-form elements -> Python ints"""
    v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
    if v.shape[0] == 0:
        return []
    return [int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 for a, b, c, d in oracle.fr_op("to_bigint", v).tolist()]


def from_int(x):
    return oracle.fr_op("from_bigint", util.ints_to_fr([x % R]))


def expected(op, a, b=None):
    """sum_i a_i (op SUM) or sum_i a_i b_i (op DOT) mod r, as a (1, 4) memory-form element"""
    xs = to_ints(a)
    if op == SUM:
        return from_int(sum(xs))
    ys = to_ints(b)
    assert len(xs) == len(ys)
    return from_int(sum(x * y for x, y in zip(xs, ys)))


def expected_support(v):
    """(trimmed_len, leading_zeros, nonzero) by numpy"""
    v = np.asarray(v, dtype=np.uint64).reshape(-1, 4)
    nz = np.nonzero(v.any(axis=1))[0]
    if nz.size == 0:
        return (0, v.shape[0], 0)
    return (int(nz[-1]) + 1, int(nz[0]), int(nz.size))


def geometry(n):
    """{blocks, threads, cap (workgroups), G} of the device call for n elements (snarkvm_hip_selftest_fr_reduce_geometry)"""
    out = np.zeros(4, dtype=np.uint32)
    assert _lib.lib().snarkvm_hip_selftest_fr_reduce_geometry(n, out.ctypes.data) == 0
    return dict(zip(("blocks", "threads", "cap", "G"), (int(x) for x in out)))


def mixed(n, seed):
    """n elements: random, with the special values 0, 1, 2, r-1, r-2, (r+-1)/2 at every fifth place"""
    v = rnd(n + seed, 1 + seed % 5)[seed:].copy()
    v[::5] = special(len(v[::5]), seed)
    return v


def max_terms(n, kind):
    """(a, b) of n elements in which every product is the largest there is: kind "max": (r-1) * (r-1) as field elements; "rawmax": both MEMORY
    images the integer r - 1, the largest limbs the arithmetic multiplies (it streams both operands raw)"""
    v = np.tile(util.ints_to_fr_mont([R - 1]), (n, 1)) if kind == "max" else raw(R - 1, n)
    return v, v.copy()


def support_cases(n, second_block=None):
    """name -> vector of n elements for the placements of the issue: zero vector, single non-zeros, one-word elements, both ends"""
    def single(i, value=None):
        v = np.zeros((n, 4), dtype=np.uint64)
        v[i] = rnd(1, 4)[0] if value is None else value
        return v

    cases = {"zero": np.zeros((n, 4), dtype=np.uint64)}
    places = [0, 63, 64, 255, 256, n - 1] + ([] if second_block is None else list(second_block))
    for i in sorted({p for p in places if 0 <= p < n}):
        cases[f"single@{i}"] = single(i)
    cases["word0_only"] = single(n // 2, np.array([1, 0, 0, 0], dtype=np.uint64))             # 32-bit word 0
    cases["word7_only"] = single(n // 3, np.array([0, 0, 0, 1 << 32], dtype=np.uint64))       # 32-bit word 7
    ends = np.zeros((n, 4), dtype=np.uint64)
    ends[0], ends[n - 1] = rnd(2, 5)
    cases["both_ends"] = ends
    cases["mixed"] = mixed(n, 2)
    return cases


def selftest_reduce(op, a, b, n, blocks, threads):
    """snarkvm_hip_selftest_fr_reduce -> (1, 4); the element behind the result is a guard"""
    out = np.full((2, 4), GUARD, dtype=np.uint64)
    pa = a.ctypes.data if a is not None and len(a) else None
    pb = b.ctypes.data if b is not None and len(b) else None
    assert _lib.lib().snarkvm_hip_selftest_fr_reduce(op, out.ctypes.data, pa, pb, n, blocks, threads) == 0
    assert (out[1] == GUARD).all()
    return out[:1]


def selftest_support(v, n, blocks, threads):
    out = np.full(4, GUARD, dtype=np.uint64)
    assert _lib.lib().snarkvm_hip_selftest_fr_support(out.ctypes.data, v.ctypes.data if n else None, n, blocks, threads) == 0
    assert out[3] == GUARD
    return tuple(int(x) for x in out[:3])


def ptr(x):
    return ctypes.c_void_p(int(x) if x else None)
