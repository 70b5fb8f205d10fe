"""Cases and expected values shared by tests/test_fr_lincomb_host.py (CPU) and tests/test_gpu_fr_lincomb.py: the operand matrix of
`snarkvm_hip_fr_lincomb` and the oracle's own AXPY chain over zero-padded operands that every result is compared with, bit for bit.
"""
import ctypes

import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib, plugin, synthetic
from snarkvm_amd.sonic_pc import FR_ONE
from tests import util

CHUNK = plugin.FR_LINCOMB_CHUNK
COUNTS = [1, 2, 5, 6, 7, 12, 13, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
R = pyref.R_MOD
SPECIAL = [0, 1, 2, R - 1, R - 2, (R + 1) // 2, (R - 1) // 2]

_pool = {}


def rnd(n, seed):
    """n Fr elements in memory (Montgomery) form, a slice of one pool per seed"""
    size = 1 << 16
    if n > size:
        return oracle.fr_op("from_bigint", synthetic.random_fr_integers(n, 0x11C0 + seed))
    if seed not in _pool:
        _pool[seed] = oracle.fr_op("from_bigint", synthetic.random_fr_integers(size, 0x11C0 + seed))
    return _pool[seed][:n]


def special(n, shift=0):
    """n elements cycling through {0, 1, 2, r-1, r-2, (r+-1)/2}, memory form"""
    base = util.ints_to_fr_mont(SPECIAL)
    return base[(np.arange(n) + shift) % len(SPECIAL)]


def raw(value, n):
    """n elements whose MEMORY limbs are the integer `value` (whatever field element that is the Montgomery form of)"""
    return np.tile(util.limbs(value, 4), (n, 1))


# the coefficient whose internal form (c * 2^261 mod r, what the kernel multiplies with) is the integer r - 1: its memory word times 2^5
RAW_MAX_COEFF = (R - 1) * pow(32, -1, R) % R


def ragged_lens(count, longest):
    """0, 1, `longest` and lengths in between, in no particular order; from the eleventh operand on one element longer each round"""
    pat = [longest, 0, 1, longest // 2 + 1, max(longest - 1, 0), longest, 3, longest // 3, 2, longest]
    return [min(pat[k % len(pat)] + k // len(pat), longest) if pat[k % len(pat)] else 0 for k in range(count)]


def make_case(count, longest, seed, kind="mixed"):
    """-> (coeffs (count, 4), [operand arrays]).  kind: mixed (random, with special values in every third operand and coefficient),
    special (only the special values), max (every product (r-1) * (r-1)), rawmax (every limb product as large as the arithmetic sees)."""
    lens = ragged_lens(count, longest)
    if kind == "max":
        return np.tile(util.ints_to_fr_mont([R - 1]), (count, 1)), [np.tile(util.ints_to_fr_mont([R - 1]), (n, 1)) for n in lens]
    if kind == "rawmax":
        return raw(RAW_MAX_COEFF, count), [raw(R - 1, n) for n in lens]
    if kind == "special":
        return special(count, seed), [special(n, k + seed) for k, n in enumerate(lens)]
    coeffs = rnd(count + seed, 7)[seed:].copy()
    coeffs[::3] = special(len(coeffs[::3]), seed)
    if count > 1:
        coeffs[1] = FR_ONE
    polys = [special(n, k) if k % 3 == 2 else rnd(n + k, 1 + k % 5)[k:] for k, n in enumerate(lens)]
    return coeffs, polys


def expected(coeffs, polys, n_out):
    """the oracle's chain: acc <- acc + c_k * pad(p_k), `add` when c_k is one"""
    acc = np.zeros((n_out, 4), dtype=np.uint64)
    for c, p in zip(np.asarray(coeffs, dtype=np.uint64).reshape(-1, 4), polys):
        padded = np.zeros((n_out, 4), dtype=np.uint64)
        padded[: len(p)] = p
        if np.array_equal(c, FR_ONE):
            acc = oracle.fr_vec_op("add", acc, padded)
        else:
            acc = oracle.fr_vec_op("axpy", acc, padded, np.tile(c, (n_out, 1)))
    return acc


def call_args(ptrs, lens, coeffs):
    """ctypes arguments (polys, lens, coeffs) of the two entry points; a zero-length operand travels as NULL"""
    k = len(ptrs)
    pp = (ctypes.c_void_p * max(1, k))(*[int(p) if n else None for p, n in zip(ptrs, lens)])
    pl = (ctypes.c_size_t * max(1, k))(*[int(n) for n in lens])
    cs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
    return pp, pl, cs


def selftest(out, n_out, ptrs, lens, coeffs):
    """snarkvm_hip_selftest_fr_lincomb over raw addresses; `out`: a numpy array or an address"""
    pp, pl, cs = call_args(ptrs, lens, coeffs)
    o = out.ctypes.data if isinstance(out, np.ndarray) else out
    return _lib.lib().snarkvm_hip_selftest_fr_lincomb(ctypes.c_void_p(o), n_out, len(ptrs), pp, pl, ctypes.c_void_p(cs.ctypes.data))
