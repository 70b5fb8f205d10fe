"""Cases and expected values shared by tests/test_fr_evaluate_host.py (CPU) and tests/test_gpu_fr_evaluate.py: the operands of
`snarkvm_hip_fr_evaluate` and what every result is compared with, bit for bit.

Expected values do not come from the library: the memory words of the coefficients are read as Python integers (the Montgomery form is
linear: sum_i (c_i R) z^i = (sum_i c_i z^i) R), the point is taken out of Montgomery form by tests/util.py, and the polynomial is evaluated
mod r in Python - Horner over blocks of 1024 coefficients, each block a sum of integer products.
"""
import ctypes
import operator

import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib, plugin
from tests import util
from tests.helpers import lincomb as lc
from tests.helpers import reduce_cases as rc

R = pyref.R_MOD
GUARD = 0x5A5A5A5A5A5A5A5A
INVALID_VALUE = 1  # hipErrorInvalidValue
MEMBERS, POINTS = plugin.FR_EVALUATE_MEMBERS, plugin.FR_EVALUATE_POINTS
GEOMETRIES = [(blocks, threads) for blocks in (1, 2, 3) for threads in (64, 128, 256)]
POINT_NAMES = ["zero", "one", "minus_one", "Z_is_one", "Z_is_minus_one", "generic"]
rnd, special, mixed = lc.rnd, lc.special, rc.mixed
_BLOCK = 1024


def mem_ints(v):
    """(n, 4) elements -> the Python integers of their memory words"""
    b = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(b[i : i + 32], "little") for i in range(0, len(b), 32)]


def from_mem_int(x):
    return util.limbs(x % R, 4).reshape(1, 4)


def point_int(z):
    return util.fr_mont_to_ints(z)[0]


def expected(poly, z):
    """sum_i poly[i] z^i mod r as a (1, 4) memory-form element; 0^0 = 1; the empty polynomial gives 0"""
    cs, x = mem_ints(poly), point_int(z)
    pw = [1] * _BLOCK
    for i in range(1, _BLOCK):
        pw[i] = pw[i - 1] * x % R
    step, acc = pw[-1] * x % R, 0
    for at in range((len(cs) - 1) // _BLOCK * _BLOCK if cs else -1, -1, -_BLOCK):
        acc = (acc * step + sum(map(operator.mul, cs[at : at + _BLOCK], pw))) % R
    return from_mem_int(acc)


def geometry(n_max):
    """what the device call launches for a longest member of n_max (snarkvm_hip_selftest_fr_evaluate_geometry)"""
    out = np.zeros(8, dtype=np.uint32)
    assert _lib.lib().snarkvm_hip_selftest_fr_evaluate_geometry(ctypes.c_size_t(n_max), ctypes.c_void_p(out.ctypes.data)) == 0
    return dict(zip(("blocks", "threads", "cap", "G", "members", "points", "pow", "bits"), (int(x) for x in out)))


G = None  # coefficients per Montgomery reduction, read off the library on first use


def group():
    global G
    if G is None:
        G = geometry(1)["G"]
    return G


def lengths(T):
    """the lengths at which a thread's walk has 0, 1, G - 1, G, G + 1, 2G and 2G + 1 elements for T threads per member"""
    g = group()
    return [0, 1, 2, T - 1, T, T + 1, g * T - 1, g * T, g * T + 1, 2 * g * T + 1]


def point(name, T):
    """(1, 4) Montgomery limbs.  With s the largest power of two that divides T: Z_is_one has order s (Z = z^T = 1), Z_is_minus_one has order
    2 s, so that z^T = (z^s)^(T / s) = (-1)^odd = -1 - order 2 T itself when T is a power of two."""
    if name == "generic":
        return rnd(1, 9).copy()
    if name in ("Z_is_one", "Z_is_minus_one"):
        lg = (T & -T).bit_length() - 1 + (name == "Z_is_minus_one")
        z = oracle.domain(lg)[0:1].copy()
        assert pow(point_int(z), T, R) == (1 if name == "Z_is_one" else R - 1)
        return z
    return util.ints_to_fr_mont([{"zero": 0, "one": 1, "minus_one": R - 1}[name]])


def coefficients(n, kind, seed=1):
    """mixed: random with 0, 1, 2, r-1, r-2, (r+-1)/2 at every fifth place and a non-zero c[0]; zero: the zero polynomial in n elements;
    top_only: only the top coefficient set; padded: mixed with the top quarter zeroed (an untrimmed buffer)"""
    if kind == "zero" or n == 0:
        return np.zeros((n, 4), dtype=np.uint64)
    if kind == "top_only":
        v = np.zeros((n, 4), dtype=np.uint64)
        v[n - 1] = rnd(1, 4)[0]
        return v
    v = np.ascontiguousarray(mixed(n, seed))
    v[0] = rnd(1, 5)[0]
    if kind == "padded":
        v[n - (n + 3) // 4 :] = 0
    return v


def call_args(ptrs, lens, points):
    """ctypes arguments (polys, lens, points) of the entry points; a zero-length member travels as NULL"""
    k = len(ptrs)
    pp = (ctypes.c_void_p * max(1, k))(*[int(p) if n else None for p, n in zip(ptrs, lens)])
    pl = (ctypes.c_size_t * max(1, k))(*[int(n) for n in lens])
    zs = np.ascontiguousarray(np.concatenate([np.asarray(z, dtype=np.uint64).reshape(1, 4) for z in points]) if k else np.zeros((0, 4), dtype=np.uint64))
    return pp, pl, zs


def selftest(polys, points, blocks, threads):
    """snarkvm_hip_selftest_fr_evaluate over numpy members -> (count, 4); the element behind the results is a guard"""
    k = len(polys)
    out = np.full((k + 1, 4), GUARD, dtype=np.uint64)
    pp, pl, zs = call_args([p.ctypes.data for p in polys], [len(p) for p in polys], points)
    assert _lib.lib().snarkvm_hip_selftest_fr_evaluate(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(k), pp, pl, ctypes.c_void_p(zs.ctypes.data), blocks, threads) == 0
    assert (out[k] == GUARD).all()
    return out[:k]


def grid_case(T):
    """every length of lengths(T) at every named point, kinds in rotation: -> (polys, points, expected (count, 4)).  60 members at 6 points."""
    kinds = ["mixed", "padded", "mixed", "top_only", "mixed", "zero"]
    polys, points, want = [], [], []
    for j, name in enumerate(POINT_NAMES):
        z = point(name, T)
        for i, n in enumerate(lengths(T)):
            polys.append(coefficients(n, "mixed" if name == "zero" else kinds[(i + j) % len(kinds)], seed=1 + i))
            points.append(z)
            want.append(expected(polys[-1], z))
    return polys, points, np.concatenate(want)


def list_case(count, n_points, longest=40):
    """`count` short members of ragged lengths at n_points distinct generic points, interleaved -> (polys, points, expected)"""
    zs = rnd(n_points + 20, 8)[20:]
    lens = lc.ragged_lens(count, longest)
    polys = [np.ascontiguousarray(rnd(n + k % 50, 1 + k % 5)[k % 50 :]) for k, n in enumerate(lens)]
    points = [zs[k % n_points : k % n_points + 1] for k in range(count)]
    return polys, points, np.concatenate([expected(p, z) for p, z in zip(polys, points)])
