"""Cases and expected values shared by tests/test_fr_open_fold_host.py (CPU) and tests/test_gpu_fr_open_fold.py: the operand matrix of
`snarkvm_hip_fr_open_fold` and what every result is compared with, bit for bit - the oracle's own AXPY chain for the combination
(tests/helpers/lincomb.py: expected), `oracle.poly_divide` by X - z for the quotient and `oracle.poly_evaluate` for the value.
"""
import ctypes
import functools

import numpy as np

from oracle import cpu as oracle
from snarkvm_amd import _lib, poly
from tests import util
from tests.helpers import lincomb as lc

CHUNK = lc.CHUNK
R = lc.R
GUARD = 0x5A5A5A5A5A5A5A5A
INVALID_VALUE = 1  # hipErrorInvalidValue

# the ownership edges of both routes: the POLY_CHUNK levels of the recursion (32, 32^2); the route switch at 2048; a workgroup's last thread,
# its first thread and a lone coefficient in a workgroup (256 threads x C = 8 coefficients = 2048 per workgroup)
SMALL_LENGTHS = [1, 2, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 1]
# C doubles past 2^19 (256 workgroups of 2048); past 2^20 the call is back on the recursion
LARGE_LENGTHS = [1 << 19, (1 << 19) + 1, 1 << 20, (1 << 20) + 1]
COUNTS = [1, 5, 6, 7, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
KINDS = ["mixed", "special", "max", "rawmax"]
POINTS = ["zero", "one", "minus_one", "random", "order_2048"]

ONE = oracle.fr_op("from_bigint", np.array([[1, 0, 0, 0]], dtype=np.uint64))


def point(name):
    """(1, 4) Montgomery limbs.  minus_one = r - 1 is the element of order 2; order_2048 generates the 2^11 domain: the scan route's tables of
    m^(256 C j), C = 8, are all ones for it."""
    if name == "random":
        return lc.rnd(1, 9).copy()
    if name == "order_2048":
        return oracle.domain(11)[0:1].copy()
    return util.ints_to_fr_mont([{"zero": 0, "one": 1, "minus_one": R - 1}[name]])


def reference(coeffs, polys, n, z):
    """-> (comb, quotient, value) from the oracle: comb (n, 4); quotient (n, 4) = comb / (X - z), zeros from its degree on (element n - 1
    always); value (1, 4) = comb(z)"""
    comb = lc.expected(coeffs, polys, n)
    quot = np.zeros((n, 4), dtype=np.uint64)
    trimmed = poly.trim(comb)
    if trimmed.shape[0] > 1:
        q, _ = oracle.poly_divide(trimmed, [(0, oracle.fr_op("neg", z)[0]), (1, ONE[0])])
        quot[: q.shape[0]] = q
    return comb, quot, oracle.poly_evaluate(comb, z)


@functools.lru_cache(maxsize=None)
def case(n, count, seed=1, kind="mixed", point_name="random", longest=None):
    """One cached case: (coeffs, polys, z, quotient, value); operand lengths lincomb.ragged_lens(count, longest or n).  Shared, never written."""
    coeffs, polys = lc.make_case(count, n if longest is None else longest, seed, kind)
    coeffs, polys = np.ascontiguousarray(coeffs), [np.ascontiguousarray(p) for p in polys]
    z = point(point_name)
    _, quot, value = reference(coeffs, polys, n, z)
    for a in [coeffs, z, quot, value] + polys:
        a.setflags(write=False)
    return coeffs, polys, z, quot, value


def call_args(ptrs, lens, coeffs, z):
    """ctypes arguments (polys, lens, coeffs, point) of the entry points; a zero-length operand travels as NULL"""
    pp, pl, cs = lc.call_args(ptrs, lens, coeffs)
    zz = np.array(z, dtype=np.uint64).reshape(1, 4)
    return pp, pl, cs, zz


def geometry(n):
    """(route, C, blocks, operands per table, terms of the fused sweep at most) of what the device call launches for n coefficients and a quotient"""
    out = (ctypes.c_uint32 * 5)()
    assert _lib.lib().snarkvm_hip_selftest_fr_open_fold_geometry(ctypes.c_size_t(n), out) == 0
    return tuple(out)


def default_geometry(n, with_quotient):
    route, C, blocks = geometry(n)[:3]
    if with_quotient and route == 1:
        return 1, C, blocks
    return 0, 32, ((n + 31) // 32 + 255) // 256


def selftest(quot, rem, n, ptrs, lens, coeffs, z, geo=None):
    """snarkvm_hip_selftest_fr_open_fold over raw addresses; quot / rem: numpy arrays, addresses or None; geo = (route, C, blocks), default:
    what the device call would launch"""
    pp, pl, cs, zz = call_args(ptrs, lens, coeffs, z)
    addr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a)  # noqa: E731
    route, C, blocks = default_geometry(n, quot is not None) if geo is None else geo
    return _lib.lib().snarkvm_hip_selftest_fr_open_fold(addr(quot), addr(rem), ctypes.c_size_t(n), ctypes.c_size_t(len(ptrs)), pp, pl,
                                                        ctypes.c_void_p(cs.ctypes.data) if len(ptrs) else None, ctypes.c_void_p(zz.ctypes.data), route, C, blocks)


def run_host(coeffs, polys, z, n, geo=None, want="qr"):
    """the host twin over numpy operands -> (quotient (n, 4) or None, value (1, 4) or None), after checking the guard words behind element n"""
    quot = np.full((n + 2, 4), GUARD, dtype=np.uint64) if "q" in want else None
    rem = np.full((2, 4), GUARD, dtype=np.uint64) if "r" in want else None
    assert selftest(quot, rem, n, [p.ctypes.data for p in polys], [len(p) for p in polys], coeffs, z, geo) == 0
    if quot is not None:
        assert (quot[n:] == GUARD).all(), "the elements behind the quotient were written"
    if rem is not None:
        assert (rem[1] == GUARD).all()
    return None if quot is None else quot[:n], None if rem is None else rem[:1]
