"""`snarkvm_hip_fr_lincomb` without a GPU (include/snarkvm_hip.h): the per-element routine of fr_lincomb_kernel (csrc/poly.hip.h:
fr_lincomb_at over Fp::sum_of_products, one Montgomery reduction per six terms) and the host-side bookkeeping of the call - validation,
longest-first order, the split into launches of FR_LINCOMB_CHUNK operands, the aliased operand's place - run on the CPU through
snarkvm_hip_selftest_fr_lincomb.  Every comparison is bit-exact against the oracle's own `fr_vec_op("axpy" | "add")` chain over
zero-padded operands (tests/helpers/lincomb.py); Fr elements have one representation, so the order of the terms cannot show.
"""
import ctypes

import numpy as np
import pytest

from snarkvm_amd import _lib, plugin, sonic_pc
from tests import util
from tests.helpers import lincomb as lc

GUARD = 0x5A5A5A5A5A5A5A5A


def run_host(coeffs, polys, n_out):
    out = np.full((n_out + 2, 4), GUARD, dtype=np.uint64)  # two elements behind the result that the call may not touch
    assert lc.selftest(out, n_out, [p.ctypes.data for p in polys], [len(p) for p in polys], coeffs) == 0
    assert (out[n_out:] == GUARD).all()
    return out[:n_out]


@pytest.mark.parametrize("count", lc.COUNTS)
def test_counts_and_ragged_lengths(count):
    """every group size, a short last group, one, two and three launches; lengths 0, 1, n_out and between; n_out at and past the longest"""
    for n_out, longest in ((1, 1), (37, 37), (37, 22), (5, 0)):
        coeffs, polys = lc.make_case(count, longest, count % 5)
        assert np.array_equal(run_host(coeffs, polys, n_out), lc.expected(coeffs, polys, n_out)), (count, n_out, longest)


@pytest.mark.parametrize("kind", ["special", "max", "rawmax"])
def test_edge_values(kind):
    """0, 1, 2, r-1, r-2, (r+-1)/2 as coefficients and elements; every term (r-1) * (r-1); and coefficient and element limbs both the integer
    r - 1 in the form the arithmetic multiplies, the largest column sums of sum_of_products"""
    for count in (1, 6, 7, lc.CHUNK, lc.CHUNK + 1):
        coeffs, polys = lc.make_case(count, 29, 1, kind)
        assert np.array_equal(run_host(coeffs, polys, 29), lc.expected(coeffs, polys, 29)), (kind, count)


@pytest.mark.parametrize("g", range(1, 7))
def test_sum_of_products_against_summed_products(g):
    """Fp::sum_of_products<G> alone (one element, G operands = one group) against G products of snarkvm_hip_selftest_field, summed by it"""
    L = _lib.lib()
    for a, b in ((lc.rnd(g, 3), lc.rnd(g + 9, 4)[9:]), (lc.special(g, g), lc.special(g, 3)), (lc.raw(lc.RAW_MAX_COEFF, g), lc.raw(lc.R - 1, g))):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        prod = np.zeros_like(a)
        assert L.snarkvm_hip_selftest_field(0, 2, ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(b.ctypes.data), ctypes.c_void_p(prod.ctypes.data), ctypes.c_size_t(g)) == 0
        want = np.zeros((1, 4), dtype=np.uint64)
        for k in range(g):
            term = np.ascontiguousarray(prod[k : k + 1])
            assert L.snarkvm_hip_selftest_field(0, 0, ctypes.c_void_p(want.ctypes.data), ctypes.c_void_p(term.ctypes.data), ctypes.c_void_p(want.ctypes.data), ctypes.c_size_t(1)) == 0
        got = run_host(a, [np.ascontiguousarray(b[k : k + 1]) for k in range(g)], 1)
        assert np.array_equal(got, want), g


def test_a_repeated_operand_and_overlapping_operands():
    p, q = lc.rnd(40, 1), lc.rnd(25, 2)
    polys = [p, q, p, p[3:20], q[:7], p]  # the same vector three times, and slices of both
    coeffs = lc.rnd(6, 7)
    assert np.array_equal(run_host(coeffs, polys, 41), lc.expected(coeffs, polys, 41))


@pytest.mark.parametrize("count", [1, 7, lc.CHUNK, lc.CHUNK + 1, 2 * lc.CHUNK + 1])
@pytest.mark.parametrize("which", ["first", "last"])
def test_out_is_the_start_of_an_operand(count, which):
    """in place: with more operands than one launch holds, the aliased operand must be read before the first launch overwrites it - also when it
    is the shortest operand and the last one listed"""
    n_out = 33
    coeffs, polys = lc.make_case(count, n_out, 2)
    k = 0 if which == "first" else count - 1
    polys[k] = lc.rnd(n_out if which == "first" else 4, 5)
    want = lc.expected(coeffs, polys, n_out)
    buf = np.zeros((n_out, 4), dtype=np.uint64)
    buf[: len(polys[k])] = polys[k]
    ptrs = [p.ctypes.data for p in polys]
    ptrs[k] = buf.ctypes.data
    assert lc.selftest(buf, n_out, ptrs, [len(p) for p in polys], coeffs) == 0
    assert np.array_equal(buf, want), (count, which)


def test_refused_arguments_leave_out_untouched():
    buf = np.full((64, 4), GUARD, dtype=np.uint64)
    p = lc.rnd(16, 1)
    c = lc.rnd(2, 7)
    before = buf.copy()
    # out one element into an operand; an operand starting inside out; an operand longer than n_out; a missing pointer
    assert lc.selftest(buf.ctypes.data + 32, 16, [buf.ctypes.data], [16], c[:1]) == -1
    assert lc.selftest(buf.ctypes.data, 16, [p.ctypes.data, buf.ctypes.data + 32 * 8], [16, 4], c) == -1
    assert lc.selftest(buf.ctypes.data, 8, [p.ctypes.data], [9], c[:1]) == -1
    pp, pl, cs = lc.call_args([0], [0], c[:1])
    pl[0] = 4
    assert _lib.lib().snarkvm_hip_selftest_fr_lincomb(ctypes.c_void_p(buf.ctypes.data), 8, 1, pp, pl, ctypes.c_void_p(cs.ctypes.data)) == -1
    assert np.array_equal(buf, before)
    # adjacent is not overlapping
    assert lc.selftest(buf.ctypes.data, 16, [buf.ctypes.data + 32 * 16], [16], c[:1]) == 0


def test_no_operands_zero_fills():
    out = np.full((9, 4), GUARD, dtype=np.uint64)
    assert lc.selftest(out, 7, [], [], np.zeros((0, 4), dtype=np.uint64)) == 0
    assert not out[:7].any() and (out[7:] == GUARD).all()
    assert lc.selftest(out, 7, [0, 0], [0, 0], lc.rnd(2, 7)) == 0  # only empty operands
    assert not out[:7].any()


# ---- the ABI itself, as far as it goes without a device ------------------------------------------------------------------
def test_nothing_to_write_is_success_and_needs_no_device():
    plugin.fr_lincomb_device(0, 0, [], [], np.zeros((0, 4), dtype=np.uint64))
    out = np.full((4, 4), 7, dtype=np.uint64)
    p = np.ones((4, 4), dtype=np.uint64)
    for on_device in (0, 1):
        pp, pl, cs = lc.call_args([p.ctypes.data], [0], lc.rnd(1, 7))
        _lib.check(_lib.lib().snarkvm_hip_fr_lincomb(out.ctypes.data, 0, 1, pp, pl, cs.ctypes.data, on_device))
    assert (out == 7).all()


def test_a_host_pointer_passed_as_device_memory_fails_loudly():
    """Without a GPU there is no device to run on; with one, host memory belongs to none: a non-zero code and a message either way"""
    p = np.ones((4, 4), dtype=np.uint64)
    out = np.full((4, 4), 7, dtype=np.uint64)
    with pytest.raises(_lib.HipError) as e:
        plugin.fr_lincomb_device(out.ctypes.data, 4, [p.ctypes.data], [4], lc.rnd(1, 7))
    assert e.value.code != 0 and e.value.message
    assert (out == 7).all()


@pytest.mark.parametrize("on_device", [0, 1])
def test_an_operand_longer_than_the_output_is_refused(on_device):
    p = np.ones((5, 4), dtype=np.uint64)
    out = np.full((5, 4), 7, dtype=np.uint64)
    pp, pl, cs = lc.call_args([p.ctypes.data], [5], lc.rnd(1, 7))
    with pytest.raises(_lib.HipError) as e:
        _lib.check(_lib.lib().snarkvm_hip_fr_lincomb(out.ctypes.data, 4, 1, pp, pl, cs.ctypes.data, on_device))
    assert e.value.code == 1 and "longer than n_out" in e.value.message  # hipErrorInvalidValue, from the argument check itself
    assert (out == 7).all()


# ---- sonic_pc.LinearCombination (data_structures.rs:525-576) -----------------------------------------------------------------
def _fr(v):
    return util.ints_to_fr_mont([v])[0]


def test_linear_combination_bookkeeping():
    LC, ONE = sonic_pc.LinearCombination, sonic_pc.ONE
    lin = LC.new("eq", [(_fr(3), "a"), (_fr(5), "b"), (_fr(lc.R - 3), "a"), (_fr(7), ONE), (_fr(4), "b")])
    # `new` merges equal terms and keeps a sum that came to zero (the reference's BTreeMap entry stays)
    assert len(lin) == 3 and lin.label == "eq" and not lin.is_empty()
    terms = list(lin.iter())
    assert [t for _, t in terms] == [ONE, "a", "b"]  # LCTerm::One sorts first
    assert np.array_equal(terms[0][0], _fr(7)) and not terms[1][0].any() and np.array_equal(terms[2][0], _fr(9))
    # `add` merges and drops a term whose coefficient becomes zero
    lin.add(_fr(lc.R - 9), "b")
    assert [t for _, t in lin.iter()] == [ONE, "a"]
    lin.add(_fr(2), "c").add(_fr(lc.R - 1), "c").add(_fr(lc.R - 7), ONE)
    assert [t for _, t in lin.iter()] == ["a", "c"] and np.array_equal(dict((t, c) for c, t in lin.iter())["c"], _fr(1))
    assert LC.empty("e").is_empty() and len(LC.empty("e")) == 0
    # the sum wraps around r exactly once
    big = LC.new("w", [(_fr(lc.R - 1), "x"), (_fr(lc.R - 1), "x")])
    assert np.array_equal(next(big.iter())[0], _fr(lc.R - 2))
