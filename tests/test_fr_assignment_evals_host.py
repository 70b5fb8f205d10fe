"""`snarkvm_hip_fr_assignment_evals` through its host twin (`snarkvm_hip_selftest_fr_assignment_evals`: the validation of the device call, then the
kernel's own per-index routine, csrc/poly.hip.h fr_assignment_at, over a forced thread count), without a GPU: every shape of
tests/helpers/assignment_cases.py against the index map restated with numpy, strided members with untouched gaps, every refusal of the header, and
the identity the first round rests on - the inverse transform of the gathered vector is z, its quotient by X^|X| - 1 is w and its remainder is
x_poly - on the committed Varuna fixture with the definitional transform of oracle/pyref.py.

Every comparison is byte for byte.
"""
import numpy as np
import pytest

from oracle import pyref
from snarkvm_amd import _lib
from tests import util
from tests.helpers import assignment_cases as ac

GUARD = ac.GUARD


@pytest.mark.parametrize("threads", ac.THREADS)
@pytest.mark.parametrize("n,input_size,num_vars", ac.CASES)
def test_the_twin_follows_the_formula(n, input_size, num_vars, threads):
    row = ac.row(num_vars, n + num_vars)
    want = ac.expected(row, n, input_size)
    got = ac.selftest(row[None], n, input_size, threads)
    assert got.shape == (1, n, 4) and got[0].tobytes() == want.tobytes()
    ratio = n // input_size
    assert np.array_equal(want[::ratio], row[:input_size])  # the public input sits on the subgroup
    private = num_vars - input_size
    if ratio > 1:
        off = want[np.arange(n) % ratio != 0]
        assert np.array_equal(off[:private], row[input_size:]) and not off[private:].any()


def test_the_fixtures_vector():
    """ratio 2 at n = 8: public (1, 8, 32, 128) and private (2, 4, 2) interleave to (1, 2, 8, 4, 32, 2, 128, 0)"""
    row = ac.mont([1, 8, 32, 128, 2, 4, 2])
    for threads in ac.THREADS:
        assert util.fr_mont_to_ints(ac.selftest(row[None], 8, 4, threads)[0]) == [1, 2, 8, 4, 32, 2, 128, 0]


@pytest.mark.parametrize("count,stride_out,stride_vars", [(1, 0, 0), (3, 40, 23), (3, 37, 30), (5, 32, 20)])
def test_strided_members_leave_the_gaps_alone(count, stride_out, stride_vars):
    """n = 32 with 20 variables per row, the strides equal to and larger than the vector lengths; count == 1 ignores the strides"""
    n, input_size, num_vars = 32, 4, 20
    rows = np.stack([ac.row(num_vars, 50 + m) for m in range(count)])
    got = ac.selftest(rows, n, input_size, 3, stride_out or n, stride_vars or num_vars)
    for m in range(count):
        assert got[m].tobytes() == ac.expected(rows[m], n, input_size).tobytes(), m
    if count == 1:  # strides below the lengths are not looked at for one member
        L = _lib.lib()
        out = np.full((n + 2, 4), GUARD, dtype=np.uint64)
        assert L.snarkvm_hip_selftest_fr_assignment_evals(out[1:].ctypes.data, n, rows.ctypes.data, num_vars, input_size, 1, 1, 1, 3) == 0
        assert np.array_equal(out[1 : n + 1], got[0]) and (out[0] == GUARD).all() and (out[n + 1] == GUARD).all()


def test_the_identity_on_the_fixture(golden):
    """iNTT_8 of the gathered vector is z_lde; its quotient by X^4 - 1 is w_lde and its remainder is iNTT_4 of the public input"""
    tv = golden["varuna"]
    poly = lambda name: [int(x) for x in tv["polynomials"][name]]
    public, private = [1, 8, 32, 128], [2, 4, 2]
    assert [int(v) for v in tv["witness"][1]] == public + private
    evals = util.fr_mont_to_ints(ac.selftest(ac.mont(public + private)[None], 8, 4, 3)[0])
    z = pyref.ntt(evals, inverse=True)
    assert z == poly("z_lde") + [0] * (8 - len(poly("z_lde")))
    quotient, rest = [0] * 4, list(z)
    for i in range(7, 3, -1):  # long division by X^4 - 1
        quotient[i - 4] = rest[i]
        rest[i - 4] = (rest[i - 4] + rest[i]) % ac.R
        rest[i] = 0
    assert quotient == poly("w_lde") + [0] * (4 - len(poly("w_lde")))
    assert rest[:4] == pyref.ntt(public, inverse=True) and not any(rest[4:])


def test_refusals_leave_out_untouched():
    L = _lib.lib()
    n, num_vars = 8, 7
    rows = ac.row(32, 1)
    out = np.full((3 * 16 + 2, 4), GUARD, dtype=np.uint64)
    before = rows.copy()

    def call(o=out[1:].ctypes.data, n=n, v=rows.ctypes.data, num_vars=num_vars, input_size=4, count=2, stride_out=16, stride_vars=10, threads=3):
        return L.snarkvm_hip_selftest_fr_assignment_evals(o, n, v, num_vars, input_size, count, stride_out, stride_vars, threads)

    def refused(**bad):
        assert call(**bad) == -1, bad
        assert (out == GUARD).all() and np.array_equal(rows, before), bad

    refused(input_size=0)
    refused(input_size=3), refused(input_size=16)                     # input_size does not divide n
    refused(n=(1 << 28) + 4)                                          # n above 2^28 (4 divides it)
    refused(num_vars=3), refused(num_vars=9)                          # num_vars below input_size, above n
    refused(count=65536, stride_out=8, stride_vars=7)
    refused(stride_out=7), refused(stride_vars=6)                     # a stride shorter than its vector
    refused(stride_out=(1 << 40) + 1), refused(stride_vars=(1 << 40) + 1)
    refused(o=None), refused(v=None)                                  # a NULL operand of non-zero length
    refused(v=out[1 + 16 + 7 :].ctypes.data)                          # vars starts inside the second member's output
    refused(o=rows[5:].ctypes.data), refused(o=rows[16:].ctypes.data)  # out starts inside the first row, on the last element of the second
    refused(threads=0)
    # successes that touch nothing: no member, no element (the other arguments valid)
    assert call(count=0) == 0 and call(count=0, o=None, v=None) == 0
    assert call(n=0, num_vars=0) == 0 and call(n=0, num_vars=5, o=None, v=None) == 0
    assert (out == GUARD).all()
    # and the call the refusals vary succeeds: two members, the gap between them untouched
    assert call() == 0
    for m in range(2):
        assert np.array_equal(out[1 + 16 * m : 1 + 16 * m + n], ac.expected(rows[10 * m : 10 * m + num_vars], n, 4))
    assert (out[0] == GUARD).all() and (out[1 + n : 17] == GUARD).all() and (out[17 + n :] == GUARD).all()


def test_the_geometry_hook():
    blocks, threads, cap = ac.geometry(1)
    assert (blocks, threads) == (1, 256) and cap >= 1
    assert ac.geometry(cap * threads) == (cap, threads, cap) and ac.geometry(cap * threads * 2) == (cap, threads, cap)
    assert ac.geometry(257)[0] == 2
    assert _lib.lib().snarkvm_hip_selftest_fr_assignment_geometry((1 << 28) + 1, np.zeros(3, dtype=np.uint32).ctypes.data) == -1
    assert _lib.lib().snarkvm_hip_selftest_fr_assignment_geometry(8, None) == -1
