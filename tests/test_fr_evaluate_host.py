"""`snarkvm_hip_selftest_fr_evaluate`: the host twin of `snarkvm_hip_fr_evaluate` (include/snarkvm_hip.h; csrc/poly.hip.h: fr_evaluate_thread,
fr_evaluate_block and the combine of fr_reduce_kernel), walked over FORCED geometries so that at small lengths a thread's Horner walk has 0, 1,
G - 1, G, G + 1, 2G and 2G + 1 elements, and `_geometry` against the rule of the reductions.

Every value is compared bit for bit with the polynomial evaluated in Python integers (tests/helpers/evaluate_cases.py).
"""
import ctypes

import numpy as np
import pytest

from snarkvm_amd import _lib
from tests.helpers import evaluate_cases as ec
from tests.helpers import reduce_cases as rc


@pytest.mark.parametrize("blocks,threads", ec.GEOMETRIES)
def test_every_length_at_every_point(blocks, threads):
    """10 lengths x 6 points in one call: 60 members, twice the points one launch holds"""
    polys, points, want = ec.grid_case(blocks * threads)
    got = ec.selftest(polys, points, blocks, threads)
    for k in range(len(polys)):
        assert np.array_equal(got[k], want[k]), (k, len(polys[k]), ec.POINT_NAMES[k // 10])


def test_conventions():
    zero, one, z = ec.point("zero", 64), ec.point("one", 64), ec.point("generic", 64)
    p = ec.coefficients(300, "mixed")
    got = ec.selftest([p, p[:0], np.zeros((300, 4), dtype=np.uint64), p[:1]], [zero, z, z, z], 2, 64)
    assert np.array_equal(got[0], p[0]) and p[0].any(), "0^0 = 1: a zero point yields c[0]"
    assert not got[1].any() and not got[2].any(), "length 0 and the zero polynomial yield 0"
    assert np.array_equal(got[3], p[0]), "a constant"
    padded = np.concatenate([p, np.zeros((77, 4), dtype=np.uint64)])
    assert np.array_equal(ec.selftest([padded], [z], 2, 64), ec.selftest([p], [z], 2, 64)), "trailing zeros change nothing"
    assert np.array_equal(ec.selftest([p], [one], 1, 128), rc.expected(rc.SUM, p)), "at one: the sum of the coefficients"


@pytest.mark.parametrize("blocks,threads", [(1, 64), (3, 128)])
def test_ragged_members_in_one_call(blocks, threads):
    T, z = blocks * threads, ec.point("generic", 64)
    lens = [0, 1, 300, 2 * ec.group() * T + 1]
    polys = [ec.coefficients(n, "mixed", seed=2 + k) for k, n in enumerate(lens)]
    got = ec.selftest(polys, [z] * 4, blocks, threads)
    assert np.array_equal(got, np.concatenate([ec.expected(p, z) for p in polys]))


def test_one_buffer_at_two_points():
    p = ec.coefficients(1000, "mixed")
    z1, z2 = ec.rnd(2, 6)[0:1], ec.rnd(2, 6)[1:2]
    got = ec.selftest([p, p, p[:500]], [z1, z2, z1], 2, 128)
    assert np.array_equal(got, np.concatenate([ec.expected(p, z1), ec.expected(p, z2), ec.expected(p[:500], z1)]))
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("n_points", [1, 2, max(5, ec.POINTS + 1)])
def test_distinct_points(n_points):
    polys, points, want = ec.list_case(2 * n_points + 1, n_points, longest=700)
    assert np.array_equal(ec.selftest(polys, points, 2, 64), want)


@pytest.mark.parametrize("count", [ec.MEMBERS, ec.MEMBERS + 1, 2 * ec.MEMBERS + 2])
def test_counts_around_the_table_size(count):
    polys, points, want = ec.list_case(count, 2)
    assert np.array_equal(ec.selftest(polys, points, 1, 64), want)


def test_the_bytes_depend_on_no_geometry():
    polys, points, want = ec.list_case(9, 4, longest=3000)
    got = [ec.selftest(polys, points, b, t).tobytes() for b, t in ((1, 64), (3, 256), (2, 128))]
    assert got[0] == got[1] == got[2] == want.tobytes()


def test_refused_geometries_and_arguments():
    p, z = ec.coefficients(10, "mixed"), ec.point("generic", 64)
    out = np.full((2, 4), ec.GUARD, dtype=np.uint64)
    pp, pl, zs = ec.call_args([p.ctypes.data], [10], [z])
    st = _lib.lib().snarkvm_hip_selftest_fr_evaluate
    args = (ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(1), pp, pl, ctypes.c_void_p(zs.ctypes.data))
    for blocks, threads in ((0, 64), (1, 32), (1, 96), (1, 512), (4096, 256)):  # no workgroup; not whole waves; not a power of two; too wide; 2^20 threads
        assert st(*args, blocks, threads) != 0, (blocks, threads)
    null = (ctypes.c_void_p * 1)(None)
    assert st(args[0], args[1], null, pl, args[4], 1, 64) != 0, "a NULL member of non-zero length"
    assert st(None, args[1], pp, pl, args[4], 1, 64) != 0 and st(args[0], args[1], pp, pl, None, 1, 64) != 0
    too_long = (ctypes.c_size_t * 1)((1 << 29) + 1)
    assert st(args[0], args[1], pp, too_long, args[4], 1, 64) != 0
    assert st(args[0], ctypes.c_size_t(65536), pp, pl, args[4], 1, 64) != 0
    assert (out == ec.GUARD).all()
    assert st(None, ctypes.c_size_t(0), None, None, None, 1, 64) == 0, "count == 0 touches nothing"


@pytest.mark.parametrize("n_max", [1, 256, 257, 1 << 19, (1 << 19) + 1])
def test_geometry_follows_the_reductions(n_max):
    g, r = ec.geometry(n_max), rc.geometry(n_max)
    assert (g["blocks"], g["threads"], g["cap"]) == (r["blocks"], r["threads"], r["cap"])
    assert g["blocks"] == min(-(-n_max // g["threads"]), g["cap"])
    assert g["cap"] * g["threads"] <= 1 << g["bits"], "every thread index has its power in the table"
    assert (g["members"], g["points"]) == (ec.MEMBERS, ec.POINTS) and 1 <= g["G"] <= 5
