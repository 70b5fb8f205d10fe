"""`snarkvm_hip_fr_selector_fold` through its host replay (`snarkvm_hip_selftest_fr_selector_fold`: the same validation, member tables and split
into launches, the CPU in the kernels' place through the kernel's own per-index routine, csrc/poly.hip.h: fr_selector_at) - no GPU needed.

Every comparison is bit for bit.  Expected values (tests/helpers/selector_cases.py): the reference's four steps per member on the C++ oracle -
scale, divide by X^n - 1, multiply by X^N - 1, divide by X^n - 1 again, the second remainder asserted zero - and the sums from the member's
evaluations over its source domain; the tiling identity of the kernel is never its own oracle.
"""
import ctypes
import itertools

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib
from tests import util
from tests.helpers import selector_cases as sel

R = sel.R
GUARD = sel.GUARD


def check(polys, src_sizes, mus, N, h_len=None, want="hxs"):
    h_len = sel.quotient_len(polys, src_sizes) if h_len is None else h_len
    got = sel.selftest(polys, src_sizes, mus, N, h_len, want)
    exp = sel.expected(polys, src_sizes, mus, N, h_len)
    for w, g, e in zip("hxs", got, exp):
        if w in want:
            assert g is not None and np.array_equal(g, e), w
        else:
            assert g is None
    return got


# ---- class shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", sel.RATIOS)
@pytest.mark.parametrize("n", sel.SRC_SIZES)
def test_class_shapes(n, ratio):
    """one member of every length around the class boundaries, h_len exact and with a zero tail"""
    mu = sel.rnd(1, n + ratio)
    for L in sel.class_lengths(n):
        p = sel.mixed(L, 7 * n + L)
        check([p], [n], mu, n * ratio)
        h, _, _ = check([p], [n], mu, n * ratio, h_len=max(L - n, 0) + 5)
        assert not h[max(L - n, 0) :].any()


# ---- member counts -----------------------------------------------------------------------------------------------------------------------------
def _members(count, n, seed):
    lens = sel.class_lengths(n)
    polys = [sel.mixed(lens[(k + seed) % len(lens)], 100 * seed + k) for k in range(count)]
    mus = sel.rnd(count, 50 + seed)
    mus[: min(count, 3)] = sel.mont(sel.MULTIPLIERS)[: min(count, 3)]
    return polys, [n] * count, mus


@pytest.mark.parametrize("count", [1, 3, 24, 25])
def test_member_counts(count):
    """25 members take a second launch that adds to the outputs; the multipliers 0, 1 and r - 1 are among them"""
    polys, srcs, mus = _members(count, 8, count)
    check(polys, srcs, mus, 16)
    check(polys, srcs, mus, 8, h_len=40)


def test_forty_nine_members_take_three_launches():
    polys, srcs, mus = _members(49, 2, 3)
    check(polys, srcs, mus, 8)


def test_mixed_source_sizes_in_one_call():
    srcs = [256, 512, 1024, 256, 1024]
    lens = [2 * 256 + 1, 512 + 3, 3 * 1024 + 5, 255, 1024]
    polys = [sel.mixed(L, 11 + k) for k, L in enumerate(lens)]
    check(polys, srcs, sel.rnd(5, 4), 1024)


def test_the_same_polynomial_twice():
    p = sel.mixed(21, 5)
    mus = sel.mont([3, R - 3])
    h, xg, sums = check([p, p], [8, 8], mus, 16)
    assert not h.any() and not xg.any() and np.array_equal(sums[0], sums[1]) and sums.any()
    check([p, p, p[:9]], [8, 4, 8], sel.rnd(3, 6), 16)  # one array under two source domains, and a prefix of it


def test_special_operands_and_multipliers():
    """operands only from {0, 1, r - 1, (r - 1) / 2, (r + 1) / 2}, every multiplier of {0, 1, r - 1}"""
    for m, mu in enumerate(sel.MULTIPLIERS):
        polys = [sel.special(L, L + m) for L in (17, 8, 29)]
        check(polys, [8, 8, 8], sel.mont([mu, sel.MULTIPLIERS[(m + 1) % 3], mu]), 16)
    top = np.tile(sel.mont([R - 1]), (3 * 64 + 5, 1))
    check([top, top], [64, 64], sel.mont([R - 1, R - 1]), 128)


def test_every_combination_of_skipped_outputs():
    polys, srcs, mus = _members(5, 8, 9)
    for r in range(4):
        for combo in itertools.combinations("hxs", r):
            check(polys, srcs, mus, 16, want="".join(combo))


def test_an_empty_member_contributes_nothing_and_its_sum_is_zero():
    polys = [sel.mixed(19, 1), sel.ZERO, sel.mixed(3, 2)]
    h, xg, sums = check(polys, [8, 8, 8], sel.rnd(3, 8), 8)
    assert not sums[1].any() and sums[0].any()
    check([sel.ZERO, sel.ZERO], [4, 2], sel.rnd(2, 9), 4, h_len=3)


def test_no_member_zero_fills():
    h, xg, sums = sel.selftest([], [], sel.ZERO, 8, 5)
    assert h.shape == (5, 4) and xg.shape == (8, 4) and not h.any() and not xg.any() and sums.shape == (0, 4)


def test_a_source_domain_larger_than_every_length():
    """n above 2^30 (the kernel's index arithmetic clamps it) and no xg: h is empty, the sum is n p[0]"""
    n = (1 << 33) + 8
    p = sel.mixed(5, 3)
    _, pp, pl, ps, mu = sel.arrays([p], [n], sel.rnd(1, 1))
    sums, h = sel.guarded(1), sel.guarded(2)
    assert _lib.lib().snarkvm_hip_selftest_fr_selector_fold(h[1:].ctypes.data, 2, None, 0, sums[1:].ctypes.data, 1, pp, pl, ps, mu.ctypes.data) == 0
    assert not sel.unguard(h, 2).any()
    assert util.fr_mont_to_ints(sel.unguard(sums, 1)) == [n * util.fr_mont_to_ints(p[0:1])[0] % R]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched():
    L = _lib.lib()
    p0, p1 = sel.mixed(21, 1), sel.mixed(9, 2)
    polys, pp, pl, ps, mu = sel.arrays([p0, p1], [8, 4], sel.rnd(2, 3))
    block = np.full((64, 4), GUARD, dtype=np.uint64)  # h at 1 (13 elements), xg at 20 (16), sums at 40 (2)
    at = lambda i: block[i:].ctypes.data
    sizes = lambda *xs: (ctypes.c_size_t * len(xs))(*xs)
    ptrs = lambda *xs: (ctypes.c_void_p * len(xs))(*xs)

    def refused(h=at(1), h_len=13, xg=at(20), N=16, sums=at(40), count=2, polys=pp, lens=pl, srcs=ps, mus=mu.ctypes.data):
        assert L.snarkvm_hip_selftest_fr_selector_fold(h, h_len, xg, N, sums, count, polys, lens, srcs, mus) == -1
        assert (block == GUARD).all()

    assert L.snarkvm_hip_selftest_fr_selector_fold(at(1), 13, at(20), 16, at(40), 2, pp, pl, ps, mu.ctypes.data) == 0  # the call the refusals vary
    assert (block[0] == GUARD).all() and (block[14:20] == GUARD).all() and (block[36:40] == GUARD).all() and (block[42:] == GUARD).all()
    block[:] = GUARD
    refused(polys=None), refused(lens=None), refused(srcs=None), refused(mus=None)  # NULL arrays with count > 0
    refused(polys=ptrs(p0.ctypes.data, None))            # a NULL member of non-zero length
    refused(srcs=sizes(8, 0))                            # n_k == 0
    refused(N=0), refused(N=(1 << 28) + 8)               # xg given: target_size 0, above 2^28
    refused(N=8 * 3 + 4), refused(srcs=sizes(8, 3))      # n_k does not divide target_size
    refused(h_len=12)                                    # shorter than the longest quotient (21 - 8)
    refused(h_len=(1 << 29) + 1)
    refused(lens=sizes(21, (1 << 29) + 1))
    big = 65536
    refused(count=big, polys=(ctypes.c_void_p * big)(), lens=(ctypes.c_size_t * big)(), srcs=(ctypes.c_size_t * big)(*([1] * big)), mus=np.zeros((big, 4), dtype=np.uint64).ctypes.data)
    # overlaps: an output with a member, an output with another output
    refused(h=p0[20:].ctypes.data), refused(xg=p1.ctypes.data), refused(sums=p0[5:].ctypes.data)
    refused(h=at(8)), refused(sums=at(13)), refused(sums=at(35)), refused(xg=at(1))
    whole = np.concatenate([p0, np.full((13, 4), GUARD, dtype=np.uint64)])  # h directly behind its member is fine, one element earlier is not
    two = ptrs(whole.ctypes.data, p1.ctypes.data)
    assert L.snarkvm_hip_selftest_fr_selector_fold(whole[20:].ctypes.data, 13, None, 0, None, 2, two, pl, ps, mu.ctypes.data) == -1
    assert (whole[21:] == GUARD).all() and np.array_equal(whole[:21], p0)
    assert L.snarkvm_hip_selftest_fr_selector_fold(whole[21:].ctypes.data, 13, None, 0, None, 2, two, pl, ps, mu.ctypes.data) == 0
    assert np.array_equal(whole[21:], sel.expected([p0, p1], [8, 4], mu, None, 13)[0])
    # successes that touch nothing
    assert L.snarkvm_hip_selftest_fr_selector_fold(None, 0, None, 0, None, 2, pp, pl, ps, mu.ctypes.data) == 0
    assert L.snarkvm_hip_selftest_fr_selector_fold(None, 13, None, 16, None, 2, pp, pl, ps, mu.ctypes.data) == 0
    assert L.snarkvm_hip_selftest_fr_selector_fold(at(1), 0, None, 0, None, 0, None, None, None, None) == 0
    assert L.snarkvm_hip_selftest_fr_selector_fold(None, 0, None, 0, at(40), 0, None, None, None, None) == 0
    assert (block == GUARD).all()


# ---- known answers held by the reference (tests/golden/varuna_circuit0.json) -------------------------------------------------------------------
def test_the_assignment_formula_gives_z_lde_of_the_fixture(golden):
    """third.rs:236-239: z = w (X^4 - 1) + x with x the interpolation of the padded public input (1, 8, 32, 128) over the input domain"""
    fx = sel.fixture_round3(golden["varuna"])
    z = oracle.mul_by_vanishing(sel.mont(fx["w_lde"]), 4)
    x = oracle.ntt(sel.mont([1, 8, 32, 128]), direction=oracle.INVERSE)
    z[:4] = oracle.fr_vec_op("add", z[:4], x)
    assert util.fr_mont_to_ints(z) == fx["z_lde"]


def test_round_three_of_the_fixture_through_the_host_replay(golden):
    """h_1, g_1 of the fixture and the three sums: M(alpha, X) by Python ints (the Lagrange coefficients of alpha over R, the dense matrices of the
    fixture, the interpolation over C), the products with z_lde by the oracle, the fold by the replay"""
    from snarkvm_amd import matrices

    fx = sel.fixture_round3(golden["varuna"])
    dom, al = fx["domain"], fx["alpha"]
    assert len(dom) == 8
    lag = [(pow(al, 8, R) - 1) * w % R * pow(8 * (al - w), -1, R) % R for w in dom]  # L_w(alpha) = w (alpha^8 - 1) / (8 (alpha - w))
    assert sum(lag) % R == 1
    z = sel.mont(fx["z_lde"])
    polys, sums_want = [], []
    for name in "ABC":
        evals = [0] * 8
        for r, row in enumerate(fx["matrices"][name]):
            for j, v in enumerate(row):
                at = matrices.reindex_by_subdomain(8, 4, j)
                evals[at] = (evals[at] + v * lag[r]) % R
        m_poly = [sum(e * pow(dom[i], -c, R) for i, e in enumerate(evals)) * pow(8, -1, R) % R for c in range(8)]  # the inverse transform by ints
        assert util.fr_mont_to_ints(oracle.ntt(sel.mont(evals), direction=oracle.INVERSE)) == m_poly
        zs = fx["z_lde"]
        prod = [sum(m_poly[a] * zs[i - a] for a in range(8) if 0 <= i - a < 8) % R for i in range(15)]
        assert util.fr_mont_to_ints(oracle.polymul(4, [sel.mont(m_poly), z])[:15]) == prod
        polys.append(sel.mont(prod))
        sums_want.append(sum(sum(c * pow(w, i, R) for i, c in enumerate(prod)) for w in dom) % R)
    mus = sel.mont([1, fx["eta_b"], fx["eta_c"]])  # |C| / N = 1
    h, xg, sums = check(polys, [8, 8, 8], mus, 8)
    assert sel.trimmed_ints(h) == fx["h_1"] and len(fx["h_1"]) == 7
    assert sel.trimmed_ints(xg[1:]) == fx["g_1"] and len(fx["g_1"]) == 7
    assert util.fr_mont_to_ints(sums) == sums_want
