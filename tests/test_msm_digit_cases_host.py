"""The case lists of tests/helpers/msm_digit_cases.py are what they claim, for every geometry tests/test_gpu_msm_digit_edges.py runs on the device
(and every table-less window width): the reference recoding reproduces every scalar, the top digit row cannot overflow for a scalar below r, every
row receives the digits at the ends of its range, and the three expected-value routes - the oracle's batched::msm, pyref's double-and-add on Python
integers, the device point arithmetic compiled for the host - agree on the scalars around r.  No GPU needed."""
import ctypes

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib
from tests import util
from tests.helpers import msm_digit_cases as mc

R = mc.R
# every geometry of the device test, then every table-less width, then (c, digit rows) = (4, 64) as tests/test_gpu_parity.py forces it on four tables
EXTRA = tuple((1, 0, c) for c in range(2, 17) if (1, 0, c) not in mc.GEOMETRIES) + ((4, 0, 4),)
ALL = mc.GEOMETRIES + EXTRA


def _id(key):
    return "%dx%d-c%d" % key


@pytest.mark.parametrize("key", ALL, ids=_id)
def test_recoding_reproduces_every_scalar_and_the_top_row_has_room(key):
    g, fam, vals, where = mc.cases(key)
    c, Wd = g.c, g.Wd
    assert g == mc.geometry(len(vals), key[2], key[0], mc.table_bits(key)) and g.nb == 1 << (c - 1) and g.Wd == g.W * g.J and g.wide == (c > 16)
    # the top row cannot overflow for any canonical scalar: the raw top digit of r - 1 still fits c bits (254-bit geometries - 127 rows of 2 bits -
    # rest on the leading bits of r: bias ~ 2/3 2^254, r ~ 0.29 2^254)
    assert R - 1 + mc.bias(c, Wd) < 1 << (c * Wd)
    assert c * Wd <= 288  # the 11-word recoding buffer of the kernels (MSM_BIAS_BITS)
    half = 1 << (c - 1)
    for s in vals:
        assert 0 <= s < R
        d, u = mc.recode(s, c, Wd)
        assert sum(dw << (c * w) for w, dw in enumerate(d)) == s
        assert all(0 <= uw < 1 << c and -half <= dw < half for uw, dw in zip(u, d))
        assert d[Wd - 1] >= 0  # s >= 0: the top row never takes a negative digit, so bucket nb - 1 of its window comes from the rows under it alone
    for name, at in where.items():
        assert tuple(vals[i] for i in at) == fam[name], name
    n = len(vals)
    assert n % 256 == 1 and n % 64 != 0 and vals[-1] == R - 1 and 300 <= n <= 1600
    # edge cases in the first block of 256, in a middle one and in the last full one; the lone scalar of the last block is one, too
    blocks = {i // 256 for at in where.values() for i in at}
    assert 0 in blocks and n // 256 - 1 in blocks and any(0 < b < n // 256 - 1 for b in blocks) and n // 256 >= 3


@pytest.mark.parametrize("key", ALL, ids=_id)
def test_every_row_receives_the_ends_of_its_digit_range(key):
    g, fam, vals, _ = mc.cases(key)
    c, Wd = g.c, g.Wd
    half = 1 << (c - 1)
    seen = [set() for _ in range(Wd)]
    alone = [set() for _ in range(Wd)]  # from scalars with at most three non-zero digits (the digit, a carry into it, a carry out of it): the other windows empty
    for members in fam.values():
        for s in set(members):
            d, _ = mc.recode(s, c, Wd)
            few = sum(1 for x in d if x) <= 3
            for w, dw in enumerate(d):
                seen[w].add(dw)
                if few:
                    alone[w].add(dw)
    top = Wd - 1
    for w in range(Wd):
        assert 1 in alone[w], (w, "+1")
        if w < top:
            assert -half in alone[w], (w, "-half: bucket nb - 1")
        # -1 and bucket nb - 2 with both signs: in every row but those that hold the leading bits of r, where the raw digit stops short of them
        # (c = 11: row 22 is bits 242 .. 252 and r >> 242 = 1 194 < 2 046).  The condition: whenever one of the two smallest scalars that give
        # row w the digit - the raw digit alone, or one less with a carry from the row below - is below r, the digit is there
        for d in mc.end_digits(c):
            routes = mc.digit_routes(c, w, d)
            assert all(mc.recode(v, c, Wd)[0][w] == d for v in routes if v < R)
            if any(v < R for v in routes):
                assert d in alone[w], (w, d)
            if c * w + c <= 252:  # rows wholly below the leading bit of r take every digit
                assert routes[0] < R
    assert min(seen[top]) >= 0 and max(seen[top]) == mc.top_digit_max(c, Wd) >= 1
    # the longest run of -half below r: raw digits half, half - 1, half - 1, ... up to the row that holds bit 252, then the carry
    s, m = 0, 0
    while s + ((half - (m > 0)) << (c * m)) < R:
        s, m = s + ((half - (m > 0)) << (c * m)), m + 1
    assert s in fam["carry_chains"] and m >= top - 1 and mc.recode(s, c, Wd)[0][: m + 1] == [-half] * m + [1]
    # 2^k - 1 = -1, 0 ..., +1 for every k up to 252
    assert all((1 << k) - 1 in fam["carry_chains"] for k in range(1, 253)) and (1 << 253) - 1 >= R
    # every row that straddles a 32-bit word of the recoding buffer has its edges, as far as they are scalars below r
    rows = mc.straddling_rows(c, Wd)
    assert (not rows) == (32 % c == 0)
    for w, b in rows:
        members = mc.word_edge_members(c, w, b)
        assert c * w < b <= c * w + c - 1 and b % 32 == 0
        for v in members:
            assert (v in fam["word_edges"]) == (v < R), (w, b)
        if c * w + c - 1 < 252:
            assert all(v < R for v in members)
    assert all(b > 252 for w, b in rows if any(v >= R for v in mc.word_edge_members(c, w, b)))  # only rows at the very top lose a member
    # the extreme bucket and bucket 0 of the next row at counts around the accumulate segment length
    for w in sorted({0, max(0, Wd - 2)}):
        for k in (g.S - 1, g.S, g.S + 1, 2 * g.S + 1):
            members = fam[f"occupancy[{w},{k}]"]
            d, _ = mc.recode(members[0], c, Wd)
            assert len(members) == k and len(set(members)) == 1 and d[w] == -half and d[w + 1] == 1 and sum(1 for x in d if x) == 2


def test_expected_value_routes_agree_on_the_scalars_around_r():
    """oracle.g1_msm (batched and standard), pyref.msm_naive and the device point arithmetic on the host over the geometry-independent part of `top`"""
    vals, want = mc.top_common()
    bases = mc.g1_bases()[: len(vals)]
    sc = mc.bigint(vals)
    for kind in (oracle.MSM_BATCHED, oracle.MSM_STANDARD):
        assert util.g1_affine_to_ints(oracle.g1_to_affine(oracle.g1_msm(bases, sc, kind)))[0] == want
    out = np.zeros(1, dtype=oracle.G1_PROJECTIVE)
    rc = _lib.lib().snarkvm_hip_selftest_g1_msm_naive(ctypes.c_void_p(bases.ctypes.data), ctypes.c_size_t(len(vals)), ctypes.c_size_t(bases.dtype.itemsize),
                                                      ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(out.ctypes.data))
    assert rc == 0 and util.g1_affine_to_ints(oracle.g1_to_affine(out))[0] == want
    # the Montgomery images are the same scalars
    assert np.array_equal(oracle.fr_op("to_bigint", mc.montgomery(vals)), sc)
    # and the oracle's G2 MSM over the same scalars equals the sum of its own scalar multiplications
    g2 = mc.g2_bases()[: len(vals)]
    total = None
    from oracle import pyref

    for p, s in zip(util.g2_affine_to_ints(g2), vals):
        total = pyref.g2_mul(p, s) if total is None else pyref.g2_add(total, pyref.g2_mul(p, s))
    assert util.g2_affine_to_ints(oracle.g2_to_affine(oracle.g2_msm(g2, sc, oracle.MSM_STANDARD)))[0] == total
