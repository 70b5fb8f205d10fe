"""The oracle's setup-time group operations (FixedBase::msm, group-element iFFT) pinned against Python big-int
elliptic-curve arithmetic."""
import numpy as np
import pytest

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import synthetic
from tests import util
from tests.helpers import group_cases


def test_fixed_base_msm_matches_scalar_multiplication(golden):
    g = util.g1_generator_affine()
    vals = [0, 1, 2, pyref.R_MOD - 1, (1 << 252) + 99] + [int(x) for x in synthetic.splitmix64(77, 20)]
    v = util.ints_to_fr_mont(vals)
    for window in (None, 3, 5, 8):
        got = util.g1_affine_to_ints(oracle.g1_to_affine(oracle.g1_fixed_base_msm(g, v, window=window)))
        want = [pyref.g1_mul(pyref.G1_GEN, x % pyref.R_MOD) for x in vals]
        assert got == want, window


@pytest.mark.parametrize("lg", [0, 1, 2, 4])
def test_group_ifft_matches_definition(golden, lg):
    """L_j = n^-1 sum_i omega^(-ij) P_i, and forward(inverse(P)) == P."""
    n = 1 << lg
    pts = util.srs_points_ints(golden["srs_g1"], n)
    aff = util.g1_affine_from_ints(pts)
    proj = np.zeros(n, dtype=oracle.G1_PROJECTIVE)
    proj["x"], proj["y"] = aff["x"], aff["y"]
    proj["z"] = np.array(pyref.to_limbs(pyref.fq_to_mont(1), 6), dtype=np.uint64)
    got = util.g1_affine_to_ints(oracle.g1_to_affine(oracle.g1_group_ntt(proj, inverse=True)))
    w = pyref.domain_group_gen(lg)
    winv = pow(w, pyref.R_MOD - 2, pyref.R_MOD)
    ninv = pow(n, pyref.R_MOD - 2, pyref.R_MOD)
    for j in range(n):
        acc = None
        for i in range(n):
            acc = pyref.g1_add(acc, pyref.g1_mul(pts[i], pow(winv, i * j, pyref.R_MOD) * ninv % pyref.R_MOD))
        assert got[j] == acc, j
    back = oracle.g1_group_ntt(oracle.g1_group_ntt(proj, inverse=True), inverse=False)
    assert util.g1_affine_to_ints(oracle.g1_to_affine(back)) == pts


@pytest.mark.parametrize("lg", [2, 4, 5, 6, 7])
def test_group_ntt_of_exceptional_inputs_matches_the_closed_form(lg):
    """Inputs a_i * G with equal, opposite and infinite points in chosen butterflies (tests/helpers/group_cases.py): the oracle's group
    transform is NTT(a)_j * G, in both directions, and has exactly the planned number of infinite outputs - which pins the oracle on the
    inputs the device is tested with and guards the case builder."""
    n = 1 << lg
    for name in group_cases.case_names(lg):
        proj, a, planned = group_cases.case(lg, name)
        assert proj.shape == (n,) and len(a) == n
        zero = np.array([v == 0 for v in a])
        assert np.array_equal(~proj["z"].any(axis=1), zero), name
        assert np.array_equal(oracle.g1_to_affine(proj)["infinity"] != 0, zero), name
        if zero.sum() > 1:  # both spellings of infinity are present
            general = proj["x"][zero].any(axis=1)  # (x, y, 0) against (0, 1, 0)
            assert general.any() and not general.all(), name
        for inverse in (True, False):
            want, closed = group_cases.expected(lg, name, inverse)
            assert util.affine_equal(want, closed), (name, inverse)
            assert group_cases.closed_form(a, inverse)[1] == planned, (name, inverse)
            assert group_cases.n_infinite(want) == planned, (name, inverse)
    assert group_cases.case(lg, "periodic(0)")[2] == n - 1 and group_cases.case(lg, "all_zero")[2] == n


@pytest.mark.parametrize("name", ["periodic(1)", "sparse_zeros"])
def test_group_ifft_of_an_exceptional_input_matches_definition(name):
    """The definition of test_group_ifft_matches_definition on four points of which two are equal / two are infinite."""
    lg, n = 2, 4
    proj, a, planned = group_cases.case(lg, name)
    pts = util.g1_affine_to_ints(oracle.g1_to_affine(proj))
    assert pts == [pyref.g1_mul(pyref.G1_GEN, v) for v in a]
    got = util.g1_affine_to_ints(group_cases.expected(lg, name, True)[0])
    winv = pow(pyref.domain_group_gen(lg), pyref.R_MOD - 2, pyref.R_MOD)
    ninv = pow(n, pyref.R_MOD - 2, pyref.R_MOD)
    for j in range(n):
        acc = None
        for i in range(n):
            acc = pyref.g1_add(acc, pyref.g1_mul(pts[i], pow(winv, i * j, pyref.R_MOD) * ninv % pyref.R_MOD))
        assert got[j] == acc, j
    assert got.count(None) == planned


def test_fixed_base_msm_at_the_window_edges():
    """FixedBase::msm of the scalars that sit on the edges of the device's 8-bit windows (group_cases.fixed_base_edges), for two bases: the
    oracle against Python big-int scalar multiplication; exactly the zero scalar gives infinity."""
    vals, fixed = group_cases.fixed_base_scalars()
    assert len(vals) == group_cases.FIXED_N and sorted(vals[i] for i in fixed) == sorted(group_cases.fixed_base_edges())
    assert vals[-1] == (2**256 - 1) % pyref.R_MOD and all(0 <= v < pyref.R_MOD for v in vals)
    for multiple in group_cases.FIXED_BASE_MULTIPLES:
        base, want, by_definition = group_cases.fixed_base_expected(multiple)
        assert util.g1_affine_to_ints(base) == [pyref.g1_mul(pyref.G1_GEN, multiple)]
        got = util.g1_affine_to_ints(want)
        assert sorted(by_definition) == list(fixed)
        for i, p in by_definition.items():
            assert got[i] == p, (multiple, i, hex(vals[i]))
        assert [p is None for p in got] == [v == 0 for v in vals]
