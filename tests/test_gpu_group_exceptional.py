"""The setup-time group operations on the device (snarkvm_amd/csrc/group.hip.h) on the inputs where elliptic-curve kernels go wrong: equal
points, opposite points and the point at infinity in chosen butterflies of the group NTT, and FixedBase::msm scalars on the edges of the
device's windows.  Every input is a_i * G for chosen integers a_i (tests/helpers/group_cases.py), so every result has a closed form next to
the oracle's; tests/test_oracle_group.py checks the two against each other without a GPU.  All comparisons are exact, after to_affine."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import group
from tests import util
from tests.helpers import group_cases

pytestmark = pytest.mark.gpu


def _check(got_proj, lg, name, inverse):
    _, _, planned = group_cases.case(lg, name)
    want, closed = group_cases.expected(lg, name, inverse)
    got = oracle.g1_to_affine(got_proj)
    where = (lg, name, "inverse" if inverse else "forward")
    assert util.affine_equal(got, want), where
    assert util.affine_equal(got, closed), where
    assert group_cases.n_infinite(got) == planned == group_cases.n_infinite(closed), where


@pytest.mark.parametrize("lg", [1, 2, 4, 5, 6, 7])
def test_group_ntt_exceptional_inputs(lg):
    """n <= 16: one lane per butterfly; n = 32: exactly one wave of four-lane butterflies; n = 64: two waves, in separate blocks; n = 128:
    several blocks.  A wave with an equal or opposite pair in any of its 16 butterflies leaves the four-lane schedule for the plain addition law
    (quad_add, msm.hip.h); periodic(k) puts such pairs into every butterfly of the first lg - k stages and infinity into everything below,
    one_pair / one_pair_stage2 into one butterfly of one wave at stage 1 / 2."""
    for name in group_cases.case_names(lg):
        proj, _, _ = group_cases.case(lg, name)
        for inverse in (True, False):
            got = group.group_ntt(proj, inverse=inverse)
            _check(got, lg, name, inverse)
            if inverse:
                back = group.group_ntt(got, inverse=False)
                assert util.affine_equal(oracle.g1_to_affine(back), oracle.g1_to_affine(proj)), (lg, name, "round trip")


def test_group_ntt_mixed_waves_repeat():
    """n = 64: one wave on the plain law next to one on the four-lane schedule (one_pair), and both waves on the plain law at stages 1 - 3 and
    on infinities after (periodic(3)); four launches in one process give the identical, oracle-equal vector."""
    lg = 6
    for name in ("one_pair", "periodic(3)"):
        proj, _, _ = group_cases.case(lg, name)
        first = None
        for launch in range(4):
            got = group.group_ntt(proj, inverse=True)
            _check(got, lg, name, True)
            first = got if first is None else first
            assert got.tobytes() == first.tobytes(), (name, launch)


def test_group_ntt_one_lane_kernels_on_exceptional_inputs(tmp_path):
    """g1_ntt_stage_kernel / g1_scale_kernel (tuning group_quad=0, a child process) on the n = 64 cases - two waves of one-lane butterflies -
    in both directions: the same group elements as the oracle."""
    lg = 6
    n = 1 << lg
    names = group_cases.case_names(lg)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); from snarkvm_amd import group; from snarkvm_amd.layout import G1_PROJECTIVE; "
            "p = np.fromfile(sys.argv[1], dtype=G1_PROJECTIVE).reshape(-1, %d); "
            "np.concatenate([group.group_ntt(c, inverse=inv) for inv in (True, False) for c in p]).tofile(sys.argv[2])" % (util.ROOT, n))
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([group_cases.case(lg, name)[0] for name in names]).tofile(src)
    r = subprocess.run([sys.executable, "-c", code, src, dst], env=dict(os.environ, SNARKVM_HIP_TUNING="group_quad=0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.fromfile(dst, dtype=oracle.G1_PROJECTIVE).reshape(2, len(names), n)
    for d, inverse in enumerate((True, False)):
        for k, name in enumerate(names):
            _check(out[d, k], lg, name, inverse)


@pytest.mark.parametrize("n", [32, 64])
def test_lagrange_basis_with_infinite_powers(golden, n):
    """UniversalParams::lagrange_basis of affine powers of which the tail and one interior record are flagged infinite - their coordinates left
    in place - equals the oracle's group iFFT with Projective::zero() at those positions (what domain.ifft pads a shorter vector with)."""
    powers = util.g1_affine_from_ints(util.srs_points_ints(golden["srs_g1"], n))
    assert powers.shape[0] == n and not powers["infinity"].any()
    flagged = [5] + list(range(n // 2 + 3, n))
    proj = group_cases.to_projective(powers)
    proj["x"][flagged], proj["y"][flagged], proj["z"][flagged] = 0, group_cases.FQ_ONE, 0
    powers["infinity"][flagged] = 1
    assert powers["x"][flagged].any(axis=1).all() and powers["y"][flagged].any(axis=1).all()
    got = group.lagrange_basis(powers)
    assert util.affine_equal(got, oracle.g1_to_affine(oracle.g1_group_ntt(proj, inverse=True)))


def test_fixed_base_msm_digit_edges():
    """g1_fixed_msm_kernel's digits: 257 scalars (one thread in a second block) with a single digit 1 and a single digit 255 in every window,
    window 31 alone (bits 248 .., read across the last word), the values around r, 0, 1 and random fill, for the bases G and 123456789 G,
    against the oracle's FixedBase::msm and, for the chosen scalars, Python big-int scalar multiplication."""
    vals, _ = group_cases.fixed_base_scalars()
    v = util.ints_to_fr_mont(vals)
    window = group.FixedBase.get_mul_window_size(len(vals))
    for multiple in group_cases.FIXED_BASE_MULTIPLES:
        base, want, by_definition = group_cases.fixed_base_expected(multiple)
        got = oracle.g1_to_affine(group.FixedBase.msm(253, window, group.FixedBase.get_window_table(253, window, base), v))
        assert util.affine_equal(got, want), multiple
        ints = util.g1_affine_to_ints(got)
        for i, p in by_definition.items():
            assert ints[i] == p, (multiple, i, hex(vals[i]))
        assert [bool(f) for f in got["infinity"]] == [x == 0 for x in vals], multiple
