"""Fr NTT on 2^27 and 2^28 domains, checked on the CPU: the pass plan, the twiddle and coset-power composition and the index maps of
snarkvm_amd/csrc/ntt.hip.h run on the host through the kernels' own __host__ __device__ code (snarkvm_hip_selftest_ntt_*).  No GPU needed."""
import ctypes
import random

import numpy as np
import pytest

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib, synthetic

W28 = pow(pyref.FR_TWO_ADIC_ROOT, 1 << (pyref.FR_TWO_ADICITY - 28), pyref.R_MOD)
G = pyref.FR_GENERATOR

# the plans the backend used for every size it supported before 2^27: they must not change
PLANS_UP_TO_26 = {
    0: [0], 1: [1], 2: [2], 3: [3], 4: [4], 5: [5], 6: [6], 7: [7], 8: [8], 9: [4, 5], 10: [5, 5], 11: [5, 6], 12: [6, 6], 13: [6, 7], 14: [7, 7],
    15: [7, 8], 16: [8, 8], 17: [5, 6, 6], 18: [6, 6, 6], 19: [6, 6, 7], 20: [6, 7, 7], 21: [7, 7, 7], 22: [7, 7, 8], 23: [7, 8, 8], 24: [8, 8, 8],
    25: [8, 8, 9], 26: [8, 9, 9],
}


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def plan(lg):
    out = (ctypes.c_int32 * 4)()
    npass = _lib.lib().snarkvm_hip_selftest_ntt_plan(ctypes.c_uint32(lg), out)
    return None if npass < 0 else list(out)[:npass]


def twiddles(kind, xs, lg=0, pass_=-1, inverse=0):
    x = np.asarray(xs, dtype=np.uint64)
    out = np.zeros((len(x), 4), dtype=np.uint64)
    rc = _lib.lib().snarkvm_hip_selftest_ntt_twiddle(ctypes.c_int(kind), ctypes.c_uint32(lg), ctypes.c_int(pass_), ctypes.c_int(inverse), _p(x),
                                                     ctypes.c_size_t(len(x)), _p(out))
    assert rc == 0
    return [pyref.from_limbs(r) for r in out]


def index_violations(lg, forced=None):
    if forced is None:
        return _lib.lib().snarkvm_hip_selftest_ntt_index(ctypes.c_uint32(lg), None, ctypes.c_int(0))
    arr = (ctypes.c_int32 * len(forced))(*forced)
    return _lib.lib().snarkvm_hip_selftest_ntt_index(ctypes.c_uint32(lg), arr, ctypes.c_int(len(forced)))


def host_transform(x, lg, direction, kind, forced=None):
    y = np.array(x, dtype=np.uint64, copy=True).reshape(-1, 4)
    arr = None if forced is None else (ctypes.c_int32 * len(forced))(*forced)
    rc = _lib.lib().snarkvm_hip_selftest_ntt_host(_p(y), ctypes.c_uint32(lg), arr, ctypes.c_int(0 if forced is None else len(forced)),
                                                  ctypes.c_int(direction), ctypes.c_int(kind))
    assert rc == 0
    return y


def _exponents(limit, seed):
    """both sides of 2^13, 2^26 and 2^27 (those below `limit`), the maximum, and a few hundred random values"""
    edges = {0, 1, 2, 3, 4, limit - 1, limit - 2}
    for b in (13, 15, 26, 27):
        for d in (-2, -1, 0, 1, 2):
            e = (1 << b) + d
            if 0 <= e < limit:
                edges.add(e)
    rng = random.Random(seed)
    return sorted(edges) + [rng.randrange(limit) for _ in range(300)]


def test_plans_up_to_2_26_are_unchanged():
    for lg, want in PLANS_UP_TO_26.items():
        assert plan(lg) == want, lg


def test_plans_of_2_27_and_2_28():
    assert plan(27) == [9, 9, 9]
    p28 = plan(28)
    assert len(p28) == 4 and all(1 <= a <= 8 for a in p28)
    for lg in range(29):
        assert sum(plan(lg)) == lg
    assert plan(29) is None
    assert plan(64) is None


@pytest.mark.parametrize("inverse", [0, 1])
def test_composed_twiddles_are_powers_of_the_2_28th_root(inverse):
    """W28^e from lo / hi / top tables for every exponent class, against Python powers of TWO_ADIC_ROOT^(2^19)"""
    w = pow(W28, -1, pyref.R_MOD) if inverse else W28
    assert pow(W28, 1 << 27, pyref.R_MOD) == pyref.R_MOD - 1  # primitive
    es = _exponents(1 << 28, 7 + inverse)
    got = twiddles(0, es, inverse=inverse)
    for e, v in zip(es, got):
        assert v == pyref.fr_to_mont(pow(w, e, pyref.R_MOD)), e


@pytest.mark.parametrize("inverse", [0, 1])
def test_composed_coset_powers(inverse):
    g = pow(G, -1, pyref.R_MOD) if inverse else G
    js = _exponents(1 << 28, 11 + inverse)
    got = twiddles(1, js, inverse=inverse)
    for j, v in zip(js, got):
        assert v == pyref.fr_to_mont(pow(g, j, pyref.R_MOD)), j


@pytest.mark.parametrize("lg", [24, 26, 27, 28])
def test_pass_twiddles_are_roots_of_the_pass_block(lg):
    """pass k multiplies by w_(2^(a + s))^(inner * k), with 2^(a + s) the block the pass works in"""
    pl = plan(lg)
    consumed = 0
    for k in range(len(pl) - 1):
        block = lg - consumed
        for inverse in (0, 1):
            root = pow(pyref.FR_TWO_ADIC_ROOT, 1 << (pyref.FR_TWO_ADICITY - block), pyref.R_MOD)
            if inverse:
                root = pow(root, -1, pyref.R_MOD)
            xs = _exponents(1 << block, 100 * lg + 10 * k + inverse)[:120]
            got = twiddles(0, xs, lg=lg, pass_=k, inverse=inverse)
            for x, v in zip(xs, got):
                assert v == pyref.fr_to_mont(pow(root, x, pyref.R_MOD)), (lg, k, x)
        consumed += pl[k]


@pytest.mark.parametrize("lg", [27, 28])
def test_index_maps_of_large_plans(lg):
    """every pass reads and writes each position once; the last pass writes coefficient f at index f (NN order)"""
    assert index_violations(lg) == 0


def test_index_maps_of_every_smaller_plan():
    for lg in range(0, 25):
        assert index_violations(lg) == 0, lg
    assert index_violations(26) == 0


@pytest.mark.parametrize("forced", [[3, 3, 3, 3], [2, 4, 3, 3], [4, 2, 2, 4], [4, 4, 4], [6, 6]])
def test_index_maps_of_forced_plans(forced):
    assert index_violations(sum(forced), forced) == 0


def test_bad_plans_are_rejected():
    assert index_violations(29) == -1
    assert index_violations(12, [3, 3, 3]) == -1  # does not sum to lg
    assert index_violations(12, [12]) == -1  # radix above 2^9
    assert index_violations(10, [2, 2, 2, 2, 2]) == -1  # five passes


def _vector(lg, seed):
    return oracle.fr_op("from_bigint", synthetic.random_fr_integers(1 << lg, seed))


@pytest.mark.parametrize("direction,kind", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_forced_four_pass_transform_matches_oracle(direction, kind):
    """the whole 2^12 transform as four radix-8 passes, computed on the host over the kernels' addressing and tables"""
    x = _vector(12, 0x4A55 + 2 * direction + kind)
    want = oracle.ntt(x, oracle.ORDER_NN, direction, kind)
    assert np.array_equal(host_transform(x, 12, direction, kind, [3, 3, 3, 3]), want)
    assert np.array_equal(host_transform(x, 12, direction, kind, [2, 4, 3, 3]), want)


@pytest.mark.parametrize("lg", [0, 1, 5, 9, 13, 14])
def test_default_plan_transform_matches_oracle(lg):
    x = _vector(lg, 0x4A60 + lg)
    for direction, kind in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert np.array_equal(host_transform(x, lg, direction, kind), oracle.ntt(x, oracle.ORDER_NN, direction, kind)), (lg, direction, kind)
