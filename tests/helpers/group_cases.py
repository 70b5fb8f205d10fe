"""Exceptional inputs of the setup-time group operations (snarkvm_amd/csrc/group.hip.h), shared by tests/test_oracle_group.py (CPU)
and tests/test_gpu_group_exceptional.py, with a closed form for every expected value.

With P_i = a_i * G the group (i)NTT of P is NTT(a)_j * G, so a case is a list of integers a_i mod r chosen to put equal points, opposite points
and the point at infinity into chosen butterflies.  The device runs decimation in frequency: stage 1 pairs (i, i + n/2), stage 2 (i, i + n/4)
inside each half, and so on; a butterfly is s = a + b, d = (a - b) * twiddle.

    periodic(k)      a_i = a_(i mod 2^k): a == b in every butterfly of stages 1 .. lg - k (s = 2a, d = infinity), then infinity +- infinity and
                     twiddle * infinity in the emptied half, generic stages after.  n - 2^k outputs are infinite; k = 0 is the constant vector
    halves_neg       a_(i + n/2) = -a_i: s = infinity, d = 2a in every butterfly of stage 1, then a full multiplication of the doubled point
    one_pair         random, a_(1 + n/2) = a_1: one doubling among the 16 butterflies of a wave
    one_pair_stage2  random, a_(j + 3n/4) = a_j + a_(j + n/2) - a_(j + n/4): the only equal pair appears at stage 2
                     (at n = 4 that is the last stage and its d = infinity is an output)
    sparse_zeros     every third a_i = 0: infinity + Q, P + infinity, P - infinity
    zero_tail        a_i = 0 from n/2 + 3 on: what domain.ifft makes of a powers vector shorter than the domain
    one_nonzero, all_zero

CPU only: numpy and the oracle, no torch."""
import functools
import random

import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from tests import util

R = pyref.R_MOD
FQ_ONE = util.limbs(pyref.fq_to_mont(1), 6)


def _fq_mont(vals):
    return np.array([pyref.to_limbs(pyref.fq_to_mont(v % pyref.Q_MOD), 6) for v in vals], dtype=np.uint64).reshape(-1, 6)


def to_projective(aff):
    """finite affine records with Z = 1"""
    proj = np.zeros(aff.shape[0], dtype=oracle.G1_PROJECTIVE)
    proj["x"], proj["y"] = aff["x"], aff["y"]
    proj["z"] = FQ_ONE
    return proj


def points(a):
    """[a_i * G] as the reference's Jacobian records, un-normalised: the Z that the oracle's double-and-add leaves, times i + 1 (so that equal
    a_i at different indices are different triples of the same point).  a_i = 0 is alternately Projective::zero() = (0, 1, 0) and (x, y, 0)
    with non-zero x, y."""
    g = util.g1_generator_affine()
    proj = np.zeros(len(a), dtype=oracle.G1_PROJECTIVE)
    for i, v in enumerate(a):
        if v % R:
            proj[i] = oracle.g1_mul(g, util.limbs(v % R, 4))[0]
    lam = _fq_mont([i + 1 for i in range(len(a))])
    lam2 = oracle.fq_op("sqr", lam)
    proj["x"] = oracle.fq_op("mul", proj["x"], lam2)
    proj["y"] = oracle.fq_op("mul", proj["y"], oracle.fq_op("mul", lam2, lam))
    proj["z"] = oracle.fq_op("mul", proj["z"], lam)
    for count, i in enumerate(i for i, v in enumerate(a) if v % R == 0):
        if count % 2 == 0:
            proj[i]["x"], proj[i]["y"] = 0, FQ_ONE
        else:
            proj[i]["x"], proj[i]["y"] = _fq_mont([0xA11CE + 7 * i])[0], _fq_mont([pyref.Q_MOD - 3 - i])[0]
        proj[i]["z"] = 0
    return proj


def closed_form(a, inverse):
    """NTT(a)_j * G through the oracle's Fr transform (natural order in and out, standard domain) -> (G1_PROJECTIVE records, number of
    infinite ones)"""
    out = oracle.ntt(util.ints_to_fr_mont(a), oracle.ORDER_NN, oracle.INVERSE if inverse else oracle.FORWARD, oracle.STANDARD)
    k = oracle.fr_op("to_bigint", out)
    g = util.g1_generator_affine()
    return np.concatenate([oracle.g1_mul(g, row) for row in k]), int((~k.any(axis=1)).sum())


def case_names(lg):
    n = 1 << lg
    names = [f"periodic({k})" for k in range(lg)] + ["halves_neg"]
    if n >= 4:
        names += ["one_pair", "one_pair_stage2"]
    names.append("sparse_zeros")
    if n >= 8:
        names.append("zero_tail")
    return names + ["one_nonzero", "all_zero"]


def scalars(lg, name):
    """-> (the integers a_i, the planned number of infinite outputs - the same in both directions, for generic random values)"""
    n = 1 << lg
    rng = random.Random(f"group_cases {lg} {name}")
    a = [rng.randrange(1, R) for _ in range(n)]
    if name.startswith("periodic("):
        k = int(name[9:-1])
        return [a[i % (1 << k)] for i in range(n)], n - (1 << k)  # only the multiples of n / 2^k survive
    if name == "halves_neg":
        return a[: n // 2] + [R - v for v in a[: n // 2]], n // 2  # every even output vanishes
    if name == "one_pair":
        a[1 + n // 2] = a[1]
        return a, 0
    if name == "one_pair_stage2":
        j = 1 if n >= 8 else 0
        a[j + 3 * n // 4] = (a[j] + a[j + n // 2] - a[j + n // 4]) % R
        return a, 1 if n == 4 else 0  # at n = 4 stage 2 is the last one: its d = infinity is output 2 = a_0 - a_1 + a_2 - a_3
    if name == "sparse_zeros":
        return [0 if i % 3 == 0 else v for i, v in enumerate(a)], 0
    if name == "zero_tail":
        return [v if i < n // 2 + 3 else 0 for i, v in enumerate(a)], 0
    if name == "one_nonzero":
        return [a[i] if i == 1 else 0 for i in range(n)], 0
    if name == "all_zero":
        return [0] * n, n
    raise KeyError(name)


def _frozen(arr):
    arr.setflags(write=False)
    return arr


@functools.lru_cache(maxsize=None)
def case(lg, name):
    """-> (G1_PROJECTIVE input, the integers, the planned number of infinite outputs); computed once, read-only"""
    a, planned = scalars(lg, name)
    return _frozen(points(a)), tuple(a), planned


@functools.lru_cache(maxsize=None)
def expected(lg, name, inverse):
    """-> (the oracle's group transform of the case, its closed form), both affine; computed once, read-only"""
    proj, a, _ = case(lg, name)
    want = oracle.g1_to_affine(oracle.g1_group_ntt(proj, inverse=inverse))
    closed, _ = closed_form(a, inverse)
    return _frozen(want), _frozen(oracle.g1_to_affine(closed))


def n_infinite(aff):
    return int(np.count_nonzero(aff["infinity"]))


# ---- FixedBase::msm: the scalars at the edges of the device's 8-bit windows ----------------------------------------------------------------------
FIXED_N = 257  # 256 + 1: one thread in a second block
FIXED_BASE_MULTIPLES = (1, 123456789)


def fixed_base_edges():
    """Scalars chosen for g1_fixed_msm_kernel's digit extraction (32 windows of 8 bits, window 31 = bits 248 ..): a single digit 1 and a single
    digit 255 in every window, only the top window set, the values around r, 0 and 1, every digit below the top 255."""
    vals = [1 << (8 * j) for j in range(32)] + [255 << (8 * j) for j in range(31)]
    vals += [1 << 252, (1 << 248) + 1, R - 1, R - 2, (R - 1) // 2, 0, 1, (1 << 248) - 1, ((1 << 256) - 1) % R]
    return vals


@functools.lru_cache(maxsize=None)
def fixed_base_scalars():
    """-> (257 integers, the indices of the non-random ones): the edges around a random middle, so that the lone thread of the second block holds one"""
    edges = fixed_base_edges()
    rng = random.Random("group_cases fixed base")
    fill = [rng.randrange(1, R) for _ in range(FIXED_N - len(edges))]
    vals = edges[:40] + fill + edges[40:]
    return tuple(vals), tuple(list(range(40)) + list(range(40 + len(fill), FIXED_N)))


@functools.lru_cache(maxsize=None)
def fixed_base_expected(multiple):
    """For the base multiple * G -> (the base, affine; the oracle's FixedBase::msm of the 257 scalars, affine; {index: pyref.g1_mul} for the non-random
    scalars)"""
    vals, fixed = fixed_base_scalars()
    base = oracle.g1_to_affine(oracle.g1_mul(util.g1_generator_affine(), util.limbs(multiple, 4)))
    want = oracle.g1_to_affine(oracle.g1_fixed_base_msm(base, util.ints_to_fr_mont(vals)))
    base_ints = util.g1_affine_to_ints(base)[0]
    return _frozen(base), _frozen(want), {i: pyref.g1_mul(base_ints, vals[i]) for i in fixed}
