"""Cases and expected values shared by tests/test_fr_rowcheck_host.py (CPU, through the host replays) and tests/test_gpu_fr_rowcheck.py: the operands
of `snarkvm_hip_fr_witness_evals` and `snarkvm_hip_fr_rowcheck_fold`, the drivers built on them (snarkvm_amd/matrices.py: witness_poly_device,
rowcheck_witness) and what every result is compared with, bit for bit.

Expected values do not come from the library and never from the coset route the round-2 driver takes.  The fold and the counts: per-element
Python integers.  The gather: numpy indexing and `oracle.fr_vec_op("sub")`.  h_0: the reference's own route (second.rs:104-122 with
selectors.rs:88-99) restated on the C++ oracle - per instance three `oracle.ntt` inverse, `oracle.polymul` on the doubled domain, the subtraction,
`oracle.poly_divide` by X^|R| - 1 with the remainder asserted empty, the scaling by instance_combiner * circuit_combiner * |R| / |R_max| - and the
instances added up with `fr_vec_op("add")`.
"""
import ctypes

import numpy as np

from oracle import cpu as oracle
from snarkvm_amd import _lib
from tests import util
from tests.helpers import selector_cases as sel

R = sel.R
GUARD = 0xFFFFFFFFFFFFFFFF  # 0xff-filled
INVALID_VALUE = 1  # hipErrorInvalidValue
COSET_GENERATOR = 22
mont, rnd, mixed, special, pad, vanishing, trimmed_ints = sel.mont, sel.rnd, sel.mixed, sel.special, sel.pad, sel.vanishing, sel.trimmed_ints


def geometry():
    """(members per launch, members per Montgomery reduction) of the library"""
    out = np.zeros(2, dtype=np.uint32)
    assert _lib.lib().snarkvm_hip_selftest_fr_rowcheck_geometry(out.ctypes.data) == 0
    return int(out[0]), int(out[1])


CHUNK = geometry()[0]
SIZES = (1, 2, 255, 256, 257, 4097)
COUNTS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
MULTIPLIERS = [0, 1, R - 1]


# ---- members -----------------------------------------------------------------------------------------------------------------------------------
class Pool:
    """three base vectors of n + 16 mixed elements (uniform values with 0, 1, r - 1 and (r +- 1) / 2 among them), as arrays and as Python ints;
    member k reads them from the offsets (k, 3 k, 5 k) mod 16: members overlap each other and, from k = 16 on, repeat"""

    SLACK = 16

    def __init__(self, n, seed):
        self.n = n
        self.arr = [mixed(n + self.SLACK, 10 * seed + j) for j in range(3)]
        self.ints = [util.fr_mont_to_ints(v) for v in self.arr]

    def offsets(self, k):
        return (k % self.SLACK, 3 * k % self.SLACK, 5 * k % self.SLACK)

    def member(self, k):
        """-> ((a, b, c) array views of n elements, (a, b, c) int lists)"""
        offs = self.offsets(k)
        return tuple(v[o : o + self.n] for v, o in zip(self.arr, offs)), tuple(v[o : o + self.n] for v, o in zip(self.ints, offs))


def members(n, count, seed):
    """-> (a, b, c: lists of `count` array views), (ai, bi, ci: the same as int lists)"""
    pool = Pool(n, seed)
    got = [pool.member(k) for k in range(count)]
    arrays = tuple([g[0][j] for g in got] for j in range(3))
    ints = tuple([g[1][j] for g in got] for j in range(3))
    return arrays, ints


def valid_members(n, count, seed):
    """members with c = a b element by element (no violation), every vector an array of its own"""
    a = [mixed(n, 100 * seed + 2 * k) for k in range(count)]
    b = [mixed(n, 100 * seed + 2 * k + 1) for k in range(count)]
    ai, bi = [util.fr_mont_to_ints(v) for v in a], [util.fr_mont_to_ints(v) for v in b]
    ci = [[x * y % R for x, y in zip(u, v)] for u, v in zip(ai, bi)]
    return (a, b, [mont(v) for v in ci]), (ai, bi, ci)


def multipliers(count, seed):
    """(count, 4) random multipliers with 0, 1 and r - 1 in front -> (array, ints)"""
    mus = rnd(count, 500 + seed) if count else sel.ZERO.copy()
    mus[: min(count, 3)] = mont(MULTIPLIERS)[: min(count, 3)]
    return mus, util.fr_mont_to_ints(mus)


def expected_fold(ints, mus, n):
    """out[i] = sum_k mu_k (a_k[i] b_k[i] - c_k[i]) by Python integers -> (n, 4)"""
    ai, bi, ci = ints
    out = [0] * n
    for a, b, c, mu in zip(ai, bi, ci, mus):
        if mu:
            out = [(o + mu * (x * y - z)) % R for o, x, y, z in zip(out, a, b, c)]
    return mont(out) if n else sel.ZERO.copy()


def expected_violations(ints):
    ai, bi, ci = ints
    return [sum(1 for x, y, z in zip(a, b, c) if x * y % R != z) for a, b, c in zip(ai, bi, ci)]


# ---- calls -------------------------------------------------------------------------------------------------------------------------------------
def pointer_lists(arrays, n):
    """the three host arrays of member pointers of the C call (the vectors are kept alive by the caller)"""
    k = len(arrays[0])
    return [(ctypes.c_void_p * max(1, k))(*[v.ctypes.data if n else None for v in vs]) for vs in arrays]


def guarded(n, width=4):
    """n elements to be written, a 0xff-filled guard element in front and behind"""
    return np.full((n + 2, width), GUARD, dtype=np.uint64)


def unguard(buf, n):
    assert (buf[0] == GUARD).all() and (buf[n + 1] == GUARD).all(), "a guard element was written"
    return buf[1 : n + 1]


def selftest_fold(arrays, mus, n, want="ov"):
    """snarkvm_hip_selftest_fr_rowcheck_fold -> (out (n, 4), violations list); None for the outputs not wanted; every output sits between two guards"""
    k = len(arrays[0])
    pa, pb, pc = pointer_lists(arrays, n)
    out = guarded(n) if "o" in want else None
    viol = guarded(k, 1) if "v" in want else None
    mu = np.ascontiguousarray(mus, dtype=np.uint64).reshape(-1, 4) if k and mus is not None else sel.ZERO.copy()
    rcode = _lib.lib().snarkvm_hip_selftest_fr_rowcheck_fold(out[1:].ctypes.data if out is not None else None, viol[1:].ctypes.data if viol is not None else None, n, k,
                                                            pa, pb, pc, mu.ctypes.data if len(mu) else None)
    assert rcode == 0
    return (None if out is None else unguard(out, n).copy(), None if viol is None else [int(x) for x in unguard(viol, k)[:, 0]])


def expected_witness_evals(w, x_evals, input_size):
    """k -> 0 on the input subgroup, w[k - k / ratio - 1] - x_evals[k] elsewhere: the positions by numpy, the subtraction by the oracle"""
    x = np.ascontiguousarray(x_evals, dtype=np.uint64).reshape(-1, 4)
    n = x.shape[0]
    if n == 0:
        return x.copy()
    ratio = n // input_size
    k = np.arange(n)
    free = k % ratio != 0
    gathered = np.zeros((n, 4), dtype=np.uint64)
    src = (k - k // ratio - 1)[free]
    have = src < len(w)
    gathered[k[free][have]] = np.asarray(w, dtype=np.uint64).reshape(-1, 4)[src[have]]
    out = oracle.fr_vec_op("sub", gathered, x)
    out[~free] = 0
    return out


def selftest_witness(w, x_evals, input_size, in_place=False):
    x = np.ascontiguousarray(x_evals, dtype=np.uint64).reshape(-1, 4)
    w = np.ascontiguousarray(w, dtype=np.uint64).reshape(-1, 4)
    n = x.shape[0]
    buf = guarded(n)
    if in_place:
        buf[1 : n + 1] = x
    src = buf[1:] if in_place else x
    rcode = _lib.lib().snarkvm_hip_selftest_fr_witness_evals(buf[1:].ctypes.data, n, w.ctypes.data if len(w) else None, len(w), src.ctypes.data, input_size)
    assert rcode == 0
    return unguard(buf, n).copy()


# ---- the committed fixture (tests/golden/varuna_circuit0.json) ---------------------------------------------------------------------------------
def fixture_rounds12(tv):
    """rounds 1 and 2 of the Varuna test vector: the public input (1, 8, 32, 128) over the input domain of 4 elements, the private variables
    (2, 4, 2), |V| = |R| = 8, combiners one.  -> dict with the known answers as Python ints (w_lde, h_0), the three dense matrices and
    z_a, z_b, z_c = M (public ++ private) padded to 8 rows, by Python integers"""
    poly = lambda name: [int(x) for x in tv["polynomials"][name]]
    public, private = [1, 8, 32, 128], [2, 4, 2]
    assert [int(v) for v in tv["witness"][1]] == public + private
    mats = {name: [[int(v) for v in row] for row in tv["instance"][name]] for name in "ABC"}
    z = public + private
    zm = {name: [sum(v * x for v, x in zip(row, z)) % R for row in mats[name]] + [0] for name in "ABC"}
    return {"public": public, "private": private, "w_lde": poly("w_lde"), "h_0": poly("h_0"), "matrices": mats, "z": zm}


# ---- h_0 by the reference's route, on the oracle -------------------------------------------------------------------------------------------------
def reference_h0(circuits, lg_max):
    """calculate_rowcheck_witness as the reference computes it.  circuits: dicts {lg_r, circuit_combiner (int), instance_combiners (ints),
    z: per instance (z_a, z_b, z_c) arrays of 2^lg_r evaluations}.  Raises ValueError like the `ensure!` of selectors.rs:92-93 on a non-zero
    remainder.  -> (2^lg_max, 4)"""
    n_max = 1 << lg_max
    h = np.zeros((n_max, 4), dtype=np.uint64)
    for c in circuits:
        n = 1 << c["lg_r"]
        for inst, (za, zb, zc) in zip(c["instance_combiners"], c["z"]):
            pa, pb, pc = (oracle.ntt(v, direction=oracle.INVERSE) for v in (za, zb, zc))
            num = oracle.fr_vec_op("sub", oracle.polymul(c["lg_r"] + 1, [pa, pb]), pad(pc, 2 * n))
            q, rem = oracle.poly_divide(num, vanishing(n))
            if rem.shape[0]:
                raise ValueError("Failed to divide by vanishing polynomial - non-zero remainder")
            mu = mont([inst * c["circuit_combiner"] % R * n % R * pow(n_max, -1, R) % R])
            if q.shape[0]:
                h = oracle.fr_vec_op("add", h, pad(oracle.fr_vec_op("scale", q, mu), n_max))
    return h


def random_circuit(seed, lg_r, instances):
    """`instances` triples with z_c = z_a z_b on all of R (the reference divides exactly), a circuit combiner and instance combiners"""
    arrays, _ = valid_members(1 << lg_r, instances, seed)
    ints = util.fr_mont_to_ints(rnd(instances + 1, 900 + seed))
    return {"lg_r": lg_r, "circuit_combiner": ints[0], "instance_combiners": ints[1:], "z": [tuple(arrays[j][i] for j in range(3)) for i in range(instances)]}
