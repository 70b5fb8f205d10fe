"""Scalars at the ends of the signed-digit range of the variable-base MSM (snarkvm_amd/csrc/msm.hip.h, msm_sort.hip.h), shared by
tests/test_msm_digit_cases_host.py (CPU) and tests/test_gpu_msm_digit_edges.py.

Every device-side MSM recodes a scalar s < r into Wd signed digits of c bits: s' = s + bias with bias = sum_w 2^(c - 1 + c w), raw digit
u_w = (s' >> c w) & (2^c - 1), signed digit d_w = u_w - half, half = 2^(c - 1); digit d feeds bucket |d| - 1 of its row's window with the sign of d.
Bucket nb - 1 (weight half) is reached by d = -half alone, that is u = 0: a raw scalar digit of half or more that carried into the next row.
Uniformly random scalars hit it with probability 2^-c per digit; the families below put it, the buckets beside it, bucket 0 with both signs, carry
chains, empty rows and the top row's largest digit into every row of a geometry on purpose.

A geometry is named by its key (tables, registered window bits, window bits passed to the call): what RegisteredBases(tables=, window_bits=) and
msm(window_bits=) take; geometry() asks the library's own planner (host code) what that makes at a given length.

    single_digit      v << c w for every row w, v in {1, half - 1, half, half + 1, 2^c - 1}: d_w = +1, half - 1 (bucket nb - 2, positive), -half with
                      a carry (bucket nb - 1), -(half - 1) with a carry (bucket nb - 2, negative), -1 with a carry; every other row stays empty
    carry_chains      2^k - 1 (digits -1, 0, 0, ..., +1), the longest run of -half below r (raw digits half, half - 1, half - 1, ...: every row
                      carries), every raw digit half (-half, then 1 - half in every row), every raw digit half - 1, half and half - 1 alternating
                      (both phases)
    top               r - 1, r - 2, (r - 1) / 2, 2^252, 2^252 + 1, the smallest scalar with the largest reachable top-row digit (every row under the
                      top is then -half), the largest scalar whose raw digits under the top row are all 2^c - 1.  The same in every geometry
                      but for the last two
    word_edges        for every row whose c bits straddle a 32-bit word of the recoding buffer: the all-ones digit, and the single bits on
                      either side of the boundary.  Rows from bit 253 on - the word boundary at bit 256 among them - hold no scalar bits: those
                      members are not below r and are left out, like every other member that is not
    occupancy[w,k]    k copies of half << c w: bucket nb - 1 of row w and bucket 0 of row w + 1 receive k points each, k around the accumulate
                      segment length S of the plan (S - 1, S, S + 1, 2 S + 1), w = 0 and w = Wd - 2.  One MSM per (w, k)
    zeros[all], zeros[one]   the all-zero vector; one non-zero scalar among zeros
    case_list()       all of the above in one vector, with random scalars between them: the edge cases lie in the first, a middle and the last
                      256-scalar block of the digit kernels, the length is 1 mod 256 and the lone scalar of the last block is r - 1

CPU only: Python integers, numpy and the oracle; no torch."""
import collections
import ctypes
import functools
import os
import random

import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib
from tests import util

R = pyref.R_MOD

TABLELESS = tuple((1, 0, c) for c in (2, 3, 8, 11, 12, 13, 16))
LEGACY = ((16, 0, 0), (16, 0, 16), (4, 0, 0), (4, 0, 16))  # the planner's window at this length, and the 16-bit windows of the product sizes
WINDOWED = ((17, 15, 15), (19, 14, 14), (22, 12, 12), (20, 13, 13), (127, 2, 2))
WIDE = ((15, 17, 17), (15, 18, 18), (13, 20, 20), (12, 22, 22), (12, 23, 23))
GEOMETRIES = TABLELESS + LEGACY + WINDOWED + WIDE
FUSING = ((17, 15, 15), (16, 0, 16), (20, 13, 13))  # handles whose batches run as one fused multi-instance launch sequence
G2_GEOMETRIES = ((17, 15, 15), (16, 0, 0), (4, 0, 0), (15, 17, 17))

Geometry = collections.namedtuple("Geometry", "c W J Wd nb S L wide")


def table_bits(key):
    """what a registered handle stores for (tables, registered window bits)"""
    tables, reg_bits, _ = key
    return reg_bits if reg_bits else 256 // tables


def geometry(n, window_bits, tables, table_bits):
    """the library's plan for an MSM of n scalars: window bits c, bucket windows W, tables J, digit rows Wd = W J, buckets per window nb, accumulate
    segment length S, fold width L, wide (u32 digits)"""
    out = (ctypes.c_uint32 * 10)()
    rc = _lib.lib().snarkvm_hip_selftest_msm_plan(ctypes.c_size_t(n), ctypes.c_int(window_bits), ctypes.c_int(tables), ctypes.c_int(table_bits), out)
    assert rc == 0, (rc, n, window_bits, tables, table_bits)
    c, W, J, Wd, nb, _, S, _, L, wide = (int(v) for v in out)
    return Geometry(c, W, J, Wd, nb, S, L, bool(wide))


def bias(c, Wd):
    return sum(1 << (c - 1 + c * w) for w in range(Wd))


def recode(s, c, Wd):
    """-> (signed digits d_w, raw digits u_w), w < Wd.  sum_w d_w 2^(c w) == s exactly when s + bias < 2^(c Wd)."""
    sp = s + bias(c, Wd)
    u = [(sp >> (c * w)) & ((1 << c) - 1) for w in range(Wd)]
    return [v - (1 << (c - 1)) for v in u], u


def straddling_rows(c, Wd):
    """[(row, bit index of the word boundary inside it)] for the rows whose c bits lie in two 32-bit words"""
    return [(w, ((c * w + c - 1) // 32) * 32) for w in range(Wd) if (c * w) // 32 != (c * w + c - 1) // 32]


def word_edge_members(c, w, boundary):
    return [((1 << c) - 1) << (c * w), 1 << (boundary - 1), 1 << boundary]


def end_digits(c):
    """the signed digits at the ends of the range: bucket 0 with both signs, bucket nb - 2 with both signs, bucket nb - 1"""
    half = 1 << (c - 1)
    return sorted({1, -1, half - 1, -(half - 1), -half})


def digit_routes(c, w, d):
    """the two smallest scalars whose row w takes the signed digit d: the raw digit d mod 2^c alone, or one less with a carry out of a raw digit
    half in the row below (w > 0)"""
    half, m = 1 << (c - 1), 1 << c
    return [(d % m) << (c * w)] + ([(((d - 1) % m) << (c * w)) + (half << (c * (w - 1)))] if w else [])


def _below_r(vals):
    out = []
    for v in vals:
        if 0 <= v < R and v not in out:
            out.append(v)
    return out


def top_digit_max(c, Wd):
    """the largest signed digit the top row takes for a scalar below r (the raw top digit does not decrease as s grows)"""
    return recode(R - 1, c, Wd)[0][Wd - 1]


def build_families(c, Wd, S):
    """name -> list of integers below r, in a fixed order"""
    half, full, top = 1 << (c - 1), (1 << c) - 1, c * (Wd - 1)
    fam = collections.OrderedDict()
    fam["single_digit"] = _below_r(v << (c * w) for w in range(Wd) for v in (1, half - 1, half, half + 1, full))
    # where r cuts a row's raw digit short (the rows that hold its leading bits), the same signed digit by the other route: one less, and a carry from below
    fam["single_digit"] = _below_r(fam["single_digit"] + [v for w in range(Wd) for d in end_digits(c) for v in digit_routes(c, w, d)[:1 + (digit_routes(c, w, d)[0] >= R)]])
    rows = range(Wd)
    fam["carry_chains"] = _below_r([(1 << k) - 1 for k in range(1, 257)])
    # raw digits by row; the first one is the longest run of the signed digit -half below r: half in row 0 carries, half - 1 and that carry do in every row above
    for pattern in (lambda w: half - (w > 0), lambda w: half, lambda w: half - 1, lambda w: half - (w & 1), lambda w: half - 1 + (w & 1)):
        s = 0
        for w in rows:  # the longest prefix of the pattern that stays below r
            t = s + (pattern(w) << (c * w))
            if t >= R:
                break
            s = t
        fam["carry_chains"] = _below_r(fam["carry_chains"] + [s])
    s_top = ((top_digit_max(c, Wd) + half) << top) - bias(c, Wd)  # s + bias = u_top 2^top: every raw digit under the top is 0
    ones_below = ((R >> top) << top) - 1                             # t 2^top + (2^top - 1) with the largest t that keeps it below r
    fam["top"] = _below_r([R - 1, R - 2, (R - 1) // 2, 1 << 252, (1 << 252) + 1, s_top, ones_below])
    fam["word_edges"] = _below_r(v for w, b in straddling_rows(c, Wd) for v in word_edge_members(c, w, b))
    for w in sorted({0, max(0, Wd - 2)}):
        for k in (S - 1, S, S + 1, 2 * S + 1):
            if (half << (c * w)) < R:
                fam[f"occupancy[{w},{k}]"] = [half << (c * w)] * k
    rng = random.Random(f"msm_digit_cases zeros {c} {Wd}")
    fam["zeros[all]"] = [0] * 65
    fam["zeros[one]"] = [0] * 40 + [rng.randrange(1, R)] + [0] * 24
    return fam


def _plan_for(key, n):
    tables, _, call_bits = key
    return geometry(n, call_bits, tables, table_bits(key))


@functools.lru_cache(maxsize=None)
def cases(key):
    """-> (Geometry at the case list's length, families: name -> tuple of integers, the case list, {name: the positions of its members in the list})"""
    n = 1024
    for _ in range(4):  # the families depend on the plan (c, Wd, S), the plan on the length of the list they make
        g0 = _plan_for(key, n)
        fam = build_families(g0.c, g0.Wd, g0.S)
        vals, where = _lay_out(fam, f"msm_digit_cases fill {key}")
        n = len(vals)
        if _plan_for(key, n) == g0:
            return g0, collections.OrderedDict((k, tuple(v)) for k, v in fam.items()), tuple(vals), where
    raise AssertionError(f"{key}: the plan does not settle at the case list's own length")


def _lay_out(fam, seed):
    """edges | random | edges | random | edges | r - 1, the last one alone in its 256-scalar block"""
    rng = random.Random(seed)
    edges, spans = [], []
    for name, vals in fam.items():
        spans.append((name, len(edges), len(edges) + len(vals)))
        edges += vals
    third = (len(edges) + 2) // 3
    blocks = (len(edges) + 2 * 96 + 255) // 256  # at least 96 random scalars in each gap
    fill = 256 * blocks - len(edges)
    cut = (third, 2 * third)
    gaps = (fill // 2, fill - fill // 2)
    out, shift = [], []
    for i, v in enumerate(edges):
        for j in (0, 1):
            if i == cut[j]:
                out += [rng.randrange(1, R) for _ in range(gaps[j])]
        shift.append(len(out))
        out.append(v)
    out.append(R - 1)
    assert len(out) % 256 == 1 and len(out) % 64 and (len(out) - 1) // 256 >= 2
    where = {name: tuple(shift[lo:hi]) for name, lo, hi in spans}
    return out, where


# ---- memory images ----------------------------------------------------------------------------------------------------------------------------
def bigint(vals):
    """(n, 4) u64 canonical integers (`Fr::to_bigint`)"""
    return np.array([pyref.to_limbs(v, 4) for v in vals], dtype=np.uint64).reshape(-1, 4)


def montgomery(vals):
    """(n, 4) u64 Fr memory images"""
    return oracle.fr_op("from_bigint", bigint(vals)) if len(vals) else bigint(vals)


def _frozen(arr):
    arr.setflags(write=False)
    return arr


# ---- bases and expected sums ------------------------------------------------------------------------------------------------------------------
N_BASES = 2048  # more than the longest case list plus the offsets the tests use


@functools.lru_cache(maxsize=None)
def _srs_ints():
    with open(os.path.join(util.ROOT, "tests", "golden", "srs_g1_32768.bin"), "rb") as f:
        return tuple(util.srs_points_ints(f.read(96 * N_BASES)))


@functools.lru_cache(maxsize=None)
def g1_bases():
    """the first 2 048 points of the SRS fixture: distinct points, so that one dropped or mis-weighted contribution changes the sum"""
    return _frozen(util.g1_affine_from_ints(list(_srs_ints())))


@functools.lru_cache(maxsize=None)
def g2_bases(distinct=None):
    """2 048 G2 points: all different, or `distinct` points tiled (equal points in one bucket: the equal-x fix kernels)"""
    from snarkvm_amd import synthetic

    return _frozen(synthetic.g2_points(N_BASES, distinct=N_BASES if distinct is None else distinct))


def g1_expected(vals, offset=0, bases=None):
    """the oracle's batched::msm of vals over bases[offset:] (default: the fixture's), affine"""
    bases = g1_bases()[offset : offset + len(vals)] if bases is None else bases
    assert len(bases) == len(vals)
    return oracle.g1_to_affine(oracle.g1_msm(bases, bigint(vals), oracle.MSM_BATCHED))


def g2_expected(vals, offset=0, distinct=None):
    bases = g2_bases(distinct)[offset : offset + len(vals)]
    assert len(bases) == len(vals)
    return oracle.g2_to_affine(oracle.g2_msm(bases, bigint(vals), oracle.MSM_STANDARD))


@functools.lru_cache(maxsize=None)
def top_common():
    """the members of `top` that every geometry shares, and their sum over the first bases by pyref's double-and-add (Python integers), computed once"""
    vals = (R - 1, R - 2, (R - 1) // 2, 1 << 252, (1 << 252) + 1)
    return vals, pyref.msm_naive(list(_srs_ints()[: len(vals)]), list(vals))
