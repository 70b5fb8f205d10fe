"""The MSMs that put the walk of the accumulate kernels (snarkvm_amd/csrc/msm_sort.hip.h) on the ends of segments and buckets, for either curve; shared by
tests/test_gpu_accumulate_segments.py (G1), tests/test_gpu_accumulate_segments_g2.py and tests/test_accumulate_segment_cases_host.py (the CPU model of the
walk that shows which ends the cases reach).

A case is a base vector and the names of the scalar patterns that run over it.  Beside the memory image every base carries its description - (multiple of
the generator, negated) or None for the point at infinity - which is what the CPU model works on.

    sizes        1, 2, 3, 127, 128, 129, 257: digit entries on, one below and one above multiples of 2 and 3
    geometries   17 tables of 15-bit windows, and one table (the planner's window at that length)
    bases        distinct       (i + 1) G
                 runs           P, P, -P, -P, P, Q, Q, -Q, ...: with equal scalars a bucket meets a doubling, an ordinary addition, a cancellation, a restart
                 inf_<pick>     distinct, with the point at infinity at first / last / every third from 0 / every third from 2 / the odd positions / everywhere
                 cancel_restart (G2) P, -P, Q, P', -P', Q', ...: the accumulator returns to infinity inside a bucket and the next entry restarts it; where a
                                bucket ends on P, -P (n = 2; n = 128 in index order, which the device does not keep for rows of 8 k digits) it is flushed
                                at infinity
    scalars      equal          one value: few buckets per digit row, so segments start inside a bucket that an earlier thread began (part_off > 0)
                 distinct_small 1 .. n: every bucket of the low window holds one entry - a flush in every iteration there
                 gappy          few digit values far apart: long runs of empty buckets between the occupied ones
                 zero, zero_mixed, uniform
    batch (G2)   one msm_batch call over the cancel_restart bases: six instances that share one fused launch sequence (the instance id is the top sort
                 key, so segments cross instance boundaries; the instance whose scalars are all zero is a run of 2^14 empty buckets), and an empty
                 instance, which the library answers without a launch

Building the cases needs no device: Python integers, numpy and the oracle.  run() is what a test's child process calls, on the device."""
import collections

import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from tests import util

SIZES = (1, 2, 3, 127, 128, 129, 257)  # x 17 windows / x the planner's: digit entries on, one below and one above multiples of 2 and 3
NMAX = max(SIZES)
GEOMETRIES = (dict(tables=17, window_bits=15), dict(tables=1))
INF_PICKS = ("first", "last", "thirds", "thirds2", "odd", "all")
BATCH_GEOMETRY = dict(tables=17, window_bits=15)
# (size, offset into the cancel_restart bases - a multiple of 3, so that every instance starts on a P -, scalar pattern)
# The all-zero instance follows 17 entries: neither a segment of 2 nor one of 3 ends there, so one of them steps over its empty window.
BATCH = ((1, 6, "uniform"), (0, 9, "zero"), (3, 252, "zero"), (129, 126, "gappy"), (2, 99, "equal"), (257, 0, "uniform"), (128, 129, "equal"))

Case = collections.namedtuple("Case", "tag bases desc names")  # desc[i]: (multiple of the generator, negated) | None
CaseSet = collections.namedtuple("CaseSet", "curve scalars scalar_ints cases batch")


def digits_scalar(ds, bits=15):
    """the scalar whose 15-bit windows are ds (low to high), below 2^253"""
    return sum(d << (bits * w) for w, d in enumerate(ds)) % (1 << 252)


def scalar_ints():
    """name -> NMAX integers below r"""
    rng = np.random.default_rng(0xACC)
    return collections.OrderedDict([
        # one bucket per digit row: segments start inside a bucket that an earlier thread began (part_off > 0)
        ("equal", [digits_scalar([5, 16383, 1, 9000] * 5)] * NMAX),
        # every bucket of the low window holds one entry: a flush in every iteration there
        ("distinct_small", list(range(1, NMAX + 1))),
        # few digit values far apart: long runs of empty buckets between the occupied ones
        ("gappy", [digits_scalar([(1, 7000, 16383, 2)[(i + w) % 4] for w in range(17)]) for i in range(NMAX)]),
        ("zero", [0] * NMAX),
        ("zero_mixed", [0 if i % 3 else 12345 + i for i in range(NMAX)]),
        ("uniform", [int.from_bytes(rng.bytes(32), "little") % pyref.R_MOD for _ in range(NMAX)]),
    ])


def _negated(p, curve):
    q = p.copy()
    if curve == "g1":
        q["y"] = pyref.to_limbs((pyref.Q_MOD - pyref.from_limbs(p["y"])) % pyref.Q_MOD, 6)  # Montgomery form of -y
    else:  # both components of y
        y = [int(v) for v in p["y"]]
        q["y"] = sum((pyref.to_limbs((pyref.Q_MOD - pyref.from_limbs(y[6 * k : 6 * k + 6])) % pyref.Q_MOD, 6) for k in (0, 1)), [])
    return q


def _distinct(curve):
    """(i + 1) G, i < NMAX"""
    if curve == "g1":
        return oracle.g1_gen_bases(util.g1_generator_affine(), 1, NMAX)
    from snarkvm_amd import synthetic

    return synthetic.g2_points(NMAX, distinct=NMAX).view(oracle.G2_AFFINE)


def infinity(curve):
    return (util.g1_affine_from_ints if curve == "g1" else util.g2_affine_from_ints)([None])[0]


def _pick(pick, n):
    return {"first": [0], "last": [n - 1], "thirds": range(0, n, 3), "thirds2": range(2, n, 3), "odd": range(1, n, 2), "all": range(n)}[pick]


def case_set(curve):
    """every case of one curve ("g1" | "g2"), in the order the device runs them"""
    assert curve in ("g1", "g2")
    ints = scalar_ints()
    scalars = collections.OrderedDict((k, util.ints_to_fr(v)) for k, v in ints.items())
    distinct = _distinct(curve)
    d_desc = [(i + 1, False) for i in range(NMAX)]
    # P, P, -P, -P, P, Q, Q, -Q, ...: with equal scalars a bucket meets a doubling, an ordinary addition, a cancellation, a restart
    runs, r_desc = distinct.copy(), []
    for i in range(NMAX):
        p = distinct[i // 5]
        runs[i] = _negated(p, curve) if i % 5 in (2, 3) else p
        r_desc.append((i // 5 + 1, i % 5 in (2, 3)))
    # P, -P, Q with fresh points in every triple
    cancel, c_desc = distinct.copy(), []
    for i in range(NMAX):
        m = 2 * (i // 3) + (i % 3 == 2)
        cancel[i] = _negated(distinct[m], curve) if i % 3 == 1 else distinct[m]
        c_desc.append((m + 1, i % 3 == 1))
    inf = infinity(curve)
    cases = []
    for n in SIZES:
        cases.append(Case("distinct", distinct[:n], d_desc[:n], list(scalars)))
        # P directly followed by P and by -P: the exceptional addition right after the prefetch rotates
        cases.append(Case("runs", runs[:n], r_desc[:n], ["equal", "uniform"]))
        # a base at infinity in the first / the last sorted position of a segment: with equal scalars the entries of a bucket that come from one digit row
        # stand in index order
        for pick in INF_PICKS:
            b, desc = distinct[:n].copy(), d_desc[:n]
            for i in _pick(pick, n):
                b[i] = inf
                desc[i] = None
            cases.append(Case("inf_" + pick, b, desc, ["equal", "uniform"]))
        if curve == "g2":
            cases.append(Case("cancel_restart", cancel[:n], c_desc[:n], ["equal"]))
    batch = Case("batch", cancel, c_desc, [name for _, _, name in BATCH]) if curve == "g2" else None
    return CaseSet(curve, scalars, ints, cases, batch)


def case_count(cs):
    """what run() counts: one per (case, scalar pattern) - each over both geometries - and one per instance of the batch"""
    return sum(len(c.names) for c in cs.cases) + (len(BATCH) if cs.batch else 0)


def run(curve):
    """Every case of the curve on the device against the oracle's MSM (G1: batched::msm, G2: standard::msm), compared by the bytes of the affine results;
    returns the count.  The tuning the process was started with applies to all of it."""
    from snarkvm_amd import msm

    cs = case_set(curve)
    if curve == "g1":
        registered, ref, to_affine = msm.RegisteredBases, lambda b, s: oracle.g1_msm(b, s, oracle.MSM_BATCHED), oracle.g1_to_affine
    else:
        registered, ref, to_affine = msm.RegisteredBasesG2, lambda b, s: oracle.g2_msm(b, s, oracle.MSM_STANDARD), oracle.g2_to_affine
    count = 0
    for case in cs.cases:
        # every named scalar pattern over the case's bases, registered once per geometry
        n = len(case.bases)
        wants = {name: to_affine(ref(case.bases, cs.scalars[name][:n])).tobytes() for name in case.names}
        for geo in GEOMETRIES:
            rb = registered(case.bases, **geo)
            for name in case.names:
                got = to_affine(rb.msm(cs.scalars[name][:n]))
                assert got.tobytes() == wants[name], (case.tag, name, n, geo)
            rb.close()
        count += len(case.names)
    if cs.batch:
        bases = cs.batch.bases
        rb = registered(bases, **BATCH_GEOMETRY)
        got = rb.msm_batch([cs.scalars[name][:n] for n, _, name in BATCH], offsets=[off for _, off, _ in BATCH])
        rb.close()
        at_infinity = to_affine(ref(bases[:1], cs.scalars["zero"][:1]))  # the oracle's image of the empty sum
        for q, (n, off, name) in enumerate(BATCH):
            want = to_affine(ref(bases[off : off + n], cs.scalars[name][:n])) if n else at_infinity
            assert to_affine(got[q : q + 1]).tobytes() == want.tobytes(), ("batch", q, n, off, name)
        count += len(BATCH)
    return count
