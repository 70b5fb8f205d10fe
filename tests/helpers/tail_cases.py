"""Partial-sum lists for the tail kernels of the variable-base MSM (snarkvm_amd/csrc/msm.hip.h 6.-7b) and what every output must be, shared by
tests/test_msm_tail_cases_host.py (CPU) and tests/test_gpu_msm_tail.py (snarkvm_hip_devtest_msm_tail launches the production kernels over these lists).

An ENTRY is (terms, seed): the sum of +- pool points (1-based signed pool indices, at most three; none = the point at infinity) and a rescale seed
(non-zero: the hook stores another representative of the same point).  The pool is 64 points, point i (index i + 1) = (3 i + 1) G, in G1 and in G2.
A case holds one list of entries per bucket, a geometry and ONE launch shape; expected() gives, per output, the signed pool indices whose sum the output
must equal - or None for an output no workgroup writes.  The expected sets follow the layout comment of msm.hip.h 7a / 7b:

    bucket k = w 2^(m + hb) + hi 2^m + lo;  L_lo = sum_hi B(hi, lo) -> slot w 2^(m+1) + lo;  H_hi = sum_lo B(hi, lo) -> slot w 2^(m+1) + 2^m + hi - 1, hi >= 1
    (H_0 and the slots from 2^m + 2^hb - 1 on are never written); tail window 2 w = the L sums, 2 w + 1 = H_1 .., entry i has weight i + 1;
    plane (tw, j) = the sum of the entries of tw whose weight has bit j.  Unfolded windows: tail window w = the nb buckets, bucket i has weight i + 1.

The group element is then one oracle MSM over the pool with the net coefficient of every point as a scalar mod r (1, r - 1, ...): expected_points().

Beside that reference stands a MODEL of the workgroup's addition order (tree_events), used for two things only: to know which G2 outputs the fast kernels
must flag - they flag an output when one of its additions met operands with equal x, P + P or P - P - and to show (host test) that the cases of the
"equal sums at level l" family make exactly the intended addition exceptional and the generic cases none.  Lane (or quad) i of n takes positions
i, i + n, ... of its list one after the other; the n lane sums are added as a perfect binary tree over the lane index (exchange distances 1, 2, 4, ..,
then the wave totals through LDS).  Sums are followed as discrete logarithms (the pool points are known multiples of G), 0 = infinity.

CPU only: Python integers, numpy and the oracle; no torch."""
import collections
import functools
import random

import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from tests import util

R = pyref.R_MOD
POOL_N = 64
DLOG = tuple(3 * i + 1 for i in range(POOL_N))
INF = ((), 0)
STAGE = {"reduce": 0, "merge": 1, "fold": 2, "sparse": 3}
ARITH = {"g1_exact": 0, "g1_lazy": 1, "g2": 2}
# (fold threads, plane threads, quads: bit 0 = planes, bit 1 = fold).  Every thread count; the quad-strided loops off and on (never with 64 threads)
SHAPES = ((64, 64, 0), (128, 128, 0), (128, 128, 3), (256, 256, 0), (256, 256, 3))


def dlog_terms(terms):
    return sum((1 if t > 0 else -1) * DLOG[abs(t) - 1] for t in terms) % R


def negated(entry):
    return (tuple(-t for t in entry[0]), entry[1])


# ---- the pools ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g1_pool():
    gen = util.g1_generator_affine()
    proj = np.concatenate([oracle.g1_mul(gen, util.limbs(d, 4)) for d in DLOG])
    out = oracle.g1_to_affine(proj)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def g2_pool():
    from snarkvm_amd import synthetic

    gen = synthetic.g2_points(1).view(oracle.G2_AFFINE)
    proj = np.concatenate([oracle.g2_mul(gen, util.limbs(d, 4)) for d in DLOG])
    out = oracle.g2_to_affine(proj)
    out.setflags(write=False)
    return out


def pool(group):
    return g1_pool() if group == "g1" else g2_pool()


@functools.lru_cache(maxsize=None)
def _sum_of(group, coeffs):
    """the oracle's MSM over the pool points with a non-zero net coefficient, scalars mod r"""
    idx = [i for i, c in enumerate(coeffs) if c % R]
    if not idx:
        idx, sc = [0], [0]
    else:
        sc = [coeffs[i] % R for i in idx]
    scalars = np.array([util.limbs(s, 4) for s in sc], dtype=np.uint64).reshape(-1, 4)
    if group == "g1":
        return oracle.g1_msm(g1_pool()[idx], scalars, oracle.MSM_STANDARD)
    return oracle.g2_msm(g2_pool()[idx], scalars, oracle.MSM_STANDARD)


def point_of(group, terms):
    """the group element sum of +- pool[|t| - 1] over the signed indices `terms`, projective (1 point)"""
    coeffs = [0] * POOL_N
    for t in terms:
        coeffs[abs(t) - 1] += 1 if t > 0 else -1
    return _sum_of(group, tuple(coeffs))


def to_affine(group, proj):
    return oracle.g1_to_affine(proj) if group == "g1" else oracle.g2_to_affine(proj)


# ---- the model of a workgroup's additions -------------------------------------------------------------------------------------------------------
def tree_events(values, leaves):
    """values: the discrete logarithm of every position of a workgroup's list (0 = infinity, or a position the kernel skips).  -> (total, events):
    events = [(level, a, b)] for every addition of two FINITE operands with equal x (a = +-b); level "chain" = the serial walk of a lane, l = the tree
    level that adds neighbouring blocks of 2^l lanes."""
    events = []

    def add(a, b, level):
        if a == 0:
            return b
        if b == 0:
            return a
        if a == b or (a + b) % R == 0:
            events.append((level, a, b))
        return (a + b) % R

    acc = [0] * leaves
    for p, v in enumerate(values):
        acc[p % leaves] = v if p < leaves else add(acc[p % leaves], v, "chain")
    level = 0
    while len(acc) > 1:
        acc = [add(acc[2 * i], acc[2 * i + 1], level) for i in range(len(acc) // 2)]
        level += 1
    return acc[0], events


def tree_additions(positions, leaves):
    """the same walk over term tuples: positions = per position the signed pool indices of its sum (None = skipped) -> [(level, terms a, terms b)] for every
    addition of two finite operands, for a check of the operands themselves against the oracle"""
    out = []

    def add(a, b, level):
        if a is None or b is None:
            return b if a is None else a
        out.append((level, a, b))
        return a + b if dlog_terms(a + b) else None

    acc = [None] * leaves
    for p, v in enumerate(positions):
        v = v if v and dlog_terms(v) else None
        acc[p % leaves] = v if p < leaves else add(acc[p % leaves], v, "chain")
    level = 0
    while len(acc) > 1:
        acc = [add(acc[2 * i], acc[2 * i + 1], level) for i in range(len(acc) // 2)]
        level += 1
    return out


class Case:
    """name, family, stage; buckets: per bucket the list of its entries; geometry (m, hb, W | nb, W | S2 | L, slot); one launch shape;
    acc: the initial accumulator of a merge (nbt * L entries); extra: outputs beyond the partial sums of a reduce round;
    claims: {output index: level} - the additions this case makes exceptional on purpose (every other addition of the case must be ordinary)."""

    def __init__(self, name, family, stage, buckets, m=0, hb=0, W=1, nb=0, S2=0, L=0, slot=0, shape=(256, 256, 0), acc=None, extra=0, claims=None):
        self.name, self.family, self.stage, self.buckets = name, family, stage, buckets
        self.m, self.hb, self.W, self.nb, self.S2, self.L, self.slot = m, hb, W, nb, S2, L, slot
        self.fold_threads, self.plane_threads, self.quads = shape
        self.acc, self.extra, self.claims = acc or [], extra, dict(claims or {})
        self.nbt = len(buckets)
        if stage == "fold":
            assert self.nbt == W << (m + hb) and 1 <= hb <= m
            self.nbits = m + 1
            self.nslots = W << (m + 1)
            self.nout = self.nslots + 2 * W * self.nbits
        elif stage == "sparse":
            assert self.nbt == W * nb
            self.nbits = nb.bit_length()  # log2(nb) + 1: weights run up to nb
            self.nslots = 0
            self.nout = W * self.nbits
        elif stage == "reduce":
            self.nout = sum(-(-len(b) // S2) for b in buckets) + extra
        else:
            assert len(self.acc) == self.nbt * L
            self.nout = self.nbt * L
        self._cache = {}

    @property
    def id(self):
        return f"{self.family}-{self.name}-{self.fold_threads}.{self.plane_threads}.q{self.quads}"

    @property
    def entries(self):
        return [e for b in self.buckets for e in b]

    # ---- what the hook takes ----
    def hook_arrays(self):
        cnt = np.array([len(b) for b in self.buckets], dtype=np.uint32)
        start = np.zeros(self.nbt + 1, dtype=np.uint32)
        start[1:] = np.cumsum(cnt)
        ents = self.entries + list(self.acc)
        terms = np.zeros((max(1, len(ents)), 3), dtype=np.int32)
        seeds = np.zeros(max(1, len(ents)), dtype=np.uint64)
        for i, (t, s) in enumerate(ents):
            terms[i, : len(t)] = t
            seeds[i] = s
        return start, cnt, terms, seeds, len(self.entries)

    def geom(self, hex2=0, run_fix=0):
        return np.array([self.m, self.hb, self.W, self.nb, self.S2, self.L, self.slot, self.fold_threads, self.plane_threads, hex2, self.quads, run_fix], dtype=np.int32)

    # ---- the lists of the layout comment ----
    def _lines(self):
        """{("c", w, lo): entries of the column, ("r", w, hi): entries of the row}, each in bucket order, from one pass over the non-empty buckets"""
        if "lines" not in self._cache:
            lines = collections.defaultdict(list)
            m, hb = self.m, self.hb
            for k, b in enumerate(self.buckets):
                if b:
                    w, hi, lo = k >> (m + hb), (k >> m) & ((1 << hb) - 1), k & ((1 << m) - 1)
                    lines["c", w, lo] += b
                    lines["r", w, hi] += b
            self._cache["lines"] = lines
        return self._cache["lines"]

    def column(self, w, lo):
        return self._lines().get(("c", w, lo), [])

    def row(self, w, hi):
        return self._lines().get(("r", w, hi), [])

    def tail_window(self, tw):
        """the lists whose sums are the entries of tail window tw (entry i has weight i + 1)"""
        if self.stage == "sparse":
            return [self.buckets[tw * self.nb + i] for i in range(self.nb)]
        w, sub = tw >> 1, tw & 1
        return [self.row(w, hi) for hi in range(1, 1 << self.hb)] if sub else [self.column(w, lo) for lo in range(1 << self.m)]

    def lists(self):
        """{output index: [list per position of the workgroup's walk]}: a position is a list of entries (one entry for a fold row / column or an unfolded
        plane, the entries of an L / H sum for a dense plane) or None where the walk skips it"""
        if "lists" in self._cache:
            return self._cache["lists"]
        out = {}
        if self.stage == "fold":
            for w in range(self.W):
                base = w << (self.m + 1)
                for lo in range(1 << self.m):
                    out[base + lo] = [[e] for e in self.column(w, lo)]
                for hi in range(1, 1 << self.hb):
                    out[base + (1 << self.m) + hi - 1] = [[e] for e in self.row(w, hi)]
        if self.stage in ("fold", "sparse"):
            ntw = 2 * self.W if self.stage == "fold" else self.W
            for tw in range(ntw):
                ent = self.tail_window(tw)
                for j in range(self.nbits):
                    if self.stage == "fold":  # one position per L / H sum
                        pos = [e if ((i + 1) >> j) & 1 else None for i, e in enumerate(ent)]
                    else:  # one position per partial sum of the window
                        pos = [[e] if ((i + 1) >> j) & 1 else None for i, b in enumerate(ent) for e in b]
                    out[self.nslots + tw * self.nbits + j] = pos
        self._cache["lists"] = out
        return out

    def expected(self):
        """per output: the signed pool indices whose sum it must equal (() = infinity, written), None = unwritten"""
        if "expected" in self._cache:
            return self._cache["expected"]
        out = [None] * self.nout
        if self.stage in ("fold", "sparse"):
            for o, pos in self.lists().items():
                out[o] = tuple(t for p in pos if p for e in p for t in e[0])
        elif self.stage == "reduce":
            o = 0
            for b in self.buckets:
                for s in range(0, len(b), self.S2):
                    out[o] = tuple(t for e in b[s : s + self.S2] for t in e[0])
                    o += 1
        else:
            for k, b in enumerate(self.buckets):
                for l in range(self.L):
                    add = b if l == self.slot else []
                    out[k * self.L + l] = tuple(self.acc[k * self.L + l][0]) + tuple(t for e in add for t in e[0])
        self._cache["expected"] = out
        return out

    def untouched(self):
        """merge: the accumulator slots the kernel must not write (another lane's slot, or no partial sum for the bucket)"""
        return [l != self.slot or not self.buckets[k] for k in range(self.nbt) for l in range(self.L)]

    def start_out(self):
        """reduce: the exclusive scan of ceil(cnt / S2), nbt + 1 values"""
        out = [0]
        for b in self.buckets:
            out.append(out[-1] + -(-len(b) // self.S2))
        return out

    def expected_points(self, group):
        """projective points (nout), the oracle's sums; unwritten outputs hold the oracle's zero"""
        key = ("points", group)
        if key not in self._cache:
            self._cache[key] = np.concatenate([point_of(group, t or ()) for t in self.expected()])
        return self._cache[key]

    # ---- the model ----
    def leaves(self, output):
        if self.stage == "sparse":
            return self.plane_threads
        if output < self.nslots:
            return self.fold_threads // 4 if self.quads & 2 else self.fold_threads
        return self.plane_threads // 4 if self.quads & 1 else self.plane_threads

    def events(self):
        """{output index: [(level, a, b)]} over the outputs of a fold / bit-plane case with at least one exceptional addition"""
        if "events" not in self._cache:
            found = {}
            for o, pos in self.lists().items():
                values = [sum(dlog_terms(e[0]) for e in p) % R if p else 0 for p in pos]
                ev = tree_events(values, self.leaves(o))[1]
                if ev:
                    found[o] = ev
            self._cache["events"] = found
        return self._cache["events"]

    def model_flags(self):
        """per output: 1 = the fast G2 kernel must flag it, 0 = must not, None = unwritten"""
        ev = self.events()
        written = self.lists()
        return [None if o not in written else int(o in ev) for o in range(self.nout)]

    def plane_inputs(self, output):
        """fold stage: the fold slots plane `output` reads with their weight's bit set"""
        tw, j = divmod(output - self.nslots, self.nbits)
        w, sub = tw >> 1, tw & 1
        n = (1 << self.hb) - 1 if sub else 1 << self.m
        return [(w << (self.m + 1)) + (sub << self.m) + i for i in range(n) if ((i + 1) >> j) & 1]


# ---- entries ------------------------------------------------------------------------------------------------------------------------------------
class Gen:
    """generic entries: one pool point or a sum of two or three different ones, random signs, every second one rescaled; |discrete log| not yet used in
    any of the lists (`groups`) the entry joins, as long as there is one left"""

    def __init__(self, rng):
        self.rng, self.used = rng, collections.defaultdict(set)

    def entry(self, *groups):
        rng = self.rng
        for attempt in range(100):
            idx = rng.sample(range(1, POOL_N + 1), rng.choice((1, 1, 2, 3)))
            terms = tuple(i if rng.random() < 0.5 else -i for i in idx)
            d = dlog_terms(terms)
            a = min(d, R - d)
            if a and not any(a in self.used[g] for g in groups):
                break
        for g in groups:
            self.used[g].add(a)
        return (terms, rng.getrandbits(62) | 1 if rng.random() < 0.5 else 0)


def _search(build, wanted=lambda case: case.claims):
    """the first of the seeded candidates whose exceptional additions are exactly the claimed ones (none for a generic case)"""
    for s in range(2000):
        case = build(random.Random(f"tail_cases {s}"))
        ev = case.events()
        want = wanted(case)
        if set(ev) == set(want) and all(len(ev[o]) == 1 and ev[o][0][0] == want[o] for o in want):
            return case
    raise AssertionError("no clean candidate")


def _fold_empty(m, hb, W):
    return [[] for _ in range(W << (m + hb))]


def _k(m, hb, w, hi, lo):
    return (w << (m + hb)) + (hi << m) + lo


def _split(rng, total, parts):
    """`total` as a random sum of `parts` non-negative counts, some of them zero"""
    cuts = sorted(rng.randrange(total + 1) for _ in range(parts - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


def _count(rng):
    r = rng.random()
    return rng.randrange(5, 10) if r < 0.04 else 2 if r < 0.34 else 1


# ---- family 1 / 2: generic lists ----------------------------------------------------------------------------------------------------------------------
def generic_fold(family, m, hb, W, shape, target=230):
    def build(rng):
        g, b = Gen(rng), _fold_empty(m, hb, W)
        p = min(0.75, target / len(b))
        for k in sorted(rng.sample(range(len(b)), round(p * len(b)))):
            w, hi, lo = k >> (m + hb), (k >> m) & ((1 << hb) - 1), k & ((1 << m) - 1)
            b[k] = [g.entry(("r", w, hi), ("c", w, lo)) for _ in range(_count(rng))]
        return Case(f"m{m}hb{hb}W{W}", family, "fold", b, m=m, hb=hb, W=W, shape=shape)

    return _search(build)


def generic_sparse(family, nb, W, target=230):
    def build(rng):
        g = Gen(rng)
        p = min(0.75, target / (W * nb))
        b = [[g.entry(("w", k // nb)) for _ in range(_count(rng))] if rng.random() < p else [] for k in range(W * nb)]
        return Case(f"nb{nb}W{W}", family, "sparse", b, nb=nb, W=W, shape=(256, 256, 0))

    return _search(build)


GEOMETRIES = {  # (m, hb, W): the shape the launcher picks for G1 or for G2 where the hook can express it, and others
    (3, 3, 3): ((256, 128, 3), (256, 64, 0)),
    (4, 3, 2): ((256, 128, 3), (128, 64, 0)),
    (5, 1, 2): ((256, 128, 3), (64, 256, 1)),
    (7, 7, 1): ((256, 256, 3), (256, 256, 1), (128, 128, 0)),
    (7, 6, 2): ((256, 256, 3), (128, 256, 1), (64, 128, 0)),
    (9, 8, 1): ((128, 256, 2), (64, 256, 0)),
}
SPARSE = tuple((nb, W) for nb in (2, 8, 64, 1024) for W in (1, 3))


# ---- family 3: list lengths against the workgroup --------------------------------------------------------------------------------------------------
def lengths(axis, part, shape):
    """(4, 4, 2): window 0 holds, per row (axis "row") or per column, lists of B - 1, B, B + 1 entries (and n - 1, n, n + 1 for n = B / 4 quads), part "a", or
    3 B + 5 entries and one bucket alone with B + 3 - for a column its LAST bucket -, part "b"; one row and one column of the window stay empty, window 1
    is empty altogether"""
    m = hb = 4
    B = shape[0]

    def build(rng):
        g, b = Gen(rng), _fold_empty(m, hb, 2)
        totals = [B - 1, B, B + 1] + ([B // 4 - 1, B // 4, B // 4 + 1] if shape[2] & 2 else []) if part == "a" else [3 * B + 5]
        for line, total in enumerate(totals, start=1):
            # the other index runs over 0 .. 14: index 15 stays empty (the empty row / column)
            for other, c in enumerate(_split(rng, total, 15)):
                hi, lo = (line, other) if axis == "row" else (other, line)
                b[_k(m, hb, 0, hi, lo)] = [g.entry(("r", hi), ("c", lo)) for _ in range(c)]
        if part == "b":
            hi, lo = (2, 5) if axis == "row" else (15, 2)
            b[_k(m, hb, 0, hi, lo)] = [g.entry(("r", hi), ("c", lo)) for _ in range(B + 3)]
        return Case(f"{axis}-{part}", "lengths", "fold", b, m=m, hb=hb, W=2, shape=shape)

    return _search(build)


# ---- family 4: infinity entries -----------------------------------------------------------------------------------------------------------------------
def _infinity_lines(g, key):
    e = lambda: g.entry(key)
    return [[INF] * 5 + [e() for _ in range(6)], [e() for _ in range(6)] + [INF] * 5, [x for _ in range(8) for x in (e(), INF)], [INF] * 9]


def infinities_fold(shape):
    """(3, 3, 2): rows 1 .. 4 of window 0 hold infinities in front, at the back, alternating, and nothing else; every bucket of window 1 is a sink pair
    (entry, infinity) or (infinity, infinity)"""
    m = hb = 3

    def build(rng):
        g, b = Gen(rng), _fold_empty(m, hb, 2)
        for hi, line in enumerate(_infinity_lines(g, "w0"), start=1):
            pos = 0
            for lo, c in enumerate(_split(rng, len(line), 8)):
                b[_k(m, hb, 0, hi, lo)] = line[pos : pos + c]
                pos += c
        for k in range(1 << (m + hb), 2 << (m + hb)):
            b[k] = [g.entry(("r", k >> m), ("c", k & 7)) if rng.random() < 0.6 else INF, INF]
        return Case("front-back-alternating-only", "infinities", "fold", b, m=m, hb=hb, W=2, shape=shape)

    return _search(build)


def infinities_sparse():
    def build(rng):
        g = Gen(rng)
        b = []
        for line in _infinity_lines(g, "w0"):
            b += [line[:3], line[3:]]
        b += [[g.entry("w1") if rng.random() < 0.6 else INF, INF] for _ in range(8)]
        return Case("front-back-alternating-only", "infinities", "sparse", b, nb=8, W=2, shape=(256, 256, 0))

    return _search(build)


# ---- family 5: equal partial sums at a chosen tree level -----------------------------------------------------------------------------------------------
VARIANTS = ("same", "negated", "rescaled")


def _second(block, variant, rng):
    if variant == "negated":
        return [negated(e) for e in block]
    if variant == "rescaled":
        return [(e[0], rng.getrandbits(62) | 1) for e in block]
    return list(block)


def levels_of(leaves):
    return list(range(leaves.bit_length() - 1)) + ["chain"]


# Where a block fills its bucket, the two crossing sums (L sums of a row case, H sums of a column case) are equal too: their weights share no bit, so no
# plane adds both
_DISJOINT_WEIGHTS = ((1, 2), (4, 8), (16, 11), (3, 12), (5, 10), (6, 9), (7, 24), (17, 14), (18, 13))
assert all(a & b == 0 for a, b in _DISJOINT_WEIGHTS) and len({w for p in _DISJOINT_WEIGHTS for w in p}) == 18


def equal_sums_fold(axis, variant, shape):
    """(5, 5, 1).  One line (row or column) per level l of the tree over n = B lanes (B / 4 quads when the fold walks quad-strided): n entries, one per lane,
    positions [a, a + 2^l) and [a + 2^l, a + 2^(l+1)) the same entries in the same order (or their negatives, or other representatives), so that the two
    blocks' sums first meet at level l, as P + P (P - P); everything else generic.  One line more for the serial walk: positions 2 and 2 + n are equal.
    The two blocks lie in different buckets, so that no crossing line (a column of a row case) sees both."""
    m = hb = 5
    n = shape[0] // 4 if shape[2] & 2 else shape[0]

    def build(rng):
        g, b, claims = Gen(rng), _fold_empty(m, hb, 1), {}
        for i, level in enumerate(levels_of(n)):
            if level == "chain":
                size, a, cut = n + 3, 2, n
                first = [g.entry(("line", i))]
                second_at = n + 2
            else:
                size = n
                a = 2 << level if (4 << level) <= n else 0
                cut = second_at = a + (1 << level)
                first = [g.entry(("line", i)) for _ in range(1 << level)]
            line = [None] * size
            line[a : a + len(first)] = first
            line[second_at : second_at + len(first)] = _second(first, variant, rng)
            line = [e if e is not None else g.entry(("line", i)) for e in line]
            w0, w1 = sorted(_DISJOINT_WEIGHTS[i])
            if axis == "row":  # row i + 1, the buckets whose columns have weights w0, w1
                k0, k1 = _k(m, hb, 0, i + 1, w0 - 1), _k(m, hb, 0, i + 1, w1 - 1)
                claims[(1 << m) + i] = level
            else:  # column i, the buckets of rows w0, w1
                k0, k1 = _k(m, hb, 0, w0, i), _k(m, hb, 0, w1, i)
                claims[i] = level
            b[k0], b[k1] = line[:cut], line[cut:]
        return Case(f"{axis}-{variant}", "equal_sums", "fold", b, m=m, hb=hb, W=1, shape=shape, claims=claims)

    return _search(build)


def equal_sums_planes(variant, shape, chain=False):
    """(m, 1, W) with 2^m = n, the lanes of a plane workgroup (B / 4 quads when the planes walk quad-strided): every L sum has a lane of its own.  Window
    w makes plane (2 w, 0) - the L sums of odd weight - meet two equal sums at level l = w of its tree: L_0 and L_(2^l) are the same group element
    (L_0 = e1 + e2 from two buckets, L_(2^l) the one entry e1 + e2) and every other L sum of even index below 2^(l+1) is empty.  Weight 1 and weight
    2^l + 1 share bit 0 only.  Level 0 joins lanes 4 and 5 (weights 5 and 6) in plane 2, L_3 and L_6 empty.
    chain: 2^m = 2 n, one window, L_0 = L_n: the two trips of lane 0."""
    hb = 1
    n = shape[1] // 4 if shape[2] & 1 else shape[1]
    lv = ["chain"] if chain else levels_of(n)[:-1]
    m = n.bit_length() - 1 + (1 if chain else 0)
    W = len(lv)

    def build(rng):
        g, b, claims = Gen(rng), _fold_empty(m, hb, W), {}
        nbits = m + 1
        for w, level in enumerate(lv):
            if level == 0:
                i1, i2, j, empty = 4, 5, 2, {3, 6}
            elif level == "chain":
                i1, i2, j, empty = 0, n, 0, set()
            else:
                i1, i2, j, empty = 0, 1 << level, 0, set(range(0, 2 << level, 2))
            e1, e2 = ((rng.randrange(1, POOL_N // 2),), 0), ((rng.randrange(POOL_N // 2, POOL_N + 1),), 0)
            both = _second([(e1[0] + e2[0], 0)], variant, rng)[0]
            for lo in range(1 << m):
                if lo == i1:
                    b[_k(m, hb, w, 0, lo)], b[_k(m, hb, w, 1, lo)] = [e1], [e2]
                elif lo == i2:
                    b[_k(m, hb, w, rng.randrange(2), lo)] = [both]
                elif lo not in empty and rng.random() < 0.5:
                    b[_k(m, hb, w, rng.randrange(2), lo)] = [g.entry(("w", w))]
            claims[(W << (m + 1)) + 2 * w * nbits + j] = level
        return Case(f"planes{'_chain' if chain else ''}-{variant}", "equal_sums", "fold", b, m=m, hb=hb, W=W, shape=shape, claims=claims)

    return _search(build)


# ---- family 6: everything equal --------------------------------------------------------------------------------------------------------------------------
def all_equal(shape, stage="fold"):
    """window 0: every entry is pool point 7 (in some representative); window 1: the same with alternating signs"""
    rng = random.Random("tail_cases all_equal")
    m = hb = 3
    sign, b = 1, []
    for k in range(2 << (m + hb) if stage == "fold" else 16):
        c = rng.choice((1, 1, 2))
        ent = []
        for _ in range(c):
            alt = k >= (1 << (m + hb) if stage == "fold" else 8)
            ent.append(((7 * (sign if alt else 1),), rng.getrandbits(62) | 1 if rng.random() < 0.5 else 0))
            sign = -sign
        b.append(ent)
    if stage == "fold":
        return Case("same-alternating", "all_equal", "fold", b, m=m, hb=hb, W=2, shape=shape)
    return Case("same-alternating", "all_equal", "sparse", b, nb=8, W=2, shape=(256, 256, 0))


# ---- family 7 / 8: reduce and merge ------------------------------------------------------------------------------------------------------------------------
def reduce_case(S2):
    """counts 0, 1, S2 - 1, S2, S2 + 1, 2 S2 + 1 over and over (more partial sums than one workgroup of the kernel takes), a segment P, P and a segment P, -P;
    37 outputs more than the round writes"""
    rng = random.Random(f"tail_cases reduce {S2}")
    g, b = Gen(rng), []
    counts = (0, 1, S2 - 1, S2, S2 + 1, 2 * S2 + 1)
    for k in range(210):
        b.append([g.entry() for _ in range(counts[k % 6])])
    p = g.entry()
    b[7] = [p, (p[0], 12345)]
    b[13] = [p, negated(p)] + ([g.entry()] if S2 > 2 else [])
    return Case(f"S{S2}", "reduce", "reduce", b, S2=S2, extra=37)


def merge_case(L, slot, given):
    """300 buckets of 0 .. 3 partial sums into lane `slot` of L; the accumulator starts as infinity or as given points; bucket 5: the incoming sum equals the
    accumulator (doubling), bucket 9: it is the accumulator's negative"""
    rng = random.Random(f"tail_cases merge {L} {slot} {given}")
    g = Gen(rng)
    b = [[g.entry() for _ in range(rng.choice((0, 1, 1, 2, 3)))] for _ in range(300)]
    acc = [g.entry() if given else INF for _ in range(300 * L)]
    if given:  # (the kernel adds the partial sums to the accumulator one after the other)
        b[5] = [g.entry()]
        acc[5 * L + slot] = (b[5][0][0], 999)
        b[9] = [g.entry(), g.entry()]
        acc[9 * L + slot] = negated((b[9][0][0], 0))
    else:
        b[5] = [b[4][0], b[4][0]] if b[4] else [g.entry()] * 2  # P + P inside the incoming sum
    return Case(f"L{L}slot{slot}-{'given' if given else 'infinity'}", "merge", "merge", b, L=L, slot=slot, acc=acc)


# ---- the list of cases --------------------------------------------------------------------------------------------------------------------------------------
def _sid(shape):
    return "%d.%d.q%d" % tuple(shape)


def _builders():
    out = collections.OrderedDict()

    def put(key, fn, *args, **kw):
        out[key] = functools.partial(fn, *args, **kw)

    for shape in SHAPES + ((256, 128, 1), (128, 256, 2)):
        put(f"generic-m3hb3W3-{_sid(shape)}", generic_fold, "generic", 3, 3, 3, shape)
    put("generic-nb8W3", generic_sparse, "generic", 8, 3)
    for (m, hb, W), shapes in GEOMETRIES.items():
        for shape in shapes:
            put(f"geometry-m{m}hb{hb}W{W}-{_sid(shape)}", generic_fold, "geometry", m, hb, W, shape, 300)
    for nb, W in SPARSE:
        put(f"geometry-nb{nb}W{W}", generic_sparse, "geometry", nb, W, min(300, 12 * nb * W))
    for shape in SHAPES:
        for axis in ("row", "column"):
            for part in ("a", "b"):
                put(f"lengths-{axis}-{part}-{_sid(shape)}", lengths, axis, part, shape)
        put(f"infinities-{_sid(shape)}", infinities_fold, shape)
        for variant in VARIANTS:
            for axis in ("row", "column"):
                put(f"equal_sums-{axis}-{variant}-{_sid(shape)}", equal_sums_fold, axis, variant, shape)
            put(f"equal_sums-planes-{variant}-{_sid(shape)}", equal_sums_planes, variant, shape)
            put(f"equal_sums-planes_chain-{variant}-{_sid(shape)}", equal_sums_planes, variant, shape, True)
        put(f"all_equal-{_sid(shape)}", all_equal, shape)
    put("infinities-nb8W2", infinities_sparse)
    put("all_equal-nb8W2", all_equal, None, "sparse")
    for S2 in (2, 8):
        put(f"reduce-S{S2}", reduce_case, S2)
    for L in (1, 3):
        for slot in range(L):
            for given in (False, True):
                put(f"merge-L{L}slot{slot}-{'given' if given else 'infinity'}", merge_case, L, slot, given)
    return out


BUILDERS = _builders()
KEYS = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(key):
    return BUILDERS[key]()


def stage_of(key):
    """without building the case"""
    family = key.split("-")[0]
    return family if family in ("reduce", "merge") else "sparse" if "-nb" in key else "fold"


def keys(family=None):
    return [k for k in KEYS if (family is None or k.split("-")[0] == family)]
