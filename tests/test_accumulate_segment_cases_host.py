"""Do the cases of tests/helpers/segment_cases.py reach the ends of segments and buckets they were written for?  A model of the walk of the accumulate
kernels (msm_sort.hip.h: msm_accumulate_lazy_kernel, msm_accumulate_seg_kernel, msm_accumulate_pair2_kernel share it) answers on the CPU.

For a case, a scalar pattern and a geometry - the library's own plan at that length (msm_digit_cases.geometry), digits by msm_digit_cases.recode - the
model lays the digit entries out bucket-major (digit row j W + w of scalar i: window w, bucket |d| - 1; a fused group: window = instance), which gives the
per-bucket counts and boff; for S = 2 and S = 3 it cuts the entries into the segments [t S, min(t S + S, total)), takes each segment's first bucket and
part_off = t - boff[k] / S, the positions at which the segment flushes (every bucket end it meets, and its own end) and the empty buckets it steps over.
Every class of CLASSES must occur in at least one case, for both curves and both S: a case set that misses one is a defect of the case set.

The classes of COUNT_CLASSES depend on the counts alone.  Those of ORDER_CLASSES also depend on the order of the entries INSIDE a bucket, which the model
takes to be (table j, index i): the order a stable sort leaves.  This test does not verify that the device sort is stable (msm_sort.hip.h says the order
inside a (tile, bin) run is LDS cursor order); the device tests do not depend on it either - they compare sums.  Where the code itself rules index order
out - a digit row read eight digits per lane: n = 128, and the whole tiles of the fused batch - the order classes are not counted (index_order_expected)."""
import functools

import numpy as np
import pytest

from tests.helpers import msm_digit_cases as mdc
from tests.helpers import segment_cases as sc

COUNT_CLASSES = (
    "part_off_ge_2",                    # a bucket spanning at least three segments
    "flush_at_every_entry",             # a full segment whose every entry ends a bucket
    "one_entry_segment",
    "last_segment_short",
    "total_multiple_of_S",
    "bucket_ends_at_segment_end",       # the flush at `end` of a segment that is not the last: the next segment starts a bucket
    "bucket_ends_one_before_segment_end",
    "empty_run_skipped_inside_segment", # at least two empty buckets between two entries of one segment
    "total_zero",
)
ORDER_CLASSES = (
    "infinity_at_segment_first",
    "infinity_at_segment_last",
    "P_P_inside_segment",
    "P_minusP_inside_segment",
    "P_P_across_segments",
    "P_minusP_across_segments",
    "flushed_at_infinity",              # the (segment, bucket) run sums to the point at infinity
    "negative_at_segment_last",         # the sign bit on the entry at hi - 1
)
CLASSES = COUNT_CLASSES + ORDER_CLASSES
G2_CLASSES = CLASSES + ("flushed_at_infinity_after_cancellation",)  # cancel_restart

_H = np.random.default_rng(0x5E6).integers(1, 1 << 62, size=(sc.NMAX + 1, 128), dtype=np.int64)  # one value per (multiple of the generator, table)


@functools.lru_cache(maxsize=None)
def _digits(s, c, Wd):
    return tuple(mdc.recode(s, c, Wd)[0])


def sorted_entries(instances, g):
    """instances: [(integers, descriptions)], one bucket window set each (a single MSM: one) -> the entries in sorted order, as arrays: bucket, identity
    (multiple of the generator and table; -1: the point at infinity), sign of the term (+-1: the base's xor the digit's), the digit's sign bit; and boff"""
    rows = np.arange(g.Wd)
    jj, ww = rows // g.W, rows % g.W
    parts = []
    for q, (ints, desc) in enumerate(instances):
        if not len(ints):
            continue
        D = np.array([_digits(s, g.c, g.Wd) for s in ints], dtype=np.int64).reshape(len(ints), g.Wd)
        ii, rr = np.nonzero(D)
        d = D[ii, rr]
        mult = np.array([0 if p is None else p[0] for p in desc], dtype=np.int64)[ii]
        bneg = np.array([False if p is None else p[1] for p in desc])[ii]
        parts.append(((q * g.W + ww[rr]) * g.nb + np.abs(d) - 1, jj[rr], ii, mult, np.where(bneg ^ (d < 0), -1, 1), d < 0))
    nbt = len(instances) * g.W * g.nb
    if not parts:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z.astype(bool), np.zeros(nbt + 1, dtype=np.int64)
    bk, j, i, mult, sgn, dneg = (np.concatenate(cols) for cols in zip(*parts))
    order = np.lexsort((i, j, bk))
    bk, j, mult, sgn, dneg = bk[order], j[order], mult[order], sgn[order], dneg[order]
    ident = np.where(mult > 0, mult * 128 + j, -1)
    boff = np.concatenate([[0], np.cumsum(np.bincount(bk, minlength=nbt))])
    return bk, ident, sgn, dneg, boff


def walk_classes(entries, S):
    """the classes the walk over segments of S entries meets"""
    bk, ident, sgn, dneg, boff = entries
    total = len(bk)
    assert boff[-1] == total
    if not total:
        return {"total_zero"}
    pos = np.arange(total)
    lo = np.arange(0, total, S)
    seglen = np.minimum(S, total - lo)
    first = pos % S == 0
    last = (pos % S == S - 1) | (pos == total - 1)
    # each segment's first bucket holds entry lo, and is not empty; part_off counts the segments since the bucket's first
    k0 = bk[lo]
    assert np.all((boff[k0] <= lo) & (lo < boff[k0 + 1]))
    part_off = lo // S - boff[k0] // S
    assert np.all(part_off >= 0)
    new_bucket = np.concatenate([[True], bk[1:] != bk[:-1]])          # entry pos opens a bucket
    step = np.concatenate([[0], bk[1:] - bk[:-1]])
    flush_inside = new_bucket & ~first                                 # `pos >= kend` inside a segment
    nflush = np.add.reduceat(flush_inside.astype(np.int64), lo) + 1    # and the flush at the segment's end
    # every partial-sum slot is written once: the first flush at start[k] + part_off, the later ones at start[k] - the layout msm_alloc_seg_kernel sizes
    cnt = np.where(boff[1:] > boff[:-1], (boff[1:] - 1) // S - boff[:-1] // S + 1, 0)
    assert nflush.sum() == cnt.sum()
    inf = ident < 0
    same = ~new_bucket & ~inf & np.concatenate([[False], (ident[1:] == ident[:-1])])
    eq = np.concatenate([[False], sgn[1:] == sgn[:-1]])
    run_start = np.flatnonzero(first | new_bucket)
    val = np.where(inf, 0, sgn * _H[np.maximum(ident, 0) // 128, np.maximum(ident, 0) % 128])
    with np.errstate(over="ignore"):
        run_sum = np.add.reduceat(val, run_start)
    run_all_inf = np.add.reduceat((~inf).astype(np.int64), run_start) == 0
    found = {
        "part_off_ge_2": np.any(part_off >= 2),
        "flush_at_every_entry": np.any((nflush == seglen) & (seglen == S)),
        "one_entry_segment": np.any(seglen == 1),
        "last_segment_short": total % S != 0,
        "total_multiple_of_S": total % S == 0,
        "bucket_ends_at_segment_end": np.any(new_bucket & first & (pos > 0)),
        "bucket_ends_one_before_segment_end": np.any(flush_inside & last),
        "empty_run_skipped_inside_segment": np.any(flush_inside & (step >= 3)),
        "infinity_at_segment_first": np.any(inf & first),
        "infinity_at_segment_last": np.any(inf & last),
        "P_P_inside_segment": np.any(same & eq & ~first),
        "P_minusP_inside_segment": np.any(same & ~eq & ~first),
        "P_P_across_segments": np.any(same & eq & first),
        "P_minusP_across_segments": np.any(same & ~eq & first),
        "flushed_at_infinity": np.any(run_sum == 0),
        "flushed_at_infinity_after_cancellation": np.any((run_sum == 0) & ~run_all_inf),
        "negative_at_segment_last": np.any(dneg & last & ~inf),
    }
    return {name for name, hit in found.items() if hit}


def _geometries(n):
    return [mdc.geometry(n, 0, geo["tables"], geo.get("window_bits", 0) or 256 // geo["tables"]) for geo in sc.GEOMETRIES]


@functools.lru_cache(maxsize=None)
def classes_by_case(curve):
    """{S: {(tag, n, scalar pattern, geometry): classes}}"""
    cs = sc.case_set(curve)
    out = {2: {}, 3: {}}
    for case in cs.cases:
        n = len(case.desc)
        for gi, g in enumerate(_geometries(n)):
            for name in case.names:
                e = sorted_entries([(cs.scalar_ints[name][:n], case.desc)], g)
                for S in out:
                    out[S][(case.tag, n, name, gi)] = walk_classes(e, S) - (set() if index_order_expected(n) else set(ORDER_CLASSES + G2_CLASSES[-1:]))
    if cs.batch:
        e, _ = batch_entries(cs)
        for S in out:
            out[S][("batch", len(sc.BATCH), "", 0)] = walk_classes(e, S) & set(COUNT_CLASSES)  # whole tiles: eight digits per lane
    return out


def index_order_expected(n):
    """A digit row whose length is a multiple of 8 is read with 16-byte loads, eight consecutive digits per lane (msm_sort.hip.h::for_each_digit_t), so
    the LDS cursors see digit k of every lane before digit k + 1 of any: such a row cannot arrive in index order, and the classes that depend on the order
    are not counted from it.  (Seen on the device: a scratch build of the pair kernel that flushes stale coordinates for a bucket at infinity changed the
    cancel_restart results at n = 2, 3, 127, 129 and 257 under seg=2, and not at n = 128.)"""
    return n % 8 != 0


def batch_entries(cs):
    """the fused group of the batch: every instance is one bucket window of a 17 x 15 geometry over the padded concatenation (SORT_TILE = 8192 positions
    per instance here).  An empty instance never joins a group (msm_batch.hip.h::msm_make_jobs): it is answered without a launch."""
    fused = [(n, off, name) for n, off, name in sc.BATCH if n]
    g = mdc.geometry(8192 * len(fused), sc.BATCH_GEOMETRY["window_bits"], sc.BATCH_GEOMETRY["tables"], sc.BATCH_GEOMETRY["window_bits"])
    assert (g.c, g.W, g.J) == (15, 1, 17)  # what a fused group needs: one bucket window per instance
    return sorted_entries([(cs.scalar_ints[name][:n], cs.batch.desc[off : off + n]) for n, off, name in fused], g), g


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_every_class_occurs(curve, S):
    by_case = classes_by_case(curve)[S]
    wanted = G2_CLASSES if curve == "g2" else CLASSES
    where = {name: [key for key, got in by_case.items() if name in got] for name in wanted}
    for name in wanted:
        print(f"{curve} S={S} {name}: {len(where[name])} of {len(by_case)} runs, first {where[name][:1]}")
    missing = [name for name in wanted if not where[name]]
    assert not missing, missing


@pytest.mark.parametrize("S", [2, 3])
def test_batch_segments_cross_instances(S):
    """in the fused group a segment runs from one instance's buckets into the next one's, and one steps over the 2^14 empty buckets of the instance whose
    scalars are all zero"""
    (bk, _, _, _, _), g = batch_entries(sc.case_set("g2"))
    inside = np.arange(1, len(bk)) % S != 0
    windows = bk[1:] // g.nb - bk[:-1] // g.nb
    assert g.nb == 1 << 14 and np.any(inside & (windows == 1)) and np.any(inside & (windows == 2))


def test_case_counts():
    """the literals the device tests assert"""
    g1, g2 = sc.case_set("g1"), sc.case_set("g2")
    assert sc.case_count(g1) == 140 and g1.batch is None
    assert sum(len(c.names) for c in g2.cases if c.tag != "cancel_restart") == 140
    assert sc.case_count(g2) == 140 + len(sc.SIZES) + len(sc.BATCH) == 154


def test_cancel_restart_buckets_end_at_infinity():
    """n = 2 and n = 128 with equal scalars: in index order every bucket's last run ends on P, -P, whatever the segment length.  (On the device the rows of
    n = 128 are read eight digits per lane, see index_order_expected: there n = 2 is the case that is flushed at infinity for certain.)"""
    cs = sc.case_set("g2")
    for case in cs.cases:
        n = len(case.desc)
        if case.tag != "cancel_restart" or n not in (2, 128):
            continue
        for g in _geometries(n):
            bk, ident, sgn, _, _ = sorted_entries([(cs.scalar_ints["equal"][:n], case.desc)], g)
            ends = np.flatnonzero(np.concatenate([bk[1:] != bk[:-1], [True]]))
            assert np.all((ident[ends] == ident[ends - 1]) & (sgn[ends] == -sgn[ends - 1]))
