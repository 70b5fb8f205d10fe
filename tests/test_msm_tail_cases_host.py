"""tests/helpers/tail_cases.py on the CPU: the expected outputs of the MSM tail kernels satisfy the identities the tail is built on (msm.hip.h 7.), and the
cases are what they claim - the generic ones make no addition exceptional, the "equal sums at level l" ones exactly the addition they name.  This pins the
reference and the case lists before tests/test_gpu_msm_tail.py shows them to a GPU.  Group arithmetic: the CPU oracle, in G1 (the lists are the same in
G1 and G2: signed indices into pools of the same multiples of the generator)."""
import numpy as np
import pytest

from oracle import cpu as oracle
from tests import util
from tests.helpers import tail_cases as tc

FOLD_KEYS = [k for k in tc.KEYS if tc.stage_of(k) == "fold"]
SPARSE_KEYS = [k for k in tc.KEYS if tc.stage_of(k) == "sparse"]


def _affine(terms):
    return oracle.g1_to_affine(tc.point_of("g1", tuple(terms)))


def _weighted(points, weights):
    """sum_i weights[i] points[i] by the oracle's MSM over the points themselves"""
    sc = np.array([util.limbs(w, 4) for w in weights], dtype=np.uint64).reshape(-1, 4)
    return oracle.g1_to_affine(oracle.g1_msm(oracle.g1_to_affine(points), sc, oracle.MSM_STANDARD))


def _weighted_entries(lists, weights):
    """sum_i weights[i] (sum of the entries of lists[i]) from the pool points directly"""
    coeffs = [0] * tc.POOL_N
    for entries, w in zip(lists, weights):
        for e in entries:
            for t in e[0]:
                coeffs[abs(t) - 1] += w if t > 0 else -w
    return oracle.g1_to_affine(tc._sum_of("g1", tuple(coeffs)))


def test_the_pools_are_the_claimed_multiples_and_distinct():
    g1, g2 = tc.g1_pool(), tc.g2_pool()
    assert len(g1) == len(g2) == tc.POOL_N and not g1["infinity"].any() and not g2["infinity"].any()
    assert len({p.tobytes() for p in g1}) == tc.POOL_N and len({p.tobytes() for p in g2}) == tc.POOL_N
    want = oracle.g1_gen_bases(util.g1_generator_affine(), 1, 3 * tc.POOL_N)[:: 3]
    assert util.affine_equal(g1, want)
    # point_of: 2 P_1 - P_3 + P_3 = 2 P_1, and P - P = infinity
    assert util.affine_equal(_affine((1, 1, -3, 3)), oracle.g1_gen_bases(util.g1_generator_affine(), 2, 1))
    assert _affine((5, -5))["infinity"][0] == 1


@pytest.mark.parametrize("key", FOLD_KEYS)
def test_fold_reference_satisfies_the_two_axis_identity(key):
    """per window: sum_b (b + 1) B_b = 2^m sum_hi hi H_hi + sum_lo (lo + 1) L_lo over the expected slots, and per tail window sum_i (i + 1) E_i =
    sum_j 2^j S_j over the expected planes; the slots the layout leaves unwritten are exactly H_0's and those from 2^m + 2^hb - 1 on"""
    c = tc.case(key)
    exp, pts = c.expected(), c.expected_points("g1")
    m, hb, nlo, nhi = c.m, c.hb, 1 << c.m, 1 << c.hb
    for w in range(c.W):
        base = w << (m + 1)
        assert [o - base for o in range(base, base + 2 * nlo) if exp[o] is None] == list(range(nlo + nhi - 1, 2 * nlo))
        nb = nlo * nhi
        buckets = c.buckets[w * nb : (w + 1) * nb]
        if not any(buckets):
            assert all(exp[o] == () for o in range(base, base + nlo + nhi - 1))
            continue
        lhs = _weighted_entries(buckets, range(1, nb + 1))
        slots = list(range(base, base + nlo + nhi - 1))
        rhs = _weighted(pts[slots], [lo + 1 for lo in range(nlo)] + [hi << m for hi in range(1, nhi)])
        assert util.affine_equal(lhs, rhs), (key, w)
        for sub in (0, 1):
            tw = 2 * w + sub
            ent = c.tail_window(tw)
            planes = [c.nslots + tw * c.nbits + j for j in range(c.nbits)]
            lhs = _weighted_entries(ent, range(1, len(ent) + 1))
            assert util.affine_equal(lhs, _weighted(pts[planes], [1 << j for j in range(c.nbits)])), (key, tw)
    assert all(e is not None for e in exp[c.nslots :])


@pytest.mark.parametrize("key", SPARSE_KEYS)
def test_unfolded_reference_satisfies_the_plane_identity(key):
    c = tc.case(key)
    pts = c.expected_points("g1")
    assert c.nbits == {2: 2, 8: 4, 64: 7, 1024: 11}[c.nb]  # the launcher's: window bits c with nb = 2^(c - 1)
    for w in range(c.W):
        ent = c.tail_window(w)
        lhs = _weighted_entries(ent, range(1, c.nb + 1))
        planes = [w * c.nbits + j for j in range(c.nbits)]
        assert util.affine_equal(lhs, _weighted(pts[planes], [1 << j for j in range(c.nbits)])), (key, w)


def test_tree_model_levels():
    """the model itself on lists small enough to follow by hand: 8 lanes, values 1 .. (their sums never repeat), one pair made equal"""
    vals = [1, 2, 4, 8, 16, 32, 64, 128]
    assert tc.tree_events(vals, 8) == (255, [])
    assert tc.tree_events([1, 1, 4, 8, 16, 32, 64, 128], 8)[1] == [(0, 1, 1)]
    assert tc.tree_events([1, 2, 3, 0, 16, 32, 64, 128], 8)[1] == [(1, 3, 3)]  # lanes 0, 1 against lanes 2, 3 (lane 3 holds infinity)
    assert tc.tree_events([1, 2, 4, 8, 6, 5, 3, 1], 8)[1] == [(2, 15, 15)]
    assert tc.tree_events(vals + [0, tc.R - 2], 8)[1] == [("chain", 2, tc.R - 2)]  # position 9 joins lane 1: P - P
    assert tc.tree_events(vals + [0, tc.R - 2], 8)[0] == 253  # ... and the lane goes on as infinity
    assert tc.tree_events([5, 0, 0, 0], 4) == (5, [])  # infinity operands are no event
    adds = tc.tree_additions([(1,), (2,), None, (3, -3), (4,)], 4)
    assert adds == [("chain", (1,), (4,)), (0, (1, 4), (2,))]


def _blocks_meet(c, output, level):
    """the two operands of the claimed addition, as term tuples, from the list and the lane arithmetic alone"""
    pos = [tuple(t for e in p for t in e[0]) if p else None for p in c.lists()[output]]
    adds = [a for a in tc.tree_additions(pos, c.leaves(output)) if a[0] == level]
    hits = [(a, b) for _, a, b in adds if tc.dlog_terms(a) in (tc.dlog_terms(b), (-tc.dlog_terms(b)) % tc.R)]
    assert len(hits) == 1, (output, level, len(hits))
    return hits[0]


EQUAL_KEYS = tc.keys("equal_sums")


@pytest.mark.parametrize("key", EQUAL_KEYS)
def test_equal_sums_cases_meet_at_the_claimed_level_and_nowhere_else(key):
    c = tc.case(key)
    n_fold, n_plane = c.leaves(0), c.leaves(c.nslots)
    want_levels = tc.levels_of(n_plane if "planes" in key else n_fold)
    if "planes" in key:
        want_levels = ["chain"] if "chain" in key else want_levels[:-1]
    assert sorted(map(str, c.claims.values())) == sorted(map(str, want_levels)), "one output per level of the tree, and one for the serial walk"
    ev = c.events()
    assert set(ev) == set(c.claims), "no other output of the case meets equal x coordinates"
    variant = key.split("-")[2]
    for o, level in c.claims.items():
        assert [e[0] for e in ev[o]] == [level]
        a, b = _blocks_meet(c, o, level)
        pa, pb = _affine(a), _affine(b)
        assert not pa["infinity"][0] and np.array_equal(pa["x"], pb["x"]), (key, o, level)
        assert np.array_equal(pa["y"], pb["y"]) == (variant != "negated"), (key, o, level)
        assert len(a) >= (1 << level if isinstance(level, int) and "planes" not in key else 1)
    assert c.model_flags().count(1) == len(c.claims)


GENERIC_KEYS = tc.keys("generic") + tc.keys("geometry") + tc.keys("lengths") + tc.keys("infinities")


@pytest.mark.parametrize("key", GENERIC_KEYS)
def test_generic_cases_meet_no_equal_sums(key):
    """... so that "every flag is 0" follows from the inputs; the counts are mixed as promised"""
    c = tc.case(key)
    assert c.events() == {} and 1 not in c.model_flags()
    if key.startswith("generic"):
        counts = {len(b) for b in c.buckets}
        assert {0, 1, 2} <= counts and counts & {5, 6, 7, 8, 9}
    assert len(c.entries) <= 4096 and c.nbt <= 1 << 17


def test_generic_operands_have_distinct_x_in_the_oracle():
    """the model's verdict on the smallest generic case checked on the affine images: no addition of any workgroup adds two points with one x"""
    c = tc.case(tc.keys("generic")[0])
    seen = {}
    for o, plist in c.lists().items():
        pos = [tuple(t for e in p for t in e[0]) if p else None for p in plist]
        for level, a, b in tc.tree_additions(pos, c.leaves(o)):
            for t in (a, b):
                if t not in seen:
                    seen[t] = _affine(t)["x"].tobytes()
            assert seen[a] != seen[b], (o, level)
    assert len(seen) > 500


def test_all_equal_cases_flag_every_sum_of_two():
    for key in tc.keys("all_equal"):
        c = tc.case(key)
        flags, lists = c.model_flags(), c.lists()
        for o, pos in lists.items():
            finite = sum(1 for p in pos if p and sum(tc.dlog_terms(e[0]) for e in p) % tc.R)
            if o < c.nslots or c.stage == "sparse":
                assert flags[o] == int(finite >= 2), (key, o)


def test_reduce_and_merge_references():
    for key in tc.keys("reduce"):
        c = tc.case(key)
        so = c.start_out()
        assert so[-1] + c.extra == c.nout and so[-1] > 256 and c.expected()[so[-1] :] == [None] * c.extra
        assert {len(b) for b in c.buckets} >= {0, 1, c.S2 - 1, c.S2, c.S2 + 1, 2 * c.S2 + 1}
        flat = [t for b in c.buckets for e in b for t in e[0]]
        assert sorted(flat) == sorted(t for e in c.expected() if e for t in e)
    for key in tc.keys("merge"):
        c = tc.case(key)
        un = c.untouched()
        assert any(un) and not all(un) and all(un[k * c.L + l] for k in range(c.nbt) for l in range(c.L) if l != c.slot)
        assert all(c.expected()[i] == c.acc[i][0] for i in range(c.nout) if un[i])
