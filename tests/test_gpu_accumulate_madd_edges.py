"""The decisions of xyzz_lazy_t::madd and fq2p::xyzz_pair_t::madd inside msm_accumulate_lazy_kernel and msm_accumulate_pair2_kernel as they ship, reached
with crafted bases and n = 2.  After the first addition of a bucket the accumulator is (x1, y1, one, one), so for the second addition U2 = v2 - q and
P = U2 - X1 is fixed by the two bases' residues v = x 2^406 mod q: the G1 filter fires exactly for low29(v2) - low29(v1) in {-3 .. 2}, the pair's per
component for {-1, 0, 1}.  The points lie on the curve, not in the prime-order subgroup: the scalars are 1 and 2^15 - 1 only (the second: digit -1 in
window 0 of a 15-bit recoding, hence a first addition with negate), and the reference is oracle/pyref.py's group law on the full curve.  Every case runs
in both base orders, over tables = 1 and tables = 17 / window_bits = 15 (only table 0 holds the crafted coordinates; scalar 1 touches only it), one MSM
call per case; the model of tests/helpers/lazy_cases.py classifies each case and the set must cover every class."""
import functools
import random

import pytest

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd.msm import RegisteredBases, RegisteredBasesG2
from tests import util
from tests.helpers import lazy_cases as lz

pytestmark = pytest.mark.gpu

Q, RQ, RINV, LIMB = lz.Q, lz.RQ, lz.RINV, lz.LIMB
SCALARS = (1, (1 << 15) - 1)
CONFIGS = ((1, 0, 0), (17, 15, 15))  # tables, window_bits of the handle, window_bits of the call


# ---- G1
@functools.lru_cache(maxsize=None)
def g1_cases():
    """[(name, p1, p2)]: for every d in -6 .. 5 a pair with v2 = v1 + d + j 2^29; the same point twice; a point and its negative"""
    rand = random.Random(0xACC1)
    out = []
    for d in range(-6, 6):
        p1 = lz._g1_base(rand)
        v1 = p1[0] * RQ % Q
        base = (rand.randrange(Q >> (LIMB + 1)) << LIMB) + (v1 & lz.FULL) + d
        for j in range(64):
            p2 = lz.g1_from_x((base + (j << LIMB)) * RINV % Q)
            if p2 is not None and 0 <= base + (j << LIMB) < Q:
                break
        assert p2 is not None and ((p2[0] * RQ % Q) - v1 - d) % (1 << LIMB) == 0
        out.append((f"low29(v2) - low29(v1) = {d}", p1, p2))
    p = lz._g1_base(rand)
    out += [("the same point twice", p, p), ("a point and its negative", p, pyref.g1_neg(p))]
    return out


def g1_class(p1, p2, negate):
    """what the second addition does, by the model: 'restart' never; 'exceptional', 'false alarm', 'below', 'above'"""
    _, acc, _ = lz.m_madd(lz.G1Acc(*([lz.norm(0)] * 4), True), *lz._lazy_base(p1), negate)
    ok, _, p0 = lz.m_madd(acc, *lz._lazy_base(p2), negate)
    low = ((p0 + (1 << 28)) & lz.FULL) - (1 << 28)
    if p1[0] == p2[0]:
        assert not ok
        return "exceptional"
    assert ok == (not -4 <= low <= 1)
    return "false alarm" if not ok else "below" if low < -4 else "above"


def test_the_g1_cases_cover_every_class():
    seen = {}
    for name, p1, p2 in g1_cases():
        assert pyref.g1_is_on_curve(p1) and pyref.g1_is_on_curve(p2)
        for a, b in ((p1, p2), (p2, p1)):
            for negate in (False, True):
                seen.setdefault(g1_class(a, b, negate), set()).add(name)
    assert set(seen) == {"exceptional", "false alarm", "below", "above"}, seen
    # the window takes d in -3 .. 2, and -d for the other base order: exactly the pairs with |d| <= 3 fire in one order or the other
    assert seen["false alarm"] == {f"low29(v2) - low29(v1) = {d}" for d in range(-3, 4)}, seen["false alarm"]
    assert {f"low29(v2) - low29(v1) = {d}" for d in (-6, -5, -4, 3, 4, 5)} <= seen["below"] | seen["above"]


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"tables{c[0]}_w{c[1]}")
def test_g1_second_addition_of_a_bucket(config):
    cases = g1_cases()
    pts = []
    for _, p1, p2 in cases:
        pts += [p1, p2, p2, p1]
    rb = RegisteredBases(util.g1_affine_from_ints(pts), tables=config[0], window_bits=config[1])
    for i, (name, p1, p2) in enumerate(cases):
        for order, (a, b) in enumerate(((p1, p2), (p2, p1))):
            for s in SCALARS:
                want = pyref.msm_naive([a, b], [s, s])
                got = oracle.g1_to_affine(rb.msm(util.ints_to_fr([s, s]), offset=4 * i + 2 * order, window_bits=config[2]))
                assert util.g1_affine_to_ints(got)[0] == want, (name, order, s)
                if want is not None:
                    assert got.tobytes() == util.g1_affine_from_ints([want]).tobytes(), (name, order, s)


# ---- G2
def _g2_from_lazy(v):
    return lz.g2_from_x((v[0] * RINV % Q, v[1] * RINV % Q))


@functools.lru_cache(maxsize=None)
def g2_cases():
    """[(name, p1, p2)]: residues of x that agree per component exactly ('same'), in the low limb only (0, +-1), just outside the window (2), or not at
    all (None); repeated and negated points; points whose y has a zero component"""
    rand = random.Random(0xACC2)
    out = []
    shapes = [(None, None), ("same", None), (None, "same"), (0, None), (None, 0), (0, 0), (1, -1), (-1, None), (None, 1), ("same", 0), (0, "same"), (2, 0), (0, -2)]
    for d in shapes:
        p1 = lz._g2_base(rand)
        v1 = (p1[0][0] * RQ % Q, p1[0][1] * RQ % Q)
        while True:
            v2 = []
            for c in range(2):
                if d[c] == "same":
                    v2.append(v1[c])
                elif d[c] is None:
                    v2.append(rand.randrange(Q))
                else:
                    v2.append(((rand.randrange(Q >> (LIMB + 1)) << LIMB) + (v1[c] & lz.FULL) + d[c]) % Q)
            p2 = _g2_from_lazy(v2)
            if p2 is not None and p2[0] != p1[0]:
                break
        out.append((f"x residues: c0 {d[0]}, c1 {d[1]}", p1, p2))
    neg = lambda p: (p[0], ((-p[1][0]) % Q, (-p[1][1]) % Q))
    p = lz._g2_base(rand)
    out += [("the same point twice", p, p), ("a point and its negative", p, neg(p))]
    for comp in (0, 1):
        z = lz.g2_point_with_zero_y_component(comp)  # found by a short search: y = (t, 0) or (0, t) with x = cbrt(y^2 - b')
        assert z[1][comp] == 0
        out += [(f"y.c{comp} = 0, twice", z, z), (f"y.c{comp} = 0 and its negative", z, neg(z))]
    return out


def g2_class(p1, p2, negate):
    z = [lz.norm(0), lz.norm(0)]
    acc, _ = lz.m_pair_madd(lz.PairAcc(z, z, z, z, True), lz._lazy2(p1[0]), lz._lazy2(p1[1]), negate)
    _, info = lz.m_pair_madd(acc, lz._lazy2(p2[0]), lz._lazy2(p2[1]), negate)
    return (info["path"], tuple(info["low"]), tuple(info["pz"]), tuple(info["rz"]))


def test_the_g2_cases_cover_every_class():
    seen = set()
    for _, p1, p2 in g2_cases():
        assert pyref.g2_is_on_curve(p1) and pyref.g2_is_on_curve(p2)
        for a, b in ((p1, p2), (p2, p1)):
            for negate in (False, True):
                seen.add(g2_class(a, b, negate))
    paths = {s[0] for s in seen}
    assert paths == {"add", "double", "inf"}, paths
    lows = {s[1] for s in seen if s[0] == "add"}
    assert lows == {(True, False), (False, True), (True, True), (False, False)}, lows  # the filter on the even lane only, the odd lane only, both, neither
    assert {(True, False), (False, True)} <= {s[2] for s in seen if s[0] == "add"}  # x.c0 equal and x.c1 not, and the reverse
    assert {(True, False), (False, True)} <= {s[3] for s in seen if s[0] == "inf"}  # R = 0 on one lane only: y with one zero component


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"tables{c[0]}_w{c[1]}")
def test_g2_second_addition_of_a_bucket(config):
    cases = g2_cases()
    pts = []
    for _, p1, p2 in cases:
        pts += [p1, p2, p2, p1]
    rg = RegisteredBasesG2(util.g2_affine_from_ints(pts), tables=config[0], window_bits=config[1])
    for i, (name, p1, p2) in enumerate(cases):
        for order, (a, b) in enumerate(((p1, p2), (p2, p1))):
            for s in SCALARS:
                want = pyref.msm_naive_g2([a, b], [s, s])
                got = oracle.g2_to_affine(rg.msm(util.ints_to_fr([s, s]), offset=4 * i + 2 * order, window_bits=config[2]))
                assert util.g2_affine_to_ints(got)[0] == want, (name, order, s)
                if want is not None:
                    assert got.tobytes() == util.g2_affine_from_ints([want]).tobytes(), (name, order, s)
