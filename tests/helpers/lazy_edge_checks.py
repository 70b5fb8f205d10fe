"""The checks of tests/helpers/lazy_cases.py's operands, written once for the host twin (snarkvm_hip_selftest_lazy_ext) and the GPU kernels
(snarkvm_hip_devtest_lazy_ext): a `Runner` is the call.  Every result is checked three ways against Python integers that share nothing with the
routine - the congruence (for the additions: the group element, oracle/pyref.py on the decoded accumulator), that it is normalised, that it lies in the
range the routine's comment promises - and then limb for limb against the column-by-column model of lazy_cases.py, whose replay has proven every
case legal (no column sum beyond 64 bits, every operand inside its precondition)."""
import numpy as np

from oracle import pyref
from snarkvm_amd import _lib
from tests.helpers import lazy_cases as lz

Q, R, FULL, LIMB, N = lz.Q, lz.R, lz.FULL, lz.LIMB, lz.N


class Runner:
    def __init__(self, device):
        self.device = device

    def run(self, name, rows):
        L = _lib.lib()
        op = lz.OPS[name]
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        n = rows.shape[0]
        assert rows.shape[1] == lz.IN_WORDS[op]
        out = np.full((n, lz.OUT_WORDS[op]), 0x5A5A5A5A, dtype=np.int32)
        if self.device:
            _lib.check(L.snarkvm_hip_devtest_lazy_ext(op, rows.ctypes.data, out.ctypes.data, n))
        else:
            assert L.snarkvm_hip_selftest_lazy_ext(op, rows.ctypes.data, out.ctypes.data, n) == 0
        return out


def _ints(row):
    return [int(x) for x in row]


def _vals(got, k):
    """column block k (13 words) of every row as limb lists"""
    return [_ints(r) for r in got[:, 13 * k : 13 * k + 13]]


def _same(got, want, c):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (c.op, "differs from the column model", c.names[int(bad[0])], _ints(got[bad[0]]), _ints(want[bad[0]]))


def _normalised_in(l, rng, what, name):
    assert lz.is_normalised(l), (what, "not normalised", name, l)
    assert lz.inside(lz.value(l), rng), (what, "outside its promised range", name, lz.value(l) * 1000 // Q / 1000)


def check_products(run):
    """mul, sqr, diff_of_products"""
    c = lz.mul_cases()
    got = run.run("mul", c.rows)
    for r, ((_, a), (_, b)), name in zip(_vals(got, 0), c.meta, c.names):
        assert (lz.value(r) * R - lz.value(a) * lz.value(b)) % Q == 0, ("mul", name)
        _normalised_in(r, lz.PROD_RNG, "mul", name)
    _same(got, c.want, c)
    c = lz.sqr_cases()
    got = run.run("sqr", c.rows)
    for r, (_, a), name in zip(_vals(got, 0), c.meta, c.names):
        assert (lz.value(r) * R - lz.value(a) ** 2) % Q == 0, ("sqr", name)
        _normalised_in(r, lz.PROD_RNG, "sqr", name)
    _same(got, c.want, c)
    c = lz.dop_cases()
    got = run.run("dop", c.rows)
    for r, q, name in zip(_vals(got, 0), c.meta, c.names):
        a, b, cc, d = (lz.value(l) for _, l in q)
        assert (lz.value(r) * R - (a * b - cc * d)) % Q == 0, ("diff_of_products", name)
        _normalised_in(r, lz.DOP_RNG, "diff_of_products", name)
    _same(got, c.want, c)


def check_conversions(run):
    """normalized, to_exact, from_exact, the raw image"""
    c = lz.normalized_cases()
    got = run.run("normalized", c.rows)
    for r, (_, a), name in zip(_vals(got, 0), c.meta, c.names):
        assert lz.is_normalised(r) and lz.value(r) == lz.value(a), ("normalized", name)
    _same(got, c.want, c)
    c = lz.to_exact_cases()
    got = run.run("to_exact", c.rows)
    i29 = pow(2, -LIMB, Q)
    for r, (_, a), name in zip(_vals(got, 0), c.meta, c.names):
        assert all(0 <= x <= FULL for x in r) and lz.value(r) == lz.value(a) * i29 % Q, ("to_exact", name)  # canonical: the one value below q
    _same(got, c.want, c)
    c = lz.from_exact_cases()
    got = run.run("from_exact", c.rows)
    for r, (_, a), name in zip(_vals(got, 0), c.meta, c.names):
        assert (lz.value(r) - a * (1 << LIMB)) % Q == 0, ("from_exact", name)
        _normalised_in(r, lz.PROD_RNG, "from_exact", name)
    _same(got, c.want, c)
    c = lz.raw_cases()
    got = run.run("raw", c.rows)
    for row, (_, a), name in zip(got, c.meta, c.names):
        img = sum((int(w) & 0xFFFFFFFF) << (32 * j) for j, w in enumerate(row[:12]))
        assert img == lz.value(a) % (1 << 384) and _ints(row[12:]) == a, ("raw image", name)
    _same(got, c.want, c)


def check_fqz(run):
    c = lz.fqz_cases()
    got = run.run("fqz", c.rows)
    seen = set()
    for row, (a, b, z), name in zip(got, c.meta, c.names):
        va, vb = lz.value(a), lz.value(b)
        for k, want in enumerate((va + vb, va - vb, 2 * va, -va)):
            r = _ints(row[13 * k : 13 * k + 13])
            assert lz.is_normalised(r) and lz.value(r) == want, ("fqz", ("+", "-", "dbl", "neg")[k], name)
        zero = lz.value(z) % Q == 0
        assert int(row[52]) == (1 if zero else 0), ("fqz is_zero", name)
        seen.add((zero, not any(z), ((z[0] + 8) & FULL) <= 16))
    # a multiple of q other than 13 zero limbs; 13 zero limbs; a false alarm of the low-limb filter; a value the filter turns away
    assert {(True, False, True), (True, True, True), (False, False, True), (False, False, False)} <= seen
    _same(got, c.want, c)


def _g1_acc(words):
    return lz.G1Acc(_ints(words[0:13]), _ints(words[13:26]), _ints(words[26:39]), _ints(words[39:52]), int(words[52]) != 0)


def check_madd(run):
    """-> {class: count}"""
    c = lz.madd_cases()
    cases, _ = c.meta
    got = run.run("madd", c.rows)
    k_seen, window_seen, classes = set(), set(), {}
    for row, cs, name in zip(got, cases, c.names):
        ok, out = int(row[0]), _g1_acc(row[1:])
        b = cs.b_pt if not cs.negate else pyref.g1_neg(cs.b_pt)
        classes[cs.cls] = classes.get(cs.cls, 0) + 1
        if cs.acc.inf:
            assert ok == 1 and not out.inf and lz.g1_decode(out) == b, name
            assert all(lz.is_normalised(l) for l in out[:4]) and lz.inside(lz.value(out.y), lz.Y_RNG) and out.zz == lz.ONE and out.zzz == lz.ONE, name
            continue
        a = lz.g1_decode(cs.acc)
        assert a == cs.a_pt, name
        # P = U2 - X1 from the closed form of the product, not from the model's madd
        ab = lz.value(cs.px) * lz.value(cs.acc.zz)
        u2 = (ab - ab * lz.QINV % R * Q) // R
        p = u2 - lz.value(cs.acc.x)
        in_window = ((p + 4) & FULL) <= 5
        if a[0] == b[0]:
            assert p % Q == 0 and in_window, name
            k_seen.add((p // Q, a[1] == b[1]))
            assert ok == 0, ("equal x coordinates but madd returned true", name)
        else:
            lowp = ((p + (1 << 28)) & FULL) - (1 << 28)
            window_seen.add(lowp if abs(lowp) < 16 else None)
            assert ok == (0 if in_window else 1), ("the window {-4 .. 1} on the low limb of P predicts otherwise", name, lowp)
        if ok == 0:
            assert out == cs.acc, ("the accumulator changed although madd returned false", name)
            continue
        assert not out.inf and lz.g1_decode(out) == pyref.g1_add(a, b), ("wrong group element", name)
        _normalised_in(out.x, lz.X_RNG, "madd x", name)
        _normalised_in(out.y, lz.Y_RNG, "madd y", name)
        _normalised_in(out.zz, lz.ZZ_RNG, "madd zz", name)
        _normalised_in(out.zzz, lz.ZZ_RNG, "madd zzz", name)
    assert k_seen == {(k, d) for k in range(-4, 2) for d in (True, False)}, k_seen  # every representative of a zero P, as a doubling and as a cancellation
    assert set(range(-6, 6)) <= window_seen and None in window_seen, window_seen  # both ends of the window straddled by P != 0
    assert set(classes) == {"ordinary", "exceptional", "window", "restart"}
    _same(got, c.want, c)
    return classes


def check_pair_helpers(run):
    c = lz.pair_help_cases()
    got = run.run("pair_help", c.rows)
    images = set()
    for row, (a, b, cc, t, y), name in zip(got, c.meta, c.names):
        p, d, k, ny, sy = (_ints(row[13 * i : 13 * i + 13]) for i in range(5))
        assert lz.is_tight(p) and lz.value(p) == lz.value(a) - lz.value(b) + Q, ("sub_norm(+1)", name)
        dv = lz.value(a) - lz.value(cc)
        # q is added by the sign of the top-limb difference: a - c in (-1 - 2 e, 1 + 2 e) comes out within [-2 e, 1 + 2 e]
        assert lz.is_tight(d) and lz.value(d) in (dv, dv + Q) and -2 * lz.E * Q <= lz.value(d) <= (1 + 2 * lz.E) * Q, ("sub_norm(-1)", name)
        kv = lz.value(k)
        assert lz.is_tight(k) and (kv - lz.value(t)) % Q == 0 and -lz.NK * Q < kv < (1 + lz.NK) * Q, ("norm_k", name, kv * 1000 // Q)
        assert lz.is_normalised(ny) and lz.value(ny) == Q - lz.value(y) and sy == y, ("cond_neg_canonical", name)
        zero = lz.value(p) % Q == 0
        assert int(row[65]) == (1 if zero else 0), ("is_zero_mod_q", name)
        if zero:
            images.add(lz.value(p) // Q)
    assert images == {-1, 0, 1}  # the three images of zero
    _same(got, c.want, c)


def check_pair_product(run):
    c = lz.pair_mul_cases()
    got = run.run("pair_mul", c.rows)
    for row, (a, b), name in zip(got, c.meta, c.names):
        a0, a1, b0, b1 = lz.value(a[0]), lz.value(a[1]), lz.value(b[0]), lz.value(b[1])
        r0, r1 = _ints(row[0:13]), _ints(row[53:66])
        assert (lz.value(r0) * R - (a0 * b0 - 5 * a1 * b1)) % Q == 0 and (lz.value(r1) * R - (a0 * b1 + a1 * b0)) % Q == 0, ("pair product", name)
        for r in (r0, r1):
            _normalised_in(r, lz.PAIR_PROD, "pair product", name)
        # what the exchange must have left: even lane X = a0, Y = -a1, recv = 5 b1; odd lane X = a0, Y = a1, recv = (b0, 0)
        assert _ints(row[13:26]) == a[0] and _ints(row[26:39]) == [-x for x in a[1]], ("even lane's a operand", name)
        assert _ints(row[66:79]) == a[0] and _ints(row[79:92]) == a[1], ("odd lane's a operand", name)
        e_recv, o_recv = _ints(row[39:53]), _ints(row[92:106])
        assert sum(x << (LIMB * i) for i, x in enumerate(e_recv)) == 5 * b1 and all(0 <= x <= FULL for x in e_recv[:13]), ("even lane's received b", name)
        assert o_recv == b[0] + [0], ("odd lane's received b", name)
    _same(got, c.want, c)


def _pair_acc(words):
    v = [_ints(words[13 * i : 13 * i + 13]) for i in range(8)]
    return lz.PairAcc([v[0], v[1]], [v[2], v[3]], [v[4], v[5]], [v[6], v[7]], int(words[104]) != 0)


def _fq2_product_exact(a, b):
    """the integers the two lanes return for a * b: (S_c - M_c q) / 2^406"""
    a0, a1, b0, b1 = lz.value(a[0]), lz.value(a[1]), lz.value(b[0]), lz.value(b[1])
    out = []
    for s in (a0 * b0 - 5 * a1 * b1, a0 * b1 + a1 * b0):
        out.append((s - s * lz.QINV % R * Q) // R)
    return out


def check_pair_madd(run):
    """-> {path: count}"""
    c = lz.pair_madd_cases()
    cases, infos = c.meta
    got = run.run("pair_madd", c.rows)
    paths, images, lows, pzs, rzs = {}, set(), set(), set(), set()
    for row, cs, info, name in zip(got, cases, infos, c.names):
        out = _pair_acc(row)
        b = cs.b_pt if not cs.negate else (cs.b_pt[0], ((-cs.b_pt[1][0]) % Q, (-cs.b_pt[1][1]) % Q))
        if cs.acc.inf:
            assert not out.inf and lz.g2_decode(out) == b, name
            paths["restart"] = paths.get("restart", 0) + 1
            continue
        a = lz.g2_decode(cs.acc)
        assert a == cs.a_pt, name
        ny = [lz.value(cs.py[k]) if not cs.negate else Q - lz.value(cs.py[k]) for k in range(2)]
        u2 = _fq2_product_exact(cs.acc.zz, cs.px)
        s2 = _fq2_product_exact(cs.acc.zzz, [lz.norm(ny[0]), lz.norm(ny[1])])
        p = [u2[k] - lz.value(cs.acc.x[k]) + Q for k in range(2)]
        r = [s2[k] - lz.value(cs.acc.y[k]) + Q for k in range(2)]
        p_zero, r_zero = all(v % Q == 0 for v in p), all(v % Q == 0 for v in r)
        assert p_zero == (a[0] == b[0]) and (not p_zero or r_zero == (a[1] == b[1])), name
        low = tuple((((v + 1) & FULL) <= 2) for v in p)
        lows.add(low + (p_zero,))
        pzs.add(tuple(v % Q == 0 for v in p))
        if p_zero:
            images.add(tuple(v // Q for v in p))
            rzs.add(tuple(v % Q == 0 for v in r))
        path = "double" if p_zero and r_zero else "inf" if p_zero else "add"
        paths[path] = paths.get(path, 0) + 1
        assert info["path"] == path, name
        if path == "inf":
            assert out.inf, ("P = 0 and R != 0 in Fq2 must give the point at infinity", name)
            continue
        assert not out.inf, ("the point at infinity without P = 0, R != 0", name)
        assert lz.g2_decode(out) == pyref.g2_add(a, b), ("wrong group element", path, name)
        for k in range(2):
            for l, what in ((out.x[k], "x"), (out.y[k], "y")):
                assert lz.is_tight(l) and -lz.NK * Q < lz.value(l) < (1 + lz.NK) * Q, ("pair madd", what, "outside [0, 1] +- 2^-19", name)
            _normalised_in(out.zz[k], lz.PAIR_PROD, "pair madd zz", name)
            _normalised_in(out.zzz[k], lz.PAIR_PROD, "pair madd zzz", name)
    # the images of a zero P per lane; the filter agreeing on one lane only and on both without P = 0; the exact test agreeing on one lane only; R = 0 on one lane only
    assert {(0, 0), (-1, 0), (0, -1), (-1, -1), (0, 1)} <= images, images  # (image q on the even lane: not constructible, see lazy_cases.py)
    assert {(True, False, False), (False, True, False), (True, True, False), (True, True, True)} <= lows, lows
    assert {(True, False), (False, True), (True, True), (False, False)} <= pzs, pzs
    assert {(True, True), (False, False), (True, False), (False, True)} <= rzs, rzs
    assert set(paths) == {"restart", "add", "double", "inf"}, paths
    _same(got, c.want, c)
    return paths


def peak_report():
    """the largest partial column sum the legality replay met, per routine, as log2"""
    import math

    return {k: round(math.log2(v), 2) for k, v in sorted(lz.PEAK.items()) if v}
