"""Operands for the lazily reduced signed-limb arithmetic of the bucket-accumulation loops (snarkvm_amd/csrc/ffl.hip.h, ffl2.hip.h, ffl2p.hip.h) at the
ends of the ranges the routines' comments state, with a Python-integer model of every routine.  Shared by tests/test_lazy_edges_host.py (CPU) and
tests/test_gpu_lazy_edges.py through tests/helpers/lazy_edge_checks.py.

A value is 13 signed limbs, value(l) = sum l_i 2^(29 i); "normalised": l_0 .. l_11 in [0, 2^29), l_12 a signed 32-bit word.  A normalised value has one
limb image, so a routine that returns a normalised value is pinned by the INTEGER it returns:
    mul / sqr            (a b - M q) / 2^406,  M = a b / q mod 2^406  in [0, 2^406)        ->  (a b / 2^406 - q, a b / 2^406]
    diff_of_products     (a b - c d + M q) / 2^406,  M = -(a b - c d) / q mod 2^406        ->  [X / 2^406, X / 2^406 + q)
The model REPLAYS every column sum of the C++ (the same order of the terms) and raises Finding when a partial sum leaves the signed 64-bit range or a
word leaves 32 bits; IllegalCase when an operand is outside the precondition stated here - that is a mistake of this file.  PEAK records the largest
partial sum per routine.

Preconditions (units of q; e = 2^-26), from the comments of the three headers and from what the addition laws feed the routines:
    fql_t::mul          normalised x normalised or normalised x difference; normalised: within X_RNG (the widest normalised operand, the accumulator's x);
                        difference: limbs 0 .. 11 in (-2^29, 2^29), value within P_RNG (P = U2 - X1, Q - X3)
    fql_t::sqr          a normalised value within X_RNG or a difference within P_RNG (the top limb reaches -3.5 * 2^29)
    diff_of_products    a: difference within R_RNG (R = S2 - Y1), b: difference within P_RNG, c: normalised within Y_RNG, d: normalised within PROD_RNG
    normalized          every limb below 2^31 - 2^3 in magnitude
    to_exact, raw image normalised (the signed 32-bit top limb: below 4.76 q in magnitude)
    from_exact          a canonical residue
    fqz_t               normalised operands whose exact results fit the signed top limb; is_zero: any normalised value
    xyzz_lazy_t::madd   x within X_RNG, y within Y_RNG, zz / zzz within ZZ_RNG, all normalised; px, py canonical residues
    pair product        both components of both operands tight: normalised, every limb below 2^29 in magnitude
    pair madd           x, y components within [0, 1 + 2 e], zz / zzz components within (-1 - e, e) or the canonical one, px, py canonical

CPU only: numpy and Python integers."""
import collections
import functools
import itertools
import random
from fractions import Fraction as Fr

import numpy as np

from oracle import pyref

Q = pyref.Q_MOD
LIMB, N, STEPS = 29, 13, 14
FULL = (1 << LIMB) - 1
RBITS = LIMB * STEPS
R = 1 << RBITS
RQ = R % Q
RINV = pow(R, -1, Q)
QINV = pow(Q, -1, R)
I64, I32 = 1 << 63, 1 << 31
TOP = LIMB * (N - 1)  # bit position of the top limb
QL = [(Q >> (LIMB * i)) & FULL for i in range(N)]
E = Fr(1, 1 << 26)
NK = Fr(1, 1 << 19)  # norm_k: the quotient comes from three single-precision roundings (2^-24 each) of a ratio below 8: 24 * 2^-24 < 2^-19

X_RNG = (Fr(-11, 10), Fr(31, 10))
Y_RNG = (Fr(-1), Fr(101, 100))  # a first addition with negate leaves -py in (-q, 0]
ZZ_RNG = (Fr(-101, 100), Fr(1))  # products, and the canonical 2^406 mod q that a first addition leaves in zz and zzz
PROD_RNG = (Fr(-1002, 1000), Fr(2, 1000))
DOP_RNG = (Fr(-2, 1000), Fr(1002, 1000))
P_RNG = (Fr(-42, 10), Fr(12, 10))
R_RNG = (Fr(-202, 100), Fr(101, 100))
X3_RNG = (Fr(-101, 100), Fr(301, 100))
PAIR_XY = (Fr(0), 1 + 2 * E)       # closed
PAIR_PROD = (-1 - E, E)            # open
PAIR_ZZ = (-1 - E, Fr(1))          # a raw product, or the canonical (2^406 mod q, 0) that a first addition leaves

OPS = {"mul": 0, "sqr": 1, "dop": 2, "normalized": 3, "to_exact": 4, "from_exact": 5, "raw": 6, "fqz": 7, "madd": 8, "pair_help": 9, "pair_mul": 10,
       "pair_madd": 11}
IN_WORDS = {0: 26, 1: 13, 2: 52, 3: 13, 4: 13, 5: 13, 6: 13, 7: 39, 8: 80, 9: 65, 10: 52, 11: 158}
OUT_WORDS = {0: 13, 1: 13, 2: 13, 3: 13, 4: 13, 5: 13, 6: 25, 7: 53, 8: 54, 9: 66, 10: 106, 11: 105}


class Finding(AssertionError):
    """a case inside the stated precondition overflows a column, a word, or leaves the promised range"""


class IllegalCase(AssertionError):
    """an operand outside the precondition: a mistake of this helper"""


def legal(cond, *what):
    if not cond:
        raise IllegalCase(what)


def fits(cond, *what):
    if not cond:
        raise Finding(what)


# ---- limbs
def value(l):
    return sum(int(x) << (LIMB * i) for i, x in enumerate(l))


def norm(v):
    top = v >> TOP
    fits(-I32 <= top < I32, "top limb leaves 32 bits", v)
    return [(v >> (LIMB * i)) & FULL for i in range(N - 1)] + [top]


def is_normalised(l):
    return len(l) == N and all(0 <= int(x) <= FULL for x in l[: N - 1]) and -I32 <= int(l[N - 1]) < I32


def inside(v, rng):
    return rng[0] * Q < v < rng[1] * Q


def inside_closed(v, rng):
    return rng[0] * Q <= v <= rng[1] * Q


def is_difference(l):
    return len(l) == N and all(-FULL <= int(x) <= FULL for x in l[: N - 1]) and -I32 <= int(l[N - 1]) < I32


def is_tight(l):
    return is_normalised(l) and abs(int(l[N - 1])) <= FULL


K377, K435, ONE = norm(pow(2, 377, Q)), norm(pow(2, 435, Q)), norm(RQ)
PEAK = {}


# ---- the column sums
def _reduce(name, col, add_q=False):
    """col(k): the product terms of column k in the routine's order.  -> (limbs, M)"""
    m, r, acc, lo, hi = [], [], 0, 0, 0
    for k in range(N + STEPS):
        terms = col(k)
        s = 1 if add_q else -1
        terms += [s * m[i] * QL[k - i] for i in range(min(k, STEPS)) if 1 <= k - i < N]
        for t in terms:
            acc += t
            if acc > hi:
                hi = acc
            elif acc < lo:
                lo = acc
        if k < STEPS:
            if add_q:
                mk = (-acc) & FULL
                acc += mk
                hi = max(hi, acc)
            else:
                mk = acc & FULL
            m.append(mk)
        elif k == N + STEPS - 1:
            fits(-I32 <= acc < I32, name, "the last column leaves 32 bits", acc)
            r.append(acc)
        else:
            r.append(acc & FULL)
        acc >>= LIMB
    fits(-I64 <= lo and hi < I64, name, "a column sum leaves 64 bits", lo, hi)
    PEAK[name] = max(PEAK.get(name, 0), hi, -lo)
    return r, value(m)


def m_mul(a, b, name="mul"):
    r, M = _reduce(name, lambda k: [a[i] * b[k - i] for i in range(N) if 0 <= k - i < N])
    assert value(r) * R == value(a) * value(b) - M * Q and M == value(a) * value(b) * QINV % R
    return r


def m_sqr(a):
    for i in range(N - 1):
        fits(-I32 <= 2 * a[i] < I32, "sqr", "a doubled limb leaves 32 bits", i, a[i])

    def col(k):
        t = []
        for i in range(N):
            j = k - i
            if i < j < N:
                t.append(2 * a[i] * a[j])
            if j == i:
                t.append(a[i] * a[i])
        return t

    r, M = _reduce("sqr", col)
    assert value(r) * R == value(a) ** 2 - M * Q
    return r


def m_dop(a, b, c, d):
    def col(k):
        t = []
        for i in range(N):
            j = k - i
            if 0 <= j < N:
                t += [a[i] * b[j], -c[i] * d[j]]
        return t

    r, M = _reduce("diff_of_products", col, add_q=True)
    assert value(r) * R == value(a) * value(b) - value(c) * value(d) + M * Q
    return r


def _carry(name, t, top_extra=0):
    """the 32-bit carry chain every normalisation runs: t (13 limb sums) -> normalised limbs"""
    r, c = [], 0
    for i in range(N - 1):
        x = t[i] + c
        fits(-I32 <= x < I32, name, "a carry step leaves 32 bits", i, x)
        r.append(x & FULL)
        c = x >> LIMB
    x = t[N - 1] + c
    fits(-I32 <= x < I32, name, "the top limb leaves 32 bits", x)
    return r + [x]


def m_normalized(a, name="normalized"):
    for x in a:
        fits(-I32 <= x < I32, name, "a limb sum leaves 32 bits", x)
    return _carry(name, list(a))


def m_to_exact(a):
    """-> the 13 limbs of the canonical fq_t"""
    t = m_mul(a, K377, "to_exact")
    for _ in range(3):
        if t[N - 1] >= 0:
            break
        t = _carry("to_exact", [x + y for x, y in zip(t, QL)])
    v = value(t)
    fits(0 <= v < 2 * Q, "to_exact", "not within [0, 2 q) before the conditional subtraction", v)
    v -= Q if v >= Q else 0
    return [(v >> (LIMB * i)) & FULL for i in range(N)]


def m_from_exact(a_limbs):
    return m_mul(list(a_limbs), K435, "from_exact")


def m_store_raw(a):
    return [(value(a) % (1 << 384) >> (32 * j)) & 0xFFFFFFFF for j in range(12)]


def sub(a, b):
    return [x - y for x, y in zip(a, b)]


def add(a, b):
    return [x + y for x, y in zip(a, b)]


def negate_if(a, s):
    return [-x for x in a] if s else list(a)


def m_fqz_is_zero(a):
    if not any(a):
        return True
    if ((a[0] + 8) & FULL) > 16:
        return False
    return not any(m_to_exact(a))


G1Acc = collections.namedtuple("G1Acc", "x y zz zzz inf")


def m_madd(acc, px, py, negate):
    """-> (returned bool, G1Acc, low limb of P or None)"""
    legal(is_normalised(px) and 0 <= value(px) < Q and is_normalised(py) and 0 <= value(py) < Q, "base not canonical")
    if acc.inf:
        return True, G1Acc(list(px), m_normalized(negate_if(py, negate), "madd"), ONE, ONE, False), None
    for l, rng, what in ((acc.x, X_RNG, "x"), (acc.y, Y_RNG, "y"), (acc.zz, ZZ_RNG, "zz"), (acc.zzz, ZZ_RNG, "zzz")):
        legal(is_normalised(l) and inside(value(l), rng), "accumulator", what)
    u2 = m_mul(px, acc.zz, "madd.mul")
    s2 = m_mul(negate_if(py, negate), acc.zzz, "madd.mul")
    p, r = sub(u2, acc.x), sub(s2, acc.y)
    fits(inside(value(p), P_RNG) and inside(value(r), R_RNG), "madd", "P or R outside its range")
    if ((p[0] + 4) & FULL) <= 5:
        return False, acc, p[0]
    pp = m_sqr(p)
    ppp = m_mul(p, pp, "madd.mul")
    q = m_mul(acc.x, pp, "madd.mul")
    rr = m_sqr(r)
    x3 = _carry("madd.x3", [a - b - 2 * c for a, b, c in zip(rr, ppp, q)])
    y3 = m_dop(r, sub(q, x3), acc.y, ppp)
    return True, G1Acc(x3, y3, m_mul(acc.zz, pp, "madd.mul"), m_mul(acc.zzz, ppp, "madd.mul"), False), p[0]


# ---- the pair (ffl2.hip.h, ffl2p.hip.h): a value is [c0 limbs, c1 limbs]
def m_times5(b):
    o, c = [], 0
    for i in range(N - 1):
        x = 5 * (b[i] & 0xFFFFFFFF) + c
        fits(x < 1 << 32, "times5", "a limb leaves 32 bits")
        o.append(x & FULL)
        c = x >> LIMB
    t = 5 * b[N - 1] + c
    return o + [t & FULL, t >> LIMB]


def m_prep(a, b):
    """-> per lane (X, Y, own, recv) as pair_ops::prep_a / prep_b leave them"""
    send_a = [list(a[0]), [-x for x in a[1]]]
    send_b = [list(b[0]) + [0], m_times5(b[1])]
    return [(list(a[0]), send_a[1], list(b[0]), send_b[1]), (send_a[0], list(a[1]), list(b[1]), send_b[0])]


def m_mul_core(X, Y, own, recv, name):
    def col(k):
        t = []
        for i in range(N):
            j = k - i
            if 0 <= j < N:
                t.append(X[i] * own[j])
            if 0 <= j <= N:
                t.append(Y[i] * recv[j])
        return t

    r, M = _reduce(name, col)
    assert value(r) * R == value(X) * value(own) + value(Y) * value(recv) - M * Q
    return r


def m_pair_mul(a, b):
    for v in (a[0], a[1], b[0], b[1]):
        legal(is_tight(v), "pair product operand not tight", v)
    lanes = m_prep(a, b)
    return [m_mul_core(*lanes[0], "pair.even"), m_mul_core(*lanes[1], "pair.odd")]


def m_sub_norm(a, b, addq):
    if addq < 0:
        addq = 1 if a[N - 1] - b[N - 1] < 0 else 0
    return _carry("sub_norm", [x - y + addq * ql for x, y, ql in zip(a, b, QL)])


def m_norm_k(t):
    kf = np.floor(np.float32(t[N - 1]) * (np.float32(1.0) / np.float32(QL[N - 1])))
    k = -int(kf)
    r, c = [], 0
    for i in range(N - 1):
        x = t[i] + k * QL[i] + c
        r.append(x & FULL)
        c = x >> LIMB
    x = t[N - 1] + k * QL[N - 1] + c
    fits(-I32 <= x < I32, "norm_k", "the top limb leaves 32 bits", x)
    return r + [x]


def m_cond_neg(y, neg):
    return _carry("cond_neg_canonical", [ql - x for x, ql in zip(y, QL)]) if neg else _carry("cond_neg_canonical", list(y))


def m_is_zero_mod_q(v):
    return v in (norm(0), norm(Q), norm(-Q))


PairAcc = collections.namedtuple("PairAcc", "x y zz zzz inf")
ONE2 = [ONE, norm(0)]


def _pmul(a, b):
    return m_pair_mul(a, b)


def m_pair_mdbl(px, ny):
    u = [_carry("mdbl.u", [2 * y - ql for y, ql in zip(ny[l], QL)]) for l in range(2)]
    v = _pmul(u, u)
    w = _pmul(u, v)
    s = _pmul(px, v)
    xx = _pmul(px, px)
    m = [m_norm_k([3 * x for x in xx[l]]) for l in range(2)]
    mm = _pmul(m, m)
    x3 = [m_norm_k([a - 2 * b for a, b in zip(mm[l], s[l])]) for l in range(2)]
    d = [m_sub_norm(s[l], x3[l], 1) for l in range(2)]
    a = _pmul(m, d)
    b = _pmul(w, ny)
    return PairAcc(x3, [m_sub_norm(a[l], b[l], -1) for l in range(2)], v, w, False)


def m_pair_madd(acc, px, py, negate):
    """-> (PairAcc, info): info = {"low": per-lane filter flags, "pz": ..., "rz": ..., "path": "restart" | "add" | "double" | "inf"}"""
    for c in range(2):
        legal(is_normalised(px[c]) and 0 <= value(px[c]) < Q and is_normalised(py[c]) and 0 <= value(py[c]) < Q, "base not canonical")
    ny = [m_cond_neg(py[c], negate) for c in range(2)]
    if acc.inf:
        return PairAcc([list(px[0]), list(px[1])], ny, ONE2[:], ONE2[:], False), {"path": "restart"}
    for c in range(2):
        legal(is_normalised(acc.x[c]) and inside_closed(value(acc.x[c]), PAIR_XY) and is_normalised(acc.y[c]) and inside_closed(value(acc.y[c]), PAIR_XY), "pair x / y")
        legal(is_normalised(acc.zz[c]) and inside(value(acc.zz[c]), PAIR_ZZ) and is_normalised(acc.zzz[c]) and inside(value(acc.zzz[c]), PAIR_ZZ), "pair zz / zzz")
    u2 = _pmul(acc.zz, px)
    s2 = _pmul(acc.zzz, ny)
    p = [m_sub_norm(u2[l], acc.x[l], 1) for l in range(2)]
    r = [m_sub_norm(s2[l], acc.y[l], 1) for l in range(2)]
    low = [((p[l][0] + 1) & FULL) <= 2 for l in range(2)]
    info = {"low": low, "pz": [m_is_zero_mod_q(p[l]) for l in range(2)], "rz": [m_is_zero_mod_q(r[l]) for l in range(2)], "p": p, "r": r}
    if all(low) and all(info["pz"]):
        if all(info["rz"]):
            info["path"] = "double"
            return m_pair_mdbl(px, ny), info
        info["path"] = "inf"
        return PairAcc(acc.x, acc.y, acc.zz, acc.zzz, True), info
    info["path"] = "add"
    pp = _pmul(p, p)
    ppp = _pmul(p, pp)
    q = _pmul(acc.x, pp)
    zz = _pmul(acc.zz, pp)
    zzz = _pmul(acc.zzz, ppp)
    b = _pmul(acc.y, ppp)
    rr = _pmul(r, r)
    x3 = [m_norm_k([x - y - 2 * z for x, y, z in zip(rr[l], ppp[l], q[l])]) for l in range(2)]
    d = [m_sub_norm(q[l], x3[l], 1) for l in range(2)]
    a = _pmul(r, d)
    return PairAcc(x3, [m_sub_norm(a[l], b[l], -1) for l in range(2)], zz, zzz, False), info


# ---- decoding an accumulator as the affine point it stands for (the 2^406 factors cancel in x / zz and y / zzz)
def g1_decode(acc):
    if acc.inf:
        return None
    x, y, zz, zzz = (value(l) % Q for l in (acc.x, acc.y, acc.zz, acc.zzz))
    assert zz and pow(zz * RINV, 3, Q) == pow(zzz * RINV, 2, Q), "zz^3 != zzz^2"
    return (x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q)


def fq2_pow(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = pyref.fq2_mul(r, r)
        if bit == "1":
            r = pyref.fq2_mul(r, a)
    return r


def g2_decode(acc):
    if acc.inf:
        return None
    x, y, zz, zzz = (tuple(value(l[c]) % Q for c in range(2)) for l in (acc.x, acc.y, acc.zz, acc.zzz))
    unr = lambda v: (v[0] * RINV % Q, v[1] * RINV % Q)
    assert zz != (0, 0) and fq2_pow(unr(zz), 3) == fq2_pow(unr(zzz), 2), "zz^3 != zzz^2"
    return (pyref.fq2_mul(x, pyref.fq2_inv(zz)), pyref.fq2_mul(y, pyref.fq2_inv(zzz)))


def g1_from_x(x):
    y = pyref.fq_sqrt((x * x * x + pyref.G1_B) % Q)
    return None if y is None else (x % Q, y)


def g2_from_x(x):
    y = pyref.fq2_sqrt(pyref.fq2_add(pyref.fq2_mul(pyref.fq2_mul(x, x), x), pyref.G2_B))
    return None if y is None else ((x[0] % Q, x[1] % Q), y)


def fq_cbrt(a):
    """q = 7 (mod 9): a cube root of a cubic residue is a^((q + 2) / 9)"""
    a %= Q
    r = pow(a, (Q + 2) // 9, Q)
    return r if pow(r, 3, Q) == a else None


def fq2_cbrt(a):
    """3 divides q^2 - 1 once: with q^2 - 1 = 3 m, a cubic residue has an order dividing m and a^(1 / 3 mod m) is a cube root"""
    m = (Q * Q - 1) // 3
    r = fq2_pow(a, pow(3, -1, m))
    return r if fq2_pow(r, 3) == (a[0] % Q, a[1] % Q) else None


# ---- operand lists
def _low_patterns():
    return [("ones", [FULL] * 12), ("0/full", [0 if i % 2 == 0 else FULL for i in range(12)]), ("full/0", [FULL if i % 2 == 0 else 0 for i in range(12)]),
            ("zeros", [0] * 12)]


def norm_values(rng, ks=None):
    """[(name, limbs)]: normalised values within the open range: k q +- 1 and k q +- 2^348 for every k, the two ends, the limb patterns under a top limb
    at both ends of its range and around zero"""
    lo, hi = rng
    out = []
    klo, khi = -((-lo.numerator) // lo.denominator) - 1, hi.numerator // hi.denominator + 1
    for k in range(klo, khi + 1) if ks is None else ks:
        for name, eps in (("", 0), ("+1", 1), ("-1", -1), ("+2^348", 1 << TOP), ("-2^348", -(1 << TOP))):
            out.append((f"{k}q{name}", k * Q + eps))
    lo_v, hi_v = (lo * Q).__floor__() + 1, (hi * Q).__ceil__() - 1
    out += [("low end", lo_v), ("high end", hi_v)]
    tops = sorted({lo_v >> TOP, (lo_v >> TOP) + 1, -1, 0, (hi_v >> TOP) - 1, hi_v >> TOP})
    for pname, low in _low_patterns():
        for top in tops:
            out.append((f"{pname} under top {top:#x}", value(low + [top])))
    seen, kept = set(), []
    for name, v in out:
        if inside(v, rng) and v not in seen:
            seen.add(v)
            kept.append((name, norm(v)))
    return kept


def diff_values(rng):
    """[(name, limbs)]: limbs of +-(2^29 - 1) in every sign pattern that matters, under a top limb at both ends of the range; then k q +- 1 normalised.
    The extremes come first."""
    lo, hi = rng
    lo_v, hi_v = (lo * Q).__floor__() + 1, (hi * Q).__ceil__() - 1
    pats = [("+full", [FULL] * 12), ("-full", [-FULL] * 12), ("+-full", [FULL if i % 2 == 0 else -FULL for i in range(12)]),
            ("-+full", [-FULL if i % 2 == 0 else FULL for i in range(12)]), ("zeros", [0] * 12)]
    out = []
    for top in ((lo_v >> TOP) + 1, (hi_v >> TOP) - 1, -FULL, FULL, 0):
        for name, low in pats:
            out.append((f"{name} under top {top:#x}", low + [top]))
    klo, khi = -((-lo.numerator) // lo.denominator), hi.numerator // hi.denominator
    for k in range(klo, khi + 1):
        out += [(f"{k}q+1", norm(k * Q + 1)), (f"{k}q-1", norm(k * Q - 1))]
    kept, seen = [], set()
    for name, l in out:
        if inside(value(l), rng) and is_difference(l) and tuple(l) not in seen:
            seen.add(tuple(l))
            kept.append((name, l))
    return kept


def random_normalised(rng, rand, n):
    lo_v, hi_v = (rng[0] * Q).__floor__() + 1, (rng[1] * Q).__ceil__() - 1
    return [(f"random {i}", norm(rand.randrange(lo_v, hi_v + 1))) for i in range(n)]


def random_difference(rng, rand, n):
    out = []
    lo_v, hi_v = (rng[0] * Q).__floor__() + 1, (rng[1] * Q).__ceil__() - 1
    while len(out) < n:
        b = [rand.choice((0, FULL, rand.randrange(FULL + 1))) for _ in range(12)] + [0]
        l = sub(norm(rand.randrange(lo_v, hi_v + 1) + value(b)), b)  # a difference of two normalised values: limbs spread over (-2^29, 2^29)
        if is_difference(l) and inside(value(l), rng):
            out.append((f"random difference {len(out)}", l))
    return out


def interleave(*classes):
    """round robin over the classes, so that neighbouring lanes (and lane pairs) of a wave hold cases of different classes"""
    out = []
    for group in itertools.zip_longest(*classes):
        out += [c for c in group if c is not None]
    return out


def rows(records):
    a = np.array(records, dtype=np.int64)
    assert a.min() >= -I32 and a.max() < I32
    a = a.astype(np.int32)
    a.setflags(write=False)
    return a


Cases = collections.namedtuple("Cases", "op rows names want meta")


@functools.lru_cache(maxsize=None)
def mul_cases():
    rand = random.Random(0x406)
    nx = norm_values(X_RNG) + random_normalised(X_RNG, rand, 8)
    df = diff_values(P_RNG) + random_difference(P_RNG, rand, 8)
    pairs = [(a, b) for a in nx for b in nx] + [(a, b) for a in nx for b in df] + [(a, b) for a in df for b in nx]
    for (_, a), (_, b) in pairs:
        legal((is_normalised(a) and inside(value(a), X_RNG) and (is_normalised(b) or is_difference(b)))
              or (is_normalised(b) and inside(value(b), X_RNG) and is_difference(a)), "mul operands")
    want = [m_mul(a, b) for (_, a), (_, b) in pairs]
    return Cases("mul", rows([a + b for (_, a), (_, b) in pairs]), [f"({x}) * ({y})" for (x, _), (y, _) in pairs], rows(want), pairs)


@functools.lru_cache(maxsize=None)
def sqr_cases():
    rand = random.Random(0x5C2)
    vals = norm_values(X_RNG) + diff_values(P_RNG) + random_normalised(X_RNG, rand, 600) + random_difference(P_RNG, rand, 1200)
    vals = interleave(vals[: len(vals) // 2], vals[len(vals) // 2:])
    want = [m_sqr(a) for _, a in vals]
    assert min(a[N - 1] for _, a in vals) <= -int(3.4 * (1 << LIMB))  # the top limb the comment of sqr names
    return Cases("sqr", rows([a for _, a in vals]), [n for n, _ in vals], rows(want), vals)


@functools.lru_cache(maxsize=None)
def dop_cases():
    rand = random.Random(0xD09)
    da = diff_values(R_RNG)[:10] + random_difference(R_RNG, rand, 1)
    db = diff_values(P_RNG)[:10] + random_difference(P_RNG, rand, 1)
    nc = [v for v in norm_values(Y_RNG) if v[0] in ("low end", "high end", "0q", "1q+1", "0q-1") or v[0].startswith(("ones", "0/full"))][:7]
    nd = [v for v in norm_values(PROD_RNG) if v[0] in ("low end", "high end", "0q", "-1q-1", "0q-1") or v[0].startswith(("ones", "full/0"))][:7]
    quads = [(a, b, c, d) for a in da for b in db for c in nc for d in nd]
    for q in quads:
        a, b, c, d = (l for _, l in q)
        legal(is_difference(a) and inside(value(a), R_RNG) and is_difference(b) and inside(value(b), P_RNG), "dop a, b")
        legal(is_normalised(c) and inside(value(c), Y_RNG) and is_normalised(d) and inside(value(d), PROD_RNG), "dop c, d")
    want = [m_dop(*(l for _, l in q)) for q in quads]
    return Cases("dop", rows([sum((l for _, l in q), []) for q in quads]), [" , ".join(n for n, _ in q) for q in quads], rows(want), quads)


@functools.lru_cache(maxsize=None)
def normalized_cases():
    rand = random.Random(0x9012)
    big = I32 - 9
    vals = [("all +max", [big] * N), ("all -max", [-big] * N), ("+-max", [big if i % 2 == 0 else -big for i in range(N)]),
            ("-+max", [-big if i % 2 == 0 else big for i in range(N)]), ("zeros", [0] * N), ("all -1", [-1] * N), ("all full", [FULL] * N),
            ("carry through every limb", [FULL + 1] + [FULL] * 11 + [0]), ("borrow through every limb", [-1] + [0] * 12)]
    for i in range(1500):
        vals.append((f"random {i}", [rand.choice((big, -big, 0, FULL, -FULL, rand.randrange(-big, big + 1))) for _ in range(N)]))
    for _, l in vals:
        legal(all(abs(x) < I32 - 8 for x in l), "normalized operand")
    want = [m_normalized(l) for _, l in vals]
    return Cases("normalized", rows([l for _, l in vals]), [n for n, _ in vals], rows(want), vals)


def _wide_normalised(rand, n_random):
    """normalised values over the whole signed top limb: k q +- 1 for |k| <= 4, the patterns under the extreme top limbs"""
    vals = [(f"{k}q{n}", norm(k * Q + eps)) for k in range(-4, 5) for n, eps in (("", 0), ("+1", 1), ("-1", -1))]
    for pname, low in _low_patterns():
        for top in (-I32, -I32 + 1, -FULL - 1, -1, 0, FULL, I32 - 1):
            vals.append((f"{pname} under top {top:#x}", low + [top]))
    vals += [(f"random {i}", [rand.randrange(FULL + 1) for _ in range(12)] + [rand.randrange(-I32, I32)]) for i in range(n_random)]
    return vals


@functools.lru_cache(maxsize=None)
def to_exact_cases():
    vals = _wide_normalised(random.Random(0x377), 1500)
    for _, l in vals:
        legal(is_normalised(l), "to_exact operand")
    want = [m_to_exact(l) for _, l in vals]
    return Cases("to_exact", rows([l for _, l in vals]), [n for n, _ in vals], rows(want), vals)


@functools.lru_cache(maxsize=None)
def from_exact_cases():
    from tests.helpers import limb_cases as lc

    rand = random.Random(0x435)
    vals = [(n, v) for n, v in zip(lc.cases(1).names, lc.cases(1).internal)] + [(f"random {i}", rand.randrange(Q)) for i in range(1500)]
    limbs = [[(v >> (LIMB * i)) & FULL for i in range(N)] for _, v in vals]
    want = [m_from_exact(l) for l in limbs]
    return Cases("from_exact", rows(limbs), [n for n, _ in vals], rows(want), vals)


@functools.lru_cache(maxsize=None)
def raw_cases():
    vals = _wide_normalised(random.Random(0x384), 1500)
    want = []
    for _, l in vals:
        img = m_store_raw(l)
        want.append([w - (1 << 32) if w >= I32 else w for w in img] + list(l))
    return Cases("raw", rows([l for _, l in vals]), [n for n, _ in vals], rows(want), vals)


FQZ_AB = (Fr(-23, 10), Fr(23, 10))


@functools.lru_cache(maxsize=None)
def fqz_cases():
    """a, b: every ordered pair of the values within (-2.3 q, 2.3 q) (a + b, a - b and 2 a stay below the 4.76 q of the top limb), then a product against
    the widest X3 (Q - X3 reaches -4.02 q); z for is_zero: every multiple of q the top limb holds, its neighbours, 13 zero limbs, and values whose low limb
    is inside and just outside the window of the filter without being a multiple"""
    rand = random.Random(0xF92)
    ab = norm_values(FQZ_AB)
    zs = [(f"{k}q{n}", norm(k * Q + eps)) for k in range(-4, 5) for n, eps in (("", 0), ("+1", 1), ("-1", -1), ("+2^29", 1 << LIMB))]
    for low in (-9, -8, 0, 8, 9):  # the filter takes low limbs -8 .. 8
        for k in (-3, 1):
            zs.append((f"low limb {low}, near {k}q", norm(((k * Q) >> LIMB << LIMB) + (low & FULL) + (5 << LIMB))))
    zs += random_normalised((Fr(-47, 10), Fr(47, 10)), rand, 16)
    pairs = [(a, b) for a in ab for b in ab]
    pairs += [(a, b) for a in norm_values(PROD_RNG) for b in norm_values(X3_RNG)]
    recs, names, want = [], [], []
    for i, ((na, a), (nb, b)) in enumerate(pairs):
        nz, z = zs[i % len(zs)]
        legal(is_normalised(a) and is_normalised(b) and is_normalised(z), "fqz operands")
        for v in (value(a) + value(b), value(a) - value(b), 2 * value(a), -value(a)):
            legal(-I32 <= v >> TOP < I32, "fqz result does not fit the top limb")
        recs.append(a + b + z)
        names.append(f"a = {na}, b = {nb}, z = {nz}")
        want.append(m_normalized(add(a, b), "fqz") + m_normalized(sub(a, b), "fqz") + m_normalized(add(a, a), "fqz") + m_normalized([-x for x in a], "fqz")
                    + [1 if m_fqz_is_zero(z) else 0])
    assert len(pairs) >= len(zs)
    return Cases("fqz", rows(recs), names, rows(want), [(a, b, zs[i % len(zs)][1]) for i, ((_, a), (_, b)) in enumerate(pairs)])


# ---- xyzz_lazy_t::madd
def _rep(v, rng, k):
    """the representative v + k q of a residue, or None outside the range"""
    return norm(v + k * Q) if inside(v + k * Q, rng) else None


def _g1_acc_for(x_val, lam, rand, y_sign=1, ky=0, kzz=-1, kzzz=-1):
    """an accumulator with the given INTEGER x over zz = lam^2, zzz = lam^3 (times 2^406), if x / zz is the x of a curve point; None otherwise"""
    zz, zzz = lam * lam % Q * RQ % Q, pow(lam, 3, Q) * RQ % Q
    pt = g1_from_x(x_val * pow(zz, -1, Q) % Q)
    if pt is None:
        return None
    yv = (y_sign * pt[1]) % Q * pow(lam, 3, Q) % Q * RQ % Q
    reps = (_rep(yv, Y_RNG, ky) or norm(yv), _rep(zz, ZZ_RNG, kzz) or _rep(zz, ZZ_RNG, -1), _rep(zzz, ZZ_RNG, kzzz) or _rep(zzz, ZZ_RNG, -1))
    return G1Acc(norm(x_val), reps[0], reps[1], reps[2], False), (pt[0], (y_sign * pt[1]) % Q)


def _g1_base(rand):
    while True:
        pt = g1_from_x(rand.randrange(Q))
        if pt is not None:
            return pt


def _lazy_base(pt):
    return norm(pt[0] * RQ % Q), norm(pt[1] * RQ % Q)


G1Case = collections.namedtuple("G1Case", "cls name acc px py negate a_pt b_pt")


@functools.lru_cache(maxsize=None)
def madd_cases():
    """classes: ordinary (accumulator coordinates at the ends of their ranges), exceptional (P = -4 q .. q, doubling and cancellation), window (P != 0
    with a low limb at -6 .. 5), restart (an accumulator at infinity)"""
    rand = random.Random(0x6A1)
    ordinary, exceptional, window, restart = [], [], [], []

    def lam_with(pred):
        while True:
            lam = rand.randrange(2, Q)
            if pred(lam):
                return lam

    # ordinary: x at the ends of (-1.1 q, 3.1 q) and at every k q +- small; y, zz, zzz representatives at both ends of theirs
    x_targets = [("low end", (X_RNG[0] * Q).__floor__() + 1, 1), ("high end", (X_RNG[1] * Q).__ceil__() - 1, -1)]
    x_targets += [(f"{k}q{'+' if s > 0 else '-'}", k * Q + s, s) for k in range(-1, 4) for s in (1, -1)]
    for name, x0, step in x_targets:
        for rep in range(6):
            got, xv = None, x0
            # zz at the high end of its range every third case: lam^2 2^406 = 0.01 q - small needs a square
            lam = rand.randrange(2, Q)
            if rep % 3 == 2:
                t = (ZZ_RNG[1] * Q).__ceil__() - 1
                while pyref.fq_sqrt(t * RINV % Q) is None:
                    t -= 1
                lam = pyref.fq_sqrt(t * RINV % Q)
            while got is None:
                got = _g1_acc_for(xv, lam, rand, y_sign=1 if rep % 2 else -1, ky=(0, 1, -1)[rep % 3], kzz=0 if rep % 3 == 2 else -1)
                xv += step
            acc, a_pt = got
            b_pt = _g1_base(rand)
            ordinary.append(G1Case("ordinary", f"x {name} #{rep}", acc, *_lazy_base(b_pt), rep % 2 == 1, a_pt, b_pt))
    # y at both ends of its range: y = Y lam^3 2^406 -> lam^3 = y / (Y 2^406) needs a cube root
    for name, y0, step in (("y low end", (Y_RNG[0] * Q).__floor__() + 1, 1), ("y high end", (Y_RNG[1] * Q).__ceil__() - 1, -1), ("y = q + 1", Q + 1, 1),
                           ("y = -1", -1, -1), ("y = 0", 0, 1)):
        for rep in range(4):
            a_pt = _g1_base(rand)
            yv = y0
            while True:
                lam = fq_cbrt(yv * pow(a_pt[1] * RQ, -1, Q)) if yv % Q else None
                if lam:
                    break
                yv += step
            zz, zzz = lam * lam % Q * RQ % Q, pow(lam, 3, Q) * RQ % Q
            xr = a_pt[0] * lam * lam % Q * RQ % Q
            acc = G1Acc(_rep(xr, X_RNG, (2, -1, 0, 1)[rep]), norm(yv), _rep(zz, ZZ_RNG, -1), _rep(zzz, ZZ_RNG, -1), False)
            b_pt = _g1_base(rand)
            ordinary.append(G1Case("ordinary", f"{name} #{rep}", acc, *_lazy_base(b_pt), rep % 2 == 1, a_pt, b_pt))
    # exceptional: the accumulator is +-B over lam; x = U2 - k q so that P = k q exactly
    for k in range(-4, 2):
        for doubling in (True, False):
            for negate in (False, True):
                for rep in range(3):
                    while True:
                        b_pt = _g1_base(rand)
                        px, py = _lazy_base(b_pt)
                        lam = rand.randrange(2, Q)
                        zz = _rep(lam * lam % Q * RQ % Q, ZZ_RNG, -1)
                        u2 = value(m_mul(px, zz, "madd.mul"))
                        if inside(u2 - k * Q, X_RNG):
                            break
                    sign = (-1 if negate else 1) * (1 if doubling else -1)  # the accumulator's y against the base's
                    yv = sign * b_pt[1] % Q * pow(lam, 3, Q) % Q * RQ % Q
                    acc = G1Acc(norm(u2 - k * Q), _rep(yv, Y_RNG, (0, -1, 1)[rep]) or norm(yv), zz, _rep(pow(lam, 3, Q) * RQ % Q, ZZ_RNG, -1), False)
                    exceptional.append(G1Case("exceptional", f"P = {k}q, {'doubling' if doubling else 'cancellation'}, negate {negate} #{rep}", acc, px, py,
                                              negate, (b_pt[0], sign * b_pt[1] % Q), b_pt))
    # window: P != 0 (mod q) with a chosen low limb
    for delta in range(-6, 6):
        for rep in range(8):
            b_pt = _g1_base(rand)
            px, py = _lazy_base(b_pt)
            lam = rand.randrange(2, Q)
            zz = _rep(lam * lam % Q * RQ % Q, ZZ_RNG, -1)
            u2 = m_mul(px, zz, "madd.mul")
            got = None
            while got is None:
                xv = rand.randrange((X_RNG[0] * Q).__floor__() + 1, (X_RNG[1] * Q).__ceil__() - (1 << LIMB)) >> LIMB << LIMB | ((u2[0] - delta) & FULL)
                if (value(u2) - xv) % Q:
                    got = _g1_acc_for(xv, lam, rand, y_sign=1 if rep % 2 else -1, ky=rep % 2)
            acc, a_pt = got
            window.append(G1Case("window", f"low limb of P = {delta} #{rep}", acc, px, py, rep % 4 >= 2, a_pt, b_pt))
    for rep in range(24):
        b_pt = _g1_base(rand) if rep else (Q - 1, 0)  # y = 0: -0 stays 0
        z = norm(0)
        restart.append(G1Case("restart", f"restart #{rep}", G1Acc(z, z, z, z, True), *_lazy_base(b_pt), rep % 2 == 1, None, b_pt))
    # the second addition of a bucket: the accumulator as a first addition leaves it, (x1, +-y1, one, one)
    for rep in range(24):
        a_pt, b_pt = _g1_base(rand), _g1_base(rand)
        _, acc, _ = m_madd(restart[0].acc, *_lazy_base(a_pt), rep % 2 == 1)
        ordinary.append(G1Case("ordinary", f"second addition of a bucket #{rep}", acc, *_lazy_base(b_pt), rep % 4 >= 2, a_pt if rep % 2 == 0 else pyref.g1_neg(a_pt), b_pt))
    return _finish_madd(interleave(ordinary, exceptional, window, restart), rand)


def _finish_madd(cases, rand):
    # fill with random ordinary additions up to a few thousand lanes, the crafted cases spread among them
    filler = []
    while len(filler) < 1800 - len(cases):
        a_pt, b_pt = _g1_base(rand), _g1_base(rand)
        lam = rand.randrange(2, Q)
        xr, yr = a_pt[0] * lam * lam % Q * RQ % Q, a_pt[1] * pow(lam, 3, Q) % Q * RQ % Q
        i = len(filler)
        acc = G1Acc(_rep(xr, X_RNG, (i % 4) - 1), _rep(yr, Y_RNG, -(i % 2)), _rep(lam * lam % Q * RQ % Q, ZZ_RNG, -1), _rep(pow(lam, 3, Q) * RQ % Q, ZZ_RNG, -1), False)
        filler.append(G1Case("ordinary", f"random #{i}", acc, *_lazy_base(b_pt), i % 3 == 0, a_pt, b_pt))
    cases = interleave(cases, filler)
    recs, want = [], []
    for c in cases:
        recs.append(c.acc.x + c.acc.y + c.acc.zz + c.acc.zzz + [1 if c.acc.inf else 0] + c.px + c.py + [1 if c.negate else 0])
        ok, acc, p0 = m_madd(c.acc, c.px, c.py, c.negate)
        want.append(([1 if ok else 0] + acc.x + acc.y + acc.zz + acc.zzz + [1 if acc.inf else 0], p0))
    return Cases("madd", rows(recs), [f"{c.cls}: {c.name}" for c in cases], rows([w for w, _ in want]), (cases, [p0 for _, p0 in want]))


# ---- the pair
def tight_values():
    e_q = (2 * E * Q).__floor__()
    out = [("0", 0), ("1", 1), ("-1", -1), ("q", Q), ("-q", -Q), ("q-1", Q - 1), ("-q+1", -Q + 1), ("q+1", Q + 1), ("-q-1", -Q - 1), ("q+2e", Q + e_q), ("-q-2e", -Q - e_q),
           ("2^348", 1 << TOP), ("-2^348", -(1 << TOP))]
    for pname, low in _low_patterns()[:3]:
        for top in (QL[N - 1] - 1, 0, -1, -QL[N - 1]):
            out.append((f"{pname} under top {top:#x}", value(low + [top])))
    kept = [(n, norm(v)) for n, v in out if abs(v) <= Q + e_q]
    for _, l in kept:
        assert is_tight(l)
    return kept


@functools.lru_cache(maxsize=None)
def pair_mul_cases():
    rand = random.Random(0x2B2)
    t = tight_values()
    rnd = random_normalised((Fr(-1), Fr(1)), rand, 6)
    comps = t + rnd
    els = [(a, b) for a in (t[3], t[4], t[9], t[10]) for b in (t[3], t[4], t[9], t[10])]  # +-q and +-(q + 2 e) in both components
    els += [(comps[i], comps[(i * 7 + 3) % len(comps)]) for i in range(len(comps))] + [(comps[i], comps[i]) for i in range(0, len(comps), 3)]
    els = list({(a[0], b[0]): (a, b) for a, b in els}.values())
    assert len(els) <= 60
    pairs = [(a, b) for a in els for b in els]
    recs, want, names = [], [], []
    for a, b in pairs:
        av, bv = [a[0][1], a[1][1]], [b[0][1], b[1][1]]
        r = m_pair_mul(av, bv)
        lanes = m_prep(av, bv)
        recs.append(av[0] + av[1] + bv[0] + bv[1])
        want.append(sum((r[c] + lanes[c][0] + lanes[c][1] + lanes[c][3] for c in range(2)), []))
        names.append(f"({a[0][0]}, {a[1][0]}) * ({b[0][0]}, {b[1][0]})")
    return Cases("pair_mul", rows(recs), names, rows(want), [([a[0][1], a[1][1]], [b[0][1], b[1][1]]) for a, b in pairs])


@functools.lru_cache(maxsize=None)
def pair_help_cases():
    """a, b -> p = a - b + q (a a raw product, b within [0, 1 + 2 e]) and is_zero_mod_q(p): the images -q, 0, q among them; a, c -> a - c (+ q by the top
    limbs), both raw products; t = rr - ppp - 2 q and 3 xx as raw limb sums at every k q +- small; y canonical"""
    rand = random.Random(0x9E1)
    e_q = (E * Q).__floor__()
    prod = norm_values(PAIR_PROD) + random_normalised(PAIR_PROD, rand, 6)
    xy = [(n, norm(v)) for n, v in (("0", 0), ("1", 1), ("q-1", Q - 1), ("q", Q), ("q+1", Q + 1), ("q+2e", Q + 2 * e_q), ("2^348", 1 << TOP), ("2^348-1", (1 << TOP) - 1))]
    xy += random_normalised((Fr(0), Fr(1)), rand, 6)
    ab = [(a, b) for a in prod for b in xy]
    # P = -q, 0, q exactly and their neighbours: a - b = -2 q, -q, 0 (+- 1)
    for d in (1, e_q - 1):
        for off in (-1, 0, 1):
            ab += [(("-q+d", norm(-Q + d)), ("q+d-off", norm(Q + d - off))), (("-d", norm(-d)), ("q-d-off", norm(Q - d - off))), (("d", norm(d)), ("d-off", norm(d - off)))]
    abc = [(a, xy[j % len(xy)], c) for a in prod for j, c in enumerate(prod)]  # every (a, c), and every (a, b): prod is the longer list
    abc += [(a, b, a) for a, b in ab[len(prod) * len(xy):]]
    assert len(prod) >= len(xy)
    # raw limb sums for norm_k: three tight values combined as the addition law does, and top limbs at k q_12 -1, 0, +1 over extreme lower limbs
    ts = []
    pv = [l for _, l in prod]
    for rr in pv[:12]:
        for ppp in pv[:12]:
            for q in pv[:6]:
                ts.append(("rr - ppp - 2 q", [x - y - 2 * z for x, y, z in zip(rr, ppp, q)]))
    ts += [("3 xx", [3 * x for x in l]) for l in pv]
    big = I32 - 1
    for k in range(-7, 8):
        for d in (-1, 0, 1):
            top = k * QL[N - 1] + d
            for lname, low in (("zeros", [0] * 12), ("+max", [big] * 12), ("-max", [-big] * 12), ("full", [FULL] * 12)):
                if abs(value(low + [top])) < 8 * Q and -I32 <= top < I32:
                    ts.append((f"top {k} q12 {d:+d} over {lname}", low + [top]))
    ys = [(n, norm(v)) for n, v in (("0", 0), ("1", 1), ("q-1", Q - 1), ("2^348", 1 << TOP), ("2^348-1", (1 << TOP) - 1), ("(q-1)/2", (Q - 1) // 2))]
    ys += random_normalised((Fr(0), Fr(1)), rand, 10)
    n = max(len(abc), len(ts), len(ys))
    recs, want, names, meta = [], [], [], []
    for i in range(n):
        (na, a), (nb, b), (nc, c) = abc[i % len(abc)]
        nt, t = ts[i % len(ts)]
        ny, y = ys[i % len(ys)]
        legal(is_normalised(a) and inside(value(a), PAIR_PROD) and is_normalised(b) and inside_closed(value(b), PAIR_XY), "sub_norm(+1) operands")
        legal(is_normalised(c) and inside(value(c), PAIR_PROD), "sub_norm(-1) operands")
        legal(abs(value(t)) < 8 * Q and all(-I32 < x < I32 for x in t), "norm_k operand")
        legal(is_normalised(y) and 0 <= value(y) < Q, "cond_neg operand")
        p = m_sub_norm(a, b, 1)
        recs.append(a + b + c + t + y)
        want.append(p + m_sub_norm(a, c, -1) + m_norm_k(t) + m_cond_neg(y, True) + m_cond_neg(y, False) + [1 if m_is_zero_mod_q(p) else 0])
        names.append(f"a = {na}, b = {nb}, c = {nc}, t = {nt}, y = {ny}")
        meta.append((a, b, c, t, y))
    return Cases("pair_help", rows(recs), names, rows(want), meta)


def fq2_scale(v, s):
    return (v[0] * s % Q, v[1] * s % Q)


def _pair_rep(v, lo):
    """per component: the residue moved into the pair's product range (lo = -1: v - q) or kept (lo = 0)"""
    return [norm(v[c] + lo * Q) if v[c] else norm(0) for c in range(2)]


def _g2_base(rand, x=None):
    while True:
        pt = g2_from_x((rand.randrange(Q), rand.randrange(Q)) if x is None else x(rand))
        if pt is not None:
            return pt


def _lazy2(v):
    return [norm(v[0] * RQ % Q), norm(v[1] * RQ % Q)]


def g2_point_with_zero_y_component(comp, start=1):
    """a point of y^2 = x^3 + b' whose y has component `comp` zero: y = (t, 0) or (0, t), x = cbrt(y^2 - b')"""
    t = start
    while True:
        y = (t, 0) if comp == 1 else (0, t)
        x = fq2_cbrt(pyref.fq2_sub(pyref.fq2_mul(y, y), pyref.G2_B))
        if x is not None:
            assert pyref.g2_is_on_curve((x, y))
            return (x, y)
        t += 1


G2Case = collections.namedtuple("G2Case", "cls name acc px py negate a_pt b_pt")


def _pair_acc(x_lazy, y_pt, lam, zz_rep=-1):
    """x_lazy: the two INTEGER x components; y_pt: the affine y the accumulator stands for"""
    l2 = pyref.fq2_mul(lam, lam)
    l3 = pyref.fq2_mul(l2, lam)
    yv = fq2_scale(pyref.fq2_mul(y_pt, l3), RQ)
    return PairAcc([norm(x_lazy[0]), norm(x_lazy[1])], [norm(yv[0]), norm(yv[1])], _pair_rep(fq2_scale(l2, RQ), zz_rep), _pair_rep(fq2_scale(l3, RQ), zz_rep), False)


def _affine_x_of(x_lazy, lam):
    l2 = pyref.fq2_mul(lam, lam)
    return pyref.fq2_mul((x_lazy[0] % Q, x_lazy[1] % Q), pyref.fq2_inv(fq2_scale(l2, RQ)))


@functools.lru_cache(maxsize=None)
def pair_madd_cases():
    """classes: ordinary (x components at 0 + small, q - small, q + small), low (the low-limb filter agrees on the even lane only, on the odd lane only, on
    both, with P != 0; and a lane whose P component IS zero beside one that is not), exceptional (P = 0 in Fq2 with every constructible combination of the
    images -q, 0, q per lane; R = 0 on both lanes (doubling), on neither, on one lane only (the point at infinity)), restart"""
    rand = random.Random(0x62A)
    e2 = (2 * E * Q).__floor__()
    ordinary, low, exceptional, restart = [], [], [], []
    rl = lambda: (rand.randrange(1, Q), rand.randrange(1, Q))

    def u2_of(lam, b_pt, zz_rep=-1):
        zz = _pair_rep(fq2_scale(pyref.fq2_mul(lam, lam), RQ), zz_rep)
        return m_pair_mul(zz, _lazy2(b_pt[0]))

    def search_x(lam, pick):
        """pick() -> candidate integer x components; the first whose affine x lies on the curve"""
        while True:
            xl = pick()
            pt = g2_from_x(_affine_x_of(xl, lam))
            if pt is not None:
                return xl, pt

    # ordinary
    ends = [("0+", lambda: rand.randrange(0, 1 << 40)), ("q-", lambda: Q - 1 - rand.randrange(0, 1 << 40)), ("q+", lambda: Q + rand.randrange(0, e2 + 1)),
            ("q+2e-", lambda: Q + e2 - rand.randrange(0, 1 << 20)), ("any", lambda: rand.randrange(Q))]
    for (n0, f0), (n1, f1) in itertools.product(ends, ends):
        for rep in range(2):
            lam = rl()
            xl, a_pt = search_x(lam, lambda: (f0(), f1()))
            if rep:
                a_pt = (a_pt[0], (Q - a_pt[1][0], Q - a_pt[1][1]))
                a_pt = (a_pt[0], (a_pt[1][0] % Q, a_pt[1][1] % Q))
            b_pt = _g2_base(rand)
            ordinary.append(G2Case("ordinary", f"x.c0 {n0}, x.c1 {n1} #{rep}", _pair_acc(xl, a_pt[1], lam), _lazy2(b_pt[0]), _lazy2(b_pt[1]), rep == 1, a_pt, b_pt))
    # low-limb agreement without P = 0
    for w0, w1 in [(w, None) for w in (-1, 0, 1)] + [(None, w) for w in (-1, 0, 1)] + [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)] + [(-2, 0), (0, 2), (2, -2), ("zero", None),
                                                                                                                                       (None, "zero"), ("zero", 1), (-1, "zero")]:
        for rep in range(3):
            lam, b_pt = rl(), _g2_base(rand)
            u2 = u2_of(lam, b_pt)

            def comp(c, w):
                if w == "zero":  # this component of P is exactly zero (image 0): x_c = U2_c + q
                    return value(u2[c]) + Q
                v = rand.randrange(Q - (1 << 30)) >> LIMB << LIMB
                return v if w is None else v | ((u2[c][0] + 1 - w) & FULL)  # P_c = U2_c - x_c + q, q = 1 (mod 2^29)

            xl, a_pt = search_x(lam, lambda: (comp(0, w0), comp(1, w1)))
            low.append(G2Case("low", f"low limbs of P: {w0}, {w1} #{rep}", _pair_acc(xl, a_pt[1], lam), _lazy2(b_pt[0]), _lazy2(b_pt[1]), rep == 2, a_pt, b_pt))
    # exceptional: the accumulator is +-B (or B with a y that differs in one component's sign - not a curve point relation, see below) over lam
    def exc(name, b_pt, lam, xl, y_pt, negate, zz_rep=-1):
        acc = _pair_acc(xl, y_pt, lam, zz_rep)
        exceptional.append(G2Case("exceptional", name, acc, _lazy2(b_pt[0]), _lazy2(b_pt[1]), negate, (b_pt[0], y_pt), b_pt))

    neg2 = lambda y: ((-y[0]) % Q, (-y[1]) % Q)
    for rep in range(6):  # image 0 on both lanes
        lam, b_pt = rl(), _g2_base(rand)
        u2 = u2_of(lam, b_pt)
        xl = (value(u2[0]) + Q, value(u2[1]) + Q)
        for doubling in (True, False):
            negate = rep % 2 == 1
            y_pt = b_pt[1] if doubling != negate else neg2(b_pt[1])
            exc(f"images 0, 0; {'doubling' if doubling else 'cancellation'} #{rep}", b_pt, lam, xl, y_pt, negate)
    # image -q: U2_c = d_c - q with 2^350 < d_c <= 2 e q, x_c = q + d_c.  lam^2 = d / (bx 2^406) in Fq2
    for which in ((0,), (1,), (0, 1)):
        for rep in range(4):
            b_pt = _g2_base(rand)
            while True:
                d = tuple(rand.randrange((1 << 350) + 1, e2) if c in which else rand.randrange(1 << 352, Q) for c in range(2))
                lam = pyref.fq2_sqrt(pyref.fq2_mul(d, pyref.fq2_inv(fq2_scale(b_pt[0], RQ))))
                if lam is not None:
                    break
            u2 = u2_of(lam, b_pt)
            assert all(value(u2[c]) == d[c] - Q for c in range(2))
            xl = tuple(Q + d[c] if c in which else d[c] for c in range(2))
            for doubling in (True, False):
                negate = rep % 2 == 1
                y_pt = b_pt[1] if doubling != negate else neg2(b_pt[1])
                exc(f"image -q on lanes {which}; {'doubling' if doubling else 'cancellation'} #{rep}", b_pt, lam, xl, y_pt, negate)
    # image q: U2_c = 0 exactly (the lane's double-width sum is zero) and x_c = 0: on the odd lane with bx and lam in Fq.  The even lane would need
    # zz or bx in u Fq, and neither exists: u t is never a square in Fq2 (its norm 5 t^2 is a non-residue), and x = u t gives x^3 + b' in u Fq.
    for lane in (1,):
        for rep in range(4):
            b_pt = _g2_base(rand, x=lambda r: (r.randrange(1, Q), 0))
            lam = None
            while lam is None:
                lam = pyref.fq_sqrt(rand.randrange(1, Q))
            lam = (lam, 0)
            u2 = u2_of(lam, b_pt, zz_rep=-1)
            assert value(u2[lane]) == 0
            for x_lane in (0, Q):  # x_c = 0: P_c = q; x_c = q: P_c = 0
                xl = tuple(x_lane if c == lane else value(u2[c]) + Q for c in range(2))
                for doubling in (True, False):
                    negate = rep % 2 == 1
                    y_pt = b_pt[1] if doubling != negate else neg2(b_pt[1])
                    exc(f"image {'q' if x_lane == 0 else '0 (x = q)'} on lane {lane}; {'doubling' if doubling else 'cancellation'} #{rep}", b_pt, lam, xl, y_pt, negate)
    # P = 0 and R = 0 on ONE lane only: a base whose y has a zero component, lam in Fq, the accumulator -B: R = 2 y lam^3 has that component zero
    for comp in (0, 1):
        for rep in range(4):
            b_pt = g2_point_with_zero_y_component(comp, start=1 + 5 * rep)
            lam = (rand.randrange(1, Q), 0)
            u2 = u2_of(lam, b_pt)
            xl = (value(u2[0]) + Q, value(u2[1]) + Q)
            negate = rep % 2 == 1
            exc(f"R = 0 on lane {comp} only (cancellation) #{rep}", b_pt, lam, xl, neg2(b_pt[1]) if not negate else b_pt[1], negate)
            exc(f"y component {comp} zero, doubling #{rep}", b_pt, lam, xl, b_pt[1] if not negate else neg2(b_pt[1]), negate)
    for rep in range(24):
        b_pt = _g2_base(rand) if rep > 1 else g2_point_with_zero_y_component(rep)
        z = [norm(0), norm(0)]
        restart.append(G2Case("restart", f"restart #{rep}", PairAcc(z, z, z, z, True), _lazy2(b_pt[0]), _lazy2(b_pt[1]), rep % 2 == 0, None, b_pt))
    # the second addition of a bucket: the accumulator as a first addition leaves it, (x1, +-y1, (one, 0), (one, 0))
    for rep in range(16):
        a_pt, b_pt = _g2_base(rand), _g2_base(rand)
        acc, _ = m_pair_madd(restart[0].acc, _lazy2(a_pt[0]), _lazy2(a_pt[1]), rep % 2 == 1)
        ordinary.append(G2Case("ordinary", f"second addition of a bucket #{rep}", acc, _lazy2(b_pt[0]), _lazy2(b_pt[1]), rep % 4 >= 2,
                               a_pt if rep % 2 == 0 else (a_pt[0], neg2(a_pt[1])), b_pt))
    filler = []
    cases = interleave(ordinary, exceptional, low, restart)
    while len(filler) < 800 - len(cases):
        lam, a_pt, b_pt = rl(), _g2_base(rand), _g2_base(rand)
        xl = fq2_scale(pyref.fq2_mul(a_pt[0], pyref.fq2_mul(lam, lam)), RQ)
        filler.append(G2Case("ordinary", f"random #{len(filler)}", _pair_acc(xl, a_pt[1], lam), _lazy2(b_pt[0]), _lazy2(b_pt[1]), len(filler) % 3 == 0, a_pt, b_pt))
    cases = interleave(cases, filler)
    recs, want, infos = [], [], []
    for c in cases:
        a = c.acc
        recs.append(a.x[0] + a.x[1] + a.y[0] + a.y[1] + a.zz[0] + a.zz[1] + a.zzz[0] + a.zzz[1] + [1 if a.inf else 0] + c.px[0] + c.px[1] + c.py[0] + c.py[1]
                    + [1 if c.negate else 0])
        o, info = m_pair_madd(a, c.px, c.py, c.negate)
        want.append(o.x[0] + o.x[1] + o.y[0] + o.y[1] + o.zz[0] + o.zz[1] + o.zzz[0] + o.zzz[1] + [1 if o.inf else 0])
        infos.append(info)
    return Cases("pair_madd", rows(recs), [f"{c.cls}: {c.name}" for c in cases], rows(want), (cases, infos))


ALL = {"mul": mul_cases, "sqr": sqr_cases, "dop": dop_cases, "normalized": normalized_cases, "to_exact": to_exact_cases, "from_exact": from_exact_cases,
       "raw": raw_cases, "fqz": fqz_cases, "madd": madd_cases, "pair_help": pair_help_cases, "pair_mul": pair_mul_cases, "pair_madd": pair_madd_cases}
