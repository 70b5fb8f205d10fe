"""Operands of the device field arithmetic (snarkvm_amd/csrc/ff.hip.h) chosen in the space the arithmetic works in, shared by
tests/test_field_limb_edges_host.py (CPU) and tests/test_gpu_field_limb_edges.py.

ff.hip.h holds an element a as N limbs of 29 bits of its INTERNAL Montgomery form I = a * 2^(29 N) mod p (Fr: N = 9, Fq: N = 13); memory holds
a * 2^256 / a * 2^384.  Carry chains, the unmasked top limb, the three-way correction of diff_of_products and the conditional subtraction all act
on the limbs of I, so the cases are integers I < p picked for their limb pattern, handed over as the memory image I * 2^(membits - 29 N) mod p
(2^-5 for Fr, 2^7 for Fq) that from_mem_mont turns into exactly I.

Expected values are plain Python integers on the memory images (R = 2^membits, the formulas of oracle/pyref.py):
    add (x + y), sub (x - y), neg (-x), mul (x y / R), sqr (x^2 / R), inverse (R^2 / x), from_bigint (x R), to_bigint (x / R),
    diff_of_products ((a b - c d) / R), all mod p.

CPU only: numpy and Python integers."""
import collections
import functools
import random

import numpy as np

from oracle import pyref

Field = collections.namedtuple("Field", "id name p N membits nl")
FIELDS = {0: Field(0, "fr", pyref.R_MOD, 9, 256, 4), 1: Field(1, "fq", pyref.Q_MOD, 13, 384, 6)}
LIMB = 29
FULL = (1 << LIMB) - 1
Cases = collections.namedtuple("Cases", "field names internal mem arr a b")


def limbs29(v, n):
    return [(v >> (LIMB * i)) & FULL for i in range(n)]


def from_limbs29(ls):
    return sum(int(l) << (LIMB * i) for i, l in enumerate(ls))


@functools.lru_cache(maxsize=None)
def _pow2(e, p):
    return pow(2, e, p)


def to_internal(f, mem):
    """what Fp::from_mem_mont makes of a memory image: the Montgomery product with 2^(2 * 29 N - membits), which divides by 2^(29 N)"""
    return mem * _pow2(LIMB * f.N - f.membits, f.p) % f.p


def to_mem(f, internal):
    return internal * _pow2(f.membits - LIMB * f.N, f.p) % f.p


def ints_to_arr(vals, nl):
    """canonical integers -> (n, nl) little-endian 64-bit limbs"""
    vals = list(vals)
    return np.frombuffer(b"".join(int(v).to_bytes(8 * nl, "little") for v in vals), dtype="<u8").reshape(len(vals), nl).astype(np.uint64)


def arr_to_ints(arr):
    arr = np.ascontiguousarray(arr, dtype="<u8")
    w = arr.shape[-1] * 8
    raw = arr.tobytes()
    return [int.from_bytes(raw[i : i + w], "little") for i in range(0, len(raw), w)]


def internal_values(f):
    """[(name, I)]: canonical internal integers, first occurrence of a value wins"""
    p, N = f.p, f.N
    top = p >> (LIMB * (N - 1))  # the modulus's top limb
    out = [("0", 0), ("1", 1), ("2", 2), ("p-1", p - 1), ("p-2", p - 2), ("(p-1)/2", (p - 1) // 2), ("(p+1)/2", (p + 1) // 2),
           ("internal one", pow(2, LIMB * N, p))]
    for k in range(N):
        out.append((f"2^(29*{k})", 1 << (LIMB * k)))
        if k >= 1:
            out.append((f"2^(29*{k})-1", (1 << (LIMB * k)) - 1))
        out.append((f"2^(29*{k}+28)", 1 << (LIMB * k + 28)))
        out.append((f"full limb {k}", FULL << (LIMB * k)))
    ones = from_limbs29([FULL] * (N - 1) + [top - 1])
    alt = from_limbs29([0x15555555 if i % 2 == 0 else 0x0AAAAAAA for i in range(N - 1)] + [top - 1])
    alt2 = from_limbs29([0x0AAAAAAA if i % 2 == 0 else 0x15555555 for i in range(N - 1)] + [top - 1])
    out += [("low limbs full", ones), ("low limbs 15555555/0aaaaaaa", alt), ("low limbs 0aaaaaaa/15555555", alt2)]
    for k in range(N):
        out.append((f"p-2^(29*{k})", p - (1 << (LIMB * k))))
    rng = random.Random(0x29 * N)
    rand = [rng.randrange(p) for _ in range(16)]
    # partners for add / sub: b = p - a (sum exactly p), p - a -+ 1, a + 1 (a - b borrows through every limb); b = a is the diagonal of the pairs
    bases = [("low limbs full", ones), ("low limbs 15555555/0aaaaaaa", alt), (f"2^(29*{N // 2})", 1 << (LIMB * (N // 2))),
             (f"full limb {N // 2 - 1}", FULL << (LIMB * (N // 2 - 1))), ("(p-1)/2", (p - 1) // 2), ("random 0", rand[0]),
             ("low limbs 0aaaaaaa/15555555", alt2), (f"2^(29*{N - 1})", 1 << (LIMB * (N - 1))), ("full limb 0", FULL), ("random 1", rand[1]),
             ("internal one", pow(2, LIMB * N, p))]
    for name, a in bases:
        out += [(f"p-({name})", p - a), (f"p-({name})-1", p - a - 1), (f"p-({name})+1", p - a + 1), (f"({name})+1", a + 1)]
    out += [(f"random {i}", v) for i, v in enumerate(rand)]
    seen, kept = set(), []
    for name, v in out:
        if 0 <= v < p and v not in seen:  # every family member must be canonical: 2^(29 k + 28) and the full limb are not for the top limb of Fr
            seen.add(v)
            kept.append((name, v))
    return kept


@functools.lru_cache(maxsize=None)
def cases(field):
    """Cases(field, names, internal, mem, arr, a, b): the list and its ordered pairs (a[i k + j], b[i k + j]) = (arr[i], arr[j])"""
    f = FIELDS[field]
    named = internal_values(f)
    names = [n for n, _ in named]
    internal = [v for _, v in named]
    mem = [to_mem(f, v) for v in internal]
    for i, m in zip(internal, mem):
        assert m < f.p and to_internal(f, m) == i  # from_mem_mont yields exactly the chosen limbs
    arr = ints_to_arr(mem, f.nl)
    k = arr.shape[0]
    a, b = np.repeat(arr, k, axis=0), np.tile(arr, (k, 1))
    for x in (arr, a, b):
        x.setflags(write=False)
    return Cases(f, names, internal, mem, arr, a, b)


def pair_name(c, idx):
    k = len(c.names)
    return f"{c.field.name}: ({c.names[idx // k]}) , ({c.names[idx % k]})"


# ---- expected values on memory images (Python integers)
def expect(f, op, x, y=None):
    p, R = f.p, 1 << f.membits
    Ri = _pow2(-f.membits, p)
    if op == "add":
        return (x + y) % p
    if op == "sub":
        return (x - y) % p
    if op in ("mul", "lazy_chain"):  # ((x + y) - y + 2p) * y, reduced == x * y
        return x * y * Ri % p
    if op == "sqr":
        return x * x * Ri % p
    if op == "neg":
        return (-x) % p
    if op == "inverse":
        return R * R * pow(x, -1, p) % p
    if op == "from_bigint":
        return x * R % p
    if op == "to_bigint":
        return x * Ri % p
    if op == "diff_of_products":  # op 9 of field_op: x*y - y*(x + y)
        return (x * y - y * ((x + y) % p)) * Ri % p
    raise KeyError(op)


def expect_dop(f, q):
    a, b, c, d = q
    return (a * b - c * d) * _pow2(-f.membits, f.p) % f.p


def first_mismatch(got, want):
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).any(axis=1))[0]
    return None if bad.size == 0 else int(bad[0])


# ---- four-operand diff_of_products
@functools.lru_cache(maxsize=None)
def dop_quads(field):
    """[(a, b, c, d)] memory images: (a, b, b, a) -> 0; (a, b, 0, 0); (0, 0, a, b) - the most negative; (small, b, p-1, d); 4 096 random"""
    c = cases(field)
    f = c.field
    k = len(c.mem)
    pairs = [(c.mem[i], c.mem[j]) for i in range(k) for j in range(k)]
    quads = [(a, b, b, a) for a, b in pairs] + [(a, b, 0, 0) for a, b in pairs] + [(0, 0, a, b) for a, b in pairs]
    pm1 = to_mem(f, f.p - 1)
    for small in (0, 1, 2):
        quads += [(to_mem(f, small), b, pm1, d) for b, d in pairs]
    rng = random.Random(0xD0B + field)
    quads += [tuple(to_mem(f, rng.randrange(f.p)) for _ in range(4)) for _ in range(4096)]
    return quads


def dop_branch_counts(f, quads):
    """Replay of Fp::diff_of_products' unreduced value: X = A B - C D on the internal integers, m = -X / p mod 2^(29 N) (the column-wise m_k put
    together), T = (X + m p) / 2^(29 N) in (-p, 2p).  -> (#T < 0, #0 <= T < p, #T >= p)"""
    p, B = f.p, LIMB * f.N
    pinv = pow(p, -1, 1 << B)
    neg = mid = hi = 0
    for q in quads:
        A, Bb, C, D = (to_internal(f, v) for v in q)
        X = A * Bb - C * D
        m = (-X * pinv) % (1 << B)
        assert (X + m * p) % (1 << B) == 0
        T = (X + m * p) >> B
        assert -p < T < 2 * p
        if T < 0:
            neg += 1
        elif T < p:
            mid += 1
        else:
            hi += 1
    return neg, mid, hi


# ---- Fq2 (memory images (c0, c1); pyref.fq2_* work on plain values)
Q = pyref.Q_MOD


@functools.lru_cache(maxsize=None)
def fq2_elements():
    c = cases(1)
    pm1 = to_mem(c.field, Q - 1)
    els = []
    for x in c.mem:
        els += [(x, 0), (0, x), (x, x), (x, pm1)]
    rng = random.Random(0xF92)
    els += [(rng.randrange(Q), rng.randrange(Q)) for _ in range(16)]
    return list(dict.fromkeys(els))


def fq2_pairs():
    """every element against four partners, and every ordered pair of the elements made of the first eight values of the list"""
    els = fq2_elements()
    n = len(els)
    pairs = [(els[i], els[(i + s) % n]) for s in (1, 7, n // 2) for i in range(n)] + [(els[i], els[n - 1 - i]) for i in range(n)]
    core = els[:32]
    pairs += [(x, y) for x in core for y in core]
    return pairs


def fq2_plain(m):
    return (pyref.fq_from_mont(m[0]), pyref.fq_from_mont(m[1]))


def fq2_mont(v):
    return (pyref.fq_to_mont(v[0]), pyref.fq_to_mont(v[1]))


def fq2_arr(els):
    """[(c0, c1), ...] or [((c0, c1), (c0, c1), ...), ...] -> rows of 6-limb elements, c0 then c1"""
    flat = []
    for e in els:
        if isinstance(e[0], tuple):
            for x in e:
                flat += [x[0], x[1]]
        else:
            flat += [e[0], e[1]]
    return ints_to_arr(flat, 6)


# ---- square roots in Fq
def fq_sqrt_cases(z_root):
    """[(label, a (plain value), expect_ok)].  z_root: the 2^46-th root of unity of the reference (plain value).  With q - 1 = 2^46 T, the element
    z^(2^(46 - k) * odd) * s^2, s of odd order, has a T-th power of order exactly 2^k: Tonelli-Shanks' first loop runs k squarings; k = 46 is a
    non-residue, k = 0 skips the loop."""
    rng = random.Random(0x5127)
    out = [("0", 0, True), ("1", 1, True), ("q-1", Q - 1, True), ("4", 4, True)]
    for k in range(47):
        for rep in range(2):
            s = pow(rng.randrange(2, Q), 1 << 46, Q)  # odd order
            odd = rng.randrange(1 << 20) | 1
            a = pow(z_root, (1 << (46 - k)) * odd, Q) * s * s % Q
            T = (Q - 1) >> 46
            b = pow(a, T, Q)
            assert pow(b, 1 << k, Q) == 1 and (k == 0 or pow(b, 1 << (k - 1), Q) != 1)
            out.append((f"order 2^{k} #{rep}", a, k < 46))
    res = nres = 0
    while res < 64 or nres < 64:
        a = rng.randrange(1, Q)
        ok = pow(a, (Q - 1) // 2, Q) == 1
        if ok and res < 64:
            res += 1
            out.append((f"residue {res}", a, True))
        elif not ok and nres < 64:
            nres += 1
            out.append((f"non-residue {nres}", a, False))
    return out


def fq2_sqrt_cases():
    """[(label, a (plain (c0, c1)))]: base-field elements (residue, non-residue, 0, q-1 = -1), elements whose norm is a non-residue, squares"""
    rng = random.Random(0x5128)
    out = [("(0, 0)", (0, 0)), ("(1, 0)", (1, 0)), ("(4, 0)", (4, 0)), ("(q-1, 0)", (Q - 1, 0))]
    res = nres = 0
    while res < 4 or nres < 4:
        a = rng.randrange(2, Q)
        ok = pow(a, (Q - 1) // 2, Q) == 1
        if ok and res < 4:
            res += 1
            out.append((f"(residue {res}, 0)", (a, 0)))
        elif not ok and nres < 4:
            nres += 1
            out.append((f"(non-residue {nres}, 0)", (a, 0)))
    n = 0
    while n < 16:
        a = (rng.randrange(Q), rng.randrange(1, Q))
        if pow((a[0] * a[0] + 5 * a[1] * a[1]) % Q, (Q - 1) // 2, Q) == Q - 1:
            n += 1
            out.append((f"non-residue norm {n}", a))
    for i in range(64):
        e = (rng.randrange(Q), rng.randrange(Q))
        out.append((f"square {i}", pyref.fq2_mul(e, e)))
    # squares of (0, y) and (x, 0)-like shapes: c1 == 0 with a root outside the base field is the reference's None (fp2.rs:210-212)
    out.append(("(0, 3)^2 = (-45, 0)", pyref.fq2_mul((0, 3), (0, 3))))
    return out
