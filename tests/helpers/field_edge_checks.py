"""The checks of tests/helpers/limb_cases.py's operands, written once for the host twin (snarkvm_hip_selftest_field / _field_ext) and the GPU
kernels (snarkvm_hip_devtest_field / _field_ext): a `Runner` is the pair of calls.  Every comparison is exact, limb for limb, against Python
integers, and additionally against the C++ oracle wherever it has the operation."""
import ctypes

import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib
from tests.helpers import limb_cases as lc

OPS = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "inverse": 4, "neg": 5, "from_bigint": 6, "to_bigint": 7, "lazy_chain": 8, "diff_of_products": 9}
FX = {"fq_dop": 0, "fr_dop": 1, "fq2_mul": 2, "fq2_sqr": 3, "fq2_inv": 4, "fq2_dop": 5, "fq_sqrt": 6, "fq2_sqrt": 7, "fq_raw": 8, "fr_raw": 9}
FX_IN = {0: 48, 1: 32, 2: 48, 3: 24, 4: 24, 5: 96, 6: 12, 7: 24, 8: 24, 9: 16}  # 32-bit words per input / output record
FX_OUT = {0: 12, 1: 8, 2: 24, 3: 24, 4: 24, 5: 24, 6: 16, 7: 28, 8: 72, 9: 48}
Q = pyref.Q_MOD


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


class Runner:
    def __init__(self, device):
        self.device = device

    def field(self, field, op, a, b=None):
        L = _lib.lib()
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = a if b is None else np.ascontiguousarray(b, dtype=np.uint64)
        out = np.zeros_like(a)
        args = (ctypes.c_int(field), ctypes.c_int(OPS[op]), _p(a), _p(b), _p(out), ctypes.c_size_t(a.shape[0]))
        if self.device:
            _lib.check(L.snarkvm_hip_devtest_field(*args))
        else:
            assert L.snarkvm_hip_selftest_field(*args) == 0
        return out

    def ext(self, name, rows):
        """rows: (n, 64-bit limbs of one input record) -> (n, 64-bit limbs of one output record)"""
        L = _lib.lib()
        op = FX[name]
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n = rows.shape[0]
        assert rows.shape[1] * 2 == FX_IN[op]
        out = np.full((n, FX_OUT[op] // 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        if self.device:
            _lib.check(L.snarkvm_hip_devtest_field_ext(op, rows.ctypes.data, out.ctypes.data, n))
        else:
            assert L.snarkvm_hip_selftest_field_ext(op, rows.ctypes.data, out.ctypes.data, n) == 0
        return out


def _same(got, want, label, namer):
    i = lc.first_mismatch(got, want)
    assert i is None, (label, namer(i), [hex(int(v)) for v in got[i]], [hex(int(v)) for v in want[i]])


def check_binary_ops(run, field):
    """add, sub, mul, op 9 (and op 8, the NTT's lazy chain, over Fr) on every ordered pair"""
    c = lc.cases(field)
    f = c.field
    ofn = oracle.fr_op if field == 0 else oracle.fq_op
    k = len(c.mem)
    for op in ("add", "sub", "mul", "diff_of_products") + (("lazy_chain",) if field == 0 else ()):
        want = lc.ints_to_arr([lc.expect(f, op, x, y) for x in c.mem for y in c.mem], f.nl)
        if op in ("add", "sub", "mul"):
            assert np.array_equal(ofn(op, c.a, c.b), want), op  # the two references agree
        _same(run.field(field, op, c.a, c.b), want, op, lambda i: lc.pair_name(c, i))
    assert k * k == c.a.shape[0]


def check_raw_internal_limbs(run, field):
    """a + b, a - b, -a, 2a, a * b and 0 * 0 - a * b on every ordered pair, read as the INTERNAL limbs the operation leaves (no to_mem_mont, whose
    multiplication would reduce them): every result must be the canonical representative - 0, never p, for a + b == p and for a - a"""
    c = lc.cases(field)
    f = c.field
    p, Bi = f.p, lc._pow2(-lc.LIMB * f.N, f.p)
    rows = np.concatenate([c.a, c.b], axis=1)
    got = run.ext("fr_raw" if field == 0 else "fq_raw", rows).reshape(rows.shape[0], 6, f.nl)
    pairs = [(x, y) for x in c.internal for y in c.internal]
    for k, (name, fn) in enumerate((("add", lambda x, y: (x + y) % p), ("sub", lambda x, y: (x - y) % p), ("neg", lambda x, y: (-x) % p),
                                    ("dbl", lambda x, y: 2 * x % p), ("mul", lambda x, y: x * y * Bi % p), ("0*0 - a*b", lambda x, y: -x * y * Bi % p))):
        want = lc.ints_to_arr([fn(x, y) for x, y in pairs], f.nl)
        _same(got[:, k, :], want, "raw " + name, lambda i: lc.pair_name(c, i))
    assert sum(1 for x, y in pairs if x and x + y == p) >= 40  # sums of exactly p are among the pairs


def check_unary_ops(run, field):
    """sqr, neg, to_bigint, from_bigint on every element; inverse on every element but zero"""
    c = lc.cases(field)
    f = c.field
    ofn = oracle.fr_op if field == 0 else oracle.fq_op
    for op in ("sqr", "neg", "to_bigint", "from_bigint"):
        want = lc.ints_to_arr([lc.expect(f, op, x) for x in c.mem], f.nl)
        assert np.array_equal(ofn(op, c.arr), want), op
        _same(run.field(field, op, c.arr), want, op, lambda i: c.names[i])
    nz = [i for i, v in enumerate(c.mem) if v != 0]
    assert len(nz) == len(c.mem) - 1  # zero is the only exclusion
    arr = c.arr[nz]
    want = lc.ints_to_arr([lc.expect(f, "inverse", c.mem[i]) for i in nz], f.nl)
    assert np.array_equal(ofn("inverse", arr), want)
    _same(run.field(field, "inverse", arr), want, "inverse", lambda i: c.names[nz[i]])


def check_diff_of_products(run, field):
    """the four-operand a*b - c*d with one signed-accumulator reduction; all three branches of its correction must be among the cases"""
    f = lc.FIELDS[field]
    quads = lc.dop_quads(field)
    neg, mid, hi = lc.dop_branch_counts(f, quads)
    assert neg > 0 and mid > 0 and hi > 0, (neg, mid, hi)  # T < 0 -> + p;  0 <= T < p;  T >= p -> - p
    rows = lc.ints_to_arr([v for q in quads for v in q], f.nl).reshape(len(quads), 4 * f.nl)
    want = lc.ints_to_arr([lc.expect_dop(f, q) for q in quads], f.nl)
    got = run.ext("fr_dop" if field == 0 else "fq_dop", rows)
    _same(got, want, "diff_of_products", lambda i: [hex(lc.to_internal(f, v)) for v in quads[i]])
    return neg, mid, hi


def check_fq2(run):
    els = lc.fq2_elements()
    plain = {e: lc.fq2_plain(e) for e in els}
    pairs = lc.fq2_pairs()
    want = lc.fq2_arr([lc.fq2_mont(pyref.fq2_mul(plain[x], plain[y])) for x, y in pairs])
    _same(run.ext("fq2_mul", lc.fq2_arr(pairs).reshape(len(pairs), 24)).reshape(-1, 6), want, "fq2 mul", lambda i: pairs[i // 2])
    want = lc.fq2_arr([lc.fq2_mont(pyref.fq2_mul(plain[x], plain[x])) for x in els])
    _same(run.ext("fq2_sqr", lc.fq2_arr(els).reshape(len(els), 12)).reshape(-1, 6), want, "fq2 sqr", lambda i: els[i // 2])
    nz = [e for e in els if (plain[e][0] ** 2 + 5 * plain[e][1] ** 2) % Q != 0]
    assert len(nz) == len(els) - 1  # -5 is a non-residue: the norm vanishes for zero alone
    want = lc.fq2_arr([lc.fq2_mont(pyref.fq2_inv(plain[x])) for x in nz])
    _same(run.ext("fq2_inv", lc.fq2_arr(nz).reshape(len(nz), 12)).reshape(-1, 6), want, "fq2 inverse", lambda i: nz[i // 2])
    n = len(pairs)
    quads = [(pairs[i][0], pairs[i][1], pairs[(i + 3) % n][1], pairs[(i + 3) % n][0]) for i in range(n)] + [(x, y, y, x) for x, y in pairs[:500]]
    want = lc.fq2_arr([lc.fq2_mont(pyref.fq2_sub(pyref.fq2_mul(plain[a], plain[b]), pyref.fq2_mul(plain[c], plain[d]))) for a, b, c, d in quads])
    _same(run.ext("fq2_dop", lc.fq2_arr(quads).reshape(len(quads), 48)).reshape(-1, 6), want, "fq2 diff_of_products", lambda i: quads[i // 2])


def two_adic_root(golden):
    fq = golden["constants"]["fq"]
    z = pyref.fq_from_mont(pyref.from_limbs(fq["TWO_ADIC_ROOT_OF_UNITY"]))
    assert pow(z, 1 << 45, Q) == Q - 1
    return z


def check_fq_sqrt(run, golden):
    cs = lc.fq_sqrt_cases(two_adic_root(golden))
    out = run.ext("fq_sqrt", lc.ints_to_arr([pyref.fq_to_mont(a) for _, a, _ in cs], 6))
    roots = lc.arr_to_ints(out[:, :6])
    for (label, a, ok), root, tail in zip(cs, roots, out[:, 6:]):
        assert int(tail[0]) == (1 if ok else 0) and int(tail[1]) == 0, label
        assert (pyref.fq_sqrt(a) is not None) == ok, label
        r = pyref.fq_from_mont(root)
        assert root < Q and (r * r % Q == a if ok else root == 0), label
    assert {ok for _, _, ok in cs} == {True, False}


def check_fq2_sqrt(run):
    cs = lc.fq2_sqrt_cases()
    out = run.ext("fq2_sqrt", lc.fq2_arr([lc.fq2_mont(a) for _, a in cs]).reshape(len(cs), 12))
    seen = set()
    for (label, a), row in zip(cs, out):
        c0, c1 = lc.arr_to_ints(row[:12].reshape(2, 6))
        ok = int(row[12])
        want = pyref.fq2_sqrt(a)
        seen.add((a[1] == 0, want is None))
        assert ok == (0 if want is None else 1) and int(row[13]) == 0, label
        if want is None:
            assert (c0, c1) == (0, 0), label
            continue
        r = lc.fq2_plain((c0, c1))
        assert c0 < Q and c1 < Q and pyref.fq2_mul(r, r) == (a[0] % Q, a[1] % Q), label
        assert r == want or r == ((-want[0]) % Q, (-want[1]) % Q), label
    assert seen == {(True, False), (True, True), (False, False), (False, True)}  # base-field and general elements, with and without a root
