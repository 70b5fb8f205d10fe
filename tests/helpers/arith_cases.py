"""Cases and expected values shared by tests/test_fr_arithmetize_host.py (CPU) and tests/test_gpu_fr_arithmetize.py: the CSR matrices and domains
of `snarkvm_hip_fr_arithmetize` / `snarkvm_hip_fr_arith_register_csr`, and what every output is compared with, bit for bit.

Expected values do not come from the library's new code: row, col and row_col_val of the entries are `sumcheck_cases.arith_py` (Python ints straight
from ahp/matrices.rs:156-181), row_col is row * col by Python ints, and the padding (1, 1, 1, 0) is tiled by numpy.  The shapes are the smallest at
which each part of the kernel can go wrong: the reindexing at its period boundaries, the row search over empty rows and rows that straddle 256
entries, the power tables at every split of small, odd and even domains, the padding.
"""
import collections
import json
import os

import numpy as np

from snarkvm_amd import _lib
from snarkvm_amd.matrices import SparseMatrix
from tests import util
from tests.helpers import reduce_cases as rc
from tests.helpers import sumcheck_cases as sc

R = rc.R
GUARD = rc.GUARD
INVALID_VALUE = 1  # hipErrorInvalidValue
OUTPUTS = ("row", "col", "row_col", "row_col_val")
LAUNCH_THREADS = 8192 * 256  # the launch cap: a thread takes a second element from here on

Case = collections.namedtuple("Case", "name matrix k lg_r lg_c lg_x")


def geometry(k, lg):
    """{blocks, threads, cap, split} of what the device call launches for k elements, and the table split of a domain of 2^lg elements
    (snarkvm_hip_selftest_fr_arithmetize_geometry)"""
    out = np.zeros(4, dtype=np.uint32)
    assert _lib.lib().snarkvm_hip_selftest_fr_arithmetize_geometry(k, lg, out.ctypes.data) == 0
    return dict(zip(("blocks", "threads", "cap", "split"), (int(x) for x in out)))


def _matrix(lens, cols, seed, col_of=None, vals=None):
    """rows of the given lengths over `cols` columns: column col_of(e) (default: pseudo-random, duplicates inside a row allowed) and value vals[e]
    (default: random) for entry e"""
    lens = [int(n) for n in lens]
    nnz = sum(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rng = np.random.default_rng(1000 + seed)
    ci = rng.integers(0, cols, nnz).astype(np.uint32) if col_of is None else np.array([col_of(e) for e in range(nnz)], dtype=np.uint32).reshape(-1)
    v = rc.rnd(nnz, 90 + seed % 5).copy() if vals is None else np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 4)
    return SparseMatrix(len(lens), cols, row_ptr, ci, v.reshape(-1, 4))


def fixture_matrices():
    """A, B, C of tests/golden/varuna_circuit0.json as SparseMatrix over 7 variables"""
    with open(os.path.join(util.ROOT, "tests", "golden", "varuna_circuit0.json")) as f:
        tv = json.load(f)
    return tv, {n: SparseMatrix.from_rows([[(int(v), j) for j, v in enumerate(row) if int(v)] for row in tv["instance"][n]], 7) for n in "ABC"}


_cases = []


def cases():
    if _cases:
        return _cases
    add = lambda name, m, k, lg_r, lg_c, lg_x: _cases.append(Case(name, m, int(k), lg_r, lg_c, lg_x))  # noqa: E731
    # ---- reindexing: every column of the variable domain once, for period 2, 4 and |V| (lg_input = 0); |V| = 2^6 for every lg_input
    for lg_x in (2, 1, 0):
        add(f"reindex_v8_x{1 << lg_x}", _matrix([0, 8, 0], 8, lg_x, col_of=lambda e: e), 8, 2, 3, lg_x)
    for lg_x in range(6):
        add(f"reindex_v64_lgx{lg_x}", _matrix([64, 0], 64, 10 + lg_x, col_of=lambda e: 63 - e), 64, 1, 6, lg_x)
    # ---- row search
    add("no_entries", _matrix([0, 0, 0, 0], 8, 20), 5, 2, 3, 1)
    add("one_entry", _matrix([0, 0, 1, 0], 8, 21), 1, 2, 3, 1)
    add("one_row_holds_all", _matrix([0, 0, 40, 0, 0], 16, 22), 40, 3, 4, 2)
    add("empty_rows_lead_trail_and_70_inside", _matrix([0, 0, 0, 3] + [0] * 70 + [2, 1, 0, 0, 0, 0], 16, 23), 8, 7, 4, 2)
    add("rows_straddle_256", _matrix([1, 2, 255, 256, 257, 600], 64, 24), 1371, 3, 6, 3)
    add("one_row_lg0", _matrix([5], 4, 25), 8, 0, 2, 1)
    add("rows_fill_the_domain", _matrix([1] * 8, 8, 26), 8, 3, 3, 2)
    # ---- tables: lg 0, 1, 2, odd, even; every exponent of both domains (so a low part of 0 and of all ones, a high part of 0 and the largest)
    add("tables_lg_r1_lg_c1", _matrix([2, 2], 2, 30, col_of=lambda e: e % 2), 4, 1, 1, 0)
    add("tables_lg_r2_lg_c2", _matrix([4] * 4, 4, 31, col_of=lambda e: e % 4), 16, 2, 2, 1)
    add("tables_lg_r5_lg_c6", _matrix([2] * 31 + [64], 64, 32, col_of=lambda e: e if e < 62 else e - 62), 128, 5, 6, 2)
    add("tables_lg_r6_lg_c5", _matrix([1] * 63 + [32], 32, 33, col_of=lambda e: (e * 7) % 32 if e < 63 else e - 63), 95, 6, 5, 3)
    # ---- padding: none, one place, k not a power of two, k far above nnz
    base = _matrix([3, 0, 17, 1, 16], 32, 40)
    for k in (base.nnz, base.nnz + 1, 100, 4096):
        add(f"padding_k{k}", base, k, 3, 5, 2)
    # ---- values: 0, 1, 2, r - 1, r - 2, (r +- 1) / 2 as matrix values
    add("special_values", _matrix([7, 0, 14], 16, 50, vals=rc.special(21, 3)), 24, 2, 4, 2)
    # ---- the committed fixture
    _, mats = fixture_matrices()
    for n in "ABC":
        add(f"fixture_{n}", mats[n], 8, 3, 3, 2)
    return _cases


def past_the_launch_cap():
    """k = 2^21 + 64: with 8192 x 256 threads the first 64 threads take a second element.  About 5 000 entries, the rest padding."""
    lens = np.random.default_rng(77).integers(0, 12, 900).tolist()
    m = _matrix(lens, 1 << 10, 60)
    k = LAUNCH_THREADS + 64
    g = geometry(k, 10)
    assert g["blocks"] == g["cap"] and g["blocks"] * g["threads"] < k  # the grid stops at the cap: a thread has a second element
    return Case("past_the_launch_cap", m, k, 10, 10, 4)


_expected = {}


def expected(case):
    """(row, col, row_col, row_col_val) as (k, 4) arrays; computed once per case and not to be written to"""
    if case.name not in _expected:
        m, nnz, pad = case.matrix, case.matrix.nnz, case.k - case.matrix.nnz
        if nnz:
            row, col, rcv = sc.arith_py(m, nnz, 1 << case.lg_r, 1 << case.lg_c, 1 << case.lg_x)
            row_col = util.ints_to_fr_mont([x * y % R for x, y in zip(sc.to_ints(row), sc.to_ints(col))])
        else:
            row = col = rcv = row_col = np.zeros((0, 4), dtype=np.uint64)
        one = np.tile(util.ints_to_fr_mont([1]), (pad, 1))
        out = tuple(np.concatenate([x, p]) for x, p in zip((row, col, row_col, rcv), (one, one, one, np.zeros((pad, 4), dtype=np.uint64))))
        for x in out:
            x.setflags(write=False)
        _expected[case.name] = out
    return _expected[case.name]


def guarded(k, want=OUTPUTS):
    """{output: (k + 2, 4) array of guards} for the wanted outputs: element 0 and element k + 1 stay guards"""
    return {w: np.full((k + 2, 4), GUARD, dtype=np.uint64) for w in want}


def check_guards(bufs, k):
    for w, b in bufs.items():
        assert (b[0] == GUARD).all() and (b[k + 1] == GUARD).all(), f"a guard around {w} was written"


def csr_ptrs(m):
    return m.row_ptr.ctypes.data, (m.col_idx.ctypes.data if m.nnz else None), (m.vals.ctypes.data if m.nnz else None)


def selftest(case, split_bits, threads, want=OUTPUTS):
    """snarkvm_hip_selftest_fr_arithmetize -> {output: (k, 4)}; guards around every output, inputs checked unchanged"""
    m, k = case.matrix, case.k
    before = (m.row_ptr.copy(), m.col_idx.copy(), m.vals.copy())
    bufs = guarded(k, want)
    ptr = lambda w: bufs[w][1:].ctypes.data if w in bufs and k else None  # noqa: E731
    rcode = _lib.lib().snarkvm_hip_selftest_fr_arithmetize(*(ptr(w) for w in OUTPUTS), k, m.rows, *csr_ptrs(m), case.lg_r, case.lg_c, case.lg_x, split_bits, threads)
    assert rcode == 0, case.name
    check_guards(bufs, k)
    assert all(np.array_equal(x, y) for x, y in zip(before, (m.row_ptr, m.col_idx, m.vals))), "an input was written"
    return {w: b[1 : k + 1] for w, b in bufs.items()}


def refusals():
    """[(name, dict)]: for every refusal of the header the arguments that differ from a valid call over `refusal_base()`; the keys are the C
    parameters, and "outs" maps an output name to an (offset in elements from its own buffer, or a callable that gets the buffers)"""
    big = (1 << 28) + 1
    return [
        ("null row_ptr", dict(row_ptr=None)),
        ("null col_idx with entries", dict(col_idx=None)),
        ("null vals with entries", dict(vals=None)),
        ("row_ptr[0] != 0", dict(row_ptr=np.array([1, 3, 3, 6], dtype=np.uint64))),
        ("row_ptr decreases", dict(row_ptr=np.array([0, 4, 3, 6], dtype=np.uint64))),
        ("more than 2^32 - 1 entries", dict(row_ptr=np.array([0, 3, 3, 1 << 32], dtype=np.uint64), k=6)),
        ("k < nnz", dict(k=5)),
        ("k > 2^28", dict(k=big)),
        ("rows > 2^lg_constraint", dict(lg_constraint=1)),
        ("lg_constraint above 28", dict(lg_constraint=29)),
        ("lg_variable above 28", dict(lg_variable=29)),
        ("lg_input above 28", dict(lg_input=29, lg_variable=28)),
        ("lg_input == lg_variable", dict(lg_input=3)),
        ("lg_input > lg_variable", dict(lg_input=4)),
        ("a column index at the variable domain size", dict(col_idx=np.array([0, 1, 2, 8, 4, 5], dtype=np.uint32))),
    ]


def refusal_base():
    """a valid call: 3 rows (3, 0, 3 entries) over 8 variables, k = 8, |R| = 4, |V| = 8, |X| = 2"""
    return Case("refusal_base", _matrix([3, 0, 3], 8, 70, col_of=lambda e: e), 8, 2, 3, 1)
