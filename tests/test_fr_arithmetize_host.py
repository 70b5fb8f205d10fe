"""`snarkvm_hip_fr_arithmetize` on the CPU: its validation and the host twin of its kernels (`snarkvm_hip_selftest_fr_arithmetize`: the kernels' own
per-element routines compiled for the host, for a GIVEN table split and thread count) over the cases of tests/helpers/arith_cases.py.

Every comparison is bit for bit.  Expected values are Python ints (`sumcheck_cases.arith_py`, row_col = row * col), `matrices.matrix_evals` as it
stands, and the committed Varuna fixture - never the twin itself.
"""
import ctypes

import numpy as np
import pytest

from snarkvm_amd import _lib, matrices
from tests import util
from tests.helpers import arith_cases as ac
from tests.helpers import sumcheck_cases as sc

CASES = ac.cases()
IDS = [c.name for c in CASES]
THREADS = (1, 64, 256, ac.LAUNCH_THREADS)


def _splits(case):
    lg = max(case.lg_r, case.lg_c)
    default = {ac.geometry(case.k, case.lg_r)["split"], ac.geometry(case.k, case.lg_c)["split"]}
    return sorted({0, 1, max(lg - 1, 0), lg, lg + 3} | default)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_against_python_ints_for_every_split_and_thread_count(case):
    want = ac.expected(case)
    seen = set()
    for split in _splits(case):
        for threads in THREADS:
            got = ac.selftest(case, split, threads)
            for w, x in zip(ac.OUTPUTS, want):
                assert np.array_equal(got[w], x), (case.name, w, split, threads)
            seen.add(b"".join(got[w].tobytes() for w in ac.OUTPUTS))
    assert len(seen) == 1  # the bytes depend on neither the split nor the thread count


@pytest.mark.parametrize("case", [c for c in CASES if c.matrix.nnz and c.k & (c.k - 1) == 0], ids=lambda c: c.name)
def test_row_col_and_row_col_val_against_matrix_evals(case):
    """the three vectors `matrices.matrix_evals` returns, for the cases whose k is a power of two (it takes no other)"""
    row, col, rcv = matrices.matrix_evals(case.matrix, case.k, 1 << case.lg_c, 1 << case.lg_x, 1 << case.lg_r)
    got = ac.selftest(case, ac.geometry(case.k, case.lg_c)["split"], 256)
    assert np.array_equal(got["row"], row) and np.array_equal(got["col"], col) and np.array_equal(got["row_col_val"], rcv)


def test_reindexing_of_every_index_of_a_domain_of_64():
    """col[e] = w_C^reindex_by_subdomain(j) for every j of |V| = 2^6 and every lg_input < 6; the largest index maps below |V|"""
    from oracle import pyref

    w = pyref.domain_group_gen(6)
    for lg_x in range(6):
        case = next(c for c in CASES if c.name == f"reindex_v64_lgx{lg_x}")
        at = [matrices.reindex_by_subdomain(64, 1 << lg_x, int(j)) for j in case.matrix.col_idx]
        assert sorted(at) == list(range(64)) and matrices.reindex_by_subdomain(64, 1 << lg_x, 63) < 64
        got = ac.selftest(case, 3, 64, want=("col",))["col"]
        assert util.fr_mont_to_ints(got) == [pow(w, x, ac.R) for x in at]


def test_the_fixture_is_the_known_answer(golden):
    """A, B, C of tests/golden/varuna_circuit0.json at |R| = |V| = |K| = 8, |X| = 4 equal the arithmetization the round-4 tests hold, and row_col is
    the product of its row and col"""
    fx = sc.fixture(golden["varuna"])
    for n in "ABC":
        case = next(c for c in CASES if c.name == f"fixture_{n}")
        got = ac.selftest(case, 2, 8)
        row, col, rcv = fx["ariths"][n]
        assert np.array_equal(got["row"], row) and np.array_equal(got["col"], col) and np.array_equal(got["row_col_val"], rcv)
        assert util.fr_mont_to_ints(got["row_col"]) == [x * y % ac.R for x, y in zip(util.fr_mont_to_ints(row), util.fr_mont_to_ints(col))]


@pytest.mark.parametrize("skip", ac.OUTPUTS)
def test_each_output_skipped_in_turn(skip):
    case = next(c for c in CASES if c.name == "padding_k100")
    want = dict(zip(ac.OUTPUTS, ac.expected(case)))
    got = ac.selftest(case, 2, 64, want=tuple(w for w in ac.OUTPUTS if w != skip))
    assert set(got) == set(ac.OUTPUTS) - {skip}
    for w, x in got.items():
        assert np.array_equal(x, want[w]), w


def test_the_launch_geometry_is_reported():
    for k, blocks in ((1, 1), (256, 1), (257, 2), (ac.LAUNCH_THREADS, 8192), (ac.LAUNCH_THREADS + 64, 8192)):
        g = ac.geometry(k, 10)
        assert (g["blocks"], g["threads"], g["cap"]) == (blocks, 256, 8192)
    assert [ac.geometry(1, lg)["split"] for lg in (0, 1, 2, 5, 6, 28)] == [0, 1, 1, 3, 3, 14]
    out = np.zeros(4, dtype=np.uint32)
    L = _lib.lib()
    assert L.snarkvm_hip_selftest_fr_arithmetize_geometry(1, 29, out.ctypes.data) == -1
    assert L.snarkvm_hip_selftest_fr_arithmetize_geometry((1 << 28) + 1, 3, out.ctypes.data) == -1
    assert L.snarkvm_hip_selftest_fr_arithmetize_geometry(1, 3, None) == -1


# ---- refusals: before a device is needed (this machine has none), with every output and the handle untouched ------------------------------------
def _call_args(base, change, bufs):
    m = base.matrix
    a = dict(k=base.k, rows=m.rows, row_ptr=m.row_ptr, col_idx=m.col_idx, vals=m.vals, lg_constraint=base.lg_r, lg_variable=base.lg_c, lg_input=base.lg_x)
    a.update(change)
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    outs = [bufs[w][1:].ctypes.data for w in ac.OUTPUTS]
    tail = (a["k"], a["rows"], p(a["row_ptr"]), p(a["col_idx"]), p(a["vals"]), a["lg_constraint"], a["lg_variable"], a["lg_input"])
    return outs, tail, a  # `a` keeps the replaced arrays alive


@pytest.mark.parametrize("name,change", ac.refusals(), ids=[n for n, _ in ac.refusals()])
def test_refusals_leave_outputs_and_handle_untouched(name, change):
    L = _lib.lib()
    base = ac.refusal_base()
    bufs = ac.guarded(base.k)
    outs, tail, _keep = _call_args(base, change, bufs)
    for on_device in (0, 1) if name in ("null row_ptr", "k > 2^28", "rows > 2^lg_constraint") or name.startswith("lg_") else (0,):
        with pytest.raises(_lib.HipError) as e:
            _lib.check(L.snarkvm_hip_fr_arithmetize(*outs, *tail, on_device))
        assert e.value.code == ac.INVALID_VALUE and "fr_arithmetize" in e.value.message, name
    assert L.snarkvm_hip_selftest_fr_arithmetize(*outs, *tail, 1, 64) == -1
    h = ctypes.c_void_p(0xDEAD)
    with pytest.raises(_lib.HipError) as e:
        _lib.check(L.snarkvm_hip_fr_arith_register_csr(ctypes.byref(h), *tail))
    assert e.value.code == ac.INVALID_VALUE and "fr_arith_register_csr" in e.value.message and not h.value, name
    assert all((b == ac.GUARD).all() for b in bufs.values()), name


def test_overlapping_outputs_and_a_null_handle_are_refused():
    L = _lib.lib()
    base = ac.refusal_base()
    m, k = base.matrix, base.k
    block = np.full((4 * k + 2, 4), ac.GUARD, dtype=np.uint64)
    at = lambda i: block[1 + i :].ctypes.data  # noqa: E731
    tail = (k, m.rows, *ac.csr_ptrs(m), base.lg_r, base.lg_c, base.lg_x)
    vals_block = np.full((k + m.nnz, 4), ac.GUARD, dtype=np.uint64)
    vals_block[k - 1 : k - 1 + m.nnz] = m.vals  # vals starts inside the last element of an output that lies in front of it
    tail_vals = (k, m.rows, m.row_ptr.ctypes.data, m.col_idx.ctypes.data, vals_block[k - 1 :].ctypes.data, base.lg_r, base.lg_c, base.lg_x)
    for outs, t in (((at(0), at(0), None, None), tail),                        # two outputs in one vector
                    ((at(0), None, at(k - 1), None), tail),                    # row_col starts inside row
                    ((None, at(k), None, at(1)), tail),                        # row_col_val ends inside col
                    ((None, None, None, vals_block.ctypes.data), tail_vals),   # an output that ends inside vals
                    ((m.vals.ctypes.data, None, None, None), tail)):           # an output that IS vals
        for on_device in (0, 1):
            with pytest.raises(_lib.HipError) as e:
                _lib.check(L.snarkvm_hip_fr_arithmetize(*outs, *t, on_device))
            assert e.value.code == ac.INVALID_VALUE and "overlap" in e.value.message
        assert L.snarkvm_hip_selftest_fr_arithmetize(*outs, *t, 1, 64) == -1
    assert (block == ac.GUARD).all() and (vals_block[: k - 1] == ac.GUARD).all() and np.array_equal(vals_block[k - 1 : k - 1 + m.nnz], m.vals)
    with pytest.raises(_lib.HipError) as e:
        _lib.check(L.snarkvm_hip_fr_arith_register_csr(None, *tail))
    assert e.value.code == ac.INVALID_VALUE
    assert L.snarkvm_hip_selftest_fr_arithmetize(at(0), None, None, None, *tail, 1, 0) == -1  # no threads


def test_outputs_right_behind_vals_are_accepted():
    """k far above nnz, the first output at the element behind the last value: the overlap rule looks at the nnz values, not at k of them"""
    case = next(c for c in CASES if c.name == "padding_k4096")
    m, k = case.matrix, case.k
    block = np.full((m.nnz + 4 * k + 1, 4), ac.GUARD, dtype=np.uint64)
    block[: m.nnz] = m.vals
    outs = [block[m.nnz + j * k :].ctypes.data for j in range(4)]
    assert _lib.lib().snarkvm_hip_selftest_fr_arithmetize(*outs, k, m.rows, m.row_ptr.ctypes.data, m.col_idx.ctypes.data, block.ctypes.data, case.lg_r, case.lg_c, case.lg_x, 3, 64) == 0
    assert np.array_equal(block[: m.nnz], m.vals) and (block[-1] == ac.GUARD).all()
    for j, x in enumerate(ac.expected(case)):
        assert np.array_equal(block[m.nnz + j * k : m.nnz + (j + 1) * k], x), j


def test_nothing_to_do_is_success_without_a_device():
    L = _lib.lib()
    base = ac.refusal_base()
    m = base.matrix
    empty = ac.Case("empty", matrices.SparseMatrix(3, 8, [0, 0, 0, 0], [], np.zeros((0, 4), dtype=np.uint64)), 0, 2, 3, 1)
    for on_device in (0, 1):
        _lib.check(L.snarkvm_hip_fr_arithmetize(None, None, None, None, base.k, m.rows, *ac.csr_ptrs(m), base.lg_r, base.lg_c, base.lg_x, on_device))
        guard = np.full((2, 4), ac.GUARD, dtype=np.uint64)
        _lib.check(L.snarkvm_hip_fr_arithmetize(guard.ctypes.data, None, None, guard[1:].ctypes.data, 0, 3, *ac.csr_ptrs(empty.matrix), 2, 3, 1, on_device))
        assert (guard == ac.GUARD).all()
    assert all(v.shape == (0, 4) for v in ac.selftest(empty, 1, 64).values())  # k == 0 on the twin: nothing written, the guards stand
