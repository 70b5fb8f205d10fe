"""`snarkvm_hip_fr_arithmetize` and `snarkvm_hip_fr_arith_register_csr` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: fr_arithmetize_kernel),
and the circuit index built on them (snarkvm_amd/matrices.py: CircuitIndex): host and device operands, guards, skipped outputs, a scope, two logical
devices, a size past the launch cap, and the index polynomials, commitments and certificate of the fixture circuit and of a random one.

Every comparison is bit for bit.  Expected values are Python ints (tests/helpers/arith_cases.py), `matrices.matrix_evals` as it stands, `oracle.ntt`,
`oracle.g1_msm` over the committed SRS points and Horner evaluation by Python ints - never the device and never the host twin, whose bytes must
equal the device's.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, matrices, plugin, sonic_pc
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.matrices import CircuitIndex, RegisteredArithmetization
from tests import util
from tests.helpers import arith_cases as ac
from tests.helpers import reduce_cases as rc
from tests.helpers import sumcheck_cases as sc

pytestmark = pytest.mark.gpu

R = ac.R
GUARD = ac.GUARD
CASES = ac.cases()
IDS = [c.name for c in CASES]


class DeviceCsr:
    """row_ptr | col_idx | vals of a SparseMatrix in one device block (each part 32-byte aligned)"""

    def __init__(self, m, device=-1):
        self.m = m
        self.at_col = (8 * (m.rows + 1) + 31) & ~31
        self.at_val = (self.at_col + 4 * m.nnz + 31) & ~31
        self.host = np.zeros(self.at_val + 32 * max(m.nnz, 1), dtype=np.uint8)
        self.host[: 8 * (m.rows + 1)] = m.row_ptr.view(np.uint8)
        self.host[self.at_col : self.at_col + 4 * m.nnz] = m.col_idx.view(np.uint8)
        self.host[self.at_val : self.at_val + 32 * m.nnz] = m.vals.reshape(-1).view(np.uint8)
        self.mem = HipMem.from_numpy(self.host, device)

    def ptrs(self):
        return self.mem.ptr, self.mem.ptr + self.at_col, self.mem.ptr + self.at_val

    def unchanged(self):
        return np.array_equal(self.mem.download(), self.host)


def run_device(case, want=ac.OUTPUTS, device=-1, call=None):
    """the call over device operands: the wanted outputs in ONE block, a guard element in front of the first and behind every one"""
    k = case.k
    host = np.full((len(want) * (k + 1) + 1, 4), GUARD, dtype=np.uint64)
    mem = HipMem.from_numpy(host, device)
    at = {w: 1 + i * (k + 1) for i, w in enumerate(want)}
    csr = DeviceCsr(case.matrix, device)
    args = [mem.ptr + 32 * at[w] if w in at else None for w in ac.OUTPUTS] + [k, case.matrix.rows, *csr.ptrs(), case.lg_r, case.lg_c, case.lg_x]
    (call or plugin.fr_arithmetize_device)(*args)
    now = mem.download(dtype=np.uint64).reshape(-1, 4)
    written = np.zeros(len(now), dtype=bool)
    for w in want:
        written[at[w] : at[w] + k] = True
    assert (now[~written] == GUARD).all(), "a guard was written"
    assert csr.unchanged(), "an input was written"
    return {w: now[at[w] : at[w] + k] for w in want}


def run_host(case, want=ac.OUTPUTS):
    """the call over host operands, guards around every output, inputs checked unchanged"""
    m, k = case.matrix, case.k
    before = (m.row_ptr.copy(), m.col_idx.copy(), m.vals.copy())
    bufs = ac.guarded(k, want)
    ptr = lambda w: bufs[w][1:].ctypes.data if w in bufs and k else None  # noqa: E731
    _lib.check(_lib.lib().snarkvm_hip_fr_arithmetize(*(ptr(w) for w in ac.OUTPUTS), k, m.rows, *ac.csr_ptrs(m), case.lg_r, case.lg_c, case.lg_x, 0))
    ac.check_guards(bufs, k)
    assert all(np.array_equal(x, y) for x, y in zip(before, (m.row_ptr, m.col_idx, m.vals))), "an input was written"
    return {w: b[1 : k + 1] for w, b in bufs.items()}


def _twin(case):
    g = ac.geometry(case.k, max(case.lg_r, case.lg_c))
    return ac.selftest(case, g["split"], g["blocks"] * g["threads"])


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_on_host_and_device_operands(case, on_device):
    want = ac.expected(case)
    got = run_device(case) if on_device else run_host(case)
    twin = _twin(case)
    for w, x in zip(ac.OUTPUTS, want):
        assert np.array_equal(got[w], x), (case.name, w)
        assert got[w].tobytes() == twin[w].tobytes(), (case.name, w)


@pytest.mark.parametrize("on_device", [0, 1])
def test_each_output_skipped_in_turn_and_pairs(on_device):
    case = next(c for c in CASES if c.name == "rows_straddle_256")
    want = dict(zip(ac.OUTPUTS, ac.expected(case)))
    wants = [tuple(w for w in ac.OUTPUTS if w != skip) for skip in ac.OUTPUTS] + [("row_col_val",), ("row_col",), ("row", "col", "row_col_val"), ("col", "row_col")]
    for keep in wants:
        got = (run_device if on_device else run_host)(case, want=keep)
        assert set(got) == set(keep)
        for w, x in got.items():
            assert np.array_equal(x, want[w]), (keep, w)


@pytest.mark.parametrize("on_device", [0, 1])
def test_outputs_right_behind_vals_are_accepted(on_device):
    """k is far above nnz and the first output starts at the element behind the LAST value: no overlap, whatever k is"""
    case = next(c for c in CASES if c.name == "padding_k4096")
    m, k = case.matrix, case.k
    want = ac.expected(case)
    block = np.full((m.nnz + 4 * k + 1, 4), GUARD, dtype=np.uint64)
    block[: m.nnz] = m.vals
    if on_device:
        mem, csr = HipMem.from_numpy(block), DeviceCsr(m)
        d_rp, d_ci, _ = csr.ptrs()
        plugin.fr_arithmetize_device(*(mem.ptr + 32 * (m.nnz + j * k) for j in range(4)), k, m.rows, d_rp, d_ci, mem.ptr, case.lg_r, case.lg_c, case.lg_x)
        block = mem.download(dtype=np.uint64).reshape(-1, 4)
    else:
        _lib.check(_lib.lib().snarkvm_hip_fr_arithmetize(*(block[m.nnz + j * k :].ctypes.data for j in range(4)), k, m.rows, m.row_ptr.ctypes.data, m.col_idx.ctypes.data,
                                                         block.ctypes.data, case.lg_r, case.lg_c, case.lg_x, 0))
    assert np.array_equal(block[: m.nnz], m.vals) and (block[-1] == GUARD).all()
    for j, x in enumerate(want):
        assert np.array_equal(block[m.nnz + j * k : m.nnz + (j + 1) * k], x), j


def test_one_size_past_the_launch_cap():
    """k = 2^21 + 64: the grid stops at 8192 workgroups and the first threads take a second element - padding places here, the entries sit in the
    first workgroups"""
    case = ac.past_the_launch_cap()
    want = ac.expected(case)
    got = run_device(case)
    for w, x in zip(ac.OUTPUTS, want):
        assert np.array_equal(got[w], x), w
    twin = ac.selftest(case, ac.geometry(case.k, 10)["split"], ac.LAUNCH_THREADS)
    assert all(got[w].tobytes() == twin[w].tobytes() for w in ac.OUTPUTS)


def test_inside_a_scope_and_a_repeat_grows_no_allocation():
    """enqueued in a scope with the inverse transform behind it: the results are there after scope_end; repeated calls, on device and on host
    operands and through registration, allocate nothing but the handle's own block"""
    case = next(c for c in CASES if c.name == "padding_k4096")
    want = ac.expected(case)
    want_poly = [oracle.ntt(x, direction=oracle.INVERSE) for x in want]
    L = _lib.lib()
    stats = np.zeros(5, dtype=np.uint64)
    k = case.k

    def in_scope(*args):
        _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(args[0])))
        try:
            plugin.fr_arithmetize_device(*args)
            plugin.NTT_device_batch(12, list(args[:4]), directions=[1] * 4, types=[0] * 4)
        finally:
            _lib.check(L.snarkvm_hip_scope_end())

    for attempt in range(2):
        if attempt == 1:
            run_device(case)  # the lane of a call outside a scope has its tables too
            L.snarkvm_hip_alloc_stats(None, 1)
        got = run_device(case, call=in_scope)
        for w, x in zip(ac.OUTPUTS, want_poly):
            assert np.array_equal(got[w], x), (attempt, w)
    got = run_device(case)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    # the blocks of run_device itself come from snarkvm_hip_malloc, which the workspace statistics do not count
    assert not stats[:4].any(), stats
    assert all(np.array_equal(got[w], x) for w, x in zip(ac.OUTPUTS, want))
    run_host(case)
    L.snarkvm_hip_alloc_stats(None, 1)
    got = run_host(case)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats
    assert all(np.array_equal(got[w], x) for w, x in zip(ac.OUTPUTS, want))
    assert k == 4096


# ---- refusals that need a device ---------------------------------------------------------------------------------------------------------------------
def test_operands_on_the_host_with_on_device_are_refused_and_nothing_is_written():
    case = ac.refusal_base()
    m, k = case.matrix, case.k
    csr = DeviceCsr(m)
    host = np.full((4 * (k + 1) + 1, 4), GUARD, dtype=np.uint64)
    mem = HipMem.from_numpy(host)
    outs = [mem.ptr + 32 * (1 + i * (k + 1)) for i in range(4)]
    host_out = np.full((k, 4), GUARD, dtype=np.uint64)
    d_rp, d_ci, d_v = csr.ptrs()
    h_rp, h_ci, h_v = ac.csr_ptrs(m)
    tail = (case.lg_r, case.lg_c, case.lg_x)
    for args in (([host_out.ctypes.data] + outs[1:], (d_rp, d_ci, d_v)),     # an output in host memory
                 ([outs[0], None, None, host_out.ctypes.data], (d_rp, d_ci, d_v)),
                 (outs, (h_rp, d_ci, d_v)),                                   # a CSR array in host memory
                 (outs, (d_rp, h_ci, d_v)),
                 (outs, (d_rp, d_ci, h_v))):
        with pytest.raises(_lib.HipError) as e:
            plugin.fr_arithmetize_device(*args[0], k, m.rows, *args[1], *tail)
        assert e.value.code == ac.INVALID_VALUE and e.value.message
    assert (host_out == GUARD).all() and np.array_equal(mem.download(dtype=np.uint64).reshape(-1, 4), host) and csr.unchanged()
    # the overlap rules hold for device pointers as well
    with pytest.raises(_lib.HipError) as e:
        plugin.fr_arithmetize_device(outs[0], outs[0] + 32 * (k - 1), None, None, k, m.rows, d_rp, d_ci, d_v, *tail)
    assert e.value.code == ac.INVALID_VALUE and "overlap" in e.value.message
    with pytest.raises(_lib.HipError) as e:
        plugin.fr_arithmetize_device(None, None, d_v, None, k, m.rows, d_rp, d_ci, d_v, *tail)
    assert e.value.code == ac.INVALID_VALUE and "overlap" in e.value.message
    assert np.array_equal(mem.download(dtype=np.uint64).reshape(-1, 4), host) and csr.unchanged()


# ---- registration -------------------------------------------------------------------------------------------------------------------------------------
def _same_evaluations(mats, ks, lg_r, lg_c, lg_x, seed):
    alpha, beta, scales = sc.scalars(seed)
    old = [RegisteredArithmetization.from_matrix(m, k, 1 << lg_c, 1 << lg_x, 1 << lg_r) for m, k in zip(mats, ks)]
    new = [RegisteredArithmetization.from_csr(m, k, lg_r, lg_c, lg_x) for m, k in zip(mats, ks)]
    want = plugin.fr_sumcheck_evals([r.handle for r in old], ks, alpha, beta, scales)
    got = plugin.fr_sumcheck_evals([r.handle for r in new], ks, alpha, beta, scales)
    for w, g in zip(want, got):
        for x, y in zip(w, g):
            assert x.any() and np.array_equal(x, y)
    for r in old + new:
        r.close()
        r.close()


def test_register_csr_gives_the_evaluations_of_the_host_arithmetization():
    _same_evaluations(sc.random_circuit(11, lg_r=9, lg_c=9, lg_k=(10, 10, 10)), [1 << 10] * 3, 9, 9, 4, 11)
    _, mats = ac.fixture_matrices()
    _same_evaluations([mats[n] for n in "ABC"], [8] * 3, 3, 3, 2, 12)


def test_register_csr_of_nothing_and_a_repeat_grows_no_workspace():
    L = _lib.lib()
    empty = matrices.SparseMatrix(3, 8, [0, 0, 0, 0], [], np.zeros((0, 4), dtype=np.uint64))
    reg = RegisteredArithmetization.from_csr(empty, 0, 2, 3, 1)
    assert reg.handle and reg.k == 0
    reg.close()
    case = next(c for c in CASES if c.name == "rows_straddle_256")
    stats = np.zeros(5, dtype=np.uint64)
    for attempt in range(2):
        if attempt == 1:
            L.snarkvm_hip_alloc_stats(None, 1)
        reg = RegisteredArithmetization.from_csr(case.matrix, case.k, case.lg_r, case.lg_c, case.lg_x)
        reg.close()
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats  # the replica itself is the handle's, released with it: no lane buffer grew


MULTI_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from snarkvm_amd import msm, plugin
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.matrices import RegisteredArithmetization
from tests.helpers import arith_cases as ac
from tests.helpers import sumcheck_cases as sc
from tests import test_gpu_fr_arithmetize as t

assert msm.num_devices() == 2, msm.num_devices()
case = next(c for c in ac.cases() if c.name == "rows_straddle_256")
want = ac.expected(case)
for device in (0, 1, 1, 0):
    got = t.run_device(case, device=device)
    for w, x in zip(ac.OUTPUTS, want):
        assert np.array_equal(got[w], x), (device, w)
# every logical device computed its own replica: the evaluations on either device equal those over the host arithmetization
alpha, beta, scales = sc.scalars(3)
reg = RegisteredArithmetization.from_csr(case.matrix, case.k, case.lg_r, case.lg_c, case.lg_x)
want_abf = sc.expected_py(want[0], want[1], want[3], alpha, beta, scales)
k = case.k
for device in (0, 1, 1, 0):
    mem = HipMem.from_numpy(np.full((3 * (k + 1), 4), sc.GUARD, dtype=np.uint64), device)
    ptrs = [mem.ptr + 32 * j * (k + 1) for j in range(3)]
    plugin.fr_sumcheck_evals_device([reg.handle], ptrs[0:1], ptrs[1:2], ptrs[2:3], alpha, beta, scales)
    now = mem.download(dtype=np.uint64).reshape(3, k + 1, 4)
    for j in range(3):
        assert np.array_equal(now[j, :k], want_abf[j]) and (now[j, k] == sc.GUARD).all(), (device, j)
    mem.free()
reg.close()
print("ARITHMETIZE_MULTI_OK")
'''


def test_two_logical_devices():
    env = dict(os.environ, SNARKVM_HIP_DEVICES="0,0")
    r = subprocess.run([sys.executable, "-c", MULTI_SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert "ARITHMETIZE_MULTI_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the circuit index ------------------------------------------------------------------------------------------------------------------------------------
def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def _srs_ck(golden, n=1024):
    powers = util.g1_affine_from_ints(util.srs_points_ints(golden["srs_g1"], n))
    return powers, sonic_pc.CommitterUnionKey(powers, powers[:4])


def _expected_index(mats, lg_r, lg_c, lg_x, circuit_id):
    """{label: (evaluations, coefficients)} by Python ints and the oracle's inverse transform"""
    out = {}
    for name, m in zip("abc", mats):
        k = 1 << matrices._domain_lg(m.nnz)
        evals = ac.expected(ac.Case(f"index_{circuit_id}_{name}", m, k, lg_r, lg_c, lg_x))
        for kind, ev in zip(matrices.INDEX_KINDS, evals):
            out[f"circuit_{circuit_id}_{kind}_{name}"] = (ev, oracle.ntt(ev, direction=oracle.INVERSE))
    return out


def _check_index(index, mats, circuit_id, golden, seed):
    want = _expected_index(mats, index.lg_r, index.lg_c, index.lg_x, circuit_id)
    assert set(index.polynomials) == set(want) and len(want) == 12
    coeffs = {}
    for label, p in index.polynomials.items():
        assert (p.label, p.degree_bound, p.hiding_bound, p.n) == (label, None, None, want[label][1].shape[0])
        got = np.empty((p.n, 4), dtype=np.uint64)
        _lib.check(_lib.lib().snarkvm_hip_memcpy_d2h(got.ctypes.data, p.ptr, 32 * p.n))
        assert np.array_equal(got, want[label][1]), label
        coeffs[label] = util.fr_mont_to_ints(got)
    # the verifying key: in the order of the sorted label strings, each the MSM of the coefficients over the SRS powers
    powers, _ = golden
    labels = sorted(want)
    assert labels[0].endswith("_col_a") and labels[-1].endswith("_row_col_val_c")
    assert [c.label for c in index.commitments] == labels
    for c in index.commitments:
        poly = want[c.label][1]
        expect = oracle.g1_to_affine(oracle.g1_msm(powers[: poly.shape[0]], oracle.fr_op("to_bigint", poly)))
        assert c.degree_bound is None and util.affine_equal(np.array([c.commitment]), expect), c.label
    # the certificate
    point, combiners = rc.rnd(1, seed), rc.rnd(12, seed + 1)
    lc, total = index.evaluate_index_polynomials(point[0], combiners)
    z, cs = util.fr_mont_to_ints(point)[0], util.fr_mont_to_ints(combiners)
    assert util.fr_mont_to_ints(np.asarray(total).reshape(1, 4)) == [sum(c * _horner(coeffs[label], z) for c, label in zip(cs, labels)) % R]
    assert lc.label == "circuit_check" and [t for _, t in lc.iter()] == labels
    assert all(np.array_equal(c, combiners[i]) for i, (c, _) in enumerate(lc.iter()))
    # prove_vk's other half: the same combination over the resident polynomials, evaluated by the opening code
    value = sonic_pc.SonicKZG10.evaluate_combinations_device([lc], list(index.polynomials.values()), [("circuit_check", ("point", point[0]))])
    assert np.array_equal(value[("circuit_check", "point")], total)
    # the opening of that combination over the resident index polynomials: the proof of the host route over their downloaded coefficients
    from snarkvm_amd import kzg10

    class Challenges:
        def __init__(self):
            self.vals, self.k = rc.rnd(4, seed + 2), 0

        def squeeze_short_nonnative_field_element(self):
            self.k += 1
            return self.vals[self.k - 1]

    resident = list(index.polynomials.values())
    rands = [kzg10.KZGRandomness.empty() for _ in resident]
    query = [("circuit_check", ("gamma", point[0]))]
    max_degree = powers.shape[0] - 1
    got = sonic_pc.SonicKZG10.open_combinations_device(max_degree, golden[1], [lc], resident, rands, query, Challenges())
    host = [sonic_pc.LabeledPolynomial(p.label, want[p.label][1]) for p in resident]
    ref = sonic_pc.SonicKZG10.open_combinations(max_degree, golden[1], [lc], host, rands, query, Challenges())
    assert len(got) == len(ref) == 1 and util.affine_equal(np.array([got[0].w]), np.array([ref[0].w])) and got[0].random_v is None and ref[0].random_v is None
    with pytest.raises(ValueError, match="No combiner left"):
        index.evaluate_index_polynomials(point[0], combiners[:11])
    with pytest.raises(ValueError, match="more combiners"):
        index.evaluate_index_polynomials(point[0], np.concatenate([combiners, combiners[:1]]))
    index.prune_row_col_evals()
    with pytest.raises(ValueError, match="row_col evaluations are not available"):
        index.evaluate_index_polynomials(point[0], combiners)


@pytest.fixture(scope="module")
def srs(golden):
    powers, ck = _srs_ck(golden)
    yield powers, ck
    ck.close()


def test_circuit_index_of_the_fixture_drives_the_rounds(golden, srs):
    """CircuitIndex.build from A, B, C alone: the index polynomials, commitments and certificate; then its registered objects, fed unchanged to the
    existing drivers, reproduce the fixture's w, h_0, h_1, g_1, g_a, g_b and h_2"""
    from tests.helpers import rowcheck_cases as rcc
    from tests.helpers import selector_cases as sel

    tv, mats = ac.fixture_matrices()
    index = CircuitIndex.build(mats["A"], mats["B"], mats["C"], 4, "fx", ck=srs[1])
    assert (index.lg_r, index.lg_c, index.lg_x, index.lg_k) == (3, 3, 2, [3, 3, 3])
    _check_index(index, [mats[n] for n in "ABC"], "fx", srs, 5)
    # rounds 1 and 2: w from x and the private variables, z_M by the registered matrices, h_0
    fx12 = rcc.fixture_rounds12(tv)
    up = lambda v: HipMem.from_numpy(np.ascontiguousarray(v, dtype=np.uint64))  # noqa: E731
    d_x = up(oracle.ntt(rcc.mont(fx12["public"]), direction=oracle.INVERSE))
    d_private, d_w, d_z = up(rcc.mont(fx12["private"])), HipMem(32 * 4), HipMem(32 * 8)
    assert matrices.witness_poly_device(d_private, len(fx12["private"]), d_x, 4, index.lg_c, d_w) == 4
    assert util.fr_mont_to_ints(d_w.download(dtype=np.uint64).reshape(-1, 4)) == fx12["w_lde"]
    assert matrices.assignment_device(d_w, 4, d_x, 4, d_z) == 8
    d_vars, zs = up(rcc.mont(fx12["public"] + fx12["private"])), HipMem(32 * 8 * 3)
    for m, reg in enumerate(index.matrices):
        reg.mul_device(zs.ptr + 32 * 8 * m, 8, d_vars)
    one = rcc.mont([1])
    h_0 = matrices.rowcheck_witness([matrices.RowcheckCircuit(index.lg_r, one[0], one, [tuple(zs.ptr + 32 * 8 * m for m in range(3))])], index.lg_r)
    assert h_0.violations == [0] and rcc.trimmed_ints(h_0.download()) == fx12["h_0"]
    # round 3 from the registered transposes
    fx3 = sel.fixture_round3(tv)
    alpha, eta_b, eta_c = (sel.mont([fx3[key]]) for key in ("alpha", "eta_b", "eta_c"))
    circuit = matrices.LinevalCircuit(index.transposes, index.lg_r, index.lg_c, one[0], one, [matrices.DevicePoly(d_z.ptr, 8, d_z)])
    h_1, _, g_1, _ = matrices.lineval_sumcheck_witness([circuit], alpha[0], eta_b[0], eta_c[0], index.lg_c)
    assert sel.trimmed_ints(h_1.download()) == fx3["h_1"] and sel.trimmed_ints(g_1.download()) == fx3["g_1"]
    # rounds 4 and 5 from the registered arithmetizations
    fx = sc.fixture(tv)
    wit = matrices.matrix_sumcheck_witness(index.ariths, index.lg_r, index.lg_c, fx["alpha"], fx["beta"], 8)
    for name, (_, _, g, _, _) in zip("ABC", wit):
        if name in fx["g"]:
            assert sc.trimmed_ints(g.download()) == fx["g"][name], name
    assert sc.trimmed_ints(matrices.h_2([w[1] for w in wit], fx["deltas"]).download()) == fx["h_2"]
    index.close()
    index.close()  # safe to call twice
    assert not index.polynomials and not index.ariths


def test_circuit_index_of_a_random_circuit(srs):
    """|R| = |V| = 2^9, |K| = 2^10 for all three matrices: the 1 024 SRS points commit polynomials of 1 024 coefficients"""
    mats = sc.random_circuit(21, lg_r=9, lg_c=9, lg_k=(10, 10, 10))
    index = CircuitIndex.build(*mats, 16, "r21", ck=srs[1])
    assert (index.lg_r, index.lg_c, index.lg_x, index.lg_k) == (9, 9, 4, [10, 10, 10])
    _check_index(index, mats, "r21", srs, 6)
    index.close()


def test_circuit_index_refuses_an_input_domain_as_large_as_the_variable_domain():
    _, mats = ac.fixture_matrices()
    with pytest.raises(ValueError, match="must be smaller"):
        CircuitIndex.build(mats["A"], mats["B"], mats["C"], 5, "fx")
    index = CircuitIndex.build(mats["A"], mats["B"], mats["C"], 4, "fx")  # no committer key: no verifying key
    assert index.commitments is None and len(index.polynomials) == 12
    index.close()
