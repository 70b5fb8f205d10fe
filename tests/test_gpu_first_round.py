"""`matrices.first_round_device`: Varuna's round 1 in lock step - for every instance of every circuit z, w, x_poly and z_a, z_b, z_c from one gather
(`snarkvm_hip_fr_assignment_evals`), one inverse transform and one division per instance, and three strided sparse products per circuit.

Compared byte for byte with the per-instance route that stays in the tree (`plugin.NTT` of the public input, `witness_poly_device`,
`assignment_device`, `z_m`), run inside a caller's scope with `rowcheck_witness` consuming its outputs there, and driven from the raw inputs of the
committed Varuna fixture (tests/golden/varuna_circuit0.json) through all five rounds to every polynomial the fixture holds.
"""
import ctypes

import numpy as np
import pytest

from snarkvm_amd import _lib, matrices, plugin
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.layout import NTTDirection, NTTInputOutputOrder, NTTType
from snarkvm_amd.matrices import CircuitIndex, DevicePoly, FirstRoundCircuit, LinevalCircuit, RegisteredMatrix, RowcheckCircuit
from tests import util
from tests.helpers import assignment_cases as ac
from tests.helpers import selector_cases as sel
from tests.helpers import spmv_cases
from tests.helpers import sumcheck_cases as sc

pytestmark = pytest.mark.gpu

R = ac.R
GUARD = ac.GUARD


def _dev(values, device=-1):
    mem = HipMem.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4), device)
    return DevicePoly(mem.ptr, len(values), mem)


class Circuit:
    """three random matrices (tests/helpers/spmv_cases.from_lengths) over num_vars variables, `instances` rows public ++ private, the arena that holds
    the rows `stride` elements apart between guards, and the per-instance route's answers, computed once"""

    def __init__(self, seed, lg_r, lg_c, lg_x, rows, num_vars, instances):
        self.lg_r, self.lg_c, self.lg_x, self.num_vars, self.instances = lg_r, lg_c, lg_x, num_vars, instances
        self.V, self.X, self.R = 1 << lg_c, 1 << lg_x, 1 << lg_r
        self.stride = num_vars + 3
        self.mats = [spmv_cases.from_lengths([(5 * r + seed + j) % 7 for r in range(rows)], num_vars, seed + 10 * j) for j in range(3)]
        self.regs = [RegisteredMatrix(m) for m in self.mats]
        self.rows = np.stack([ac.row(num_vars, 100 * seed + i) for i in range(instances)])
        flat = np.full(((instances - 1) * self.stride + num_vars + 1, 4), GUARD, dtype=np.uint64)
        for i in range(instances):
            flat[i * self.stride : i * self.stride + num_vars] = self.rows[i]
        self.flat = flat
        self.arena = HipMem.from_numpy(flat)
        self.old = [self._old_route(self.rows[i]) for i in range(instances)]
        for answers in self.old:
            for a in answers.values():
                a.setflags(write=False)

    def first_round_circuit(self):
        return FirstRoundCircuit(self.regs, self.lg_r, self.lg_c, self.lg_x, self.arena, self.num_vars, self.stride, self.instances)

    def _old_route(self, row):
        """x_poly by an inverse transform at |X|, w by witness_poly_device, z by assignment_device, z_M by z_m: one instance at a time"""
        public, private = row[: self.X].copy(), row[self.X :].copy()
        x_poly = public.copy()
        plugin.NTT(self.X, x_poly, NTTInputOutputOrder.NN, NTTDirection.Inverse, NTTType.Standard)
        d_private, d_x = _dev(private), _dev(x_poly)
        d_w, d_z = HipMem(32 * max(self.V - self.X, 1)), HipMem(32 * self.V)
        w_len = matrices.witness_poly_device(d_private, len(private), d_x, self.X, self.lg_c, d_w)
        z_len = matrices.assignment_device(d_w, w_len, d_x, self.X, d_z)
        out = {"x_poly": x_poly, "w": d_w.download(32 * w_len, dtype=np.uint64).reshape(-1, 4), "z": d_z.download(32 * z_len, dtype=np.uint64).reshape(-1, 4)}
        for name, reg in zip("abc", self.regs):
            out["z_" + name] = matrices.z_m(reg, public, private, self.R)
        return out

    def check(self, got):
        """a FirstRoundWitness against the per-instance route; the arena is unchanged"""
        assert [len(x) for x in got] == [self.instances] * 5
        for i, old in enumerate(self.old):
            assert (got.z[i].n, got.w[i].n, got.x_poly[i].n) == (self.V, self.V - self.X, self.X)
            assert got.w[i].download().tobytes() == old["w"].tobytes(), i
            assert got.x_poly[i].download().tobytes() == old["x_poly"].tobytes(), i
            z = got.z[i].download()
            assert z[: len(old["z"])].tobytes() == old["z"].tobytes() and not z[len(old["z"]) :].any(), i
            for j, name in enumerate("abc"):
                assert got.z_m[i][j].n == self.R and got.z_m[i][j].download().tobytes() == old["z_" + name].tobytes(), (i, name)
        assert np.array_equal(self.arena.download(dtype=np.uint64).reshape(-1, 4), self.flat), "the arena was written"

    def close(self):
        for r in self.regs:
            r.close()
        self.arena.free()


@pytest.fixture(scope="module")
def two_circuits():
    """|V| = 2^10 with |X| = 2^4, |R| = 2^9 and 3 instances; |V| = 2^6 with |X| = 2^2, |R| = 2^5 and 1 instance"""
    cs = [Circuit(1, 9, 10, 4, 500, 1000, 3), Circuit(2, 5, 6, 2, 30, 60, 1)]
    yield cs
    for c in cs:
        c.close()


def test_two_circuits_equal_the_per_instance_route(two_circuits):
    got = matrices.first_round_device([c.first_round_circuit() for c in two_circuits], circuit_ids=["7a", "7b"], hiding_bound=1)
    assert len(got) == 2
    for c, g in zip(two_circuits, got):
        c.check(g)
    labels = [[p.label for p in g.w_labeled] for g in got]
    assert labels == [["circuit_7a_w_00000000", "circuit_7a_w_00000001", "circuit_7a_w_00000002"], ["circuit_7b_w_00000000"]]
    for g in got:
        for p, w in zip(g.w_labeled, g.w):
            assert (p.ptr, p.n, p.degree_bound, p.hiding_bound) == (w.ptr, w.n, None, 1)
    assert got[0].w[0].download().any() and got[0].z_m[2][1].download().any()
    # the default labels carry the position of the circuit; no circuit, no instance: nothing to do
    assert matrices.first_round_device([]) == []
    empty = matrices.first_round_device([two_circuits[1].first_round_circuit()._replace(instances=0)])
    assert [len(x) for x in empty[0]] == [0] * 5
    again = matrices.first_round_device([two_circuits[1].first_round_circuit()])
    assert [p.label for p in again[0].w_labeled] == ["circuit_0_w_00000000"] and again[0].w_labeled[0].hiding_bound is None
    two_circuits[1].check(again[0])


def test_refusals_of_the_driver(two_circuits):
    c = two_circuits[0].first_round_circuit()
    for bad in (c._replace(lg_x=11), c._replace(num_vars=8), c._replace(num_vars=1025), c._replace(matrices=c.matrices[:2]), c._replace(lg_r=8),
                c._replace(stride=999), c._replace(num_vars=999)):
        with pytest.raises(ValueError, match="first_round_device"):
            matrices.first_round_device([bad])
    with pytest.raises(ValueError, match="one circuit id per circuit"):
        matrices.first_round_device([c], circuit_ids=[])


def _violations(circuits):
    """{(circuit, instance): the rows with z_a z_b != z_c}, by Python integers"""
    out = {}
    for ci, c in enumerate(circuits):
        for i, answers in enumerate(c.old):
            za, zb, zc = (util.fr_mont_to_ints(answers["z_" + n]) for n in "abc")
            out[(ci, i)] = sum(1 for a, b, x in zip(za, zb, zc) if a * b % R != x)
    return out


def test_inside_a_callers_scope_with_the_rowcheck_consuming_its_outputs(two_circuits):
    """first_round_device and rowcheck_witness enqueued in ONE scope of the caller's: nothing is waited for in between; after scope_end the round-1
    outputs equal the per-instance route's and h_0 equals that of the same rowcheck over uploaded copies of the per-instance z_M (the random
    circuits are not satisfied: the counts of violated rows, equal to those by Python integers, arrive with scope_end)"""
    L = _lib.lib()
    combiners = [(sel.rnd(1, 60 + i)[0], sel.rnd(c.instances, 70 + i)) for i, c in enumerate(two_circuits)]

    def in_scope(run):
        _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(two_circuits[0].arena.ptr)))
        try:
            return run()
        finally:
            _lib.check(L.snarkvm_hip_scope_end())

    def both_rounds():
        assert L.snarkvm_hip_scope_stream()
        got = matrices.first_round_device([c.first_round_circuit() for c in two_circuits])
        # the polynomials are read before round 2 consumes z_a, z_b, z_c: copies inside the same scope
        keep = [[HipMem(32 * 3 * c.R) for _ in range(c.instances)] for c in two_circuits]
        for c, g, ks in zip(two_circuits, got, keep):
            for triple, k in zip(g.z_m, ks):
                for j, p in enumerate(triple):
                    k.copy_from(32 * c.R * j, p.ptr, 32 * c.R)
        rcs = [RowcheckCircuit(c.lg_r, cc, ic, g.z_m) for c, g, (cc, ic) in zip(two_circuits, got, combiners)]
        return got, keep, matrices.rowcheck_witness(rcs, 9)

    got, keep, h_0 = in_scope(both_rounds)
    for c, g, ks in zip(two_circuits, got, keep):
        for i, k in enumerate(ks):
            copies = k.download(dtype=np.uint64).reshape(3, c.R, 4)
            for j, name in enumerate("abc"):
                assert copies[j].tobytes() == c.old[i]["z_" + name].tobytes(), (i, name)
            assert g.w[i].download().tobytes() == c.old[i]["w"].tobytes()
            assert g.x_poly[i].download().tobytes() == c.old[i]["x_poly"].tobytes()
            assert g.z[i].download().tobytes() == c.old[i]["z"].tobytes()
    want_viol = _violations(two_circuits)
    assert dict(zip(h_0.members, h_0.violations)) == want_viol and any(want_viol.values())

    def old_rowcheck():
        ups = [[tuple(_dev(answers["z_" + n]) for n in "abc") for answers in c.old] for c in two_circuits]
        rcs = [RowcheckCircuit(c.lg_r, cc, ic, u) for c, u, (cc, ic) in zip(two_circuits, ups, combiners)]
        return ups, matrices.rowcheck_witness(rcs, 9)

    _, h_old = in_scope(old_rowcheck)
    assert dict(zip(h_old.members, h_old.violations)) == want_viol
    assert h_0.n == 512 and h_0.download().tobytes() == h_old.download().tobytes() and h_0.download().any()


def test_circuit_0_from_raw_inputs_through_every_round(golden):
    """CircuitIndex.build -> first_round_device -> rowcheck_witness (both in one scope of the caller's) -> lineval_sumcheck_witness ->
    matrix_sumcheck_witness -> h_2 from the fixture's A, B, C as CSR, public (1, 8, 32, 128), private (2, 4, 2) and its challenges (alpha =
    challenges[0], eta_b, eta_c = [2], [3], beta = [4], deltas = [5:8], combiners one, non-hiding: tests/helpers/selector_cases.fixture_round3,
    sumcheck_cases.fixture): w_lde, z_lde, h_0, g_1, h_1, g_a, g_b, h_2 of the fixture.  g_c: the fixture's g_c is a copy of its g_b (the reference's
    dump wrote g_b twice), so g_c is compared with the oracle's chain over C's arithmetization (sumcheck_cases.chain_expected); C is pinned by
    h_2 as well."""
    tv = golden["varuna"]
    poly = lambda name: [int(x) for x in tv["polynomials"][name]]
    f3, f4 = sel.fixture_round3(tv), sc.fixture(tv)
    assert poly("g_c") == poly("g_b")
    public, private = [1, 8, 32, 128], [2, 4, 2]
    assert [int(v) for v in tv["witness"][1]] == public + private
    a, b, c = (sel.sparse(f3["matrices"][name], 7) for name in "ABC")
    idx = CircuitIndex.build(a, b, c, 4, 0)
    assert (idx.lg_r, idx.lg_c, idx.lg_x, idx.lg_k) == (3, 3, 2, [3, 3, 3])
    d_vars = HipMem.from_numpy(ac.mont(public + private))
    one = ac.mont([1])
    L = _lib.lib()
    _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(d_vars.ptr)))
    try:
        (first,) = matrices.first_round_device([FirstRoundCircuit(idx.matrices, idx.lg_r, idx.lg_c, idx.lg_x, d_vars, 7, 7, 1)])
        h_0 = matrices.rowcheck_witness([RowcheckCircuit(idx.lg_r, one[0], one, first.z_m)], idx.lg_r)
    finally:
        _lib.check(L.snarkvm_hip_scope_end())
    assert h_0.ensure_divisible() is h_0 and h_0.violations == [0]
    assert first.w_labeled[0].label == "circuit_0_w_00000000"
    assert sel.trimmed_ints(first.w[0].download()) == poly("w_lde")
    assert sel.trimmed_ints(first.z[0].download()) == poly("z_lde")
    assert util.fr_mont_to_ints(first.x_poly[0].download()) == util.fr_mont_to_ints(_x_poly(public))
    assert sel.trimmed_ints(h_0.download()) == poly("h_0")
    alpha, eta_b, eta_c = (ac.mont([f3[k]]) for k in ("alpha", "eta_b", "eta_c"))
    lineval = LinevalCircuit(idx.transposes, idx.lg_r, idx.lg_c, one[0], one, first.z)
    h_1, _, g_1, _ = matrices.lineval_sumcheck_witness([lineval], alpha[0], eta_b[0], eta_c[0], idx.lg_c)
    assert sel.trimmed_ints(h_1.download()) == poly("h_1") and sel.trimmed_ints(g_1.download()) == poly("g_1")
    wit = matrices.matrix_sumcheck_witness(idx.ariths, idx.lg_r, idx.lg_c, f4["alpha"], f4["beta"], 8)
    for name, (_, _, g, _, _) in zip("ABC", wit):
        if name == "C":
            assert np.array_equal(g.download(), sc.chain_expected(*f4["ariths"]["C"], f4["alpha"], f4["beta"], f4["scales"], 8)[2])
        else:
            assert sel.trimmed_ints(g.download()) == poly("g_" + name.lower()), name
    assert sel.trimmed_ints(matrices.h_2([w[1] for w in wit], f4["deltas"]).download()) == poly("h_2")
    idx.close(), d_vars.free()


def _x_poly(public):
    x = ac.mont(public)
    plugin.NTT(len(public), x, NTTInputOutputOrder.NN, NTTDirection.Inverse, NTTType.Standard)
    return x
