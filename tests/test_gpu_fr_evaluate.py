"""`snarkvm_hip_fr_evaluate` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: fr_evaluate_kernel and fr_reduce_final_kernel), and what is
built on it: `SonicKZG10.evaluate_polynomials_device` and the linear route of `SonicKZG10.evaluate_combinations_device`.

Every value is compared bit for bit with the polynomial evaluated in Python integers (tests/helpers/evaluate_cases.py).  The case lists are
those of tests/test_fr_evaluate_host.py, on host and on device operands; then the sizes at which the production geometry first matters: 2^19 - 1
and 2^19 (a thread has at most one coefficient and every exponent below 2^19 occurs), 2^19 + 1 (the first second element) and
(G + 1) 2^19 + 3 (a full group and a tail).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, plugin, sonic_pc
from snarkvm_amd.devmem import HipMem
from tests import util
from tests.helpers import evaluate_cases as ec
from tests.test_gpu_fr_lincomb import Arena

pytestmark = pytest.mark.gpu

R = ec.R


def run(polys, points, on_device):
    """one call over host arrays, or over one device arena with a guard element behind every member (checked afterwards)"""
    k = len(polys)
    if not on_device:
        out = np.full((k + 1, 4), ec.GUARD, dtype=np.uint64)
        pp, pl, zs = ec.call_args([p.ctypes.data for p in polys], [len(p) for p in polys], points)
        _lib.check(_lib.lib().snarkvm_hip_fr_evaluate(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(k), pp, pl, ctypes.c_void_p(zs.ctypes.data), 0))
        assert (out[k] == ec.GUARD).all()
        return out[:k]
    arena = Arena(polys, 0)
    got = plugin.fr_evaluate_device([arena.ptr(j) if len(p) else None for j, p in enumerate(polys)], [len(p) for p in polys], np.concatenate(points))
    arena.result()
    return got


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("T", [64, 768])
def test_every_length_at_every_point(T, on_device):
    polys, points, want = ec.grid_case(T)
    got = run(polys, points, on_device)
    for k in range(len(polys)):
        assert np.array_equal(got[k], want[k]), (k, len(polys[k]), ec.POINT_NAMES[k // 10])


@pytest.mark.parametrize("on_device", [0, 1])
def test_member_lists(on_device):
    z = ec.point("generic", 64)
    lens = [0, 1, 300, 2 * ec.group() * 768 + 1]
    polys = [ec.coefficients(n, "mixed", seed=2 + k) for k, n in enumerate(lens)]
    assert np.array_equal(run(polys, [z] * 4, on_device), np.concatenate([ec.expected(p, z) for p in polys])), "ragged lengths"
    for n_points in (1, 2, max(5, ec.POINTS + 1)):
        polys, points, want = ec.list_case(2 * n_points + 1, n_points, longest=700)
        assert np.array_equal(run(polys, points, on_device), want), n_points
    for count in (ec.MEMBERS, ec.MEMBERS + 1, 2 * ec.MEMBERS + 2):
        polys, points, want = ec.list_case(count, 2)
        assert np.array_equal(run(polys, points, on_device), want), count


def test_python_layer_and_one_buffer_at_two_points():
    p = ec.coefficients(1000, "mixed")
    z1, z2 = ec.rnd(2, 6)[0:1], ec.rnd(2, 6)[1:2]
    want = np.concatenate([ec.expected(p, z1), ec.expected(p, z2), ec.expected(p[:500], z1)])
    assert np.array_equal(plugin.fr_evaluate([p, p, p[:500]], np.concatenate([z1, z2, z1])), want)
    mem = HipMem.from_numpy(p)
    assert np.array_equal(plugin.fr_evaluate_device([mem.ptr, mem.ptr, mem.ptr], [1000, 1000, 500], np.concatenate([z1, z2, z1])), want)
    assert np.array_equal(plugin.fr_evaluate_device([], [], np.zeros((0, 4), dtype=np.uint64)), np.zeros((0, 4), dtype=np.uint64))
    assert not plugin.fr_evaluate_device([None, None], [0, 0], np.concatenate([z1, z2])).any()
    with pytest.raises(ValueError, match="length mismatch"):
        plugin.fr_evaluate_device([mem.ptr], [1000, 1000], z1)
    with pytest.raises(ValueError, match="length mismatch"):
        plugin.fr_evaluate([p, p], z1)


# ---- the production geometry: 2048 workgroups of 256 threads ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """(G + 1) 2^19 + 3 random coefficients (about 84 MB for G = 4), on the host and resident; shared, never written"""
    g = ec.geometry(1 << 30)
    T = g["cap"] * g["threads"]
    assert g["blocks"] == g["cap"] and T == 1 << 19
    host = ec.rnd((g["G"] + 1) * T + 3, 7)
    host.setflags(write=False)
    mem = HipMem.from_numpy(host)
    yield T, host, mem
    mem.free()


def test_around_one_coefficient_per_thread(big):
    """prefixes of one buffer in one call: T - 1, T and T + 1 coefficients at a generic point and at minus one, and T at zero"""
    T, host, mem = big
    z, m1, zero = ec.point("generic", T), ec.point("minus_one", T), ec.point("zero", T)
    lens = [T - 1, T, T + 1, T + 1, T]
    points = [z, z, z, m1, zero]
    got = plugin.fr_evaluate_device([mem.ptr] * 5, lens, np.concatenate(points))
    for k, (n, x) in enumerate(zip(lens, points)):
        assert np.array_equal(got[k : k + 1], ec.expected(host[:n], x)), (n, k)


def test_a_full_group_and_a_tail(big):
    T, host, mem = big
    z = ec.point("generic", T)
    got = plugin.fr_evaluate_device([mem.ptr], [len(host)], z)
    assert np.array_equal(got, ec.expected(host, z))
    assert np.array_equal(mem.download(64, 32 * (len(host) - 2), dtype=np.uint64).reshape(2, 4), host[-2:])


@pytest.mark.parametrize("n", [1, 5000, (1 << 19) + 1])
def test_equals_the_remainder_of_the_divisions(big, n):
    """snarkvm_hip_fr_divide_by_linear's remainder and snarkvm_hip_fr_open_fold without a quotient, on the same resident operand"""
    _, host, mem = big
    z = ec.point("generic", 64)
    L = _lib.lib()
    rem = np.zeros((1, 4), dtype=np.uint64)
    _lib.check(L.snarkvm_hip_fr_divide_by_linear(None, ctypes.c_void_p(rem.ctypes.data), ctypes.c_void_p(mem.ptr), ctypes.c_size_t(n), ctypes.c_void_p(z.ctypes.data), 1))
    fold = plugin.fr_open_fold_device(None, n, [mem.ptr], [n], sonic_pc.FR_ONE.reshape(1, 4), z)
    got = plugin.fr_evaluate_device([mem.ptr], [n], z)
    assert np.array_equal(got, rem) and np.array_equal(got, fold)


# ---- refusals, scopes, devices ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_results_untouched():
    p, z = ec.coefficients(100, "mixed"), ec.point("generic", 64)
    mem = HipMem.from_numpy(p)
    L = _lib.lib()
    out = np.full((3, 4), ec.GUARD, dtype=np.uint64)
    o, one = ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(1)
    zs = ctypes.c_void_p(z.ctypes.data)
    for on_device, ptr in ((0, p.ctypes.data), (1, mem.ptr)):
        pp, pl, _ = ec.call_args([ptr], [100], [z])
        null = (ctypes.c_void_p * 1)(None)
        too_long = (ctypes.c_size_t * 1)((1 << 29) + 1)
        for err in (L.snarkvm_hip_fr_evaluate(None, one, pp, pl, zs, on_device), L.snarkvm_hip_fr_evaluate(o, one, None, pl, zs, on_device),
                    L.snarkvm_hip_fr_evaluate(o, one, pp, None, zs, on_device), L.snarkvm_hip_fr_evaluate(o, one, pp, pl, None, on_device),
                    L.snarkvm_hip_fr_evaluate(o, one, null, pl, zs, on_device), L.snarkvm_hip_fr_evaluate(o, one, pp, too_long, zs, on_device),
                    L.snarkvm_hip_fr_evaluate(o, ctypes.c_size_t(65536), pp, pl, zs, on_device)):
            with pytest.raises(_lib.HipError) as e:
                _lib.check(err)
            assert e.value.code == ec.INVALID_VALUE
        _lib.check(L.snarkvm_hip_fr_evaluate(None, ctypes.c_size_t(0), None, None, None, on_device))  # count == 0: nothing is touched
    assert (out == ec.GUARD).all()
    with pytest.raises(_lib.HipError):  # a host pointer among device members
        plugin.fr_evaluate_device([mem.ptr, p.ctypes.data], [100, 100], np.concatenate([z, z]))


def test_inside_a_scope_behind_a_transform():
    """ntt_device -> fr_evaluate of the transform (twice, at two points) and of an untouched neighbour, all enqueued inside one scope: the values
    arrive at scope_end and are those of the oracle's transform; the same calls outside a scope give the same bytes; a repeat grows no workspace"""
    lg = 12
    n = 1 << lg
    x, y = ec.rnd(n, 1).copy(), ec.rnd(n, 2)
    transformed = oracle.ntt(x)
    z1, z2 = ec.rnd(2, 6)[0:1], ec.rnd(2, 6)[1:2]
    points = np.concatenate([z1, z2, z1])
    want = np.concatenate([ec.expected(transformed, z1), ec.expected(transformed, z2), ec.expected(y[:777], z1)])
    L = _lib.lib()
    stats = np.zeros(5, dtype=np.uint64)
    results = []
    arena = Arena([x, y], 0)
    for attempt in range(3):
        arena.mem.upload(x)  # the transform is in place
        in_scope = attempt < 2
        if in_scope:
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(arena.mem.ptr)))
        try:
            _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(arena.ptr(0)), lg, 0, 0, 0))
            got = plugin.fr_evaluate_device([arena.ptr(0), arena.ptr(0), arena.ptr(1)], [n, n, 777], points)
            if in_scope:
                assert not got.any(), "inside a scope the call is only enqueued"
        finally:
            if in_scope:
                _lib.check(L.snarkvm_hip_scope_end())
        if attempt == 0:
            L.snarkvm_hip_alloc_stats(None, 1)
        elif attempt == 1:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        assert np.array_equal(got, want), attempt
        now = arena.mem.download(dtype=np.uint64).reshape(-1, 4)
        assert np.array_equal(now[:n], transformed) and np.array_equal(now[n + 1 : 2 * n + 1], y)
        assert (now[n] == ec.GUARD).all() and (now[2 * n + 1 :] == ec.GUARD).all()
        results.append(got.tobytes())
    assert not stats[:4].any(), stats
    assert results[0] == results[1] == results[2]


def test_a_repeated_host_call_grows_no_workspace():
    polys, points, want = ec.list_case(9, 4, longest=3000)
    L = _lib.lib()
    run(polys, points, 0)
    L.snarkvm_hip_alloc_stats(None, 1)
    got = run(polys, points, 0)
    stats = np.zeros(5, dtype=np.uint64)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats
    assert np.array_equal(got, want)


MULTI_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from snarkvm_amd import msm, plugin
from snarkvm_amd.devmem import HipMem
from tests.helpers import evaluate_cases as ec

assert msm.num_devices() == 2, msm.num_devices()
polys, points, want = ec.list_case(7, 3, longest=2500)
lens = [len(p) for p in polys]
flat = np.concatenate([p for p in polys if len(p)] + [np.full((1, 4), ec.GUARD, dtype=np.uint64)])
offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
mems = []
for device in (0, 1, 1, 0):
    mem = HipMem.from_numpy(flat, device)
    got = plugin.fr_evaluate_device([mem.ptr + 32 * int(o) if n else None for o, n in zip(offs, lens)], lens, np.concatenate(points))
    assert np.array_equal(got, want), device
    assert np.array_equal(mem.download(dtype=np.uint64).reshape(-1, 4), flat), device
    mems.append(mem)
# members of two LOGICAL devices that are one physical device share its memory: one call takes both (the refusal of members on different
# devices goes by the physical device and needs two GPUs to show)
got = plugin.fr_evaluate_device([mems[0].ptr, mems[1].ptr], [lens[0], lens[0]], np.concatenate(points[:2]))
assert np.array_equal(got, np.concatenate([ec.expected(polys[0], points[0]), ec.expected(polys[0], points[1])]))
assert np.array_equal(plugin.fr_evaluate(polys, np.concatenate(points)), want)
print("EVALUATE_MULTI_OK")
'''


def test_two_logical_devices():
    env = dict(os.environ, SNARKVM_HIP_DEVICES="0,0")
    r = subprocess.run([sys.executable, "-c", MULTI_SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert "EVALUATE_MULTI_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- SonicKZG10.evaluate_polynomials_device / evaluate_combinations_device --------------------------------------------------------------------
def gamma_shape(circuits):
    """(labels, combinations) of a gamma point (ahp.rs:173-389): g_a, g_b, g_c of every circuit alone, then h_2 with the a_poly_* / b_poly_* of every
    circuit in one combination that also carries a ONE term"""
    singles = [f"g_{m}_{c}" for c in range(circuits) for m in "abc"]
    inner = ["h_2"] + [f"{ab}_poly_{m}_{c}" for c in range(circuits) for m in "abc" for ab in "ab"]
    return singles + inner, [(s, [s], False) for s in singles] + [("matrix_sumcheck", inner, True)]


def beta_shape(instances):
    """g_1, mask_poly, h_1 in one combination, every w_j alone"""
    ws = [f"w_{j}" for j in range(instances)]
    return ["g_1", "mask_poly", "h_1"] + ws, [("lineval_sumcheck", ["g_1", "mask_poly", "h_1"], True)] + [(w, [w], False) for w in ws]


def combination_value(terms, constant, coeffs_of, z):
    """(sum_k a_k p_k)(z) + constant by Python integers: the combination is formed coefficient by coefficient, then evaluated"""
    n = max(len(coeffs_of[t]) for _, t in terms)
    comb = [0] * n
    for a, t in terms:
        ai = ec.point_int(a)
        for i, c in enumerate(ec.mem_ints(coeffs_of[t])):
            comb[i] = (comb[i] + ai * c) % R
    comb_mem = np.concatenate([ec.from_mem_int(c) for c in comb])
    value = int.from_bytes(ec.expected(comb_mem, z).tobytes(), "little")
    return ec.from_mem_int(value + (int.from_bytes(np.ascontiguousarray(constant).tobytes(), "little") if constant is not None else 0))


@pytest.mark.parametrize("shape,param", [("gamma", 1), ("gamma", 2), ("beta", 1), ("beta", 4)])
def test_combinations_by_both_routes(shape, param):
    n = 1 << 10
    labels, combos = gamma_shape(param) if shape == "gamma" else beta_shape(param)
    coeffs_of = {t: np.ascontiguousarray(ec.rnd(n + j, 1 + j % 5)[j:]) if j % 3 else ec.coefficients(n - 5 * j, "padded", seed=j) for j, t in enumerate(labels)}
    res = [sonic_pc.ResidentPolynomial(t, HipMem.from_numpy(coeffs_of[t]), len(coeffs_of[t])) for t in labels]
    a = ec.rnd(len(labels) + 2, 8)
    z, z_other = ec.rnd(2, 21)[0:1], ec.rnd(2, 21)[1:2]
    lcs, terms_of, const_of = [], {}, {}
    for name, members, with_one in combos:
        terms = [(a[labels.index(t)], t) for t in members]
        const_of[name] = a[-1] if with_one else None
        terms_of[name] = terms
        lcs.append(sonic_pc.LinearCombination.new(name, terms + ([(a[-1], sonic_pc.ONE)] if with_one else [])))
    query_set = [(name, (shape, z)) for name, _, _ in combos] + [(combos[0][0], ("other", z_other))]
    S = sonic_pc.SonicKZG10
    fold = S.evaluate_combinations_device(lcs, res, query_set, route="fold")
    linear = S.evaluate_combinations_device(lcs, res, query_set, route="linear")
    default = S.evaluate_combinations_device(lcs, res, query_set)
    assert set(fold) == set(linear) == set(default) == {(label, name) for label, (name, _) in query_set}
    for label, (name, point) in query_set:
        want = combination_value(terms_of[label], const_of[label], coeffs_of, point)
        assert np.array_equal(linear[(label, name)].reshape(1, 4), want), (label, name)
        assert fold[(label, name)].tobytes() == linear[(label, name)].tobytes() == default[(label, name)].tobytes(), (label, name)
    # the single polynomials of the point: a proof's `evaluations`
    singles = [(t, (shape, z)) for t in labels[:4]] + [(labels[0], ("other", z_other))]
    values = S.evaluate_polynomials_device(res, singles)
    assert set(values) == {(t, name) for t, (name, _) in singles}
    for t, (name, point) in singles:
        assert np.array_equal(values[(t, name)].reshape(1, 4), ec.expected(coeffs_of[t], point)), (t, name)
    with pytest.raises(sonic_pc.PCError, match=r"MissingEval\(nope\)"):
        S.evaluate_polynomials_device(res, [("nope", (shape, z))])
    with pytest.raises(sonic_pc.PCError, match="MissingEval"):
        S.evaluate_combinations_device(lcs, res, [("nope", (shape, z))], route="linear")
    with pytest.raises(ValueError):
        S.evaluate_combinations_device(lcs, res, query_set, route="other")
    L = _lib.lib()
    _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(res[0].ptr)))
    try:
        with pytest.raises(sonic_pc.PCError, match="not inside a scope"):
            S.evaluate_polynomials_device(res, singles)
        with pytest.raises(sonic_pc.PCError, match="not inside a scope"):
            S.evaluate_combinations_device(lcs, res, query_set, route="linear")
    finally:
        _lib.check(L.snarkvm_hip_scope_end())


def test_the_evaluations_of_the_fixture(golden):
    """tests/golden/varuna_circuit0.json: g_1 at beta = challenges[4] and g_a, g_b, g_c at gamma = challenges[8], from the fixture's coefficient lists"""
    tv = golden["varuna"]
    ch = [int(x) for x in tv["challenges"].split()]
    assert len(ch) == 9
    beta, gamma = util.ints_to_fr_mont([ch[4]]), util.ints_to_fr_mont([ch[8]])
    ints = {name: [int(x) for x in tv["polynomials"][name]] for name in ("g_1", "g_a", "g_b", "g_c")}
    res = [sonic_pc.ResidentPolynomial(name, HipMem.from_numpy(util.ints_to_fr_mont(cs)), len(cs)) for name, cs in ints.items()]
    query_set = [("g_1", ("beta", beta)), ("g_a", ("gamma", gamma)), ("g_b", ("gamma", gamma)), ("g_c", ("gamma", gamma))]
    values = sonic_pc.SonicKZG10.evaluate_polynomials_device(res, query_set)
    for name, (point_name, _) in query_set:
        x = ch[4] if point_name == "beta" else ch[8]
        want = sum(c * pow(x, i, R) for i, c in enumerate(ints[name])) % R
        assert util.fr_mont_to_ints(values[(name, point_name)]) == [want], name
