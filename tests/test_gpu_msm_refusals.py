"""What the registered-bases / registered-MSM entry points of G1 and G2 REFUSE, pinned call by call: the numeric code, the message (with the
`api.hip:<line>` number masked - it moves with the source) and that a refused call leaves its output bytes alone.  The expected texts are those of
the sources; the two curves differ on purpose in places (the window_bits refusal is a std::runtime_error with code 1 for G1 and a HIP failure for
G2, the batch entry points share the texts of the common dispatch) and the table below says where.  Also the valid edge n == 0 on every single-MSM
entry point, outside a scope and inside an ASYNC_MSM scope: the point at infinity - on return for G2, after scope_end at the latest for G1.  Only the
G2 side pins the scope rule for empty MSMs (answered on return, never queued): for G1 "after scope_end at the latest" holds whether or not the empty
call was enqueued, so this file cannot tell."""
import ctypes
import re

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, synthetic
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.layout import G1_AFFINE, G2_AFFINE
from tests import util

pytestmark = pytest.mark.gpu

N1, N2 = 8, 4  # registered G1 / G2 bases
SCOPE_ASYNC_MSM = 1
FILL = 0xA5
TABLES_TEXT = "tables must be 1, 2, 4, 8 or 16, or 254 <= tables * window_bits <= 288 with window_bits in 2..23"
NOT_A_DEVICE_POINTER = "device pointer does not belong to a device in use (snarkvm_hip_set_devices)"


def hip_invalid(what):
    """a hip_failure{hipErrorInvalidValue, what}: code 1, the source position masked"""
    return 1, f"snarkvm_hip: {what} failed at api.hip:#: invalid argument"


def runtime_error(what):
    """a std::runtime_error: code 1, no source position"""
    return 1, f"snarkvm_hip: {what}"


def refusal(err):
    with pytest.raises(_lib.HipError) as ei:
        _lib.check(err)
    return ei.value.code, re.sub(r"api\.hip:\d+", "api.hip:#", ei.value.message)


class Env:
    def __init__(self):
        L = self.L = _lib.lib()
        self.g1 = np.ascontiguousarray(oracle.g1_gen_bases(util.g1_generator_affine(), 1, N1), dtype=G1_AFFINE)
        self.g2 = np.ascontiguousarray(synthetic.g2_points(N2), dtype=G2_AFFINE)
        self.sc = synthetic.random_fr_integers(2 * N1, 0x5EF)
        self.h16, self.hw, self.g16, self.gw = (ctypes.c_void_p() for _ in range(4))
        _lib.check(L.snarkvm_hip_register_bases_tables(ctypes.byref(self.h16), self.g1.ctypes.data, N1, 104, 0, 16))
        _lib.check(L.snarkvm_hip_register_bases_windowed(ctypes.byref(self.hw), self.g1.ctypes.data, N1, 104, 0, 17, 15))
        _lib.check(L.snarkvm_hip_register_bases_g2(ctypes.byref(self.g16), self.g2.ctypes.data, N2, 200, 16, 0))
        _lib.check(L.snarkvm_hip_register_bases_g2(ctypes.byref(self.gw), self.g2.ctypes.data, N2, 200, 17, 15))
        self.dsc = HipMem.from_numpy(self.sc)  # the same scalars in device memory

    def close(self):
        self.L.snarkvm_hip_free_bases(self.h16)
        self.L.snarkvm_hip_free_bases(self.hw)
        self.L.snarkvm_hip_free_bases_g2(self.g16)
        self.L.snarkvm_hip_free_bases_g2(self.gw)
        self.dsc.free()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def _check_cases(cases, out):
    """cases: [(label, call(out_address) -> RustError, (code, text))]; `out` must come back untouched from every one"""
    for label, call, want in cases:
        out[:] = FILL
        got = refusal(call(out.ctypes.data))
        assert got == want, label
        assert (out == FILL).all(), label + ": a refused call wrote to its output"


def _single_cases(fn, name, h, n, sc, window_bits_refusal, ex):
    """the refusals of one single-MSM entry point over handle h of n bases.  ex: the two-range form (off0, n0, off1, n1, ..., montgomery)."""
    if ex:
        call = lambda out, h=h, off=0, cnt=n, s=sc, dev=0, wb=0, off1=0, n1=0: fn(out, h, off, cnt, off1, n1, s, dev, 0, wb)
    else:
        call = lambda out, h=h, off=0, cnt=n, s=sc, dev=0, wb=0: fn(out, h, off, cnt, s, dev, wb)
    cases = [
        ("null handle", lambda o: call(o, h=None), hip_invalid(f"{name}: range exceeds the registered bases")),
        ("null out", lambda o: call(None), hip_invalid(f"{name}: null argument")),
        ("null scalars", lambda o: call(o, s=None), hip_invalid(f"{name}: null argument")),
        ("range one past the end", lambda o: call(o, off=1), hip_invalid(f"{name}: range exceeds the registered bases")),
        ("count one past the end", lambda o: call(o, cnt=n + 1), hip_invalid(f"{name}: range exceeds the registered bases")),
        ("window_bits 1", lambda o: call(o, wb=1), window_bits_refusal(f"{name}: window_bits must be 0 or 2..23")),
        ("window_bits 24", lambda o: call(o, wb=24), window_bits_refusal(f"{name}: window_bits must be 0 or 2..23")),
        ("host pointer as device pointer", lambda o: call(o, dev=1), hip_invalid(NOT_A_DEVICE_POINTER)),
    ]
    if ex:
        cases.append(("second range one past the end", lambda o: call(o, cnt=1, off1=n, n1=1), hip_invalid(f"{name}: range exceeds the registered bases")))
    return cases


def test_g1_single_entry_points_refuse(env):
    out = np.zeros(144, dtype=np.uint8)
    for h in (env.h16, env.hw):
        _check_cases(_single_cases(env.L.snarkvm_hip_msm_registered, "msm_registered", h, N1, env.sc.ctypes.data, runtime_error, False), out)
        _check_cases(_single_cases(env.L.snarkvm_hip_msm_registered_ex, "msm_registered_ex", h, N1, env.sc.ctypes.data, runtime_error, True), out)


def test_g2_single_entry_point_refuses(env):
    out = np.zeros(288, dtype=np.uint8)
    for h in (env.g16, env.gw):
        _check_cases(_single_cases(env.L.snarkvm_hip_msm_g2_registered, "msm_g2_registered", h, N2, env.sc.ctypes.data, hip_invalid, False), out)


def _batch_cases(fn, name, h, n, sc, window_bits_refusal, form):
    """form: 'g1' (.., on_device, montgomery, window_bits), 'g1_ex' (two ranges), 'g2' (.., on_device, window_bits).  The range, the null scalar vector
    and the device check are the common dispatch's (msm_batch.hip.h): their texts say msm_registered_batch whatever the entry point."""
    one = lambda v: (ctypes.c_size_t * 1)(v)

    def call(out, h=h, off=0, cnt=n, s=sc, dev=0, wb=0, outs_null=False, arrays=True, off1=0, n1=0):
        ptrs = (ctypes.c_void_p * 1)(s)
        offs, ns = (one(off), one(cnt)) if arrays else (None, None)
        o = None if outs_null else out
        if form == "g1":
            return fn(o, h, 1, offs, ns, ptrs, dev, 0, wb)
        if form == "g1_ex":
            return fn(o, h, 1, offs, ns, one(off1) if arrays else None, one(n1) if arrays else None, ptrs, dev, 0, wb)
        return fn(o, h, 1, offs, ns, ptrs, dev, wb)

    cases = [
        ("null handle", lambda o: call(o, h=None), hip_invalid(f"{name}: null handle")),
        ("null outs", lambda o: call(o, outs_null=True), hip_invalid(f"{name}: null argument")),
        ("null offsets and counts", lambda o: call(o, arrays=False), hip_invalid(f"{name}: null argument")),
        ("null scalar vector", lambda o: call(o, s=None), hip_invalid("msm_registered_batch: null scalar vector")),
        ("range one past the end", lambda o: call(o, off=1), hip_invalid("msm_registered_batch: range exceeds the registered bases")),
        ("window_bits 1", lambda o: call(o, wb=1), window_bits_refusal(f"{name}: window_bits must be 0 or 2..23")),
        ("window_bits 24", lambda o: call(o, wb=24), window_bits_refusal(f"{name}: window_bits must be 0 or 2..23")),
        ("host pointer as device pointer", lambda o: call(o, dev=1), hip_invalid("msm_registered_batch: scalars are not on a device in use")),
    ]
    if form == "g1_ex":
        cases.append(("second range one past the end", lambda o: call(o, cnt=1, off1=n, n1=1), hip_invalid("msm_registered_batch: range exceeds the registered bases")))
    return cases


def test_batch_entry_points_refuse(env):
    L, sc = env.L, env.sc.ctypes.data
    out = np.zeros(288, dtype=np.uint8)
    for h in (env.h16, env.hw):
        _check_cases(_batch_cases(L.snarkvm_hip_msm_registered_batch, "msm_registered_batch", h, N1, sc, runtime_error, "g1"), out)
        _check_cases(_batch_cases(L.snarkvm_hip_msm_registered_batch_ex, "msm_registered_batch_ex", h, N1, sc, runtime_error, "g1_ex"), out)
    for h in (env.g16, env.gw):
        _check_cases(_batch_cases(L.snarkvm_hip_msm_g2_registered_batch, "msm_g2_registered_batch", h, N2, sc, hip_invalid, "g2"), out)


def test_registrations_refuse(env):
    L = env.L
    sentinel = 0x5A5A5A5A5A5A5A5A
    g1, g2 = env.g1.ctypes.data, env.g2.ctypes.data
    tables_g1 = runtime_error("register_bases: " + TABLES_TEXT)
    tables_g2 = runtime_error("register_bases_g2: " + TABLES_TEXT)
    # every G1 form ends in the same checks; (label, call(address of the handle) -> RustError, expected)
    forms = {
        "register_bases": lambda hp, p=g1, n=N1, st=104, dev=0: L.snarkvm_hip_register_bases(hp, p, n, st, dev),
        "register_bases_tables": lambda hp, p=g1, n=N1, st=104, dev=0, t=16: L.snarkvm_hip_register_bases_tables(hp, p, n, st, dev, t),
        "register_bases_windowed": lambda hp, p=g1, n=N1, st=104, dev=0, t=17, wb=15: L.snarkvm_hip_register_bases_windowed(hp, p, n, st, dev, t, wb),
    }
    cases = []
    for name, f in forms.items():
        cases += [
            (f"{name}: null handle", lambda hp, f=f: f(None), hip_invalid("register_bases: null handle")),
            (f"{name}: null points", lambda hp, f=f: f(hp, p=None), hip_invalid("register_bases: null points")),
            (f"{name}: stride 96", lambda hp, f=f: f(hp, st=96), hip_invalid("register_bases: bad stride")),
            (f"{name}: stride 105", lambda hp, f=f: f(hp, st=105), hip_invalid("register_bases: bad stride")),
            (f"{name}: host pointer as device pointer", lambda hp, f=f: f(hp, dev=1), hip_invalid(NOT_A_DEVICE_POINTER)),
        ]
    tb, wd = forms["register_bases_tables"], forms["register_bases_windowed"]
    cases += [
        ("register_bases_tables: tables 3", lambda hp: tb(hp, t=3), tables_g1),
        ("register_bases_windowed: tables 3", lambda hp: wd(hp, t=3), tables_g1),
        ("register_bases_windowed: window_bits 1", lambda hp: wd(hp, wb=1), tables_g1),
        ("register_bases_windowed: window_bits 24", lambda hp: wd(hp, wb=24), tables_g1),
        ("register_bases_windowed: window_bits 0", lambda hp: wd(hp, wb=0), hip_invalid("register_bases_windowed: window_bits must be positive")),
    ]
    rg = lambda hp, p=g2, n=N2, st=200, t=16, wb=0: L.snarkvm_hip_register_bases_g2(hp, p, n, st, t, wb)
    cases += [
        ("register_bases_g2: null handle", lambda hp: rg(None), hip_invalid("register_bases_g2: null argument")),
        ("register_bases_g2: null points", lambda hp: rg(hp, p=None), hip_invalid("register_bases_g2: null argument")),
        ("register_bases_g2: stride 192", lambda hp: rg(hp, st=192), hip_invalid("register_bases_g2: bad stride")),
        ("register_bases_g2: stride 201", lambda hp: rg(hp, st=201), hip_invalid("register_bases_g2: bad stride")),
        ("register_bases_g2: tables 3", lambda hp: rg(hp, t=3), tables_g2),
        ("register_bases_g2: window_bits 1", lambda hp: rg(hp, wb=1), tables_g2),
        ("register_bases_g2: window_bits 24", lambda hp: rg(hp, wb=24), tables_g2),
    ]
    for label, call, want in cases:
        h = ctypes.c_void_p(sentinel)
        assert refusal(call(ctypes.byref(h))) == want, label
        assert h.value == sentinel, label + ": a refused registration wrote the handle"


def test_g2_one_shot_refuses(env):
    L, sc, g2 = env.L, env.sc.ctypes.data, env.g2.ctypes.data
    out = np.zeros(288, dtype=np.uint8)
    _check_cases(
        [
            ("null out", lambda o: L.snarkvm_hip_msm_g2(None, g2, N2, sc, 200), hip_invalid("msm_g2: null output")),
            ("null points", lambda o: L.snarkvm_hip_msm_g2(o, None, N2, sc, 200), hip_invalid("msm_g2: null argument")),
            ("null scalars", lambda o: L.snarkvm_hip_msm_g2(o, g2, N2, None, 200), hip_invalid("msm_g2: null argument")),
            ("stride 192", lambda o: L.snarkvm_hip_msm_g2(o, g2, N2, sc, 192), hip_invalid("msm: bad ffi_affine_sz for this curve")),
            ("stride 201", lambda o: L.snarkvm_hip_msm_g2(o, g2, N2, sc, 201), hip_invalid("msm: bad ffi_affine_sz for this curve")),
        ],
        out,
    )


def _is_infinity(out):
    """a Jacobian memory image with Z == 0"""
    return not out[2 * len(out) // 3 :].any()


@pytest.mark.parametrize("in_scope", [False, True])
@pytest.mark.parametrize("on_device", [0, 1])
def test_empty_msm_is_the_point_at_infinity(env, in_scope, on_device):
    L = env.L
    scalars = env.dsc.ptr if on_device else None
    singles = []
    for h in (env.h16, env.hw):
        singles.append((144, False, lambda o, h=h: L.snarkvm_hip_msm_registered(o, h, 0, 0, scalars, on_device, 0)))
        singles.append((144, False, lambda o, h=h: L.snarkvm_hip_msm_registered_ex(o, h, 0, 0, 0, 0, scalars, on_device, 0, 0)))
    for h in (env.g16, env.gw):
        singles.append((288, True, lambda o, h=h: L.snarkvm_hip_msm_g2_registered(o, h, 0, 0, scalars, on_device, 0)))
    outs = [np.full(size, FILL, dtype=np.uint8) for size, _, _ in singles]
    if in_scope:
        _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(env.dsc.ptr), SCOPE_ASYNC_MSM))
    try:
        for (size, on_return, call), out in zip(singles, outs):
            _lib.check(call(out.ctypes.data))
            if on_return or not in_scope:  # G2 answers on return also inside a scope; a G1 call there may only have been enqueued
                assert _is_infinity(out)
    finally:
        if in_scope:
            _lib.check(L.snarkvm_hip_scope_end())
    assert all(_is_infinity(out) for out in outs)
