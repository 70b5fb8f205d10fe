"""`snarkvm_hip_fr_assignment_evals` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: fr_assignment_evals_kernel): the shapes of the host file
with host and device operands, strided members with untouched gaps, one size past the cap of the launch grid, refusals, inside a scope, a repeated
call that grows nothing, and two logical devices.

Every comparison is byte for byte.  Expected values: tests/helpers/assignment_cases.py (the index map restated with numpy); the host twin of the
kernel must give the same bytes as the device.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from snarkvm_amd import _lib, plugin, poly
from snarkvm_amd.devmem import HipMem
from tests import util
from tests.helpers import assignment_cases as ac

pytestmark = pytest.mark.gpu

GUARD = ac.GUARD


def _laid_out(rows, stride):
    """rows (count, num_vars, 4) `stride` elements apart in one guard-filled array with one guard element behind"""
    count, num_vars = rows.shape[0], rows.shape[1]
    flat = np.full(((count - 1) * stride + num_vars + 1, 4), GUARD, dtype=np.uint64)
    for m in range(count):
        flat[m * stride : m * stride + num_vars] = rows[m]
    return flat


def _members(buf, n, count, stride):
    """the members of a guarded output (one guard in front, the rest behind and between) -> (count, n, 4); everything else must be the guard"""
    inside = np.zeros(len(buf), dtype=bool)
    for m in range(count):
        inside[1 + m * stride : 1 + m * stride + n] = True
    assert (buf[~inside] == GUARD).all(), "an element outside the members was written"
    return np.stack([buf[1 + m * stride : 1 + m * stride + n] for m in range(count)])


def run(rows, n, input_size, stride_out, stride_vars, on_device, device=-1):
    """-> (count, n, 4) through snarkvm_hip_fr_assignment_evals; the rows, the gaps and the guards are checked to be unchanged"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    count, num_vars = rows.shape[0], rows.shape[1]
    src = _laid_out(rows, stride_vars)
    out = np.full(((count - 1) * stride_out + n + 2, 4), GUARD, dtype=np.uint64)
    if not on_device:
        before = src.copy()
        _lib.check(_lib.lib().snarkvm_hip_fr_assignment_evals(out[1:].ctypes.data, n, src.ctypes.data, num_vars, input_size, count, stride_out, stride_vars, 0))
        assert np.array_equal(src, before), "vars was written"
        return _members(out, n, count, stride_out)
    d_src, d_out = HipMem.from_numpy(src, device), HipMem.from_numpy(out, device)
    plugin.fr_assignment_evals_device(d_out.ptr + 32, n, d_src.ptr, num_vars, input_size, count, stride_out, stride_vars)
    got = _members(d_out.download(dtype=np.uint64).reshape(-1, 4), n, count, stride_out)
    assert np.array_equal(d_src.download(dtype=np.uint64).reshape(-1, 4), src), "vars was written"
    d_src.free(), d_out.free()
    return got


@pytest.mark.parametrize("on_device", [0, 1])
def test_the_cases_of_the_host_file(on_device):
    for n, input_size, num_vars in ac.CASES:
        row = ac.row(num_vars, n + num_vars)
        want = ac.expected(row, n, input_size)
        got = run(row[None], n, input_size, n, num_vars, on_device)
        assert got[0].tobytes() == want.tobytes(), (n, input_size, num_vars)
        assert got[0].tobytes() == ac.selftest(row[None], n, input_size, 256)[0].tobytes(), (n, input_size, num_vars)
        if not on_device:
            assert poly.assignment_evals(row, n, input_size)[0].tobytes() == want.tobytes(), (n, input_size, num_vars)
    assert util.fr_mont_to_ints(run(ac.mont([1, 8, 32, 128, 2, 4, 2])[None], 8, 4, 8, 7, on_device)[0]) == [1, 2, 8, 4, 32, 2, 128, 0]


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("count", [1, 3, 49])
def test_member_counts_with_strides_larger_than_the_vectors(count, on_device):
    """n = 2^10, |X| = 16, 1000 variables per row; outputs 1024 + 7 and rows 1000 + 11 elements apart: the gaps between members stay untouched"""
    n, input_size, num_vars = 1 << 10, 16, 1000
    rows = np.stack([ac.row(num_vars, 200 + m) for m in range(count)])
    got = run(rows, n, input_size, n + 7, num_vars + 11, on_device)
    for m in range(count):
        assert got[m].tobytes() == ac.expected(rows[m], n, input_size).tobytes(), m
    if not on_device:
        assert poly.assignment_evals(rows, n, input_size).tobytes() == got.tobytes()


def test_one_size_past_the_cap_of_the_launch_grid():
    """one member of twice as many elements as the launch has threads (the geometry hook reports the cap: 8192 workgroups of 256 -> n = 2^22): every
    thread takes a second trip through the grid-stride loop"""
    _, threads, cap = ac.geometry(1)
    n = 2 * cap * threads
    assert n & (n - 1) == 0 and ac.geometry(n)[0] == cap and ac.geometry(n // 2)[0] == cap and ac.geometry(n // 4)[0] == cap // 2
    input_size, num_vars = 16, n - 5
    row = ac.rnd(num_vars, 9)
    d_row, d_out = HipMem.from_numpy(row), HipMem(32 * (n + 1))
    d_out.fill(0, 0xFF, 32 * (n + 1))
    plugin.fr_assignment_evals_device(d_out.ptr, n, d_row.ptr, num_vars, input_size)
    got = d_out.download(dtype=np.uint64).reshape(-1, 4)
    assert (got[n] == GUARD).all()
    assert np.array_equal(got[:n], ac.expected(row, n, input_size))
    d_row.free(), d_out.free()


def _refused(fn):
    with pytest.raises(_lib.HipError) as e:
        fn()
    assert e.value.code == ac.INVALID_VALUE and e.value.message, e.value


def test_refusals_leave_out_untouched():
    L = _lib.lib()
    n, num_vars = 8, 7
    rows = ac.row(32, 1)
    host = np.full((64, 4), GUARD, dtype=np.uint64)
    d_rows, d_out = HipMem.from_numpy(rows), HipMem.from_numpy(host)

    def call(o=d_out.ptr, n=n, v=d_rows.ptr, num_vars=num_vars, input_size=4, count=2, stride_out=16, stride_vars=10, on_device=1):
        return lambda: _lib.check(L.snarkvm_hip_fr_assignment_evals(o, n, v, num_vars, input_size, count, stride_out, stride_vars, on_device))

    for bad in (dict(input_size=0), dict(input_size=3), dict(input_size=16), dict(n=(1 << 28) + 4), dict(num_vars=3), dict(num_vars=9),
                dict(count=65536, stride_out=8, stride_vars=7), dict(stride_out=7), dict(stride_vars=6), dict(stride_out=(1 << 40) + 1),
                dict(stride_vars=(1 << 40) + 1), dict(o=None), dict(v=None),
                dict(v=d_out.ptr + 32 * 23), dict(o=d_rows.ptr + 32 * 5), dict(o=d_rows.ptr + 32 * 16),  # out overlapping vars
                dict(v=host.ctypes.data), dict(o=host.ctypes.data),                                          # operands that are not on one device
                dict(o=None, on_device=0), dict(v=None, on_device=0), dict(input_size=3, on_device=0, o=host.ctypes.data, v=rows.ctypes.data)):
        _refused(call(**bad))
    assert (host == GUARD).all()
    assert (d_out.download(dtype=np.uint64).reshape(-1, 4) == GUARD).all()
    # successes that touch nothing and need no device
    call(count=0)(), call(count=0, o=None, v=None)(), call(n=0, num_vars=0)(), call(n=0, num_vars=5, o=None, v=None)()
    assert (d_out.download(dtype=np.uint64).reshape(-1, 4) == GUARD).all()
    call()()  # and the call the refusals vary succeeds
    got = d_out.download(dtype=np.uint64).reshape(-1, 4)
    for m in range(2):
        assert np.array_equal(got[16 * m : 16 * m + n], ac.expected(rows[10 * m : 10 * m + num_vars], n, 4))
    assert (got[n:16] == GUARD).all() and (got[16 + n :] == GUARD).all()
    assert np.array_equal(d_rows.download(dtype=np.uint64).reshape(-1, 4), rows)
    d_rows.free(), d_out.free()


def test_inside_a_scope_and_a_repeated_call_grows_nothing():
    """in a scope the call is only enqueued, in order with a transform of its output: after scope_end the bytes are those of the call outside a scope
    followed by the transform; repeated calls, with host operands too, grow no workspace"""
    from oracle import cpu as oracle

    L = _lib.lib()
    n, input_size, num_vars, count = 1 << 10, 16, 1000, 3
    rows = np.stack([ac.row(num_vars, 300 + m) for m in range(count)])
    want = np.stack([ac.expected(r, n, input_size) for r in rows])
    want_z = np.stack([oracle.ntt(v, direction=oracle.INVERSE) for v in want])
    stats = np.zeros(5, dtype=np.uint64)
    d_rows = HipMem.from_numpy(rows)
    for attempt in range(3):
        d_out = HipMem(32 * count * n)
        _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(d_out.ptr)))
        try:
            plugin.fr_assignment_evals_device(d_out.ptr, n, d_rows.ptr, num_vars, input_size, count, n, num_vars)
            plugin.NTT_device_batch(10, [d_out.ptr + 32 * n * m for m in range(count)], directions=[1] * count, types=[0] * count)
        finally:
            _lib.check(L.snarkvm_hip_scope_end())
        assert np.array_equal(d_out.download(dtype=np.uint64).reshape(count, n, 4), want_z), attempt
        assert poly.assignment_evals(rows, n, input_size).tobytes() == want.tobytes()
        if attempt == 0:
            L.snarkvm_hip_alloc_stats(None, 1)
        elif attempt == 1:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        d_out.free()
    assert not stats[:4].any(), stats
    d_rows.free()


MULTI_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from snarkvm_amd import msm, plugin, poly
from snarkvm_amd.devmem import HipMem
from tests.helpers import assignment_cases as ac

assert msm.num_devices() == 2, msm.num_devices()
n, input_size, num_vars, count = 300, 100, 280, 3
rows = np.stack([ac.row(num_vars, 400 + m) for m in range(count)])
want = np.stack([ac.expected(r, n, input_size) for r in rows])
for device in (0, 1, 1, 0):
    d_rows = HipMem.from_numpy(rows, device)
    d_out = HipMem.from_numpy(np.full((count * n + 1, 4), ac.GUARD, dtype=np.uint64), device)
    plugin.fr_assignment_evals_device(d_out.ptr, n, d_rows.ptr, num_vars, input_size, count, n, num_vars)
    now = d_out.download(dtype=np.uint64).reshape(-1, 4)
    assert np.array_equal(now[: count * n].reshape(count, n, 4), want) and (now[count * n] == ac.GUARD).all(), device
    d_rows.free(), d_out.free()
assert np.array_equal(poly.assignment_evals(rows, n, input_size), want)
print("ASSIGNMENT_MULTI_OK")
'''


def test_two_logical_devices():
    env = dict(os.environ, SNARKVM_HIP_DEVICES="0,0")
    r = subprocess.run([sys.executable, "-c", MULTI_SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert "ASSIGNMENT_MULTI_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
