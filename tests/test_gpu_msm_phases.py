"""Pins the MSM enqueue path (csrc/msm_run.hip.h::msm_run and its stages): for every entry point and window width the result
equals the oracle's AND the ordered list of profiling phases equals a literal list.  With snarkvm_hip_set_profiling(1) the
scope and the coalescer decline, so each call takes the synchronous path and leaves its phases behind
(snarkvm_hip_get_phase_count / _name).  2^10 pairs everywhere: the paths differ by window width and entry point, not by size.

The stand-alone digit matrix in front of a WIDE sort (tuning fused=0) is read once per process: its coverage is the `fused=0`
leg of tests/test_gpu_multidevice.py::test_ab_switches_are_bit_exact."""
import ctypes

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, plugin, synthetic
from snarkvm_amd.msm import RegisteredBases, RegisteredBasesG2
from tests import util

pytestmark = pytest.mark.gpu

N = 1 << 10
SORT_NARROW = ["msm_digits", "msm_sort_level1", "msm_sort_level2"]
SORT_WIDE_FUSED = ["msm_scalar_read", "msm_sort_level1", "msm_sort_level2", "msm_sort_level3"]
DEVICE_TAIL = ["msm_accumulate", "msm_reduce_partials", "msm_bucket_reduce"]
# msm_run_sync adds the host's Horner chain; the host-scalar drivers (msm_registered_host_scalars, msm_host_chunked) finish outside any phase
NARROW = SORT_NARROW + DEVICE_TAIL + ["msm_host_finish"]
WIDE_FUSED = SORT_WIDE_FUSED + DEVICE_TAIL + ["msm_host_finish"]
HOST_SCALARS = ["msm_h2d"] + SORT_NARROW + DEVICE_TAIL
HOST_BUFFERS = ["msm_h2d", "msm_convert_bases"] + SORT_NARROW + DEVICE_TAIL
G2_NARROW = SORT_NARROW + DEVICE_TAIL + ["msm_host_finish"]


@pytest.fixture(scope="module")
def data():
    import torch

    bases = oracle.g1_gen_bases(util.g1_generator_affine(), 1, 2 * N)
    sc = synthetic.random_fr_integers(N, 0x9A5E)
    sc[0] = 0
    sc[1] = [1, 0, 0, 0]
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    mont = oracle.fr_op("from_bigint", sc)
    d_mont = torch.from_numpy(np.ascontiguousarray(mont).view(np.int64)).cuda()
    torch.cuda.synchronize()
    want = oracle.g1_to_affine(oracle.g1_msm(bases[:N], sc, oracle.MSM_BATCHED))
    return {"bases": bases, "sc": sc, "d_sc": d_sc, "d_mont": d_mont, "want": want}


def _profiled(call):
    """call() with profiling on -> (its result, the phase names it left, in order)"""
    L = _lib.lib()
    L.snarkvm_hip_set_profiling(1)
    try:
        got = call()
        return got, [L.snarkvm_hip_get_phase_name(i).decode() for i in range(L.snarkvm_hip_get_phase_count())]
    finally:
        L.snarkvm_hip_set_profiling(0)


def _check_g1(got, want, phases, expected):
    print("phases:", phases)
    assert util.affine_equal(oracle.g1_to_affine(got), want)
    assert phases == expected


def test_g1_registered_device_scalars_narrow(data):
    rb = RegisteredBases(data["bases"][:N])
    try:
        got, phases = _profiled(lambda: rb.msm(device_ptr=data["d_sc"].data_ptr(), npoints=N, window_bits=13))
        _check_g1(got, data["want"], phases, NARROW)
    finally:
        rb.close()


def test_g1_wide_window_fused_scalar_read(data):
    """15 tables of 17-bit windows: one bucket window of 2^16 buckets; the level-1 partition reads the scalars itself."""
    rb = RegisteredBases(data["bases"][:N], tables=15, window_bits=17)
    try:
        got, phases = _profiled(lambda: rb.msm(device_ptr=data["d_sc"].data_ptr(), npoints=N, window_bits=17))
        _check_g1(got, data["want"], phases, WIDE_FUSED)
    finally:
        rb.close()


def test_g1_two_base_ranges_montgomery_scalars(data):
    """snarkvm_hip_msm_registered_ex: bases [3, 3 + n0) then [off1, off1 + n1) against n0 + n1 Montgomery-form scalars."""
    bases = data["bases"]
    off0, n0, off1, n1 = 3, N - 100, N + 7, 100
    rb = RegisteredBases(bases)
    try:
        out = np.zeros(1, dtype=oracle.G1_PROJECTIVE)
        _, phases = _profiled(lambda: _lib.check(_lib.lib().snarkvm_hip_msm_registered_ex(
            ctypes.c_void_p(out.ctypes.data), rb._h, ctypes.c_size_t(off0), ctypes.c_size_t(n0), ctypes.c_size_t(off1), ctypes.c_size_t(n1),
            ctypes.c_void_p(data["d_mont"].data_ptr()), 1, 1, 13)))
        both = np.concatenate([bases[off0 : off0 + n0], bases[off1 : off1 + n1]])
        want = oracle.g1_to_affine(oracle.g1_msm(both, data["sc"], oracle.MSM_BATCHED))
        _check_g1(out, want, phases, NARROW)
    finally:
        rb.close()


def test_g1_registered_host_scalars(data):
    rb = RegisteredBases(data["bases"][:N])
    try:
        got, phases = _profiled(lambda: rb.msm(data["sc"], window_bits=13))
        _check_g1(got, data["want"], phases, HOST_SCALARS)
    finally:
        rb.close()


def test_snarkvm_msm_host_buffers(data):
    """The reference's symbol: bases and scalars uploaded and converted per call; the planner picks a narrow window at 2^10 pairs."""
    got, phases = _profiled(lambda: plugin.msm(data["bases"][:N], data["sc"]))
    _check_g1(got, data["want"], phases, HOST_BUFFERS)


def test_g2_registered_narrow(data):
    g2 = synthetic.g2_points(N, distinct=64)
    want = oracle.g2_to_affine(oracle.g2_msm(g2.view(oracle.G2_AFFINE), data["sc"], oracle.MSM_STANDARD)).tobytes()
    rg = RegisteredBasesG2(g2, tables=16)
    try:
        got, phases = _profiled(lambda: rg.msm(device_ptr=data["d_sc"].data_ptr(), npoints=N))
        print("phases:", phases)
        assert oracle.g2_to_affine(got).tobytes() == want
        assert phases == G2_NARROW
    finally:
        rg.close()
