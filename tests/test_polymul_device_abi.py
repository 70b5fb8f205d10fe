"""snarkvm_hip_polymul_device without a GPU: the two outcomes that need no device."""
import ctypes

import numpy as np
import pytest

from snarkvm_amd import _lib, plugin


def test_zero_operands_is_success_and_needs_no_device():
    plugin.polymul_device(10, 0)
    out = np.full((4, 4), 7, dtype=np.uint64)
    plugin.polymul_device(2, out.ctypes.data)
    assert (out == 7).all()


def test_an_operand_that_is_not_device_memory_fails_loudly():
    """Without a GPU there is no device to run on; with one, host memory belongs to none: either way a non-zero code and a message, never a
    product computed somewhere else (the contract of test_abi.py::test_no_gpu_means_loud_failure_not_fallback)."""
    a = np.ones((4, 4), dtype=np.uint64)
    out = np.full((4, 4), 7, dtype=np.uint64)
    pp = (ctypes.c_void_p * 1)(a.ctypes.data)
    pl = (ctypes.c_size_t * 1)(4)
    err = _lib.lib().snarkvm_hip_polymul_device(out.ctypes.data, 1, pp, pl, 0, None, None, 2)
    with pytest.raises(_lib.HipError) as e:
        _lib.check(err)
    assert e.value.code != 0 and e.value.message
    assert (out == 7).all()
