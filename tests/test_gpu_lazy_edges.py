"""The lazily reduced signed-limb arithmetic of the bucket-accumulation loops as gfx950 compiles it: the cases of tests/test_lazy_edges_host.py through
snarkvm_hip_devtest_lazy_ext - one lane per case in 64-thread workgroups, and for the pair ops one DPP lane pair per case (fq2p::xp_dev: the lane
exchange the host twin does not share), neighbouring pairs of a wave holding cases of different classes."""
import numpy as np
import pytest

from snarkvm_amd import _lib
from tests.helpers import lazy_edge_checks as lx

pytestmark = pytest.mark.gpu

RUN = lx.Runner(device=True)


def test_products_at_the_range_ends():
    lx.check_products(RUN)


def test_normalized_to_exact_from_exact_and_the_raw_image():
    lx.check_conversions(RUN)


def test_fqz_operators_and_is_zero():
    lx.check_fqz(RUN)


def test_madd_on_every_representative_of_p_and_both_sides_of_the_window():
    lx.check_madd(RUN)


def test_pair_helpers_and_the_three_images_of_zero():
    lx.check_pair_helpers(RUN)


def test_pair_product_and_what_the_exchange_leaves():
    lx.check_pair_product(RUN)


def test_pair_madd_with_the_lanes_disagreeing():
    lx.check_pair_madd(RUN)


def test_device_hook_refuses_bad_arguments():
    L = _lib.lib()
    buf = np.zeros(256, dtype=np.int32)
    for args in ((12, buf.ctypes.data, buf.ctypes.data, 1), (-1, buf.ctypes.data, buf.ctypes.data, 1), (0, None, buf.ctypes.data, 1), (0, buf.ctypes.data, None, 1)):
        with pytest.raises(_lib.HipError) as e:
            _lib.check(L.snarkvm_hip_devtest_lazy_ext(*args))
        assert e.value.code == 1  # hipErrorInvalidValue
    _lib.check(L.snarkvm_hip_devtest_lazy_ext(0, None, None, 0))
