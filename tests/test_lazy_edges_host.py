"""The lazily reduced signed-limb arithmetic of the bucket-accumulation loops (snarkvm_amd/csrc/ffl.hip.h, ffl2.hip.h, ffl2p.hip.h) compiled for the
host, on operands at the ends of the ranges the routines' comments state (tests/helpers/lazy_cases.py): the field routines, fqz_t's operators,
xyzz_lazy_t::madd on every representative of a zero P and on both sides of its low-limb window, the lane-pair product, its helpers and the pair's
mixed addition with the lanes disagreeing about the filter, about P = 0 and about R = 0.  Building a case list replays every column sum in Python
integers: a case that leaves 64 bits or its promised range raises lazy_cases.Finding, an operand outside the stated precondition IllegalCase.  No GPU
needed; the same cases run on the device in tests/test_gpu_lazy_edges.py."""
import numpy as np
import pytest

from tests.helpers import lazy_cases as lz
from tests.helpers import lazy_edge_checks as lx

RUN = lx.Runner(device=False)


# log2 of the largest partial column sum each routine's comment allows (ffl.hip.h: mul with the wide top limbs of the addition law, sqr, diff_of_products;
# ffl2p.hip.h: (14 + 6.4 + 2) 2^58 on the even lane, 26 * 2^58 on the odd one)
PEAK_BOUND = {"mul": 62.6, "madd.mul": 62.6, "to_exact": 62.6, "from_exact": 62.6, "sqr": 62.7, "diff_of_products": 62.9, "pair.even": 62.5, "pair.odd": 62.71}


@pytest.mark.parametrize("name", sorted(lz.ALL))
def test_every_case_is_legal_and_every_column_fits(name):
    """building the list IS the proof: the replay raises on a column beyond 64 bits, a word beyond 32, an operand outside its precondition; and the
    largest partial sum of every routine stays under the figure its comment states.  A few thousand records per op where a record is cheap; the two
    additions hold 1 800 and 800 (a replay of one pair addition takes 17 ms of Python, and the GPU tests build the same lists)"""
    c = lz.ALL[name]()
    op = lz.OPS[name]
    assert c.rows.shape == (len(c.names), lz.IN_WORDS[op]) and c.want.shape == (len(c.names), lz.OUT_WORDS[op])
    assert len(c.names) >= (800 if name == "pair_madd" else 1200)
    peaks = lx.peak_report()
    print(name, len(c.names), "cases; largest partial column sums so far (log2):", peaks)
    assert set(peaks) <= set(PEAK_BOUND) and all(v < PEAK_BOUND[k] for k, v in peaks.items()), peaks


def test_products_at_the_range_ends():
    lx.check_products(RUN)


def test_normalized_to_exact_from_exact_and_the_raw_image():
    lx.check_conversions(RUN)


def test_fqz_operators_and_is_zero():
    lx.check_fqz(RUN)


def test_madd_on_every_representative_of_p_and_both_sides_of_the_window():
    print(lx.check_madd(RUN))


def test_pair_helpers_and_the_three_images_of_zero():
    lx.check_pair_helpers(RUN)


def test_pair_product_and_what_the_exchange_leaves():
    lx.check_pair_product(RUN)


def test_pair_madd_with_the_lanes_disagreeing():
    print(lx.check_pair_madd(RUN))


def test_hook_refuses_bad_arguments():
    from snarkvm_amd import _lib

    L = _lib.lib()
    buf = np.zeros(256, dtype=np.int32)
    assert L.snarkvm_hip_selftest_lazy_ext(12, buf.ctypes.data, buf.ctypes.data, 1) == 1
    assert L.snarkvm_hip_selftest_lazy_ext(-1, buf.ctypes.data, buf.ctypes.data, 1) == 1
    assert L.snarkvm_hip_selftest_lazy_ext(0, None, buf.ctypes.data, 1) == 1
    assert L.snarkvm_hip_selftest_lazy_ext(0, buf.ctypes.data, None, 1) == 1
    assert L.snarkvm_hip_selftest_lazy_ext(0, None, None, 0) == 0
