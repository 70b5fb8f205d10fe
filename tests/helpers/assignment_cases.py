"""Cases and expected values shared by tests/test_fr_assignment_evals_host.py (CPU, through the host twin), tests/test_gpu_fr_assignment_evals.py
and tests/test_gpu_first_round.py: the rows of `snarkvm_hip_fr_assignment_evals` and what every result is compared with, byte for byte.

Expected values do not come from the library: the index map of include/snarkvm_hip.h restated with numpy indexing (the call does no arithmetic,
so there is nothing else to restate).
"""
import numpy as np

from snarkvm_amd import _lib
from tests.helpers import selector_cases as sel

R = sel.R
GUARD = 0xFFFFFFFFFFFFFFFF  # 0xff-filled
INVALID_VALUE = 1  # hipErrorInvalidValue
mont, rnd, mixed = sel.mont, sel.rnd, sel.mixed

# (n, input_size, num_vars)
CASES = (
    (8, 4, 7),          # the fixture's shape: ratio 2
    (8, 1, 8),          # ratio = n, num_vars == n
    (8, 1, 1),          # ratio = n, nothing but the one public value
    (8, 1, 5),          # ratio = n, a short private part
    (8, 8, 8),          # ratio 1: every position is an input position, num_vars == n
    (16, 4, 4),         # num_vars == input_size: everything off the subgroup is zero
    (16, 4, 16),        # num_vars == n
    (16, 4, 9),         # a short private part: zeros from num_vars on
    (48, 16, 40),       # ratio 3: the sizes need not be powers of two
    (300, 100, 299),    # ratio 3, more than one workgroup
    (1024, 16, 1000),   # the first-round driver's shape
    (4097, 1, 4097),    # odd, ratio = n
)
THREADS = (1, 3, 256)


def geometry(n):
    """(workgroups, threads per workgroup, cap on the workgroups) of what the device call launches per member of n elements"""
    out = np.zeros(3, dtype=np.uint32)
    assert _lib.lib().snarkvm_hip_selftest_fr_assignment_geometry(n, out.ctypes.data) == 0
    return int(out[0]), int(out[1]), int(out[2])


def expected(row, n, input_size):
    """one member: row (num_vars, 4) -> (n, 4) by the formula of the header"""
    row = np.ascontiguousarray(row, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros((n, 4), dtype=np.uint64)
    if n == 0:
        return out
    ratio = n // input_size
    k = np.arange(n)
    j = np.where(k % ratio == 0, k // ratio, input_size + k - k // ratio - 1)
    have = j < row.shape[0]
    out[k[have]] = row[j[have]]
    return out


def row(num_vars, seed):
    """num_vars mixed elements (uniform values with 0, 1, r - 1, (r +- 1) / 2 among them), none of them the guard pattern"""
    return mixed(num_vars, seed)


def selftest(rows, n, input_size, threads, stride_out=None, stride_vars=None):
    """snarkvm_hip_selftest_fr_assignment_evals over `rows` ((count, num_vars, 4)) laid stride_vars apart -> (count, n, 4); the gaps between the
    members of the output, a guard element in front and one behind are checked to be untouched"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    count, num_vars = rows.shape[0], rows.shape[1]
    so = n if stride_out is None else stride_out
    sv = num_vars if stride_vars is None else stride_vars
    src = np.full((max(count - 1, 0) * sv + num_vars + 1, 4), GUARD, dtype=np.uint64)
    for m in range(count):
        src[m * sv : m * sv + num_vars] = rows[m]
    before = src.copy()
    buf = np.full((max(count - 1, 0) * so + n + 2, 4), GUARD, dtype=np.uint64)
    rcode = _lib.lib().snarkvm_hip_selftest_fr_assignment_evals(buf[1:].ctypes.data, n, src.ctypes.data, num_vars, input_size, count, so, sv, threads)
    assert rcode == 0
    assert np.array_equal(src, before), "vars was written"
    inside = np.zeros(len(buf), dtype=bool)
    for m in range(count):
        inside[1 + m * so : 1 + m * so + n] = True
    assert (buf[~inside] == GUARD).all(), "an element outside the members was written"
    return np.stack([buf[1 + m * so : 1 + m * so + n] for m in range(count)]) if count else np.zeros((0, n, 4), dtype=np.uint64)
