"""The G2 accumulate kernels at the ends of segments and buckets: the twin of tests/test_gpu_accumulate_segments.py.

msm_accumulate_pair2_kernel (msm_sort.hip.h; tuning lazy2 = 1, the default) walks a segment on a lane pair (t = gt >> 1, a grid of 2 * nthreads), without
look-ahead of the bucket bookkeeping, steps over empty buckets in a do-while, skips a base at infinity on a word both lanes read, and flushes zeros when the
accumulator is at infinity; the lanes exchange operands by DPP inside madd while other pairs of the wave flush, skip or have left the loop.  With
lazy2 = 0 the exact kernel msm_accumulate_seg_kernel<fq2_t, 1, PREFETCH> runs instead: PREFETCH up to 2^22 digit entries, the plain loop beyond.

The cases (tests/helpers/segment_cases.py; tests/test_accumulate_segment_cases_host.py shows on the CPU which ends they reach) are the G1 set over G2 points -
7 sizes x (6 scalar patterns + repeated / negated bases + 6 placements of bases at infinity x 2 scalar patterns) x {17 x 15 tables, tables=1} = 140 -
plus cancel_restart at every size (P, -P, Q: the accumulator returns to infinity inside a bucket; at n = 2 the bucket is flushed at infinity) and
the 7 instances of one msm_batch call (a fused group: segments cross instance boundaries and step over the 2^14 empty buckets of an all-zero instance; the
empty instance comes back as the point at infinity): 154.  Every result is compared, by the bytes of its affine form, with the oracle's standard::msm.

Which tuning reaches which kernel:
    seg=2, seg=3, ""                  msm_accumulate_pair2_kernel, then g2_pair_partials_to_exact_kernel
    lazy2=0,seg=2, lazy2=0,seg=3      msm_accumulate_seg_kernel<fq2_t, 1, true>
    the multi-round test, ""          msm_accumulate_pair2_kernel on a multi-round grid, msm_reduce_kernel<fq2_t>, the fold and bit planes without a bucket sink
    the multi-round test, lazy2=0     msm_accumulate_seg_kernel<fq2_t, 1, false>, and the same tail

SNARKVM_HIP_TUNING is parsed once per process: one child process per setting, all cases of the setting inside it."""
import os
import subprocess
import sys

import pytest

from tests import util

pytestmark = pytest.mark.gpu

SCRIPT = r'''
import sys
sys.path.insert(0, %r)
from tests.helpers import segment_cases
print("SEGMENTS_G2_OK", segment_cases.run("g2"))
'''

# 17 x 250 001 = 4 250 017 digit entries: the smallest convenient size past the 2^22 = 4 194 304 at which msm_layout leaves the single-round, one-wave route;
# n is odd, so the last segment is short.  The bases are ((i mod 512) + 1) G: the sum is k G with k = sum_j (j + 1) sum_(i = j mod 512) s_i mod r, one scalar
# multiplication on the CPU.
ROUTE_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib, synthetic
from snarkvm_amd.msm import RegisteredBasesG2
from tests import util
from tests.helpers import msm_digit_cases

n, period = 250001, 512
g = msm_digit_cases.geometry(n, 0, 17, 15)
assert g.Wd * n > 2**22 and (g.c, g.W, g.J) == (15, 1, 17), g  # past the threshold of msm_layout: not single_round, no prefetch
bases = synthetic.g2_points(n, distinct=period)
sc = synthetic.random_fr_integers(n, 0x6A2)
sc[0] = 0
sc[1] = [1, 0, 0, 0]
sc[2] = pyref.to_limbs(pyref.R_MOD - 1, 4)
# per-residue sums of the 32-bit halves of the limbs (< 2^9 terms of < 2^32 each), then Python integers
halves = np.zeros(((n + period - 1) // period * period, 4, 2), dtype=np.uint64)
halves[:n, :, 0] = sc & np.uint64(0xFFFFFFFF)
halves[:n, :, 1] = sc >> np.uint64(32)
sums = halves.reshape(-1, period, 4, 2).sum(axis=0)
k = sum((j + 1) * sum(int(sums[j, l, h]) << (64 * l + 32 * h) for l in range(4) for h in range(2)) for j in range(period)) %% pyref.R_MOD
want = oracle.g2_to_affine(oracle.g2_mul(bases[:1].view(oracle.G2_AFFINE), pyref.to_limbs(k, 4))).tobytes()

rb = RegisteredBasesG2(bases, tables=17, window_bits=15)
L = _lib.lib()
L.snarkvm_hip_set_profiling(1)
try:
    got = rb.msm(sc)
    phases = [L.snarkvm_hip_get_phase_name(i).decode() for i in range(L.snarkvm_hip_get_phase_count())]
finally:
    L.snarkvm_hip_set_profiling(0)
print("phases:", phases)
assert oracle.g2_to_affine(got).tobytes() == want, "profiled call"
# the whole tail ran in this MSM, nothing was left to a bucket sink (msm_reduce_partials is logged by single-round MSMs too: the plan above is what
# shows the route)
assert all(p in phases for p in ("msm_accumulate", "msm_reduce_partials", "msm_bucket_reduce")) and "msm_bucket_merge" not in phases, phases
assert oracle.g2_to_affine(rb.msm(sc)).tobytes() == want, "plain call"
rb.close()
print("ROUTE_G2_OK")
'''


def _child(script, tuning):
    env = dict(os.environ, SNARKVM_HIP_TUNING=tuning)
    return subprocess.run([sys.executable, "-c", script % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)


@pytest.mark.parametrize("tuning", ["seg=2", "seg=3", "", "lazy2=0,seg=2", "lazy2=0,seg=3"])
def test_segment_and_bucket_ends_g2(tuning):
    """140 cases as for G1, cancel_restart at 7 sizes, 7 instances of one fused batch."""
    r = _child(SCRIPT, tuning)
    print(r.stdout[-500:])
    assert r.returncode == 0 and "SEGMENTS_G2_OK 154" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("tuning", ["", "lazy2=0"])
def test_registered_multi_round_route_g2(tuning):
    """250 001 points over 17 x 15 tables: more than 2^22 digit entries, against the closed form."""
    r = _child(ROUTE_SCRIPT, tuning)
    print(r.stdout[-500:])
    assert r.returncode == 0 and "ROUTE_G2_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
