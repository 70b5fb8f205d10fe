"""The G1 accumulate kernels walk segments of S sorted digit entries with a two-stage prefetch (index of entry pos + 2, base of entry
pos + 1) whose loads are issued unconditionally on clamped positions, and with the bucket bookkeeping (boff[k + 2], start[k]) requested in
every iteration (msm_sort.hip.h::msm_accumulate_lazy_kernel / msm_accumulate_seg_kernel).  What such a loop can get wrong sits at the ends
of segments and buckets: the clamp at hi - 1, a segment of one entry, a segment that starts inside a bucket begun by an earlier thread, a
flush in every iteration, runs of empty buckets, a base at infinity or an exceptional addition right after the prefetch rotates.  The
cases (tests/helpers/segment_cases.py; tests/test_accumulate_segment_cases_host.py shows on the CPU that they reach these ends) put each of
them on segments of 2 and 3 entries (tuning seg: nearly every iteration is then a segment's first or last), on the planner's own segment
length, and on one accumulate workgroup per CU; every result is compared with oracle.cpu.g1_msm.

Which tuning reaches which kernel:
    seg=2, seg=3, "", acc_one_wg=1    msm_accumulate_lazy_kernel (lazy = 1 is the default), then g1_partials_to_exact_kernel or the lazy tail
    lazy=0,seg=2, lazy=0,seg=3        msm_accumulate_seg_kernel<fq_t, 1, true>, the exact kernel with the prefetch: every case has fewer than 2^22 digit
                                      entries.  (<fq_t, 1, false> belongs to bigger MSMs; its G2 twin runs in tests/test_gpu_accumulate_segments_g2.py.)

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
print("SEGMENTS_OK", segment_cases.run("g1"))
'''


@pytest.mark.parametrize("tuning", ["seg=2", "seg=3", "", "acc_one_wg=1", "lazy=0,seg=2", "lazy=0,seg=3"])
def test_segment_and_bucket_ends(tuning):
    """7 sizes x (6 scalar patterns + repeated / negated bases + 6 placements of bases at infinity x 2 scalar patterns) x {17 x 15 tables, tables=1}."""
    env = dict(os.environ, SNARKVM_HIP_TUNING=tuning)
    r = subprocess.run([sys.executable, "-c", SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert r.returncode == 0 and "SEGMENTS_OK 140" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
