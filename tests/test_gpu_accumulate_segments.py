"""The accumulate kernels walk segments of S sorted digit entries with a two-stage prefetch (index of entry pos + 2, base of entry
pos + 1) whose loads are issued unconditionally on clamped positions, and with the bucket bookkeeping (boff[k + 2], start[k]) requested in
every iteration (msm_sort.hip.h::msm_accumulate_lazy_kernel / msm_accumulate_seg_kernel).  What such a loop can get wrong sits at the ends
of segments and buckets: the clamp at hi - 1, a segment of one entry, a segment that starts inside a bucket begun by an earlier thread, a
flush in every iteration, runs of empty buckets, a base at infinity or an exceptional addition right after the prefetch rotates.  The
cases below put each of these on segments of 2 and 3 entries (tuning seg: nearly every iteration is then a segment's first or last), on
the planner's own segment length, and on one accumulate workgroup per CU; every result is compared with oracle.cpu.g1_msm.

SNARKVM_HIP_TUNING is parsed once per process: one child process per setting, all cases of the setting inside it."""
import os
import subprocess
import sys

import pytest

from tests import util

pytestmark = pytest.mark.gpu

SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import msm
from tests import util

G = util.g1_generator_affine()
SIZES = (1, 2, 3, 127, 128, 129, 257)  # x 17 windows / x the planner's: digit entries on, one below and one above multiples of 2 and 3
NMAX = max(SIZES)
GEOMETRIES = (dict(tables=17, window_bits=15), dict(tables=1))
INF = util.g1_affine_from_ints([None])[0]


def negated(p):
    q = p.copy()
    q["y"] = pyref.to_limbs(pyref.Q_MOD - pyref.from_limbs(p["y"]), 6)  # Montgomery form of -y
    return q


def digits_scalar(ds, bits=15):
    """the scalar whose 15-bit windows are ds (low to high), below 2^253"""
    return sum(d << (bits * w) for w, d in enumerate(ds)) %% (1 << 252)


distinct = oracle.g1_gen_bases(G, 1, NMAX)  # (i + 1) G
# P, P, -P, -P, P, Q, Q, -Q, ...: with equal scalars a bucket meets a doubling, an ordinary addition, a cancellation, a restart
runs = distinct.copy()
for i in range(NMAX):
    p = distinct[i // 5]
    runs[i] = negated(p) if i %% 5 in (2, 3) else p
rng = np.random.default_rng(0xACC)
SCALARS = {
    # one bucket per digit row: segments start inside a bucket that an earlier thread began (part_off > 0)
    "equal": util.ints_to_fr([digits_scalar([5, 16383, 1, 9000] * 5)] * NMAX),
    # every bucket of the low window holds one entry: a flush in every iteration there
    "distinct_small": util.ints_to_fr(list(range(1, NMAX + 1))),
    # few digit values far apart: long runs of empty buckets between the occupied ones
    "gappy": util.ints_to_fr([digits_scalar([(1, 7000, 16383, 2)[(i + w) %% 4] for w in range(17)]) for i in range(NMAX)]),
    "zero": util.ints_to_fr([0] * NMAX),
    "zero_mixed": util.ints_to_fr([0 if i %% 3 else 12345 + i for i in range(NMAX)]),
    "uniform": util.ints_to_fr([int.from_bytes(rng.bytes(32), "little") %% pyref.R_MOD for _ in range(NMAX)]),
}


count = 0


def check(tag, bases, names):
    """every named scalar pattern over `bases`, registered once per geometry"""
    global count
    n = len(bases)
    wants = {name: oracle.g1_to_affine(oracle.g1_msm(bases, SCALARS[name][:n], oracle.MSM_BATCHED)).tobytes() for name in names}
    for geo in GEOMETRIES:
        rb = msm.RegisteredBases(bases, **geo)
        for name in names:
            got = oracle.g1_to_affine(rb.msm(SCALARS[name][:n]))
            assert got.tobytes() == wants[name], (tag, name, n, geo)
        rb.close()
    count += len(names)


for n in SIZES:
    check("distinct", distinct[:n], list(SCALARS))
    # P directly followed by P and by -P: the exceptional addition right after the prefetch rotates
    check("runs", runs[:n], ["equal", "uniform"])
    # a base at infinity in the first / the last sorted position of a segment: with equal scalars a digit row is one bucket in index
    # order, so base i sits at position i (mod the segment length) of its row
    for pick in ("first", "last", "thirds", "thirds2", "odd", "all"):
        b = distinct[:n].copy()
        idx = {"first": [0], "last": [n - 1], "thirds": range(0, n, 3), "thirds2": range(2, n, 3), "odd": range(1, n, 2), "all": range(n)}[pick]
        for i in idx:
            b[i] = INF
        check("inf_" + pick, b, ["equal", "uniform"])
print("SEGMENTS_OK", count)
'''


@pytest.mark.parametrize("tuning", ["seg=2", "seg=3", "", "acc_one_wg=1"])
def test_segment_and_bucket_ends(tuning):
    """7 sizes x (6 scalar patterns + repeated / negated bases + 6 placements of bases at infinity x 2 scalar patterns) x {17 x 15 tables, tables=1}."""
    env = dict(os.environ, SNARKVM_HIP_TUNING=tuning)
    r = subprocess.run([sys.executable, "-c", SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert r.returncode == 0 and "SEGMENTS_OK 140" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
