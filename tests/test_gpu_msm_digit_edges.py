"""The variable-base MSM on scalars chosen digit by digit (tests/helpers/msm_digit_cases.py; tests/test_msm_digit_cases_host.py shows on the CPU that
the lists are what they claim): the last bucket of every window - reached by the signed digit -2^(c-1) alone -, the buckets beside it, bucket 0 with both
signs, carry chains, empty rows, the top row's largest digit, digits across the 32-bit words of the recoding buffer, and one bucket filled to counts
around the accumulate segment length.  One MSM per family through registered bases, so that a failure names the family; then the whole list through every
way scalars reach the device.  The stand-alone digit kernels are also compared digit by digit with the reference recoding
(snarkvm_hip_devtest_msm_digits).  Every comparison is exact: affine equality with the oracle's sums, integer equality of digits."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, plugin
from snarkvm_amd.msm import RegisteredBases, RegisteredBasesG2, VariableBase, msm_g2
from tests import util
from tests.helpers import msm_digit_cases as mc

pytestmark = pytest.mark.gpu


def _id(key):
    return "%dx%d-c%d" % key


@pytest.fixture(scope="module")
def registered():
    """one handle per (tables, registered window bits) over the 2 048 bases, shared by the geometries and legs that use it"""
    handles = {}

    def get(key, g2_distinct=False):
        k = (key[0], key[1], g2_distinct)
        if k not in handles:
            if g2_distinct is False:
                handles[k] = RegisteredBases(mc.g1_bases(), tables=key[0], window_bits=key[1])
            else:
                handles[k] = RegisteredBasesG2(mc.g2_bases(g2_distinct), tables=key[0], window_bits=key[1])
        return handles[k]

    yield get
    for h in handles.values():
        h.close()


def _dev(arr):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _eq(got, want, what):
    assert util.affine_equal(oracle.g1_to_affine(got), want), what


@pytest.mark.parametrize("key", mc.GEOMETRIES, ids=_id)
def test_g1_msm_digit_edges(registered, key):
    g, fam, vals, where = mc.cases(key)
    rb, c, n = registered(key), g.c, len(vals)
    print(f"{key}: c = {g.c}, {g.W} windows x {g.J} tables, S = {g.S}, {n} scalars")
    # one MSM per family, the window width of the list's geometry forced (a short family alone would get another plan)
    for name, members in fam.items():
        if members:
            _eq(rb.msm(mc.bigint(members), window_bits=c), mc.g1_expected(members), name)
    common, want_naive = mc.top_common()
    assert fam["top"][: len(common)] == common
    assert util.g1_affine_to_ints(oracle.g1_to_affine(rb.msm(mc.bigint(common), window_bits=c)))[0] == want_naive, "top against pyref.msm_naive"
    # the whole list
    sc, want = mc.bigint(vals), mc.g1_expected(vals)
    _eq(rb.msm(sc, window_bits=c), want, "host scalars, forced")
    _eq(rb.msm(sc, window_bits=key[2]), want, "host scalars, the key's own call")
    _eq(rb.msm(sc), want, "host scalars, the planner's choice")
    d_sc = _dev(sc)
    _eq(rb.msm(device_ptr=d_sc.data_ptr(), npoints=n, window_bits=c), want, "device scalars")
    _eq(rb.msm(device_ptr=d_sc.data_ptr(), npoints=n), want, "device scalars, the planner's choice")
    # Montgomery scalars on the device against two base ranges
    d_mont = _dev(mc.montgomery(vals))
    n0, off1 = n - 100, n + 29
    both = np.concatenate([mc.g1_bases()[3 : 3 + n0], mc.g1_bases()[off1 : off1 + 100]])
    out = np.zeros(1, dtype=oracle.G1_PROJECTIVE)
    _lib.check(_lib.lib().snarkvm_hip_msm_registered_ex(ctypes.c_void_p(out.ctypes.data), rb._h, ctypes.c_size_t(3), ctypes.c_size_t(n0), ctypes.c_size_t(off1),
                                                        ctypes.c_size_t(100), ctypes.c_void_p(d_mont.data_ptr()), 1, 1, c))
    _eq(out, mc.g1_expected(vals, bases=both), "device Montgomery scalars, two base ranges")
    # a sub-range with an offset: the list shifted by three scalars against the digit kernels' blocks
    _eq(rb.msm(sc[3 : n - 5], offset=11, window_bits=c), mc.g1_expected(vals[3 : n - 5], offset=11), "sub-range")
    if key in mc.FUSING:
        k = n // 2 + 1
        want_k = mc.g1_expected(vals[:k])
        for mont in (False, True):
            lists = [mc.montgomery(vals), mc.montgomery(vals[:k])] if mont else [sc, sc[:k]]
            got = rb.msm_batch(lists, window_bits=c, montgomery=mont)
            _eq(got[0:1], want, ("fused batch", mont, 0))
            _eq(got[1:2], want_k, ("fused batch", mont, 1))
    if key in mc.TABLELESS:
        bases = mc.g1_bases()[:n]
        _eq(VariableBase.msm(bases, sc), want, "VariableBase.msm")
        _eq(plugin.msm(bases, sc), want, "plugin.msm")


# the stand-alone digit kernels: u16 (c = 2, 8, 13, 15, 16), u32 (c = 17, 22, 23), and the fused batch's kernel over two instances
DIGIT_KEYS = ((127, 2, 2), (1, 0, 8), (20, 13, 13), (17, 15, 15), (1, 0, 16), (15, 17, 17), (12, 22, 22), (12, 23, 23))


def _digits(key, vals, montgomery, multi):
    g = mc.cases(key)[0]
    n = len(vals)
    pad = lambda k: (k + 8191) // 8192 * 8192
    cols = pad(n) + pad(n - n // 2) if multi else n
    dt = np.uint32 if g.c > 16 else np.uint16
    out = np.zeros((g.Wd, cols), dtype=dt)
    info = (ctypes.c_uint32 * 6)()
    sc = mc.montgomery(vals) if montgomery else mc.bigint(vals)
    _lib.check(_lib.lib().snarkvm_hip_devtest_msm_digits(sc.ctypes.data, n, key[2], key[0], mc.table_bits(key), int(montgomery), int(multi), out.ctypes.data,
                                                          out.nbytes, info))
    assert list(info) == [g.c, g.Wd, out.itemsize, cols, pad(n) if multi else 0, n - n // 2 if multi else 0]
    return out


def _reference_digits(key, vals):
    g = mc.cases(key)[0]
    return np.array([mc.recode(s, g.c, g.Wd)[1] for s in vals], dtype=np.int64).T  # [rows][n]


@pytest.mark.parametrize("montgomery", [False, True], ids=["bigint", "montgomery"])
@pytest.mark.parametrize("key", DIGIT_KEYS, ids=_id)
def test_digit_matrix_against_the_reference_recoding(key, montgomery):
    vals = mc.cases(key)[2]
    got = _digits(key, vals, montgomery, False)
    want = _reference_digits(key, vals)
    bad = np.argwhere(got.astype(np.int64) != want)
    assert bad.size == 0, [(int(w), hex(vals[i]), int(got[w, i]), int(want[w, i])) for w, i in bad[:5]]


@pytest.mark.parametrize("montgomery", [False, True], ids=["bigint", "montgomery"])
@pytest.mark.parametrize("key", mc.FUSING, ids=_id)
def test_digit_matrix_of_a_fused_batch(key, montgomery):
    g, _, vals, _ = mc.cases(key)
    n = len(vals)
    got = _digits(key, vals, montgomery, True).astype(np.int64)
    ref = _reference_digits(key, vals)
    p1 = (n + 8191) // 8192 * 8192
    want = np.full(got.shape, 1 << (g.c - 1), dtype=np.int64)  # padding: the zero digit
    want[:, :n] = ref
    want[:, p1 : p1 + n - n // 2] = ref[:, n // 2 :]
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(w), int(i), int(got[w, i]), int(want[w, i])) for w, i in bad[:5]]


def test_digit_hook_refuses_bad_arguments():
    L = _lib.lib()
    sc = mc.bigint([1, 2, 3])
    out = np.zeros(127 * 3, dtype=np.uint16)
    info = (ctypes.c_uint32 * 6)()
    for args in ((sc.ctypes.data, 3, 2, 1, 256, 0, 0, out.ctypes.data, out.nbytes - 2, info),  # wrong size
                 (None, 3, 2, 1, 256, 0, 0, out.ctypes.data, out.nbytes, info),
                 (sc.ctypes.data, 0, 2, 1, 256, 0, 0, out.ctypes.data, 0, info),
                 (sc.ctypes.data, 3, 24, 1, 256, 0, 0, out.ctypes.data, out.nbytes, info),
                 (sc.ctypes.data, 3, 2, 3, 85, 0, 0, out.ctypes.data, out.nbytes, info),           # no such tables
                 (sc.ctypes.data, 3, 2, 1, 256, 0, 1, out.ctypes.data, out.nbytes, info)):         # a table-less MSM never fuses
        with pytest.raises(_lib.HipError):
            _lib.check(L.snarkvm_hip_devtest_msm_digits(*args))
    _lib.check(L.snarkvm_hip_devtest_msm_digits(sc.ctypes.data, 3, 2, 1, 256, 0, 0, out.ctypes.data, out.nbytes, info))
    assert list(info)[:4] == [2, 127, 2, 3]


# ---- wide windows through the stand-alone u32 digit matrix (tuning fused=0, read once per process) ----------------------------------------------
UNFUSED_SCRIPT = r'''
import sys
sys.path.insert(0, %r)
from oracle import cpu as oracle
from snarkvm_amd.msm import RegisteredBases
from tests import util
from tests.helpers import msm_digit_cases as mc

for key in ((15, 17, 17), (12, 22, 22)):
    g, fam, vals, _ = mc.cases(key)
    rb = RegisteredBases(mc.g1_bases(), tables=key[0], window_bits=key[1])
    for name, members in list(fam.items()) + [("the whole list", vals)]:
        if members:
            assert util.affine_equal(oracle.g1_to_affine(rb.msm(mc.bigint(members), window_bits=g.c)), mc.g1_expected(members)), (key, name)
    rb.close()
print("UNFUSED_OK")
'''


def test_wide_windows_through_the_stand_alone_digit_matrix():
    r = subprocess.run([sys.executable, "-c", UNFUSED_SCRIPT % util.ROOT], capture_output=True, text=True, env=dict(os.environ, SNARKVM_HIP_TUNING="fused=0"),
                       timeout=600, cwd=util.ROOT)
    assert r.returncode == 0 and "UNFUSED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- G2: its own accumulate, fold and bit-plane kernels behind the same digits ------------------------------------------------------------------
def _eq2(got, want, what):
    assert oracle.g2_to_affine(got).tobytes() == want.tobytes(), what


@pytest.mark.parametrize("key", mc.G2_GEOMETRIES, ids=_id)
def test_g2_msm_digit_edges(registered, key):
    g, fam, vals, _ = mc.cases(key)
    n = len(vals)
    rg, c = registered(key, g2_distinct=None), g.c
    for name, members in fam.items():
        if members:
            _eq2(rg.msm(mc.bigint(members), window_bits=c), mc.g2_expected(members), name)
    sc, want = mc.bigint(vals), mc.g2_expected(vals)
    _eq2(rg.msm(sc, window_bits=c), want, "host scalars, forced")
    _eq2(rg.msm(sc), want, "host scalars, the planner's choice")
    d_sc = _dev(sc)
    _eq2(rg.msm(device_ptr=d_sc.data_ptr(), npoints=n, window_bits=c), want, "device scalars")
    _eq2(rg.msm(sc[3 : n - 5], offset=11, window_bits=c), mc.g2_expected(vals[3 : n - 5], offset=11), "sub-range")


def test_g2_one_shot_and_repeated_bases(registered):
    """the one-shot symbol on the case list, and the list over 40 distinct points tiled: equal points meet in the buckets, the equal-x fix kernels run"""
    key = (17, 15, 15)
    g, _, vals, _ = mc.cases(key)
    n, sc = len(vals), mc.bigint(vals)
    _eq2(msm_g2(mc.g2_bases()[:n], sc), mc.g2_expected(vals), "one-shot")
    want = mc.g2_expected(vals, distinct=40)
    _eq2(msm_g2(mc.g2_bases(40)[:n], sc), want, "one-shot, 40 distinct points")
    _eq2(registered(key, g2_distinct=40).msm(sc, window_bits=g.c), want, "registered, 40 distinct points")
