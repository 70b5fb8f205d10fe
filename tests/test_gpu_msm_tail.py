"""The tail kernels of the variable-base MSM - msm_reduce_kernel, msm_bucket_merge_kernel, msm_fold_kernel, msm_bitplane_kernel<., DENSE> and the G2 fix
kernels - launched once each, unmodified, over the lists of tests/helpers/tail_cases.py (snarkvm_hip_devtest_msm_tail), on the exact G1 arithmetic, the
lazy G1 arithmetic and G2.  EVERY output is compared as a group element (affine bytes) with the CPU oracle's sum of exactly the entries the layout comment
of msm.hip.h 7a / 7b assigns to it; an output no workgroup writes must come back as the hook's fill pattern, a written one never.  No tolerance: these are
group elements.  G2: the flag words of the fast kernels must be what the lists imply (none for generic lists, the named output for the equal-sums cases),
an unflagged output must be right WITHOUT the fix kernels, every output with them.  tests/test_msm_tail_cases_host.py pins the lists and the reference on
the CPU.  Every case is launched once; test_gpu_parity.py::test_g2_tail_kernels_give_the_same_sums_on_every_launch keeps the repeat job."""
import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib
from tests.helpers import tail_cases as tc

pytestmark = pytest.mark.gpu

ARITHS = ("g1_exact", "g1_lazy", "g2")
NO_FLAG = 0xFFFFFFFF


def _group(arith):
    return "g2" if arith == "g2" else "g1"


def _launch(c, which, hex2=0, run_fix=0, **override):
    """-> (points, status, flags, aux) of one hook call; override: arguments by name (an array stands for its address)"""
    group = _group(which)
    pool = tc.pool(group)
    start, cnt, terms, seeds, nent = c.hook_arrays()
    geom = c.geom(hex2, run_fix)
    out = np.zeros(c.nout, dtype=oracle.G1_PROJECTIVE if group == "g1" else oracle.G2_PROJECTIVE)
    status = np.full(c.nout, 77, dtype=np.uint32)
    flags = np.full(c.nout, 77, dtype=np.uint32)
    aux = np.full(c.nbt + 1, 77, dtype=np.uint32)
    args = dict(arith=tc.ARITH[which], stage=tc.STAGE[c.stage], geom=geom, points=pool, npoints=len(pool), terms=terms, seeds=seeds, nentries=nent, start=start,
                cnt=cnt, nbt=c.nbt, out=out, status=status, flags=flags, nout=c.nout, aux=aux)
    args.update(override)
    _lib.check(_lib.lib().snarkvm_hip_devtest_msm_tail(*[v.ctypes.data if isinstance(v, np.ndarray) else v for v in args.values()]))
    return out, status, flags, aux


def _rows(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _wrong(c, group, out, status):
    """the indices of the written outputs that are not the oracle's sum; asserts that exactly the outputs the layout leaves alone hold the fill pattern"""
    written = np.array([e is not None for e in c.expected()])
    assert np.array_equal(status == 1, ~written), ("fill pattern", c.id, np.flatnonzero((status == 1) != ~written)[:8].tolist())
    safe = out.copy()
    safe[~written] = tc.point_of(group, ())[0]
    got, want = tc.to_affine(group, safe), tc.to_affine(group, c.expected_points(group))
    return np.flatnonzero((_rows(got) != _rows(want)).any(axis=1) & written)


def _check_planes_and_folds(c, arith):
    group = _group(arith)
    if arith != "g2":
        out, status, flags, _ = _launch(c, arith)
        bad = _wrong(c, group, out, status)
        assert bad.size == 0, (c.id, arith, bad[:8].tolist())
        assert not flags.any()
        return
    mf = c.model_flags()
    written = np.array([f is not None for f in mf])
    want_flags = np.array([NO_FLAG if f is None else f for f in mf], dtype=np.uint32)
    # without the fix kernels a flagged fold slot holds no sum: a plane over it can neither be predicted nor checked
    solid = np.array([o < c.nslots or c.stage == "sparse" or not any(mf[i] for i in c.plane_inputs(o)) for o in range(c.nout)])
    if c.family in ("generic", "geometry", "lengths", "infinities"):
        assert not want_flags[written].any() and solid.all(), "these lists meet no equal x coordinates: the fast kernels alone compute every output"
    for o in c.claims:
        assert want_flags[o] == 1
    for hex2 in (0, 1):
        out, status, flags, _ = _launch(c, arith, hex2, 0)
        assert np.isin(flags[written], (0, 1)).all() and (flags[~written] == NO_FLAG).all(), (c.id, hex2)
        assert np.array_equal(flags[solid], want_flags[solid]), (c.id, hex2, "flags", np.flatnonzero(solid & (flags != want_flags))[:8].tolist())
        bad = _wrong(c, group, out, status)
        bad = bad[(flags[bad] == 0) & solid[bad]]
        assert bad.size == 0, (c.id, hex2, "an unflagged output of the fast kernels", bad[:8].tolist())
        out, status, flags, _ = _launch(c, arith, hex2, 1)
        assert np.array_equal(flags, want_flags), (c.id, hex2, "flags with the fix kernels", np.flatnonzero(flags != want_flags)[:8].tolist())
        bad = _wrong(c, group, out, status)
        assert bad.size == 0, (c.id, hex2, "with the fix kernels", bad[:8].tolist())


def _fold_keys(family):
    return [k for k in tc.keys(family) if tc.stage_of(k) == "fold"]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("key", _fold_keys("generic"))
def test_fold_and_dense_planes_generic_lists(key, arith):
    _check_planes_and_folds(tc.case(key), arith)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("key", _fold_keys("geometry"))
def test_fold_and_dense_planes_geometries(key, arith):
    _check_planes_and_folds(tc.case(key), arith)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("key", _fold_keys("lengths"))
def test_fold_list_lengths_against_the_workgroup(key, arith):
    _check_planes_and_folds(tc.case(key), arith)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("key", _fold_keys("infinities"))
def test_fold_infinity_entries(key, arith):
    _check_planes_and_folds(tc.case(key), arith)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("key", _fold_keys("equal_sums"))
def test_fold_and_dense_planes_equal_sums_at_every_tree_level(key, arith):
    _check_planes_and_folds(tc.case(key), arith)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("key", _fold_keys("all_equal"))
def test_fold_everything_equal(key, arith):
    _check_planes_and_folds(tc.case(key), arith)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("key", [k for k in tc.KEYS if tc.stage_of(k) == "sparse"])
def test_unfolded_planes(key, arith):
    """msm_bitplane_kernel<., false> at the launcher's 256 threads: generic lists at nb = 2, 8, 64, 1024 over one and three windows, infinity entries, everything equal"""
    _check_planes_and_folds(tc.case(key), arith)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("key", tc.keys("reduce"))
def test_reduce_round(key, arith):
    c = tc.case(key)
    out, status, flags, aux = _launch(c, arith)
    assert aux.tolist() == c.start_out(), "start_out is the exclusive scan of ceil(cnt / S2)"
    bad = _wrong(c, _group(arith), out, status)
    assert bad.size == 0, (key, arith, bad[:8].tolist())


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("key", tc.keys("merge"))
def test_bucket_merge(key, arith):
    c = tc.case(key)
    out, status, flags, _ = _launch(c, arith)
    bad = _wrong(c, _group(arith), out, status)
    assert bad.size == 0, (key, arith, bad[:8].tolist())
    untouched = np.array(c.untouched())
    assert (status[untouched] == 2).all(), "another lane's slot, or the slot of a bucket without partial sums, must come back bit for bit"
    assert (status[~untouched] != 1).all()


def test_hook_refuses_bad_arguments():
    fold, sparse = tc.case("generic-m3hb3W3-64.64.q0"), tc.case("generic-nb8W3")

    def geom(c, **kw):
        g = c.geom()
        for name, v in kw.items():
            g[("m", "hb", "W", "nb", "S2", "L", "slot", "fold_threads", "plane_threads", "hex", "quads", "run_fix").index(name)] = v
        return g

    short = fold.hook_arrays()[1].copy()
    short[-1] += 1  # the last list overruns the entries
    moved = fold.hook_arrays()[0].copy()
    moved[3] += 1
    bad = [(fold, dict(points=None)), (fold, dict(terms=None)), (fold, dict(start=None)), (fold, dict(out=None)), (fold, dict(flags=None)), (fold, dict(geom=None)),
           (fold, dict(geom=geom(fold, hb=4))),                      # hb > m
           (fold, dict(geom=geom(fold, m=12, hb=12))),               # hb > 11
           (sparse, dict(geom=geom(sparse, nb=2048))),               # nb > 1024
           (sparse, dict(geom=geom(sparse, nb=6))),
           (fold, dict(geom=geom(fold, fold_threads=96))), (fold, dict(geom=geom(fold, plane_threads=512))), (sparse, dict(geom=geom(sparse, plane_threads=32))),
           (fold, dict(geom=geom(fold, quads=2))), (fold, dict(geom=geom(fold, quads=1))),   # a quad-strided loop with 64 threads
           (fold, dict(geom=geom(fold, hex=1))),                     # a G2 switch on G1
           (fold, dict(cnt=short)), (fold, dict(start=moved)),
           (fold, dict(nout=fold.nout - 1)), (fold, dict(arith=3)), (fold, dict(stage=4))]
    for c, override in bad:
        with pytest.raises(_lib.HipError):
            _launch(c, "g1_exact", **override)
    out, status, _, _ = _launch(fold, "g1_exact")
    assert _wrong(fold, "g1", out, status).size == 0
