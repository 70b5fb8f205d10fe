#!/usr/bin/env python3
"""Every route of the MSM front end (csrc/msm_registered.hip.h, base_cache.hip.h) once, on seeded inputs, one SHA-256 per output (of its affine form): what a refactor of the
host side must leave bit for bit.  One thread, so the coalescer's "another caller recently" test never fires and every route is deterministic.

    python tools/msm_routes.py                      # prints "<route> <sha256>" lines
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/msm_routes.py      # the same under a kernel trace, a process of its own
    python tools/msm_routes.py --compare A_kernel_trace.csv B_kernel_trace.csv             # dispatch counts and the positions that differ

SNARKVM_HIP_LIB selects the library (snarkvm_amd/_lib.py)."""
import argparse
import csv
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(a, b):
    """Two kernel traces as sequences of (kernel, grid, workgroup).  Several lanes (streams) work at once on the chunked and the batched routes, so the order
    of START TIMES over the whole device differs between two runs of one library; what the host decides is the order in which it SUBMITS (Dispatch_Id)
    and the order on each queue, and those must not differ."""
    def rows(path):
        with open(path, newline="") as f:
            return list(csv.DictReader(f))

    sig = lambda x: (x["Kernel_Name"], x["Grid_Size_X"], x["Grid_Size_Y"], x["Grid_Size_Z"], x["Workgroup_Size_X"], x["Workgroup_Size_Y"], x["Workgroup_Size_Z"])

    def ordered(r, key):
        return [sig(x) for x in sorted(r, key=lambda x: int(x[key]))]

    def differing(x, y):
        return [i for i in range(min(len(x), len(y))) if x[i] != y[i]]

    ra, rb = rows(a), rows(b)
    same_set = sorted(map(sig, ra)) == sorted(map(sig, rb))
    print(f"dispatches: {len(ra)} vs {len(rb)}; as multisets of (kernel, grid, workgroup): {'identical' if same_set else 'DIFFERENT'}")
    bad = len(ra) != len(rb) or not same_set
    for key in ("Dispatch_Id", "Start_Timestamp"):
        if key in ra[0]:
            d = differing(ordered(ra, key), ordered(rb, key))
            print(f"positions that differ in {key} order: {len(d)}" + (f" (first: {d[0]}: {ordered(ra, key)[d[0]]} | {ordered(rb, key)[d[0]]})" if d else ""))
            bad = bad or (key == "Dispatch_Id" and bool(d))
    if "Queue_Id" in ra[0]:  # queue ids are per process: the k-th queue to appear in one trace against the k-th of the other
        def by_queue(r):
            q = {}
            for x in sorted(r, key=lambda x: int(x["Start_Timestamp"])):
                q.setdefault(x["Queue_Id"], []).append(sig(x))
            return list(q.values())
        qa, qb = by_queue(ra), by_queue(rb)
        d = sum(len(differing(x, y)) + abs(len(x) - len(y)) for x, y in zip(qa, qb)) if len(qa) == len(qb) else -1
        print(f"queues: {len(qa)} vs {len(qb)}; positions that differ queue by queue (queues in order of first use): {d}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar="CSV")
    ap.add_argument("--lg-big", type=int, default=23, help="the big handle: 2^k generated bases (host-scalar chunks at 2^(k-1) and 2^k)")
    ap.add_argument("--raw", action="store_true", help="hash the Jacobian images as returned (they differ from run to run of ONE library)")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)

    import numpy as np

    from snarkvm_amd import _lib, plugin, synthetic
    from oracle import cpu as oracle
    from snarkvm_amd.devmem import HipMem
    from snarkvm_amd.layout import G1_AFFINE, G1_PROJECTIVE, G2_PROJECTIVE
    from snarkvm_amd.msm import RegisteredBases, RegisteredBasesG2

    L = _lib.lib()

    def show(route, out):
        """a group element is hashed as its affine form: the Jacobian image an MSM returns is one of many of the same point (which one depends on the order
        the device happened to add in) and differs between two runs of one library"""
        out = np.ascontiguousarray(out)
        if a.raw or (out.dtype == np.uint64 and out.ndim == 1):  # the bytes as they came (counters always)
            data = out.tobytes()
        elif out.nbytes % 288 == 0 and route.startswith("g2"):
            data = oracle.g2_to_affine(out.view(np.uint8).view(G2_PROJECTIVE)).tobytes()
        else:
            data = oracle.g1_to_affine(out.view(np.uint8).view(G1_PROJECTIVE)).tobytes()
        print(route, hashlib.sha256(data).hexdigest(), flush=True)

    def scope(flags, ptr):
        _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(ptr), flags))

    def one_ex(h, off0, n0, off1, n1, sc, on_dev, mont=0, wb=0):
        out = np.zeros(144, dtype=np.uint8)
        _lib.check(L.snarkvm_hip_msm_registered_ex(out.ctypes.data, h._h, off0, n0, off1, n1, sc, on_dev, mont, wb))
        return out

    def batch_ex(h, off0, n0, off1, n1, ptrs, on_dev):
        k = len(ptrs)
        arr = lambda v: (ctypes.c_size_t * k)(*v)
        out = np.zeros(144 * k, dtype=np.uint8)
        _lib.check(L.snarkvm_hip_msm_registered_batch_ex(out.ctypes.data, h._h, k, arr(off0), arr(n0), arr(off1), arr(n1), (ctypes.c_void_p * k)(*ptrs), on_dev, 0, 0))
        return out

    # ---- G1 bases: 2^lg_big generated on the device; the small vector is their first 2^12
    nbig, n = 1 << a.lg_big, 1 << 12
    dbases = HipMem(nbig * 104)
    _lib.check(L.snarkvm_hip_g1_generate_bases_device(ctypes.c_void_p(dbases.ptr), 1, nbig))
    small = dbases.download(n * 104).view(G1_AFFINE)
    sc_big = synthetic.random_fr_integers(nbig, 0xB16)
    sc = sc_big[: 2 * n]
    dsc = HipMem.from_numpy(sc)

    # registration from host points, from device points, from serialized bytes
    hh = RegisteredBases(small, tables=16)
    hd = RegisteredBases(device_ptr=dbases.ptr, npoints=nbig, tables=1)
    hd16 = RegisteredBases(device_ptr=dbases.ptr, npoints=n, tables=16)
    raw = np.zeros(n * 96, dtype=np.uint8)
    _lib.check(L.snarkvm_hip_g1_serialize(raw.ctypes.data, small.ctypes.data, n, 104, 0))
    hs = RegisteredBases.from_serialized(raw.tobytes(), n, compressed=False, validate=True, tables=16)
    for name, h in (("host", hh), ("device", hd16), ("serialized", hs)):
        show(f"g1 registered from {name} points, msm 2^12 host scalars (coalesced)", h.msm(sc[:n]))
    show("g1 host scalars 2^12, window_bits 13 (not coalescible: host-scalar route)", hh.msm(sc[:n], window_bits=13))
    show(f"g1 host scalars 2^{a.lg_big - 1} (two geometric chunks, sink)", hd.msm(sc_big[: nbig // 2]))
    show(f"g1 host scalars 2^{a.lg_big} (three geometric chunks, sink)", hd.msm(sc_big))
    show("g1 device scalars 2^12 (coalesced)", hh.msm(device_ptr=dsc.ptr, npoints=n))
    show("g1 device scalars 2^12, window_bits 13 (owner's lane)", hh.msm(device_ptr=dsc.ptr, npoints=n, window_bits=13))
    scope(1, dsc.ptr)
    in_scope = hh.msm(device_ptr=dsc.ptr, npoints=n)
    in_scope_ex = one_ex(hh, 0, n // 2, n // 4, n // 2, dsc.ptr, 1)
    _lib.check(L.snarkvm_hip_scope_end())
    show("g1 device scalars 2^12 inside an ASYNC_MSM scope", in_scope)
    show("g1 _ex two ranges, device scalars inside an ASYNC_MSM scope", in_scope_ex)
    show("g1 _ex two ranges, host scalars", one_ex(hh, 0, n // 2, n // 4, n // 2, sc.ctypes.data, 0))
    show("g1 _ex two ranges, device scalars", one_ex(hh, 0, n // 2, n // 4, n // 2, dsc.ptr, 1))
    show("g1 _ex two ranges, host scalars, window_bits 13", one_ex(hh, 0, n // 2, n // 4, n // 2, sc.ctypes.data, 0, wb=13))
    show("g1 _batch host scalars", hh.msm_batch([sc[:n], sc[n : 2 * n], sc[:100]], offsets=[0, 0, 7]))
    show("g1 _batch device scalars", hh.msm_batch(device_ptrs=[dsc.ptr, dsc.at(n * 32), dsc.ptr], npoints=[n, n, 100], offsets=[0, 0, 7]))
    show("g1 _batch_ex host scalars", batch_ex(hh, [0, 5], [n // 2, 100], [n // 4, 9], [n // 2, 50], [sc.ctypes.data, sc[n:].ctypes.data], 0))
    show("g1 _batch_ex device scalars", batch_ex(hh, [0, 5], [n // 2, 100], [n // 4, 9], [n // 2, 50], [dsc.ptr, dsc.at(n * 32)], 1))

    # ---- snarkvm_msm over host bases: stateless, the sampled cache, the verified cache
    mine = np.array(small, copy=True)  # the caller's long-lived vector
    plugin.set_base_cache(0)
    show("snarkvm_msm stateless", plugin.msm(mine, sc[:n]))
    plugin.set_base_cache(16, False)
    for step in ("first sighting", "second sighting (registers)", "hit"):
        show(f"snarkvm_msm sampled cache: {step}", plugin.msm(mine, sc[:n]))
    plugin.set_base_cache(16, True)
    for step in ("first sighting", "second sighting (registers)", "hit"):
        show(f"snarkvm_msm verified cache: {step}", plugin.msm(mine, sc[:n]))
    mine[5]["infinity"] = 1  # one byte of the caller's slice changes: the hit must be refused and computed from the bytes passed in
    show("snarkvm_msm verified cache: mismatch", plugin.msm(mine, sc[:n]))
    show("snarkvm_msm base cache counters (lookups, hits, registrations, mismatches)", np.array([plugin.base_cache_stats()[k] for k in ("lookups", "hits", "registrations", "mismatches")], dtype=np.uint64))
    plugin.set_base_cache(0)

    # ---- G2 over 2^10 bases
    n2 = 1 << 10
    g2 = synthetic.g2_points(n2)
    hg = RegisteredBasesG2(g2, tables=16)
    show("g2 host scalars (coalesced)", hg.msm(sc[:n2]))
    show("g2 host scalars, window_bits 13 (upload on the held lane)", hg.msm(sc[:n2], window_bits=13))
    show("g2 device scalars (coalesced)", hg.msm(device_ptr=dsc.ptr, npoints=n2))
    show("g2 device scalars, window_bits 13 (owner's lane)", hg.msm(device_ptr=dsc.ptr, npoints=n2, window_bits=13))
    scope(1, dsc.ptr)
    in_scope = hg.msm(device_ptr=dsc.ptr, npoints=n2)
    _lib.check(L.snarkvm_hip_scope_end())
    show("g2 device scalars inside an ASYNC_MSM scope", in_scope)
    show("g2 batch host scalars", hg.msm_batch([sc[:n2], sc[n2 : 2 * n2], sc[:33]], offsets=[0, 0, 3]))
    show("g2 batch device scalars", hg.msm_batch(device_ptrs=[dsc.ptr, dsc.at(n2 * 32)], npoints=[n2, n2]))
    for h in (hh, hd, hd16, hs, hg):
        h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
