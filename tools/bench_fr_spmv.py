#!/usr/bin/env python3
"""What the device-resident sparse product is worth against what its absence forces on a caller whose vectors live in HBM.

    device:    snarkvm_hip_fr_spmv on resident operands over a registered matrix.  Device time: two events on the scope's stream around
               `--launches` (>= 20) enqueued products, after a warm-up; the median over `--runs` such regions, divided by the launches.
    replaced:  snarkvm_hip_memcpy_d2h of x plus snarkvm_hip_memcpy_h2d of y - the transfers ALONE, host wall clock around the synchronous calls.  A lower
               bound: the caller's CPU product between the two copies is left out entirely.

Shapes: credits.aleo/transfer_private (51 002 constraints, variable domain 2^16, 111 472 entries, |R| = 2^16) and
transfer_public (12 325, 2^14, 38 006, |R| = 2^14); for each the matrix (z_M = M z, y of |R| elements) and its transpose (M^T l_alpha, x = the |R|
Lagrange coefficients), batches of 1 and 8 (shared x).  The matrices come from synthetic.r1cs_like_matrix - an ASSUMED row-length distribution, see
its docstring.  Skew check: the transpose against a matrix of the same rows, columns and entries whose rows all have the same length.

`--variant NAME=PATH` (repeatable) also times every point on another build of the library (csrc/poly.hip.h built with -DFR_SPMV_SEG=... or
-DFR_SPMV_WIDTH=...) in a child process and records the device times beside this build's.
A variant is built with `python -m snarkvm_amd.build -DFR_SPMV_SEG=512 --out=snarkvm_amd/lib/variants/libsnarkvm_hip_seg512.so` (a full build of
its own, objects kept apart from the product build's).

    python tools/bench_fr_spmv.py [--runs 11] [--launches 20] [--variant NAME=PATH ...] [--out profiles/fr_spmv.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"transfer_private": (51002, 16, 111472), "transfer_public": (12325, 14, 38006)}  # constraints, lg of the variable / constraint domain, entries


def uniform_like(t):
    """rows, cols and entries of `t`, every row the same length (the first nnz % rows one longer), the same values, columns cycling"""
    import numpy as np

    from snarkvm_amd.matrices import SparseMatrix

    lens = np.full(t.rows, t.nnz // t.rows, dtype=np.int64)
    lens[: t.nnz % t.rows] += 1
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return SparseMatrix(t.rows, t.cols, row_ptr, (np.arange(t.nnz, dtype=np.uint64) * 7919 % t.cols).astype(np.uint32), t.vals)


def measure(runs, launches):
    import numpy as np
    import torch

    from snarkvm_amd import _lib, matrices, synthetic
    from snarkvm_amd.devmem import HipMem
    from snarkvm_amd.matrices import RegisteredMatrix, SparseMatrix

    L = _lib.lib()
    geo = np.zeros(4, dtype=np.uint32)
    points = []
    for shape, (constraints, lg, nnz) in SHAPES.items():
        n = 1 << lg
        m = SparseMatrix(constraints, n, *synthetic.r1cs_like_matrix(constraints, n, nnz, 0x7A))
        t = matrices.transpose(m, n, 1 << 8)
        for name, mat in (("matrix", m), ("transpose", t), ("uniform_like_transpose", uniform_like(t))):
            reg = RegisteredMatrix(mat)
            n_out = n
            x_elems = max(mat.cols, 1)
            x = synthetic.random_fr_integers(x_elems, 0xB1)
            mem = HipMem(32 * (x_elems + 8 * n_out))
            mem.upload(x)
            d_x, d_y = mem.ptr, mem.ptr + 32 * x_elems
            host_x, host_y = np.empty((x_elems, 4), dtype=np.uint64), np.zeros((8 * n_out, 4), dtype=np.uint64)
            lens = mat.row_lengths()
            row = {"shape": shape, "matrix": name, "rows": mat.rows, "cols": mat.cols, "nnz": mat.nnz, "longest_row": int(lens.max()),
                   "median_row": float(np.median(lens[lens > 0])), "launches": launches, "runs": runs}
            for count in (1, 8):
                def enqueue():
                    reg.mul_device(d_y, n_out, d_x, count, 0, n_out)

                def region():
                    _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(mem.ptr)))
                    try:
                        stream = torch.cuda.ExternalStream(L.snarkvm_hip_scope_stream())
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        for _ in range(launches):
                            enqueue()
                        e1.record(stream)
                    finally:
                        _lib.check(L.snarkvm_hip_scope_end())
                    e1.synchronize()
                    return e0.elapsed_time(e1) / launches

                region()
                L.snarkvm_hip_alloc_stats(None, 1)
                ts = [region() for _ in range(runs)]
                stats = np.zeros(5, dtype=np.uint64)
                L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
                if stats[:4].any():
                    raise SystemExit(f"bench_fr_spmv: workspace grew inside the timed regions: {stats.tolist()}")

                def transfers():
                    t0 = time.perf_counter()
                    _lib.check(L.snarkvm_hip_memcpy_d2h(host_x.ctypes.data, d_x, 32 * mat.cols))
                    _lib.check(L.snarkvm_hip_memcpy_h2d(d_y, host_y.ctypes.data, 32 * count * n_out))
                    return (time.perf_counter() - t0) * 1e3

                transfers()
                tr = statistics.median(transfers() for _ in range(runs))
                dev = statistics.median(ts)
                row[f"count{count}"] = {"device_us": round(dev * 1e3, 2), "device_min_us": round(min(ts) * 1e3, 2), "transfers_us": round(tr * 1e3, 2),
                                        "transfers_over_device": round(tr / dev, 2)}
            points.append(row)
            print(json.dumps(row), flush=True)
            reg.close()
            mem.free()
    assert L.snarkvm_hip_selftest_fr_spmv_geometry(51002, 111472, geo.ctypes.data) == 0
    return {"S": int(geo[0]), "width_at_transfer_private": int(geo[1]), "threads": int(geo[2]), "points": points}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_spmv.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20 or args.runs < 5:
        raise SystemExit("bench_fr_spmv: at least 20 launches per region and 5 regions")
    if args.child:
        print("RESULT " + json.dumps(measure(args.runs, args.launches)))
        return
    variants = {}
    for spec in args.variant:  # before this process opens the GPU
        name, path = spec.split("=", 1)
        env = dict(os.environ, SNARKVM_HIP_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--launches", str(args.launches)], env=env,
                           capture_output=True, text=True, timeout=300)
        if r.returncode:
            raise SystemExit(f"bench_fr_spmv: the {name} child failed with status {r.returncode}\n{r.stdout}\n{r.stderr}")
        variants[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    res = {"tool": "tools/bench_fr_spmv.py",
           "what": "snarkvm_hip_fr_spmv on resident operands (events around the enqueued launches, per launch) vs memcpy_d2h of x + memcpy_h2d of y alone "
                   "(host wall clock; the caller's CPU product is NOT counted); medians; matrices from synthetic.r1cs_like_matrix (an assumed distribution)"}
    res.update(measure(args.runs, args.launches))

    def dev(points, shape, matrix, count=1):
        return next(p for p in points if p["shape"] == shape and p["matrix"] == matrix)[f"count{count}"]["device_us"]

    res["skew"] = {shape: round(dev(res["points"], shape, "transpose") / dev(res["points"], shape, "uniform_like_transpose"), 3) for shape in SHAPES}
    if variants:
        res["variants"] = {}
        for name, v in variants.items():
            res["variants"][name] = {"S": v["S"], "width_at_transfer_private": v["width_at_transfer_private"],
                                     "device_us": {f"{p['shape']}/{p['matrix']}/count{c}": p[f"count{c}"]["device_us"] for p in v["points"] for c in (1, 8)}}
        res["variants"]["committed"] = {"S": res["S"], "width_at_transfer_private": res["width_at_transfer_private"],
                                        "device_us": {f"{p['shape']}/{p['matrix']}/count{c}": p[f"count{c}"]["device_us"] for p in res["points"] for c in (1, 8)}}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
