#!/usr/bin/env python3
"""What the fused round-4 evaluation pass is worth against the chain of entry points a caller had before it, both on device memory.

    fused:  ONE snarkvm_hip_fr_matrix_sumcheck_evals over the three registered arithmetizations of a circuit -> a, b, f of A, B and C.
    chain:  the same nine vectors from EXISTING entry points over resident row, col, row_col_val, per matrix
                t1 = alpha - row, t2 = beta - col      fr_vec_op 7 (scalar minus vector), twice
                d = t1 * t2                            fr_vec_op 2
                b = d * b_scale, a = rcv * a_scale     fr_vec_op 4, twice
                d <- f_scale / d (zeros stay)          fr_batch_inversion_and_mul
                f = d * rcv                            fr_vec_op 2
            seven launches per matrix, 21 per circuit; these entry points are identical on the commit before the fused pass.

Both are checked for equality (all nine vectors, bit for bit) before anything is timed.  Device time: two events on the scope's stream around
`--launches` (>= 20) enqueued repetitions, after a warm-up region; the median over `--runs` such regions, per repetition.  Bytes moved are
computed from the shapes (vectors read or written per element x 32 B), not measured.  Shapes: |K| = 2^17 for the three matrices
(credits.aleo/transfer_private) and 2^20.  Operands are random field elements: no pass here depends on the values.

`--variant NAME=PATH` (repeatable) also times the FUSED call on another build of the library (csrc/poly.hip.h built with
-DFR_SUMCHECK_E_MIN=n -DFR_SUMCHECK_E_MAX=n: a fixed share of n elements per thread, or -DFR_SUMCHECK_THREADS=n) in a child process.
A variant is built with `python -m snarkvm_amd.build -DFR_SUMCHECK_E_MIN=32 -DFR_SUMCHECK_E_MAX=32 --out=snarkvm_amd/lib/variants/libsnarkvm_hip_share32.so`.

    python tools/bench_fr_sumcheck.py [--runs 11] [--launches 20] [--variant NAME=PATH ...] [--out profiles/fr_sumcheck.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LG_SIZES = (17, 20)
MATRICES = 3
# vectors of |K| elements read or written per matrix
FUSED_VECTORS = 2 + 1 + 3 + 1 + 3   # forward: row, col in, running product out; backward: row, col, rcv and the parked product in, a, b, f out
CHAIN_VECTORS = 2 + 2 + 3 + 2 + 2 + 5 + 3  # the seven launches above (batch inversion: v in, scratch out, v and scratch in, v out)
CHAIN_LAUNCHES = 7


def measure(runs, launches, fused_only):
    import numpy as np
    import torch

    from snarkvm_amd import _lib, plugin, synthetic
    from snarkvm_amd.devmem import HipMem
    from snarkvm_amd.matrices import RegisteredArithmetization

    L = _lib.lib()
    geo = np.zeros(4, dtype=np.uint32)
    points = []
    scal = synthetic.random_fr_integers(5, 0xA1FA)
    # canonical integers below r, taken as memory-form elements: any residues serve
    alpha, beta, scales = scal[0:1].copy(), scal[1:2].copy(), scal[2:5].copy()
    for lg in LG_SIZES:
        k = 1 << lg
        ops = []
        for m in range(MATRICES):
            v = synthetic.random_fr_integers(3 * k, 0xC0 + m)
            ops.append((v[:k], v[k : 2 * k], v[2 * k :]))
        regs = [RegisteredArithmetization(*o) for o in ops]
        # per matrix: row | col | rcv | a b f (fused) | a b f (chain) | t1 t2 (chain)
        mems = [HipMem(32 * 11 * k) for _ in range(MATRICES)]
        at = lambda m, j: mems[m].ptr + 32 * j * k
        for m, o in enumerate(ops):
            for j in range(3):
                mems[m].upload(o[j], 32 * j * k)

        def fused():
            plugin.fr_sumcheck_evals_device([r.handle for r in regs], [at(m, 3) for m in range(MATRICES)], [at(m, 4) for m in range(MATRICES)],
                                            [at(m, 5) for m in range(MATRICES)], alpha, beta, scales)

        def vec_op(op, out, a, b, scalar):
            _lib.check(L.snarkvm_hip_fr_vec_op(op, out, a, b, None, scalar.ctypes.data if scalar is not None else None, k, 1))

        def chain():
            for m in range(MATRICES):
                row, col, rcv, a, b, f, t1, t2 = (at(m, j) for j in (0, 1, 2, 6, 7, 8, 9, 10))
                vec_op(7, t1, row, None, alpha)
                vec_op(7, t2, col, None, beta)
                vec_op(2, t1, t1, t2, None)
                vec_op(4, b, t1, None, scales[1:2])
                vec_op(4, a, rcv, None, scales[0:1])
                _lib.check(L.snarkvm_hip_fr_batch_inversion_and_mul(t1, k, scales[2:3].ctypes.data, 1))
                vec_op(2, f, t1, rcv, None)

        fused()
        if not fused_only:
            chain()
            for m in range(MATRICES):
                got = mems[m].download(32 * 6 * k, 32 * 3 * k, dtype=np.uint64).reshape(2, 3 * k, 4)
                if not np.array_equal(got[0], got[1]):
                    raise SystemExit(f"bench_fr_sumcheck: the fused pass and the chain differ at 2^{lg}, matrix {m}")

        def region(enqueue):
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(mems[0].ptr)))
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

        legs = [("fused", fused)] + ([] if fused_only else [("chain", chain)])
        for _, fn in legs:
            region(fn)
        L.snarkvm_hip_alloc_stats(None, 1)
        times = {name: [] for name, _ in legs}
        for _ in range(runs):  # the two legs alternate: drift of the box hits both alike
            for name, fn in legs:
                times[name].append(region(fn))
        stats = np.zeros(5, dtype=np.uint64)
        L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        if stats[:4].any():
            raise SystemExit(f"bench_fr_sumcheck: workspace grew inside the timed regions: {stats.tolist()}")
        assert L.snarkvm_hip_selftest_fr_sumcheck_geometry(k, geo.ctypes.data) == 0
        row = {"lg_k": lg, "matrices": MATRICES, "threads_per_member": int(geo[0]), "share": int(geo[3]), "launches_per_region": launches, "runs": runs,
               "checked_equal": not fused_only}
        for name, _ in legs:
            ts = times[name]
            vectors = FUSED_VECTORS if name == "fused" else CHAIN_VECTORS
            row[name] = {"kernel_launches": 1 if name == "fused" else CHAIN_LAUNCHES * MATRICES, "bytes_moved": 32 * k * vectors * MATRICES,
                         "median_us": round(statistics.median(ts) * 1e3, 2), "min_us": round(min(ts) * 1e3, 2), "max_us": round(max(ts) * 1e3, 2)}
        if not fused_only:
            row["chain_over_fused"] = round(row["chain"]["median_us"] / row["fused"]["median_us"], 2)
        points.append(row)
        print(json.dumps(row), flush=True)
        for r in regs:
            r.close()
        for mem in mems:
            mem.free()
    return {"device": torch.cuda.get_device_name(0), "points": points}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_sumcheck.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20 or args.runs < 5:
        raise SystemExit("bench_fr_sumcheck: at least 20 launches per region and 5 regions")
    if args.child:
        print("RESULT " + json.dumps(measure(args.runs, args.launches, True)))
        return
    variants = {}
    for spec in args.variant:  # before this process opens the GPU
        name, path = spec.split("=", 1)
        env = dict(os.environ, SNARKVM_HIP_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--launches", str(args.launches)], env=env,
                           capture_output=True, text=True, timeout=300)
        if r.returncode:
            raise SystemExit(f"bench_fr_sumcheck: the {name} child failed with status {r.returncode}\n{r.stdout}\n{r.stderr}")
        variants[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    res = {"tool": "tools/bench_fr_sumcheck.py",
           "what": "snarkvm_hip_fr_matrix_sumcheck_evals (three members, one launch) vs the chain of fr_vec_op 7, 2, 4 and fr_batch_inversion_and_mul "
                   "producing the same nine vectors on device memory; events around the enqueued repetitions, per repetition, medians; bytes from shapes"}
    res.update(measure(args.runs, args.launches, False))
    if variants:
        res["variants"] = {name: {f"2^{p['lg_k']}": {"threads_per_member": p["threads_per_member"], "share": p["share"], "fused_median_us": p["fused"]["median_us"],
                                                      "fused_min_us": p["fused"]["min_us"]} for p in v["points"]} for name, v in variants.items()}
        res["variants"]["committed"] = {f"2^{p['lg_k']}": {"threads_per_member": p["threads_per_member"], "share": p["share"], "fused_median_us": p["fused"]["median_us"],
                                                           "fused_min_us": p["fused"]["min_us"]} for p in res["points"]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
