#!/usr/bin/env python3
"""What snarkvm_hip_fr_lincomb is worth against the sequence of calls it replaces, on device memory inside a scope.

    single:    one snarkvm_hip_fr_lincomb call over K operands of n elements (reads K vectors, writes one).
    sequence:  snarkvm_hip_fr_vec_op `scale` (out = c_0 p_0), then K - 1 `axpy` (out += c_k p_k): 3K - 1 vectors of traffic, K launches.

K in {4, 16, 24, 48} at n = 2^17 (an opening of a proof) and 2^24.  Every timed region is scope_begin .. the calls .. scope_end (which
waits), host wall clock, after a warm-up; the median of `--runs` regions; snarkvm_hip_alloc_stats must show that nothing grew.  The two
results are compared bit for bit at every point before anything is timed.

`--variant NAME=PATH` (repeatable) also times K = 16, n = 2^24 on another build of the library (the kernel with one Montgomery reduction per
term, or with its group loop unrolled: built once to choose the shape) in a child process and records the figure beside this build's.

    python tools/bench_fr_lincomb.py [--runs 11] [--variant NAME=PATH ...] [--out profiles/fr_lincomb.json]
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

KS = (4, 16, 24, 48)
LGS = (17, 24)


def measure(points, runs):
    import numpy as np

    from snarkvm_amd import _lib, plugin, synthetic
    from snarkvm_amd.devmem import HipMem

    L = _lib.lib()
    rng = np.random.default_rng(0xF1)
    results = []
    for lg in sorted({lg for _, lg in points}):
        n = 1 << lg
        kmax = max(k for k, l in points if l == lg)
        # canonical values < 2^252 are valid memory words of SOME field elements: all the arithmetic needs
        base = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        base[:, 3] >>= 11
        arena = HipMem(32 * n * (kmax + 2))
        arena.upload(base)
        for k in range(1, kmax):
            arena.copy_from(32 * n * k, arena.ptr, 32 * n)
        ptrs = [arena.ptr + 32 * n * k for k in range(kmax)]
        out_a, out_b = arena.ptr + 32 * n * kmax, arena.ptr + 32 * n * (kmax + 1)
        coeffs = synthetic.random_fr_integers(kmax, 0xC0)  # canonical integers read as Montgomery words: field elements all the same
        cp = [ctypes.c_void_p(coeffs[k : k + 1].ctypes.data) for k in range(kmax)]

        def single(K):
            plugin.fr_lincomb_device(out_a, n, ptrs[:K], [n] * K, coeffs[:K])

        def sequence(K):
            _lib.check(L.snarkvm_hip_fr_vec_op(4, ctypes.c_void_p(out_b), ctypes.c_void_p(ptrs[0]), None, None, cp[0], ctypes.c_size_t(n), 1))
            for k in range(1, K):
                _lib.check(L.snarkvm_hip_fr_vec_op(6, ctypes.c_void_p(out_b), ctypes.c_void_p(out_b), ctypes.c_void_p(ptrs[k]), None, cp[k], ctypes.c_size_t(n), 1))

        def region(fn, K):
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(arena.ptr)))
            t0 = time.perf_counter()
            try:
                fn(K)
            finally:
                _lib.check(L.snarkvm_hip_scope_end())
            return (time.perf_counter() - t0) * 1e3

        for K in [k for k, l in points if l == lg]:
            region(single, K), region(sequence, K)
            a = arena.download(32 * n, 32 * n * kmax)
            b = arena.download(32 * n, 32 * n * (kmax + 1))
            if not np.array_equal(a, b):
                raise SystemExit(f"bench_fr_lincomb: K={K} n=2^{lg}: the single call and the sequence disagree")
            for _ in range(2):
                region(single, K), region(sequence, K)
            L.snarkvm_hip_alloc_stats(None, 1)
            ts = [region(single, K) for _ in range(runs)]
            tq = [region(sequence, K) for _ in range(runs)]
            stats = np.zeros(5, dtype=np.uint64)
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
            if stats[:4].any():
                raise SystemExit(f"bench_fr_lincomb: workspace grew inside the timed regions: {stats.tolist()}")
            ms, ms_seq = statistics.median(ts), statistics.median(tq)
            results.append({"K": K, "lg_n": lg, "single_ms": round(ms, 4), "single_min_ms": round(min(ts), 4), "single_GBps": round((K + 1) * 32 * n / ms / 1e6, 1),
                            "sequence_ms": round(ms_seq, 4), "sequence_min_ms": round(min(tq), 4), "sequence_over_single": round(ms_seq / ms, 3),
                            "traffic_ratio_bound": round((3 * K - 1) / (K + 1), 3), "runs": runs})
            print(json.dumps(results[-1]), flush=True)
        arena.free()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_lincomb.json"))
    ap.add_argument("--child-point", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.runs < 10:
        raise SystemExit("bench_fr_lincomb: at least 10 runs per point")
    if args.child_point:
        K, lg = (int(x) for x in args.child_point.split(","))
        print("RESULT " + json.dumps(measure([(K, lg)], args.runs)[0]))
        return
    variants = {}
    for spec in args.variant:  # before this process opens the GPU
        name, path = spec.split("=", 1)
        env = dict(os.environ, SNARKVM_HIP_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-point", "16,24", "--runs", str(args.runs)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode:
            raise SystemExit(f"bench_fr_lincomb: the {name} child failed with status {r.returncode}\n{r.stdout}\n{r.stderr}")
        variants[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    points = measure([(K, lg) for lg in LGS for K in KS], args.runs)
    res = {"tool": "tools/bench_fr_lincomb.py", "what": "one snarkvm_hip_fr_lincomb call vs scale + (K - 1) axpy calls of snarkvm_hip_fr_vec_op; device memory, inside a scope, "
           "host wall clock around scope_begin .. scope_end, median of `runs`; GB/s on (K + 1) * 32 * n bytes", "points": points,
           "single_call_faster_everywhere": all(p["sequence_over_single"] > 1 for p in points)}
    if variants:
        mine = next(p for p in points if p["K"] == 16 and p["lg_n"] == 24)
        res["kernel_shape"] = {"point": "K = 16, n = 2^24, single call", "committed": {"ms": mine["single_ms"], "min_ms": mine["single_min_ms"], "GBps": mine["single_GBps"]}}
        for name, v in variants.items():
            res["kernel_shape"][name] = {"ms": v["single_ms"], "min_ms": v["single_min_ms"], "GBps": v["single_GBps"]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
