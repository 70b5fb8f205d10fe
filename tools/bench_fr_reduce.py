#!/usr/bin/env python3
"""What the one-pass reductions are worth against the route they replace, on device-resident operands.

    one pass:  snarkvm_hip_fr_reduce (SUM, DOT) / snarkvm_hip_fr_support on device memory: the 32-byte / 24-byte answer is all that returns.
    replaced:  SUM      snarkvm_hip_memcpy_d2h of the vector, then a host sum (numpy column sums of the 16-bit pieces, one `% r` in Python);
               DOT      snarkvm_hip_fr_mul_device into a scratch vector, then the same download and host sum;
               support  the download alone (what numpy does with the copy is not counted).

n = 2^16, 2^18, 2^20, 2^24.  Every timed region is host wall clock around synchronous calls, after a warm-up; the median of `--runs` regions
(`--slow-runs` for the replaced routes, whose downloads take tens of milliseconds at 2^24); snarkvm_hip_alloc_stats must show that nothing grew
inside the one-pass regions.  The one-pass results are compared with the replaced route's before anything is timed.  `fraction_of_hbm_peak`:
the algorithmic bytes (32 n for SUM and support, 64 n for DOT) over the time, against the 8 TB/s of DESIGN.md section 7.

`--variant NAME=PATH` (repeatable) also times n = 2^24 on another build of the library (another group size of the inner product, another cap on
the grid: built once to choose the shape) in a child process and records the figures beside this build's.

    python tools/bench_fr_reduce.py [--runs 21] [--slow-runs 5] [--variant NAME=PATH ...] [--out profiles/fr_reduce.json]
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

LGS = (16, 18, 20, 24)
HBM_PEAK = 8.0e12  # bytes/s, DESIGN.md section 7
R_MOD = 8444461749428370424248824938781546531375899335154063827935233455917409239041


def host_sum(v):
    """sum of n memory-form elements mod r without the oracle: column sums of the sixteen 16-bit pieces (each < 2^40 for n <= 2^24)"""
    import numpy as np

    total = 0
    for limb in range(4):
        col = v[:, limb]
        for piece in range(4):
            total += int(np.sum((col >> np.uint64(16 * piece)) & np.uint64(0xFFFF), dtype=np.uint64)) << (64 * limb + 16 * piece)
    return total % R_MOD


def as_int(res):
    return sum(int(x) << (64 * i) for i, x in enumerate(res.reshape(-1)))


def measure(lgs, runs, slow_runs, with_replaced=True):
    import numpy as np

    from snarkvm_amd import _lib, plugin
    from snarkvm_amd.devmem import HipMem

    L = _lib.lib()
    rng = np.random.default_rng(0xF2)
    results = []
    for lg in lgs:
        n = 1 << lg
        # canonical values < 2^252 are valid memory words of SOME field elements: all the arithmetic needs
        base = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        base[:, 3] >>= 11
        arena = HipMem(32 * n * 3)
        arena.upload(base)
        arena.upload(np.roll(base, 1, axis=0), 32 * n)
        a, b, scratch = arena.ptr, arena.ptr + 32 * n, arena.ptr + 64 * n
        host = np.empty((n, 4), dtype=np.uint64)

        def timed(fn, k):
            ts = []
            for _ in range(k):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return ts

        def d2h(src):
            _lib.check(L.snarkvm_hip_memcpy_d2h(host.ctypes.data, src, 32 * n))

        one = {"sum": lambda: plugin.fr_reduce_device(plugin.FR_REDUCE_SUM, a, None, n), "dot": lambda: plugin.fr_reduce_device(plugin.FR_REDUCE_DOT, a, b, n),
               "support": lambda: plugin.fr_support_device(a, n)}

        def replaced_sum():
            d2h(a)
            return host_sum(host)

        def replaced_dot():
            _lib.check(L.snarkvm_hip_fr_mul_device(ctypes.c_void_p(scratch), ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_size_t(n)))
            d2h(scratch)
            return host_sum(host)

        replaced = {"sum": replaced_sum, "dot": replaced_dot, "support": lambda: d2h(a)}
        # the same answers, before anything is timed
        if as_int(one["sum"]()) != replaced_sum() or as_int(one["dot"]()) != replaced_dot():
            raise SystemExit(f"bench_fr_reduce: n=2^{lg}: the one-pass result and the replaced route disagree")
        if tuple(int(x) for x in one["support"]()) != (n, 0, int(base.any(axis=1).sum())):
            raise SystemExit(f"bench_fr_reduce: n=2^{lg}: wrong support")
        row = {"lg_n": lg, "runs": runs, "slow_runs": slow_runs}
        for name in ("sum", "dot", "support"):
            timed(one[name], 3)
            L.snarkvm_hip_alloc_stats(None, 1)
            ts = timed(one[name], runs)
            stats = np.zeros(5, dtype=np.uint64)
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
            if stats[:4].any():
                raise SystemExit(f"bench_fr_reduce: workspace grew inside the timed regions: {stats.tolist()}")
            ms = statistics.median(ts)
            nbytes = (64 if name == "dot" else 32) * n
            row[name] = {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "GBps": round(nbytes / ms / 1e6, 1), "fraction_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}
            if with_replaced:
                timed(replaced[name], 1)
                tr = statistics.median(timed(replaced[name], slow_runs))
                row[name].update({"replaced_ms": round(tr, 4), "replaced_over_one_pass": round(tr / ms, 2)})
        results.append(row)
        print(json.dumps(row), flush=True)
        arena.free()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--slow-runs", type=int, default=5)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_reduce.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.runs < 10:
        raise SystemExit("bench_fr_reduce: at least 10 runs per point")
    if args.child:
        print("RESULT " + json.dumps(measure((24,), args.runs, 0, with_replaced=False)[0]))
        return
    variants = {}
    for spec in args.variant:  # before this process opens the GPU
        name, path = spec.split("=", 1)
        env = dict(os.environ, SNARKVM_HIP_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode:
            raise SystemExit(f"bench_fr_reduce: the {name} child failed with status {r.returncode}\n{r.stdout}\n{r.stderr}")
        variants[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    points = measure(LGS, args.runs, args.slow_runs)
    res = {"tool": "tools/bench_fr_reduce.py",
           "what": "snarkvm_hip_fr_reduce (SUM, DOT) and snarkvm_hip_fr_support on device memory vs the route they replace (fr_mul_device for DOT, memcpy_d2h, numpy "
                   "host sum; support: the download alone); synchronous calls, host wall clock, medians; fraction_of_hbm_peak = algorithmic bytes / time / 8 TB/s",
           "points": points, "one_pass_faster_everywhere": all(p[k]["replaced_over_one_pass"] > 1 for p in points for k in ("sum", "dot", "support"))}
    if variants:
        mine = next(p for p in points if p["lg_n"] == 24)
        res["kernel_shape"] = {"point": "n = 2^24, ms (median) of the one-pass calls", "committed": {k: mine[k]["ms"] for k in ("sum", "dot", "support")}}
        for name, v in variants.items():
            res["kernel_shape"][name] = {k: v[k]["ms"] for k in ("sum", "dot", "support")}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
