#!/usr/bin/env python3
"""Fr NTT and polymul at the SRS-sized domains (2^24 .. 2^28), written to profiles/ntt_large.json.

  * all four NN transforms (forward / inverse x standard / coset), device-resident (snarkvm_amd.devmem, no torch), 2^24 .. 2^28;
  * snarkvm_ntt on a host buffer (upload + transform + download) at 2^27;
  * snarkvm_polymul of two dense operands of 2^(lg - 1) coefficients at 2^27 and 2^28 (host buffers, as the reference's caller passes them);
  * the CPU restatement (oracle/, the reference's CPU transform on OpenMP threads) of the forward transform at 2^27 and 2^28, once each.

Every timed call is preceded by warm-up calls and framed by device synchronisation; the figure is the median of --reps runs.
usage: python tools/ntt_large.py [--reps 5] [--no-cpu] [--out profiles/ntt_large.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import cpu as oracle  # noqa: E402
from snarkvm_amd import _lib, plugin, synthetic  # noqa: E402
from snarkvm_amd.devmem import HipMem  # noqa: E402

TRANSFORMS = {"forward": (0, 0), "inverse": (1, 0), "coset_forward": (0, 1), "coset_inverse": (1, 1)}


def vector(lg, seed):
    """a dense vector of 2^lg canonical elements: a random 2^20 block repeated (values do not change the timing)"""
    base = oracle.fr_op("from_bigint", synthetic.random_fr_integers(1 << min(lg, 20), seed))
    return np.tile(base, (1 << max(lg - 20, 0), 1))


def timed(fn, reps, warmup):
    L = _lib.lib()
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        _lib.check(L.snarkvm_hip_synchronize())
        t0 = time.perf_counter()
        fn()
        _lib.check(L.snarkvm_hip_synchronize())
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lg-min", type=int, default=24)
    ap.add_argument("--lg-max", type=int, default=28)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement (about 30 s at 2^27 and 60 s at 2^28 on 16 threads)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_large.json"))
    args = ap.parse_args()
    assert args.reps >= 5, "the median of at least five runs"
    L = _lib.lib()
    res = {"what": __doc__.splitlines()[0], "reps": args.reps, "warmup": args.warmup, "device_ntt_ms": {}, "host_ntt_ms": {}, "polymul_ms": {}, "cpu_ntt_ms": {}}

    for lg in range(args.lg_min, args.lg_max + 1):
        x = vector(lg, 0x1A00 + lg)
        buf = HipMem.from_numpy(x)
        del x
        res["device_ntt_ms"][str(lg)] = {}
        for name, (d, t) in TRANSFORMS.items():
            call = lambda: _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(buf.ptr), ctypes.c_uint32(lg), 0, d, t))  # noqa: E731
            r = timed(call, args.reps, args.warmup)
            res["device_ntt_ms"][str(lg)][name] = r
            print(f"device NTT 2^{lg} {name}: {r['median_ms']} ms", flush=True)
        buf.free()

    if args.lg_max >= 27:
        lg = 27
        h = vector(lg, 0x2B00)
        r = timed(lambda: plugin.NTT(1 << lg, h, 0, 0, 0), args.reps, args.warmup)
        res["host_ntt_ms"][str(lg)] = {"forward": r}
        print(f"snarkvm_ntt 2^{lg} forward (host buffer): {r['median_ms']} ms", flush=True)
        del h

    for lg in range(max(args.lg_min, 27), args.lg_max + 1):
        a, b = vector(lg - 1, 0x3A00 + lg), vector(lg - 1, 0x3B00 + lg)
        r = timed(lambda: plugin.polymul(1 << lg, [a, b], []), args.reps, 1)
        res["polymul_ms"][str(lg)] = {"two_dense_operands": r}
        print(f"snarkvm_polymul 2^{lg} (two operands of 2^{lg - 1}): {r['median_ms']} ms", flush=True)
        del a, b

    if not args.no_cpu:
        oracle.set_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
        for lg in range(max(args.lg_min, 27), args.lg_max + 1):
            x = vector(lg, 0x4C00 + lg)
            t0 = time.perf_counter()
            oracle.ntt(x)
            ms = (time.perf_counter() - t0) * 1e3
            res["cpu_ntt_ms"][str(lg)] = {"forward": round(ms, 1), "threads": oracle.max_threads(), "runs": 1}
            print(f"CPU restatement 2^{lg} forward: {ms:.0f} ms", flush=True)
            del x

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
