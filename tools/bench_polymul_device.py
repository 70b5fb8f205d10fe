#!/usr/bin/env python3
"""What snarkvm_hip_polymul_device is worth against the sequence a device-resident caller composes without it.

    composed: memcpy_d2d + memset per operand (a domain-sized row each), snarkvm_hip_ntt_device_batch (forward, in place),
              snarkvm_hip_fr_vec_op (MUL, once per further operand), snarkvm_hip_ntt_device (inverse) - snarkvm_amd/proofs.py::replay_single;
    fused:    one snarkvm_hip_polymul_device call over the operands where they are.

Both run device-resident inside a snarkvm_hip_scope: one sample = scope_begin, `reps` products, scope_end, wall clock / reps; the median of
`samples` samples after `warmup` is reported, with min and max.  Shapes: two operands of n / 2 coefficients at 2^17, 2^18 and 2^24, three
operands at 2^18.  The pass kernel is ALU-bound: the product load adds m - 1 Fr products per element to one pass and takes away a
96 n-byte pass and the row preparation; which one wins is what this tool measures.

Condition per shape: median(fused) <= median(composed) + (max - min)(composed) - the margin is the noise of the baseline itself.

The composed sequence is meant to run on a build of the PARENT commit (--baseline-lib path/to/libsnarkvm_hip.so of that build; it uses only calls
that commit has) and the fused call on this checkout's library, on the same box, each in a child process of its own (one library per process).
Without --baseline-lib both run on this checkout's library, and the JSON says so.  --ntt24 adds the in-place Fr NTT at 2^24 on both libraries (one
snarkvm_hip_ntt_device_batch call of 10 transforms, as bench.py --full times it): the plain-load instantiations must not have moved.

    python tools/bench_polymul_device.py [--baseline-lib PATH] [--ntt24] [--out profiles/polymul_device.json]
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(17, 2), (18, 2), (24, 2), (18, 3)]  # (lg, operands of n / 2 coefficients; three operands: n / 4 each)


def stats(xs):
    return {"median_ms": statistics.median(xs) * 1e3, "min_ms": min(xs) * 1e3, "max_ms": max(xs) * 1e3, "samples": len(xs)}


class RustError(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("message", ctypes.c_void_p)]


def load(path):
    """The handful of calls this tool times, bound by hand: snarkvm_amd._lib resolves EVERY symbol of this checkout's header, which a
    library built from the parent commit does not have."""
    V, Z, I, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
    sigs = {"snarkvm_hip_malloc": [ctypes.POINTER(V), Z, I], "snarkvm_hip_free": [V], "snarkvm_hip_memcpy_h2d": [V, V, Z], "snarkvm_hip_memcpy_d2h": [V, V, Z],
            "snarkvm_hip_memcpy_d2d": [V, V, Z], "snarkvm_hip_memset": [V, I, Z], "snarkvm_hip_scope_begin": [V], "snarkvm_hip_scope_end": [],
            "snarkvm_hip_ntt_device": [V, U, I, I, I], "snarkvm_hip_ntt_device_batch": [V, Z, U, I, V, V], "snarkvm_hip_fr_vec_op": [I, V, V, V, V, V, Z, I],
            "snarkvm_hip_polymul_device": [V, Z, V, V, Z, V, V, U]}
    L = ctypes.CDLL(path)
    for name, argtypes in sigs.items():
        if name == "snarkvm_hip_polymul_device" and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = RustError, argtypes
    return L


def check(err):
    if err.code:
        raise SystemExit(f"snarkvm_hip error {err.code}: {ctypes.string_at(err.message).decode(errors='replace') if err.message else ''}")


def child(mode, samples, warmup, ntt24, only=None):
    """mode: composed | fused.  Prints one JSON object."""
    import numpy as np

    from snarkvm_amd import synthetic

    path = os.environ.get("SNARKVM_HIP_LIB") or os.path.join(ROOT, "snarkvm_amd", "lib", "libsnarkvm_hip.so")
    L = load(path)
    out = {"lib": path, "mode": mode, "shapes": {}}

    def dev(nbytes, data=None):
        p = ctypes.c_void_p()
        check(L.snarkvm_hip_malloc(ctypes.byref(p), nbytes, 0))
        if data is not None:
            data = np.ascontiguousarray(data)
            check(L.snarkvm_hip_memcpy_h2d(p, data.ctypes.data, data.nbytes))
        return p.value

    def sampled(fn, anchor, reps):
        xs = []
        for i in range(warmup + samples):
            t0 = time.perf_counter()
            check(L.snarkvm_hip_scope_begin(anchor))
            try:
                for _ in range(reps):
                    fn()
            finally:
                check(L.snarkvm_hip_scope_end())
            if i >= warmup:
                xs.append((time.perf_counter() - t0) / reps)
        return xs

    for lg, m in SHAPES:
        if only and f"2p{lg}_x{m}" not in only:
            continue
        n = 1 << lg
        ln = n // 2 if m == 2 else n // 4
        reps = 4 if lg >= 22 else 32
        # any canonical integers below r are Fr elements for the purpose of timing
        ops = [dev(32 * ln, synthetic.random_fr_integers(ln, 0xB0 + k)) for k in range(m)]
        rows = [dev(32 * n) for _ in range(m)]
        if mode == "fused":
            pp = (ctypes.c_void_p * m)(*ops)
            pl = (ctypes.c_size_t * m)(*([ln] * m))

            def fn():
                check(L.snarkvm_hip_polymul_device(rows[0], m, pp, pl, 0, None, None, lg))
        else:
            ptrs = (ctypes.c_void_p * m)(*rows)

            def fn():
                for o, r in zip(ops, rows):
                    check(L.snarkvm_hip_memcpy_d2d(r, o, 32 * ln))
                    check(L.snarkvm_hip_memset(r + 32 * ln, 0, 32 * (n - ln)))
                check(L.snarkvm_hip_ntt_device_batch(ptrs, m, lg, 0, None, None))
                for r in rows[1:]:
                    check(L.snarkvm_hip_fr_vec_op(2, rows[0], rows[0], r, None, None, n, 1))
                check(L.snarkvm_hip_ntt_device(rows[0], lg, 0, 1, 0))

        xs = sampled(fn, rows[0], reps)
        out["shapes"][f"2p{lg}_x{m}"] = dict(stats(xs), reps_per_sample=reps, operand_len=ln)
        got = np.empty(4 * n, dtype=np.uint64)
        check(L.snarkvm_hip_memcpy_d2h(got.ctypes.data, rows[0], got.nbytes))
        out.setdefault("digest", {})[f"2p{lg}_x{m}"] = int(np.bitwise_xor.reduce(got))  # both modes must leave the same product
        for b in ops + rows:
            check(L.snarkvm_hip_free(b))
    if ntt24:
        lg, k = 24, 10
        v = dev(32 << lg, synthetic.random_fr_integers(1 << lg, 0xB7))
        ptrs = (ctypes.c_void_p * k)(*([v] * k))
        dirs = (ctypes.c_int * k)(*[i & 1 for i in range(k)])
        xs = []
        for i in range(warmup + samples):
            t0 = time.perf_counter()
            check(L.snarkvm_hip_ntt_device_batch(ptrs, k, lg, 0, dirs, None))
            if i >= warmup:
                xs.append((time.perf_counter() - t0) / k)
        out["ntt_2p24"] = dict(stats(xs), transforms_per_sample=k)
        check(L.snarkvm_hip_free(v))
    print(json.dumps(out))


def run_child(lib, mode, args):
    env = dict(os.environ)
    if lib:
        env["SNARKVM_HIP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--samples", str(args.samples), "--warmup", str(args.warmup)] + (["--ntt24"] if args.ntt24 else [])
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
    if r.returncode:
        raise SystemExit(f"bench_polymul_device: the {mode} child failed with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline-lib", help="libsnarkvm_hip.so built from the parent commit: the composed sequence (and its NTT) run on it")
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ntt24", action="store_true")
    ap.add_argument("--child", choices=["composed", "fused"])
    ap.add_argument("--only", action="append", metavar="SHAPE", help="--child: only this shape (2p18_x2 ...; repeatable) - for a run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polymul_device.json"))
    args = ap.parse_args()
    if args.samples < 5:
        raise SystemExit("at least 5 samples")
    if args.child:
        child(args.child, args.samples, args.warmup, args.ntt24, args.only)
        return
    composed = run_child(args.baseline_lib, "composed", args)
    fused = run_child(None, "fused", args)
    res = {"tool": "tools/bench_polymul_device.py", "baseline": "parent-commit build" if args.baseline_lib else "this checkout's library (no --baseline-lib)",
           "method": "device-resident, inside a scope; sample = (scope_begin, reps products, scope_end) / reps; median of samples after warm-up",
           "condition": "median(fused) <= median(composed) + (max - min)(composed)", "shapes": {}}
    for key, c in composed["shapes"].items():
        f = fused["shapes"][key]
        spread = c["max_ms"] - c["min_ms"]
        res["shapes"][key] = {"composed": c, "fused": f, "baseline_spread_ms": spread, "speedup": c["median_ms"] / f["median_ms"],
                              "condition_met": f["median_ms"] <= c["median_ms"] + spread, "same_product": composed["digest"][key] == fused["digest"][key]}
    if args.ntt24:
        c, f = composed["ntt_2p24"], fused["ntt_2p24"]
        spread = c["max_ms"] - c["min_ms"]
        res["ntt_2p24"] = {"baseline": c, "this": f, "baseline_spread_ms": spread, "unchanged": abs(f["median_ms"] - c["median_ms"]) <= spread}
    res["all_conditions_met"] = all(s["condition_met"] for s in res["shapes"].values())
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
