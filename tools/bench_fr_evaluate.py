#!/usr/bin/env python3
"""What snarkvm_hip_fr_evaluate is worth against the calls that yield the same values today, on device memory inside a scope.

    new:  ONE snarkvm_hip_fr_evaluate over the distinct (polynomial, point) pairs of the shape.  For a shape with combinations the values are
          combined on the host afterwards (sum_k a_k value_k in Python integers: `host_combine_us`, measured once, NOT part of `new_us`).
    (a):  one snarkvm_hip_fr_open_fold without a quotient per (combination, point): SonicKZG10.evaluate_combinations_device, route "fold".
    (b):  per combination one snarkvm_hip_fr_lincomb into a buffer, then snarkvm_hip_fr_divide_by_linear without a quotient over it.
    (c):  one snarkvm_hip_fr_divide_by_linear without a quotient per distinct (polynomial, point) pair (combined on the host like `new`).

Shapes: one polynomial at 2^16, 2^17, 2^20 and 2^24 coefficients; the `evaluations` of a proof (varuna.rs:583-592) - g_1 at beta and g_a, g_b, g_c of
C = 1, 2, 3 circuits at gamma, 3 C + 1 polynomials at two points, 2^17; the gamma point's combinations of tools/bench_fr_open_fold.py (10 / 19 / 28
members in 4 / 7 / 10 combinations) at 2^17 and 2^20; its beta point for 1, 4, 16 instances at 2^16 and 2^18.

The values of the four routes are compared bit for bit at every shape before anything is timed.  A timed region is scope_begin .. `reps`
repetitions of the route's calls .. scope_end (which waits and delivers the values), host wall clock, reported per repetition in microseconds;
every round times (a), new, (b), (c), (a) in that order, so that the two (a) series bracket the others; medians over `--runs` rounds after a
warm-up; snarkvm_hip_alloc_stats must show that nothing grew.  `a_spread_us` is the distance between the medians of the two (a) series - what
(a) itself moves by within the session - and a shape counts as LOST when the median of `new` exceeds that of (a) by more than it.  From 2^20
coefficients on, `share_of_8TBs` is 32 bytes x the coefficients `new` reads, over its time, over the 8 TB/s of DESIGN.md section 7.

`--variant NAME=PATH` (repeatable) also times `new` at the one-polynomial and gamma shapes on another build of the library (csrc/poly.hip.h built
with -DFR_EVALUATE_G=... or -DFR_EVALUATE_POW=1: `python -m snarkvm_amd.build -DFR_EVALUATE_G=1 --out=snarkvm_amd/lib/variants/NAME.so`), each in
a child process of its own that runs before this one opens the GPU.

    python tools/bench_fr_evaluate.py [--runs 15] [--variant NAME=PATH ...] [--out profiles/fr_evaluate.json]

Results and the decision they led to: profiles/fr_evaluate.md.
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


def gamma_point(circuits):
    """member indices per combination: g_a, g_b, g_c of every circuit alone, then h_2 with the a_poly_* / b_poly_* of every circuit"""
    lcs = [[k] for k in range(3 * circuits)]
    lcs.append(list(range(3 * circuits, 9 * circuits + 1)))
    return 9 * circuits + 1, lcs


def beta_point(instances):
    """g_1, mask_poly, h_1 in one combination, every w_j alone"""
    return 3 + instances, [[0, 1, 2]] + [[3 + j] for j in range(instances)]


def shapes():
    """-> dicts {kind, param, lg, members, combos: [(member indices, point index)]}; point 0 = beta, 1 = gamma"""
    out = [{"kind": "single", "param": 1, "lg": lg, "members": 1, "combos": [([0], 1)]} for lg in (16, 17, 20, 24)]
    out += [{"kind": "evaluations", "param": c, "lg": 17, "members": 3 * c + 1, "combos": [([0], 0)] + [([k], 1) for k in range(1, 3 * c + 1)]} for c in (1, 2, 3)]
    for lg in (17, 20):
        for c in (1, 2, 3):
            k, lcs = gamma_point(c)
            out.append({"kind": "gamma", "param": c, "lg": lg, "members": k, "combos": [(ks, 1) for ks in lcs]})
    for lg in (16, 18):
        for i in (1, 4, 16):
            k, lcs = beta_point(i)
            out.append({"kind": "beta", "param": i, "lg": lg, "members": k, "combos": [(ks, 0) for ks in lcs]})
    return out


def reps_for(lg):
    return 32 if lg <= 18 else (8 if lg <= 20 else 4)


def measure(runs, variant_shapes_only=False):
    import numpy as np

    from snarkvm_amd import _lib, plugin, sonic_pc, synthetic
    from snarkvm_amd.devmem import HipMem

    L = _lib.lib()
    geo = np.zeros(8, dtype=np.uint32)
    assert L.snarkvm_hip_selftest_fr_evaluate_geometry(ctypes.c_size_t(1 << 24), ctypes.c_void_p(geo.ctypes.data)) == 0
    rng = np.random.default_rng(0xE7)
    todo = [s for s in shapes() if not variant_shapes_only or s["kind"] in ("single", "gamma")]
    results = []
    for lg in sorted({s["lg"] for s in todo}):
        n = 1 << lg
        here = [s for s in todo if s["lg"] == lg]
        kmax = max(s["members"] for s in here)
        lmax = max(len(s["combos"]) for s in here)
        # canonical values < 2^252 are valid memory words of SOME field elements: all the arithmetic needs
        base = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        base[:, 3] >>= 11
        arena = HipMem(32 * n * (kmax + lmax))
        for k in range(kmax):  # members that differ: member k is the base rotated by k elements
            arena.upload(np.roll(base, k, axis=0), 32 * n * k)
        members = [arena.ptr + 32 * n * k for k in range(kmax)]
        lc_out = [arena.ptr + 32 * n * (kmax + j) for j in range(lmax)]
        a_k = synthetic.random_fr_integers(kmax, 0xC0)  # canonical integers read as Montgomery words: field elements all the same
        zs = synthetic.random_fr_integers(2, 0xC2)
        for s in here:
            combos, reps = s["combos"], reps_for(lg)
            pairs = {}  # (member, point) -> row of the one call
            for ks, q in combos:
                for k in ks:
                    pairs.setdefault((k, q), len(pairs))
            order = sorted(pairs, key=pairs.get)
            e_ptrs, e_lens, e_points = [members[k] for k, _ in order], [n] * len(order), np.stack([zs[q] for _, q in order])
            got, keep = {}, []  # keep: every array a deferred value is delivered into stays alive until its scope has ended

            def divide(rem, src, q):
                _lib.check(L.snarkvm_hip_fr_divide_by_linear(None, ctypes.c_void_p(rem.ctypes.data), ctypes.c_void_p(src), ctypes.c_size_t(n),
                                                             ctypes.c_void_p(zs[q].ctypes.data), 1))

            def new():
                got["new"] = plugin.fr_evaluate_device(e_ptrs, e_lens, e_points)
                keep.append(got["new"])

            def route_a():
                got["a"] = [plugin.fr_open_fold_device(None, n, [members[k] for k in ks], [n] * len(ks), a_k[ks], zs[q]) for ks, q in combos]
                keep.append(got["a"])

            def route_b():
                got["b"] = [np.zeros((1, 4), dtype=np.uint64) for _ in combos]
                keep.append(got["b"])
                for j, (ks, q) in enumerate(combos):
                    plugin.fr_lincomb_device(lc_out[j], n, [members[k] for k in ks], [n] * len(ks), a_k[ks])
                    divide(got["b"][j], lc_out[j], q)

            def route_c():
                got["c"] = np.zeros((len(order), 4), dtype=np.uint64)
                keep.append(got["c"])
                for row, (k, q) in enumerate(order):
                    divide(got["c"][row : row + 1], members[k], q)

            def combine(values):
                out = []
                for ks, q in combos:
                    acc = None
                    for k in ks:
                        acc = sonic_pc._fr_add(acc, sonic_pc._fr_mul(a_k[k], values[pairs[(k, q)]]))
                    out.append(acc)
                return out

            def region(fn, reps=reps):
                _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(arena.ptr)))
                t0 = time.perf_counter()
                try:
                    for _ in range(reps):
                        fn()
                finally:
                    _lib.check(L.snarkvm_hip_scope_end())
                us = (time.perf_counter() - t0) * 1e6 / reps
                keep.clear()
                return us

            name = f"{s['kind']} {s['param']} n=2^{lg}"
            region(new, 1), region(route_a, 1)
            t0 = time.perf_counter()
            by_new = combine(got["new"])
            host_combine_us = (time.perf_counter() - t0) * 1e6
            if any(x.tobytes() != y.reshape(4).tobytes() for x, y in zip(by_new, got["a"])):
                raise SystemExit(f"bench_fr_evaluate: {name}: new and (a) disagree")
            if variant_shapes_only:
                for _ in range(2):
                    region(new)
                tn = [region(new) for _ in range(runs)]
                results.append({"shape": name, "new_us": round(statistics.median(tn), 2), "new_min_us": round(min(tn), 2)})
                print(json.dumps(results[-1]), flush=True)
                continue
            region(route_b, 1), region(route_c, 1)
            if any(x.tobytes() != y.reshape(4).tobytes() for x, y in zip(by_new, got["b"])) or got["c"].tobytes() != got["new"].tobytes():
                raise SystemExit(f"bench_fr_evaluate: {name}: (b) or (c) disagrees with new")
            for _ in range(2):
                region(route_a), region(new), region(route_b), region(route_c)
            L.snarkvm_hip_alloc_stats(None, 1)
            ta1, tn, tb, tc, ta2 = [], [], [], [], []
            for _ in range(runs):
                ta1.append(region(route_a)), tn.append(region(new)), tb.append(region(route_b)), tc.append(region(route_c)), ta2.append(region(route_a))
            stats = np.zeros(5, dtype=np.uint64)
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
            if stats[:4].any():
                raise SystemExit(f"bench_fr_evaluate: workspace grew inside the timed regions: {stats.tolist()}")
            med = statistics.median
            new_us, a_us, b_us, c_us = med(tn), med(ta1 + ta2), med(tb), med(tc)
            spread = abs(med(ta1) - med(ta2))
            p = {"shape": name, "kind": s["kind"], "param": s["param"], "lg_n": lg, "members": s["members"], "combinations": len(combos), "pairs": len(order),
                 "new_us": round(new_us, 2), "new_min_us": round(min(tn), 2), "a_us": round(a_us, 2), "a_spread_us": round(spread, 2), "b_us": round(b_us, 2),
                 "c_us": round(c_us, 2), "a_over_new": round(a_us / new_us, 3), "b_over_new": round(b_us / new_us, 3), "c_over_new": round(c_us / new_us, 3),
                 "host_combine_us": round(host_combine_us, 1), "lost_to_a": bool(new_us > a_us + spread), "runs": runs, "reps_per_region": reps}
            if lg >= 20:
                p["share_of_8TBs"] = round(32 * n * len(order) / (new_us * 1e-6) / 8e12, 3)
            results.append(p)
            print(json.dumps(p), flush=True)
        arena.free()
    return {"G": int(geo[3]), "pow": int(geo[6]), "members_per_launch": int(geo[4]), "points_per_launch": int(geo[5]), "points": results}


def markdown(points):
    rows = ["| shape | pairs | new us | (a) us | (a) spread us | (b) us | (c) us | (a) / new | (b) / new | (c) / new | share of 8 TB/s | |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for p in points:
        rows.append(f"| {p['shape']} | {p['pairs']} | {p['new_us']} | {p['a_us']} | {p['a_spread_us']} | {p['b_us']} | {p['c_us']} | {p['a_over_new']} | {p['b_over_new']} | "
                    f"{p['c_over_new']} | {p.get('share_of_8TBs', '')} | {'LOST' if p['lost_to_a'] else ''} |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_evaluate.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.runs < 10:
        raise SystemExit("bench_fr_evaluate: at least 10 runs per point")
    if args.child:
        print("RESULT " + json.dumps(measure(args.runs, variant_shapes_only=True)))
        return
    variants = {}
    for spec in args.variant:  # before this process opens the GPU
        name, path = spec.split("=", 1)
        env = dict(os.environ, SNARKVM_HIP_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode:
            raise SystemExit(f"bench_fr_evaluate: the {name} child failed with status {r.returncode}\n{r.stdout}\n{r.stderr}")
        variants[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    res = {"tool": "tools/bench_fr_evaluate.py",
           "what": "one snarkvm_hip_fr_evaluate vs (a) fr_open_fold without a quotient per combination, (b) fr_lincomb + fr_divide_by_linear without a quotient per "
                   "combination, (c) fr_divide_by_linear without a quotient per (polynomial, point); device memory, inside a scope, host wall clock around scope_begin .. "
                   "reps_per_region repetitions .. scope_end, microseconds per repetition, median of `runs` rounds of (a), new, (b), (c), (a); a_spread_us = |median of the "
                   "first (a) series - median of the second|; lost_to_a = new_us > a_us + a_spread_us; host_combine_us (Python integers, once) is not part of new_us or c_us"}
    res.update(measure(args.runs))
    res["lost_to_a"] = [p["shape"] for p in res["points"] if p["lost_to_a"]]
    if variants:
        committed = {p["shape"]: p["new_us"] for p in res["points"] if p["kind"] in ("single", "gamma")}
        res["variants"] = {"committed": {"G": res["G"], "pow": res["pow"], "new_us": committed}}
        for name, v in variants.items():
            res["variants"][name] = {"G": v["G"], "pow": v["pow"], "new_us": {p["shape"]: p["new_us"] for p in v["points"]}}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    print(markdown(res["points"]))  # the table of profiles/fr_evaluate.md


if __name__ == "__main__":
    main()
