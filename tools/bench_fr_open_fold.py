#!/usr/bin/env python3
"""What snarkvm_hip_fr_open_fold is worth against the chain of calls it replaces, on device memory inside a scope.

    fused:  one snarkvm_hip_fr_open_fold over the K members of a query point, the opening challenges folded into their coefficients on the
            host (not timed: K + L products of Python integers).
    chain:  one snarkvm_hip_fr_lincomb per linear combination (L result vectors), one more that folds the L results with the opening
            challenges, then snarkvm_hip_fr_divide_by_linear: L + 4 launches, L + 1 intermediate vectors.

Shapes (snark/varuna/ahp/ahp.rs:173-389): the gamma point of 1 / 2 / 3 circuits - g_a, g_b, g_c alone and one combination of h_2 with the six
a_poly_* / b_poly_* of every circuit: 10 / 19 / 28 members in 4 / 7 / 10 combinations - at 2^17 and 2^20 coefficients; the beta point of
1 / 4 / 16 instances - one combination of g_1, mask_poly, h_1 and every w_j alone - at 2^16 and 2^18; and the value alone (quotient = NULL)
against snarkvm_hip_fr_divide_by_linear with a NULL quotient: one member with coefficient one, and the 10 members of a gamma point against
one fr_lincomb plus that division.

The quotient (n - 1 coefficients) and the remainder of the two are compared bit for bit at every shape before anything is timed.  A timed
region is scope_begin .. REPS repetitions of the calls .. scope_end (which waits), host wall clock, reported per repetition; every round
times chain, fused, chain in that order, so the two chain series bracket the fused one; medians over `--runs` rounds after a warm-up;
snarkvm_hip_alloc_stats must show that nothing grew.  `spread` is the distance between the medians of the two chain series - what the chain
itself moves by within the session - and a shape counts as LOST when the fused median exceeds the chain's by more than that.

    python tools/bench_fr_open_fold.py [--runs 15] [--out profiles/fr_open_fold.json]

Results: profiles/fr_open_fold.md.  With a quotient the fused call won every shape (1.16 - 2.05x); ONE SHAPE LOSES: the value alone over the 10
members of a gamma point runs at 0.68 of the speed of fr_lincomb + fr_divide_by_linear (no buffer to park the combination in).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 4


def gamma_point(circuits):
    """member indices per combination: g_a, g_b, g_c of every circuit alone, then h_2 with the a_poly_* / b_poly_* of every circuit"""
    lcs = [[k] for k in range(3 * circuits)]
    lcs.append(list(range(3 * circuits, 9 * circuits + 1)))
    return 9 * circuits + 1, lcs


def beta_point(instances):
    """g_1, mask_poly, h_1 in one combination, every w_j alone"""
    return 3 + instances, [[0, 1, 2]] + [[3 + j] for j in range(instances)]


SHAPES = ([("gamma", c, lg) + gamma_point(c) for lg in (17, 20) for c in (1, 2, 3)] + [("beta", i, lg) + beta_point(i) for lg in (16, 18) for i in (1, 4, 16)])
VALUE_ONLY = [("value", 1, 17, 1, [[0]]), ("value", 1, 20, 1, [[0]]), ("value_gamma", 1, 17, 10, [list(range(10))])]


def measure(runs):
    import numpy as np

    from snarkvm_amd import _lib, plugin, sonic_pc, synthetic
    from snarkvm_amd.devmem import HipMem

    L = _lib.lib()
    rng = np.random.default_rng(0xF2)
    results = []
    for lg in sorted({s[2] for s in SHAPES + VALUE_ONLY}):
        n = 1 << lg
        shapes = [s for s in SHAPES + VALUE_ONLY if s[2] == lg]
        kmax = max(s[3] for s in shapes)
        lmax = max(len(s[4]) for s in shapes)
        # canonical values < 2^252 are valid memory words of SOME field elements: all the arithmetic needs
        base = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        base[:, 3] >>= 11
        arena = HipMem(32 * n * (kmax + lmax + 3))
        for k in range(kmax):  # members that differ: member k is the base rotated by k elements
            arena.upload(np.roll(base, k, axis=0), 32 * n * k)
        members = [arena.ptr + 32 * n * k for k in range(kmax)]
        lc_out = [arena.ptr + 32 * n * (kmax + j) for j in range(lmax)]
        comb, q_chain, q_fused = (arena.ptr + 32 * n * (kmax + lmax + j) for j in range(3))
        a = synthetic.random_fr_integers(kmax, 0xC0)  # canonical integers read as Montgomery words: field elements all the same
        xi = synthetic.random_fr_integers(lmax, 0xC1)
        z = synthetic.random_fr_integers(1, 0xC2)
        for kind, param, _, K, lcs in shapes:
            nl = len(lcs)
            value_only = kind.startswith("value")
            if kind == "value":
                a_use, xi_use = sonic_pc.FR_ONE.reshape(1, 4), sonic_pc.FR_ONE.reshape(1, 4)
            else:
                a_use, xi_use = a[:K], (sonic_pc.FR_ONE.reshape(1, 4) if value_only else xi[:nl])
            folded = np.stack([sonic_pc._fr_mul(xi_use[j], a_use[k]) for j, ks in enumerate(lcs) for k in ks])
            order = [k for ks in lcs for k in ks]
            rem_chain, rem_fused = np.zeros((1, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)

            def divide(quot, rem, src):
                _lib.check(L.snarkvm_hip_fr_divide_by_linear(ctypes.c_void_p(quot) if quot else None, ctypes.c_void_p(rem.ctypes.data), ctypes.c_void_p(src),
                                                             ctypes.c_size_t(n), ctypes.c_void_p(z.ctypes.data), 1))

            def chain():
                if kind == "value":  # the plain evaluation of one polynomial
                    divide(None, rem_chain, members[0])
                    return
                for j, ks in enumerate(lcs):
                    plugin.fr_lincomb_device(lc_out[j], n, [members[k] for k in ks], [n] * len(ks), a_use[ks])
                if value_only:  # one combination: nothing to fold
                    divide(None, rem_chain, lc_out[0])
                    return
                plugin.fr_lincomb_device(comb, n, lc_out[:nl], [n] * nl, xi_use)
                divide(q_chain, rem_chain, comb)

            def fused():
                got = plugin.fr_open_fold_device(None if value_only else q_fused, n, [members[k] for k in order], [n] * len(order), folded, z)
                fused.rem = got  # filled when the scope ends

            def region(fn, reps=REPS):
                _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(arena.ptr)))
                t0 = time.perf_counter()
                try:
                    for _ in range(reps):
                        fn()
                finally:
                    _lib.check(L.snarkvm_hip_scope_end())
                return (time.perf_counter() - t0) * 1e3 / reps

            region(chain, 1), region(fused, 1)
            rem_fused = fused.rem
            if not np.array_equal(rem_chain, rem_fused):
                raise SystemExit(f"bench_fr_open_fold: {kind} {param} n=2^{lg}: the remainders disagree")
            if not value_only:
                qa = arena.download(32 * (n - 1), q_chain - arena.ptr)
                qb = arena.download(32 * n, q_fused - arena.ptr)
                if not np.array_equal(qa, qb[: 32 * (n - 1)]) or qb[32 * (n - 1) :].any():
                    raise SystemExit(f"bench_fr_open_fold: {kind} {param} n=2^{lg}: the quotients disagree")
            for _ in range(2):
                region(chain), region(fused)
            L.snarkvm_hip_alloc_stats(None, 1)
            ta, tf, tb = [], [], []
            for _ in range(runs):
                ta.append(region(chain)), tf.append(region(fused)), tb.append(region(chain))
            stats = np.zeros(5, dtype=np.uint64)
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
            if stats[:4].any():
                raise SystemExit(f"bench_fr_open_fold: workspace grew inside the timed regions: {stats.tolist()}")
            chain_ms, fused_ms = statistics.median(ta + tb), statistics.median(tf)
            spread = abs(statistics.median(ta) - statistics.median(tb))
            results.append({"point": kind, "param": param, "lg_n": lg, "members": K, "combinations": nl, "fused_ms": round(fused_ms, 4), "fused_min_ms": round(min(tf), 4),
                            "chain_ms": round(chain_ms, 4), "chain_min_ms": round(min(ta + tb), 4), "chain_spread_ms": round(spread, 4),
                            "chain_over_fused": round(chain_ms / fused_ms, 3), "lost": bool(fused_ms > chain_ms + spread), "runs": runs, "reps_per_region": REPS})
            print(json.dumps(results[-1]), flush=True)
        arena.free()
    return results


def markdown(points):
    rows = ["| point | n | members | combinations | fused ms | chain ms | chain spread ms | chain / fused | |", "|---|---|---|---|---|---|---|---|---|"]
    for p in points:
        rows.append(f"| {p['point']} {p['param']} | 2^{p['lg_n']} | {p['members']} | {p['combinations']} | {p['fused_ms']} | {p['chain_ms']} | {p['chain_spread_ms']} | "
                    f"{p['chain_over_fused']} | {'LOST' if p['lost'] else ''} |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_open_fold.json"))
    args = ap.parse_args()
    if args.runs < 10:
        raise SystemExit("bench_fr_open_fold: at least 10 runs per point")
    points = measure(args.runs)
    res = {"tool": "tools/bench_fr_open_fold.py", "what": "one snarkvm_hip_fr_open_fold vs fr_lincomb per combination + the folding fr_lincomb + fr_divide_by_linear; device memory, "
           f"inside a scope, host wall clock around scope_begin .. {REPS} repetitions .. scope_end, per repetition, median of `runs` rounds of chain, fused, chain; "
           "chain_spread_ms = |median of the first chain series - median of the second|; lost = fused_ms > chain_ms + chain_spread_ms", "points": points,
           "lost": [f"{p['point']} {p['param']} 2^{p['lg_n']}" for p in points if p["lost"]]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    print(markdown(points))  # the table of profiles/fr_open_fold.md


if __name__ == "__main__":
    main()
