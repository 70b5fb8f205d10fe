#!/usr/bin/env python3
"""What the fused round-3 selector fold is worth against the chain of entry points a caller had before it, both on device memory.

    fused:  ONE snarkvm_hip_fr_selector_fold over all members -> h_1, x g_1 and the sums.
    chain:  apply_randomized_selector (ahp/selectors.rs:100-121) and the running sums of third.rs:189-194 from EXISTING entry points, per member
                s = mu p                                  fr_vec_op 4
                (q, r) = s / (X^n - 1)                    fr_divide_by_vanishing
                t = r (X^N - 1)                           fr_mul_by_vanishing
                (q2, r2) = t / (X^n - 1)                  fr_divide_by_vanishing
                r2 == 0 ?                                 fr_support
                h += q, xg += q2                          fr_vec_op 0, twice
            seven launches per member over sums zeroed by two fills; these entry points are identical on the commit before the fused pass.
            (The chain does not produce the per-member sums over the source domain: the fused call's third output is extra work on its side.)

Both are checked for equality (h and xg, bit for bit, every remainder test zero) before anything is timed.  Device time: two events on the
scope's stream around `--launches` (>= 20) enqueued repetitions, after a warm-up region; the median over `--runs` such regions, per repetition,
fused and chain alternating in one process.  Bytes moved are computed from the shapes (elements read or written x 32 B), not measured.
Shapes: |C| = n = 2^16 with members of 2^17 + 2 coefficients (credits.aleo/transfer_private: an assignment of |C| + 3 coefficients), 3 and 24
members, N = n and N = 4 n; and |C| = 2^20.  Operands are random field elements: no pass here depends on the values.

`--variant NAME=PATH` (repeatable) also times the FUSED call on another build of the library in a child process and compares a digest of its
outputs with the committed build's - the bytes must not depend on the variant:
    python -m snarkvm_amd.build -DFR_SELECTOR_G=3 --out=snarkvm_amd/lib/variants/libsnarkvm_hip_sel_g3.so      members per Montgomery reduction (1 .. 6)
    python -m snarkvm_amd.build -DFR_SELECTOR_TILE=0 --out=snarkvm_amd/lib/variants/libsnarkvm_hip_sel_notile.so   every index recomputes its class sum

    python tools/bench_fr_selector.py [--runs 11] [--launches 20] [--variant NAME=PATH ...] [--out profiles/fr_selector.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (lg n, members, N / n)
SHAPES = ((16, 3, 1), (16, 24, 1), (16, 3, 4), (16, 24, 4), (20, 3, 1), (20, 24, 1), (20, 3, 4), (20, 24, 4))
CHAIN_LAUNCHES = 7


def measure(runs, launches, fused_only):
    import numpy as np
    import torch

    from snarkvm_amd import _lib, plugin, synthetic
    from snarkvm_amd.devmem import HipMem

    L = _lib.lib()
    points = []
    for lg, members, ratio in SHAPES:
        n = 1 << lg
        N, length = n * ratio, 2 * n + 2
        h_len = length - n
        # canonical integers below r, taken as memory-form elements: any residues serve
        mus = synthetic.random_fr_integers(members, 0x5E1 + lg)
        ops = HipMem(32 * length * members)
        seedling = synthetic.random_fr_integers(length, 0xC0 + lg)
        for k in range(members):  # distinct device vectors; member k is the first one rotated by k elements
            ops.upload(np.roll(seedling, k, axis=0), 32 * length * k)
        ptrs = [ops.ptr + 32 * length * k for k in range(members)]
        # fused h | xg | sums || chain h | xg | s | q | r | t | q2 | r2
        sizes = [h_len, N, members, h_len, N, length, h_len, n, n + N, N, n]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        mem = HipMem(32 * int(offs[-1]))
        at = lambda j: mem.ptr + 32 * int(offs[j])
        supports = []

        def fused():
            plugin.fr_selector_fold_device(at(0), h_len, at(1), N, at(2), ptrs, [length] * members, [n] * members, mus)

        def chain():  # inside a scope the remainder tests are delivered when the scope ends: `supports` keeps their arrays alive until then
            mem.fill(32 * int(offs[3]), 0, 32 * (h_len + N))
            for k in range(members):
                _lib.check(L.snarkvm_hip_fr_vec_op(4, at(5), ptrs[k], None, None, mus[k : k + 1].ctypes.data, length, 1))
                _lib.check(L.snarkvm_hip_fr_divide_by_vanishing(at(6), at(7), at(5), length, n, 1))
                _lib.check(L.snarkvm_hip_fr_mul_by_vanishing(at(8), at(7), n, N, 1))
                _lib.check(L.snarkvm_hip_fr_divide_by_vanishing(at(9), at(10), at(8), n + N, n, 1))
                supports.append(plugin.fr_support_device(at(10), n))
                _lib.check(L.snarkvm_hip_fr_vec_op(0, at(3), at(3), at(6), None, None, h_len, 1))
                _lib.check(L.snarkvm_hip_fr_vec_op(0, at(4), at(4), at(9), None, None, N, 1))

        fused()
        out = mem.download(32 * (h_len + N + members), 0, dtype=np.uint64)
        digest = hashlib.sha256(out.tobytes()).hexdigest()
        if not fused_only:
            chain()
            got = mem.download(32 * (h_len + N), 32 * int(offs[3]), dtype=np.uint64)
            if not np.array_equal(out[: 4 * (h_len + N)], got) or any(int(s[0]) for s in supports):
                raise SystemExit(f"bench_fr_selector: the fused pass and the chain differ at n = 2^{lg}, {members} members, N = {ratio} n")
            del supports[:]

        def region(enqueue):
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
            if any(int(s[0]) for s in supports):
                raise SystemExit("bench_fr_selector: a remainder of the chain is not zero")
            del supports[:]  # only now: every deferred result has been delivered
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
            raise SystemExit(f"bench_fr_selector: workspace grew inside the timed regions: {stats.tolist()}")
        # elements: fused reads every member once and one period of xg for the tiling, writes h, xg and the sums; the chain per member: scale 2 L,
        # first division 2 L, product n + (n + N), second division 2 (n + N), remainder test n, the two accumulations 3 (L - n) and 3 N; two fills
        fused_elems = members * length + h_len + N + members + (N - n)
        chain_elems = members * (4 * length + 5 * n + 6 * N + 3 * h_len) + h_len + N
        row = {"lg_n": lg, "members": members, "target_over_n": ratio, "member_len": length, "launches_per_region": launches, "runs": runs,
               "checked_equal": not fused_only, "sha256": digest}
        for name, _ in legs:
            ts = times[name]
            row[name] = {"kernel_launches": (-(-members // plugin.FR_SELECTOR_CHUNK)) if name == "fused" else CHAIN_LAUNCHES * members + 2,
                         "bytes_moved": 32 * (fused_elems if name == "fused" else chain_elems),
                         "median_us": round(statistics.median(ts) * 1e3, 2), "min_us": round(min(ts) * 1e3, 2), "max_us": round(max(ts) * 1e3, 2)}
            row[name]["gb_per_s"] = round(row[name]["bytes_moved"] / (row[name]["median_us"] * 1e-6) / 1e9, 1)
        if not fused_only:
            row["chain_over_fused"] = round(row["chain"]["median_us"] / row["fused"]["median_us"], 2)
        points.append(row)
        print(json.dumps(row), flush=True)
        ops.free(), mem.free()
    return {"device": torch.cuda.get_device_name(0), "points": points}


def _key(p):
    return f"n=2^{p['lg_n']} members={p['members']} N={p['target_over_n']}n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_selector.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20 or args.runs < 5:
        raise SystemExit("bench_fr_selector: at least 20 launches per region and 5 regions")
    if args.child:
        print("RESULT " + json.dumps(measure(args.runs, args.launches, True)))
        return
    variants = {}
    # before this process opens the GPU.  With variants the committed build is timed in a child of its own too: fused calls alone, like theirs
    # (next to the chain, in the parent, the small shapes run up to 2x slower)
    for spec in (["committed="] + args.variant) if args.variant else []:
        name, path = spec.split("=", 1)
        env = dict(os.environ, SNARKVM_HIP_LIB=os.path.abspath(path)) if path else dict(os.environ)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--launches", str(args.launches)], env=env,
                           capture_output=True, text=True, timeout=400)
        if r.returncode:
            raise SystemExit(f"bench_fr_selector: the {name} child failed with status {r.returncode}\n{r.stdout}\n{r.stderr}")
        variants[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    res = {"tool": "tools/bench_fr_selector.py",
           "what": "snarkvm_hip_fr_selector_fold (one call) vs per member fr_vec_op 4, fr_divide_by_vanishing, fr_mul_by_vanishing, fr_divide_by_vanishing, "
                   "fr_support and two fr_vec_op 0 producing the same h_1 and x g_1 on device memory; events around the enqueued repetitions, per repetition, "
                   "medians; bytes from shapes"}
    res.update(measure(args.runs, args.launches, False))
    if variants:
        brief = lambda v: {_key(p): {"fused_median_us": p["fused"]["median_us"], "fused_min_us": p["fused"]["min_us"], "sha256": p["sha256"]} for p in v["points"]}
        res["variants"] = {name: brief(v) for name, v in variants.items()}
        mine = brief(res)
        for name, v in res["variants"].items():
            for key, p in v.items():
                if p["sha256"] != mine[key]["sha256"]:
                    raise SystemExit(f"bench_fr_selector: variant {name} gives other bytes than the committed build at {key}")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
