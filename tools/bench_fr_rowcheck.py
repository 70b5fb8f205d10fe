#!/usr/bin/env python3
"""What the fused round-2 route (one coset per domain size, `snarkvm_hip_fr_rowcheck_fold`) is worth against the per-instance chain of entry points
a caller had before it, both on device memory, and what `matrices.witness_poly_device` (round 1) costs.

    fused:  the steps of matrices.rowcheck_witness over I instances of one domain size |R| = n, on buffers allocated once:
                one check-only fr_rowcheck_fold, ntt_device_batch inverse (3 I vectors), ntt_device_batch forward / Coset (3 I vectors),
                one fr_rowcheck_fold into h, ntt_device_batch inverse / Coset (h alone)
    chain:  second.rs:104-122 per instance from entry points that exist on the commit before the fused pass:
                ntt_device_batch inverse (z_a, z_b, z_c)           3 transforms at n
                polymul_device on 2 n (z_a, z_b)                   two forward transforms and one inverse at 2 n
                fr_vec_op sub (the low n coefficients -= z_c)
                fr_divide_by_vanishing by X^n - 1                  quotient n coefficients, remainder n
                fr_vec_op axpy  h += mu q
            over an h zeroed by one fill.  (The chain does not test its remainders; the fused route's check pass is extra work on its side.)

Both routes consume their inputs, so every repetition of either starts with ONE device-to-device copy that restores the 3 I vectors from a pristine
block; that copy is timed alone too (`restore`) and the ratio is given with it (as measured) and net of it; so are the two fr_rowcheck_fold launches
(`check_alone`, `fold_alone`, over the restored vectors).  z_c = z_a z_b element by element, so
the division is exact and both routes must give the same bytes: checked before anything is timed, together with matrices.rowcheck_witness itself.
Device time: two events on the scope's stream around `--launches` (>= 20) enqueued repetitions, after a warm-up region; the median over `--runs`
such regions, per repetition, the legs alternating in one process.  Where the host enqueues more slowly than the device runs (the small shapes) the
figure is the host's enqueue rate - the same for a caller.  witness_poly_device allocates, opens its own scope and waits: wall clock around the
call, median over `--runs`.

`--variant NAME=PATH` (repeatable) also times the FUSED route on another build of the library in a child process and compares a digest of h_0
with the committed build's - the bytes must not depend on the variant:
    python -m snarkvm_amd.build -DFR_ROWCHECK_G=1 --out=snarkvm_amd/lib/variants/libsnarkvm_hip_row_g1.so      members per Montgomery reduction (1 .. 3)

    python tools/bench_fr_rowcheck.py [--runs 11] [--launches 20] [--variant NAME=PATH ...] [--out profiles/fr_rowcheck.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (lg |R|, instances)
SHAPES = tuple((lg, inst) for lg in (12, 16, 18) for inst in (1, 4, 16))
R_MOD = 8444461749428370424248824938781546531375899335154063827935233455917409239041


def measure(runs, launches, fused_only):
    import numpy as np
    import torch

    from snarkvm_amd import _lib, matrices, plugin, synthetic
    from snarkvm_amd.devmem import HipMem

    L = _lib.lib()
    geometry = np.zeros(2, dtype=np.uint32)
    L.snarkvm_hip_selftest_fr_rowcheck_geometry(geometry.ctypes.data)
    points = []
    for lg, inst in SHAPES:
        n = 1 << lg
        combiners = [int(x) for x in np.random.default_rng(lg * 100 + inst).integers(2, 1 << 62, size=inst)]
        g_inv = pow(pow(22, n, R_MOD) - 1, -1, R_MOD)
        mus_chain = matrices._mont_limbs(combiners)
        mus_fused = matrices._mont_limbs([c * g_inv % R_MOD for c in combiners])
        # pristine: per instance z_a | z_b | z_c;  work: the same layout;  then h_fused (n) | h_chain (n) | product (2 n) | quotient (n) | remainder (n)
        pristine, work = HipMem(32 * 3 * n * inst), HipMem(32 * (3 * n * inst + 6 * n))
        for i in range(inst):
            for j in range(2):  # canonical integers below r, taken as memory-form elements: any residues serve
                pristine.upload(synthetic.random_fr_integers(n, 0xA0 + 2 * i + j + lg), 32 * n * (3 * i + j))
            base = pristine.ptr + 32 * n * 3 * i
            _lib.check(L.snarkvm_hip_fr_vec_op(2, base + 64 * n, base, base + 32 * n, None, None, n, 1))
        z = lambda i, j: work.ptr + 32 * n * (3 * i + j)
        tail = work.ptr + 32 * 3 * n * inst
        d_hf, d_hc, d_prod, d_q, d_r = tail, tail + 32 * n, tail + 64 * n, tail + 128 * n, tail + 160 * n
        a, b, c = ([z(i, j) for i in range(inst)] for j in range(3))
        every = a + b + c
        counts = []

        def restore():
            work.copy_from(0, pristine.ptr, 32 * 3 * n * inst)

        def fused():  # inside a scope the counts are delivered when the scope ends: `counts` keeps their arrays alive until then
            restore()
            counts.append(plugin.fr_rowcheck_fold_device(None, n, a, b, c, None))
            plugin.NTT_device_batch(lg, every, directions=[1] * len(every), types=[0] * len(every))
            plugin.NTT_device_batch(lg, every, directions=[0] * len(every), types=[1] * len(every))
            plugin.fr_rowcheck_fold_device(d_hf, n, a, b, c, mus_fused, violations=False)
            plugin.NTT_device_batch(lg, [d_hf], directions=[1], types=[1])

        def chain():
            restore()
            work.fill(32 * (3 * n * inst + n), 0, 32 * n)
            for i in range(inst):
                plugin.NTT_device_batch(lg, [z(i, 0), z(i, 1), z(i, 2)], directions=[1] * 3, types=[0] * 3)
                plugin.polymul_device(lg + 1, d_prod, polys=[(z(i, 0), n), (z(i, 1), n)])
                _lib.check(L.snarkvm_hip_fr_vec_op(1, d_prod, d_prod, z(i, 2), None, None, n, 1))
                _lib.check(L.snarkvm_hip_fr_divide_by_vanishing(d_q, d_r, d_prod, 2 * n, n, 1))
                _lib.check(L.snarkvm_hip_fr_vec_op(6, d_hc, d_hc, d_q, None, mus_chain[i : i + 1].ctypes.data, n, 1))

        fused()
        if any(int(x) for arr in counts for x in arr):
            raise SystemExit("bench_fr_rowcheck: the operands violate a row")
        del counts[:]
        h_fused = work.download(32 * n, 32 * 3 * n * inst, dtype=np.uint64)
        digest = hashlib.sha256(h_fused.tobytes()).hexdigest()
        restore()
        one = matrices._mont_limbs([1])
        driver = matrices.rowcheck_witness([matrices.RowcheckCircuit(lg, one[0], mus_chain, [(z(i, 0), z(i, 1), z(i, 2)) for i in range(inst)])], lg)
        if driver.download().view(np.uint64).tobytes() != h_fused.tobytes():
            raise SystemExit(f"bench_fr_rowcheck: matrices.rowcheck_witness and the steps timed here differ at |R| = 2^{lg}, {inst} instances")
        del driver
        if not fused_only:
            chain()
            if work.download(32 * n, 32 * (3 * n * inst + n), dtype=np.uint64).tobytes() != h_fused.tobytes():
                raise SystemExit(f"bench_fr_rowcheck: the fused route and the chain differ at |R| = 2^{lg}, {inst} instances")

        def region(enqueue):
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(work.ptr)))
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
            if any(int(x) for arr in counts for x in arr):
                raise SystemExit("bench_fr_rowcheck: a violation was counted inside a timed region")
            del counts[:]  # only now: every deferred result has been delivered
            return e0.elapsed_time(e1) / launches

        def check_alone():  # after `restore`: the pristine vectors, no violation, no atomic
            counts.append(plugin.fr_rowcheck_fold_device(None, n, a, b, c, None))

        def fold_alone():
            plugin.fr_rowcheck_fold_device(d_hf, n, a, b, c, mus_fused, violations=False)

        # in this order: the two kernels alone read what `restore` left and write no member
        legs = [("restore", restore), ("check_alone", check_alone), ("fold_alone", fold_alone), ("fused", fused)] + ([] if fused_only else [("chain", chain)])
        for _, fn in legs:
            region(fn)
        L.snarkvm_hip_alloc_stats(None, 1)
        times = {name: [] for name, _ in legs}
        for _ in range(runs):  # the legs alternate: drift of the box hits all alike
            for name, fn in legs:
                times[name].append(region(fn))
        stats = np.zeros(5, dtype=np.uint64)
        L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        if stats[:4].any():
            raise SystemExit(f"bench_fr_rowcheck: workspace grew inside the timed regions: {stats.tolist()}")
        row = {"lg_r": lg, "instances": inst, "launches_per_region": launches, "runs": runs, "checked_equal": not fused_only, "sha256": digest,
               "members_per_launch": int(geometry[0]), "members_per_reduction": int(geometry[1]),
               "transforms": {"fused": f"{6 * inst + 1} at n", "chain": f"{3 * inst} at n + {3 * inst} at 2n"}}
        for name, _ in legs:
            ts = times[name]
            row[name] = {"median_us": round(statistics.median(ts) * 1e3, 2), "min_us": round(min(ts) * 1e3, 2), "max_us": round(max(ts) * 1e3, 2)}
        if not fused_only:
            rest = row["restore"]["median_us"]
            row["chain_over_fused"] = round(row["chain"]["median_us"] / row["fused"]["median_us"], 2)
            row["chain_over_fused_net_of_restore"] = round((row["chain"]["median_us"] - rest) / max(row["fused"]["median_us"] - rest, 1e-3), 2)
        points.append(row)
        print(json.dumps(row), flush=True)
        pristine.free(), work.free()
    res = {"device": torch.cuda.get_device_name(0), "points": points}
    if not fused_only:
        res["witness_poly_device"] = witness_poly(runs)
    return res


def witness_poly(runs, lg_v=16, input_size=1 << 10):
    """wall clock of matrices.witness_poly_device at |V| = 2^lg_v (allocation, five enqueued calls, one wait, the remainder test)"""
    from snarkvm_amd import matrices, synthetic
    from snarkvm_amd.devmem import HipMem

    V = 1 << lg_v
    d_w = HipMem.from_numpy(synthetic.random_fr_integers(V - input_size, 0x71))
    d_x = HipMem.from_numpy(synthetic.random_fr_integers(input_size, 0x72))
    out = HipMem(32 * (V - input_size))
    ts = []
    for k in range(runs + 3):  # three warm-up calls
        t0 = time.perf_counter()
        matrices.witness_poly_device(d_w, V - input_size, d_x, input_size, lg_v, out)
        if k >= 3:
            ts.append((time.perf_counter() - t0) * 1e6)
    return {"lg_v": lg_v, "input_size": input_size, "clock": "wall clock around the call", "runs": runs, "median_us": round(statistics.median(ts), 1),
            "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}


def _key(p):
    return f"R=2^{p['lg_r']} instances={p['instances']}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_rowcheck.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20 or args.runs < 5:
        raise SystemExit("bench_fr_rowcheck: at least 20 launches per region and 5 regions")
    if args.child:
        print("RESULT " + json.dumps(measure(args.runs, args.launches, True)))
        return
    variants = {}
    # before this process opens the GPU.  With variants the committed build is timed in a child of its own too: the fused route alone, like theirs
    for spec in (["committed="] + args.variant) if args.variant else []:
        name, path = spec.split("=", 1)
        env = dict(os.environ, SNARKVM_HIP_LIB=os.path.abspath(path)) if path else dict(os.environ)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--launches", str(args.launches)], env=env,
                           capture_output=True, text=True, timeout=400)
        if r.returncode:
            raise SystemExit(f"bench_fr_rowcheck: the {name} child failed with status {r.returncode}\n{r.stdout}\n{r.stderr}")
        variants[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    res = {"tool": "tools/bench_fr_rowcheck.py",
           "what": "the steps of matrices.rowcheck_witness (check-only fr_rowcheck_fold, inverse and forward-coset ntt_device_batch, fr_rowcheck_fold, one inverse "
                   "coset transform) vs per instance ntt_device_batch inverse, polymul_device on 2|R|, fr_vec_op sub, fr_divide_by_vanishing, fr_vec_op axpy "
                   "producing the same h_0 on device memory; both start with one d2d restore of the inputs (timed alone as `restore`); events around the enqueued "
                   "repetitions, per repetition, medians"}
    res.update(measure(args.runs, args.launches, False))
    if variants:
        brief = lambda v: {_key(p): {"fused_median_us": p["fused"]["median_us"], "fused_min_us": p["fused"]["min_us"], "restore_median_us": p["restore"]["median_us"],
                                     "check_alone_median_us": p["check_alone"]["median_us"], "fold_alone_median_us": p["fold_alone"]["median_us"],
                                     "members_per_reduction": p["members_per_reduction"], "sha256": p["sha256"]} for p in v["points"]}
        res["variants"] = {name: brief(v) for name, v in variants.items()}
        mine = brief(res)
        for name, v in res["variants"].items():
            for key, p in v.items():
                if p["sha256"] != mine[key]["sha256"]:
                    raise SystemExit(f"bench_fr_rowcheck: variant {name} gives other bytes than the committed build at {key}")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
