#!/usr/bin/env python3
"""What round 1 in lock step (`matrices.first_round_device`: one gather, one inverse transform and one division per instance, three strided sparse
products per circuit, everything enqueued in one scope) is worth against the per-instance chain it replaces, which stays in the tree - and what the
gather `snarkvm_hip_fr_assignment_evals` costs alone.

    lock:       matrices.first_round_device over ONE circuit of I instances whose rows (padded public input ++ private variables) live in a device
                arena: one block allocated, 3 + ceil(I / 48) + 3 calls enqueued in a scope of its own, ONE host wait, nothing read back
    chain:      per instance, from the same arena:
                    the public input copied out and interpolated at |X| (ntt_device_batch inverse: x_poly, prover/state.rs:150)
                    matrices.witness_poly_device   (allocates |V| + |X|, forward transform, gather, inverse transform, division, fr_support, ONE wait)
                    matrices.assignment_device     (fr_mul_by_vanishing, fr_lincomb)
                    matrices.z_m x 3               (HOST arrays, as the function is: concatenation on the host, one upload and one download each)
    chain_dev:  the same with RegisteredMatrix.mul_device on the arena's row in z_m's place (no host array anywhere) - what a caller that kept its
                variables resident would have written before the lock-step route
    block:      the allocation and release of the one output block of the lock-step route, alone (inside `lock` the allocation is timed, the
                release is not: the outputs die after the clock has stopped)

Shapes: (|V|, |X|) = (2^14, 2^4) and (2^16, 2^4), |R| = |V|, I in {1, 4, 16}.  The public-input size of the credits circuits is not in the tree:
|X| = 2^4 is ASSUMED.  Matrices: synthetic.r1cs_like_matrix (an ASSUMED row-length distribution, see its docstring), |R| - 3 rows over |V| - 5
variables with two entries per row on average.  The three routes must give identical bytes for z, w, x_poly, z_a, z_b and z_c: checked before
anything is timed.  Clock: the chain waits on the host inside every instance, so all three legs are timed by the wall clock around the whole round
(outputs of the chain preallocated, those of the lock-step route allocated inside the timed call as the driver does); the legs alternate in one
process, median over `--runs` (>= 5) after two warm-up rounds.

The steps of the lock-step route alone at |V| = 2^16 with 16 instances (the gather, the inverse transforms, the division at |X| = 2^4 and at 2^10, the
three strided products): device time between two events, as below.

The gather alone: one member of 2^24 elements (|X| = 2^4, a full private part) against `snarkvm_hip_fr_witness_evals` at the same n, both on device
memory; two events on the scope's stream around `--launches` (>= 20) enqueued repetitions, median over `--runs` regions, the legs alternating.
Bytes moved per element: 32 read + 32 written by the assignment gather, 64 read + 32 written by the witness gather.

    python tools/bench_fr_first_round.py [--runs 11] [--launches 20] [--out profiles/fr_first_round.json]
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

# (lg |V|, lg |X|, instances)
SHAPES = tuple((lg_v, 4, inst) for lg_v in (14, 16) for inst in (1, 4, 16))
GATHER_LG = 24


def rounds(runs):
    import numpy as np

    from snarkvm_amd import matrices, plugin, synthetic
    from snarkvm_amd.devmem import HipMem
    from snarkvm_amd.matrices import FirstRoundCircuit, RegisteredMatrix, SparseMatrix

    points, regs_by_lg = [], {}
    for lg_v, lg_x, inst in SHAPES:
        V, X = 1 << lg_v, 1 << lg_x
        R, rows, num_vars = V, V - 3, V - 5
        if lg_v not in regs_by_lg:
            regs_by_lg[lg_v] = [RegisteredMatrix(SparseMatrix(rows, num_vars, *synthetic.r1cs_like_matrix(rows, num_vars, 2 * rows, 0xF1 + 16 * lg_v + j))) for j in range(3)]
        regs = regs_by_lg[lg_v]
        stride = num_vars + 5
        host_rows = [synthetic.random_fr_integers(num_vars, 0xB0 + 64 * lg_v + i) for i in range(inst)]  # canonical integers below r taken as memory-form elements
        arena = HipMem(32 * stride * inst)
        for i, row in enumerate(host_rows):
            arena.upload(row, 32 * stride * i)
        circuit = FirstRoundCircuit(regs, lg_v, lg_v, lg_x, arena, num_vars, stride, inst)
        # the chain's outputs, allocated once: per instance x_poly (X) | w (V - X) | z (V) | z_a, z_b, z_c (3 R)
        per = X + (V - X) + V + 3 * R
        work = HipMem(32 * per * inst)
        at = lambda i, off: work.ptr + 32 * (per * i + off)
        host_zm = {}

        def lock():
            return matrices.first_round_device([circuit])[0]

        def chain(device_products):
            for i in range(inst):
                d_x, d_w, d_z = at(i, 0), at(i, X), at(i, V)
                work.copy_from(32 * per * i, arena.ptr + 32 * stride * i, 32 * X)
                plugin.NTT_device_batch(lg_x, [d_x], directions=[1], types=[0])
                matrices.witness_poly_device(arena.ptr + 32 * (stride * i + X), num_vars - X, d_x, X, lg_v, d_w)
                matrices.assignment_device(d_w, V - X, d_x, X, d_z)
                for j, reg in enumerate(regs):
                    if device_products:
                        reg.mul_device(at(i, 2 * V + R * j), R, arena.ptr + 32 * stride * i)
                    else:
                        host_zm[(i, j)] = matrices.z_m(reg, host_rows[i][:X], host_rows[i][X:], R)

        got = lock()
        for device_products in (False, True):
            work.fill(0, 0xA5, 32 * per * inst)
            chain(device_products)
            for i in range(inst):
                block = work.download(32 * per, 32 * per * i, dtype=np.uint64).reshape(-1, 4)
                same = (np.array_equal(got.x_poly[i].download(), block[:X]) and np.array_equal(got.w[i].download(), block[X:V])
                        and np.array_equal(got.z[i].download(), block[V : 2 * V]))
                for j in range(3):
                    want = block[2 * V + R * j : 2 * V + R * (j + 1)] if device_products else host_zm[(i, j)]
                    same = same and np.array_equal(got.z_m[i][j].download(), want)
                if not same:
                    raise SystemExit(f"bench_fr_first_round: the lock-step route and the chain differ at |V| = 2^{lg_v}, instance {i} of {inst}")
        del got
        def block():  # the one block of device memory the lock-step route allocates per circuit, allocated and released alone
            HipMem(32 * inst * (2 * V + 3 * R)).free()

        legs = [("lock", lock), ("chain", lambda: chain(False)), ("chain_dev", lambda: chain(True)), ("block", block)]
        for _ in range(2):
            for _, fn in legs:
                fn()
        times = {name: [] for name, _ in legs}
        for _ in range(runs):  # the legs alternate: drift of the machine hits all alike
            for name, fn in legs:
                t0 = time.perf_counter()
                keep = fn()  # the lock-step outputs die after the clock has stopped
                times[name].append((time.perf_counter() - t0) * 1e6)
                del keep
        row = {"lg_v": lg_v, "lg_x": lg_x, "lg_x_is": "ASSUMED", "lg_r": lg_v, "instances": inst, "runs": runs, "clock": "wall clock around the whole round",
               "checked_equal": True, "transforms": {"lock": f"{inst} at |V|", "chain": f"{2 * inst} at |V| + {inst} at |X|"},
               "host_waits": {"lock": 1, "chain": "at least 3 per instance", "chain_dev": "at least 3 per instance"}}
        for name, _ in legs:
            ts = times[name]
            row[name] = {"median_us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}
        row["block"]["what"] = "allocation and release of the lock-step route's output block alone (the release is outside `lock`'s clock)"
        row["chain_over_lock"] = round(row["chain"]["median_us"] / row["lock"]["median_us"], 2)
        row["chain_dev_over_lock"] = round(row["chain_dev"]["median_us"] / row["lock"]["median_us"], 2)
        points.append(row)
        print(json.dumps(row), flush=True)
        arena.free(), work.free()
    for regs in regs_by_lg.values():
        for r in regs:
            r.close()
    return points


def gather(runs, launches):
    import numpy as np
    import torch

    from snarkvm_amd import _lib, plugin, synthetic
    from snarkvm_amd.devmem import HipMem

    L = _lib.lib()
    n, X = 1 << GATHER_LG, 1 << 4
    geometry = np.zeros(3, dtype=np.uint32)
    L.snarkvm_hip_selftest_fr_assignment_geometry(n, geometry.ctypes.data)
    d_vars, d_x, d_out = HipMem.from_numpy(synthetic.random_fr_integers(n, 0xC1)), HipMem.from_numpy(synthetic.random_fr_integers(n, 0xC2)), HipMem(32 * n)

    def assignment():
        plugin.fr_assignment_evals_device(d_out.ptr, n, d_vars.ptr, n, X)

    def witness():  # the private part of the same row as w, the other vector as x_evals
        plugin.fr_witness_evals_device(d_out.ptr, n, d_vars.ptr + 32 * X, n - X, d_x.ptr, X)

    def region(enqueue):
        _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(d_out.ptr)))
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

    legs = [("assignment_evals", assignment, 64), ("witness_evals", witness, 96)]
    for _, fn, _ in legs:
        region(fn)
    times = {name: [] for name, _, _ in legs}
    for _ in range(runs):
        for name, fn, _ in legs:
            times[name].append(region(fn))
    out = {"n": n, "lg_n": GATHER_LG, "input_size": X, "launches_per_region": launches, "runs": runs, "clock": "events on the scope's stream, per launch",
           "workgroups": int(geometry[0]), "threads_per_workgroup": int(geometry[1]), "device": torch.cuda.get_device_name(0)}
    for name, _, bytes_per_element in legs:
        ts = times[name]
        med = statistics.median(ts)
        out[name] = {"median_us": round(med * 1e3, 2), "min_us": round(min(ts) * 1e3, 2), "max_us": round(max(ts) * 1e3, 2), "bytes_per_element": bytes_per_element,
                     "tb_per_s": round(bytes_per_element * n / (med * 1e-3) / 1e12, 3)}
    print(json.dumps(out), flush=True)
    for m in (d_vars, d_x, d_out):
        m.free()
    return out


def steps(runs, launches, lg_v=16, inst=16):
    """device time of every step of the lock-step route alone at |V| = 2^lg_v, `inst` instances, on one block: events on the scope's stream around
    `launches` enqueued repetitions, median over `runs` regions, the steps alternating.  The division is timed at |X| = 2^4 (the ASSUMED input size)
    and at |X| = 2^10: a thread of fr_fold_vanishing_kernel walks its residue class, |V| / |X| terms at the most."""
    import torch

    from snarkvm_amd import _lib, plugin, synthetic
    from snarkvm_amd.devmem import HipMem
    from snarkvm_amd.matrices import RegisteredMatrix, SparseMatrix

    L = _lib.lib()
    V, X = 1 << lg_v, 1 << 4
    R, rows, num_vars = V, V - 3, V - 5
    regs = [RegisteredMatrix(SparseMatrix(rows, num_vars, *synthetic.r1cs_like_matrix(rows, num_vars, 2 * rows, 0xF1 + 16 * lg_v + j))) for j in range(3)]
    arena = HipMem.from_numpy(synthetic.random_fr_integers(num_vars * inst, 0xD1))
    mem = HipMem(32 * inst * (2 * V + 3 * R))
    d_z, d_w, d_zm = mem.ptr, mem.ptr + 32 * inst * V, mem.ptr + 32 * inst * 2 * V
    ptrs = [d_z + 32 * V * i for i in range(inst)]

    def divide(x):
        return lambda: _lib.check(L.snarkvm_hip_fr_divide_by_vanishing_strided(d_w, d_w + 32 * (V - x), d_z, V, x, inst, V))

    def products():
        for j, m in enumerate(regs):
            m.mul_device(d_zm + 32 * inst * R * j, R, arena, inst, num_vars, R)

    legs = [("assignment_evals", lambda: plugin.fr_assignment_evals_device(d_z, V, arena.ptr, num_vars, X, inst, V, num_vars)),
            ("inverse_transforms", lambda: plugin.NTT_device_batch(lg_v, ptrs, directions=[1] * inst, types=[0] * inst)),
            ("divide_by_vanishing_x16", divide(X)), ("divide_by_vanishing_x1024", divide(1 << 10)), ("three_products", products)]

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
        return e0.elapsed_time(e1) / launches

    for _, fn in legs:
        region(fn)
    times = {name: [] for name, _ in legs}
    for _ in range(runs):
        for name, fn in legs:
            times[name].append(region(fn))
    out = {"lg_v": lg_v, "lg_r": lg_v, "instances": inst, "launches_per_region": launches, "runs": runs, "clock": "events on the scope's stream, per repetition"}
    for name, _ in legs:
        ts = times[name]
        out[name] = {"median_us": round(statistics.median(ts) * 1e3, 2), "min_us": round(min(ts) * 1e3, 2), "max_us": round(max(ts) * 1e3, 2)}
    print(json.dumps(out), flush=True)
    for r in regs:
        r.close()
    arena.free(), mem.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_first_round.json"))
    args = ap.parse_args()
    if args.launches < 20 or args.runs < 5:
        raise SystemExit("bench_fr_first_round: at least 20 launches per region and 5 runs")
    res = {"tool": "tools/bench_fr_first_round.py",
           "what": "matrices.first_round_device (lock step: z, w, x_poly, z_a, z_b, z_c of every instance from one gather, one inverse transform and one division per "
                   "instance and three strided products) vs per instance an inverse transform at |X|, witness_poly_device, assignment_device and three z_m (host "
                   "arrays; chain_dev: mul_device on the resident row), identical bytes, wall clock around the round, medians; and the gather alone at 2^24 "
                   "against fr_witness_evals_kernel, events on the stream.  |X| = 2^4 and the row-length distribution of the matrices are ASSUMED",
           "rounds": rounds(args.runs), "steps": steps(args.runs, args.launches), "gather": gather(args.runs, args.launches)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
