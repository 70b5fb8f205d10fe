#!/usr/bin/env python3
"""What computing the arithmetization of a circuit where it will live is worth against shipping a host-side one across.

    arithmetize:    snarkvm_hip_fr_arithmetize(on_device = 1) on a resident CSR matrix, all four outputs and the three a registration keeps.  Device
                    time: two events on the scope's stream around `--launches` (>= 20) enqueued calls (each builds its tables), after a warm-up; the
                    median over `--runs` such regions, divided by the launches.
    register_csr:   snarkvm_hip_fr_arith_register_csr: host wall clock around the call (allocation of the replica, the upload of the CSR arrays, the
                    tables, the pass, the wait); the handle is freed outside the clock.  Median over `--runs`.
    (a) register:   snarkvm_hip_fr_arith_register of three FINISHED host arrays, the same clock: the transfer every host-side arithmetization pays at
                    the least - the host's own work is left out entirely.
    (b) as before:  matrices.matrix_evals (Python big ints; ONCE, it takes seconds) plus (a): what the parent commit does.

Shapes: |K| = 2^17 (credits.aleo/transfer_private: 51 002 constraints, 2^16 variables, 111 472 entries) and the same row
distribution scaled by eight to |K| = 2^20.  The matrices come from synthetic.r1cs_like_matrix - an ASSUMED row-length distribution, see its docstring.
The device results are compared with matrix_evals's arrays before anything is timed.

`--variant NAME=PATH` (repeatable) also times the device calls on another build of the library in a child process - csrc/poly.hip.h built with
-DFR_ARITH_FULL_TABLE=1 (w_C^x gathered from one |V|-element table, no product) or -DFR_ARITH_ROW_INDEX=1 (a host-expanded uint32 row per entry
instead of the binary search) - checks that its bytes equal this build's, and records its times beside this build's.  A variant is built with
`python -m snarkvm_amd.build -DFR_ARITH_FULL_TABLE=1 --out=snarkvm_amd/lib/variants/libsnarkvm_hip_arith_fulltable.so`.

    python tools/bench_fr_arithmetize.py [--runs 11] [--launches 20] [--variant NAME=PATH ...] [--out profiles/fr_arithmetize.json]
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

# lg |K|: (constraints, lg of the constraint domain, lg of the variable domain, entries, lg of the input domain)
SHAPES = {17: (51002, 16, 16, 111472, 8), 20: (8 * 51002, 19, 19, 8 * 111472, 8)}


def measure(runs, launches, with_host_side):
    import numpy as np
    import torch

    from snarkvm_amd import _lib, matrices, plugin, synthetic
    from snarkvm_amd.devmem import HipMem
    from snarkvm_amd.matrices import SparseMatrix

    L = _lib.lib()
    points = []
    for lg_k, (constraints, lg_r, lg_c, nnz, lg_x) in SHAPES.items():
        k = 1 << lg_k
        m = SparseMatrix(constraints, 1 << lg_c, *synthetic.r1cs_like_matrix(constraints, 1 << lg_c, nnz, 0x7A))
        # row_ptr | the row of every entry (read by the FR_ARITH_ROW_INDEX variant alone) | col_idx | vals, each part 32-byte aligned
        row_of = np.repeat(np.arange(m.rows, dtype=np.uint32), m.row_lengths())
        at_col = (8 * (m.rows + 1) + 4 * m.nnz + 31) & ~31
        at_val = (at_col + 4 * m.nnz + 31) & ~31
        csr = HipMem(at_val + 32 * m.nnz)
        csr.upload(m.row_ptr), csr.upload(row_of, 8 * (m.rows + 1)), csr.upload(m.col_idx, at_col), csr.upload(m.vals, at_val)
        out = HipMem(32 * 4 * k)
        ptrs = [out.ptr + 32 * k * j for j in range(4)]
        tail = (k, m.rows, csr.ptr, csr.ptr + at_col, csr.ptr + at_val, lg_r, lg_c, lg_x)
        plugin.fr_arithmetize_device(*ptrs, *tail)
        got = out.download(dtype=np.uint64).reshape(4, k, 4)
        row = {"lg_k": lg_k, "rows": m.rows, "nnz": m.nnz, "lg_constraint": lg_r, "lg_variable": lg_c, "lg_input": lg_x, "launches": launches, "runs": runs,
               "sha256": hashlib.sha256(got.tobytes()).hexdigest()}
        host_arrays = (got[0].copy(), got[1].copy(), got[3].copy())
        if with_host_side:
            t0 = time.perf_counter()
            want = matrices.matrix_evals(m, k, 1 << lg_c, 1 << lg_x, 1 << lg_r)
            row["matrix_evals_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            if not all(np.array_equal(x, y) for x, y in zip(want, host_arrays)):
                raise SystemExit("bench_fr_arithmetize: the device arithmetization differs from matrices.matrix_evals")
            host_arrays = want

        def region(outs):
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(out.ptr)))
            try:
                stream = torch.cuda.ExternalStream(L.snarkvm_hip_scope_stream())
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(launches):
                    plugin.fr_arithmetize_device(*outs, *tail)
                e1.record(stream)
            finally:
                _lib.check(L.snarkvm_hip_scope_end())
            e1.synchronize()
            return e0.elapsed_time(e1) / launches

        for name, outs in (("arithmetize_4_outputs", ptrs), ("arithmetize_3_outputs", [ptrs[0], ptrs[1], None, ptrs[3]])):
            region(outs)
            L.snarkvm_hip_alloc_stats(None, 1)
            ts = [region(outs) for _ in range(runs)]
            stats = np.zeros(5, dtype=np.uint64)
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
            if stats[:4].any():
                raise SystemExit(f"bench_fr_arithmetize: workspace grew inside the timed regions: {stats.tolist()}")
            row[name] = {"device_us": round(statistics.median(ts) * 1e3, 2), "device_min_us": round(min(ts) * 1e3, 2)}

        def wall(make):
            t0 = time.perf_counter()
            reg = make()
            dt = (time.perf_counter() - t0) * 1e3
            reg.close()
            return dt

        def timed(make):
            wall(make)
            ts = [wall(make) for _ in range(runs)]
            return {"wall_ms": round(statistics.median(ts), 3), "wall_min_ms": round(min(ts), 3)}

        row["register_csr"] = timed(lambda: matrices.RegisteredArithmetization.from_csr(m, k, lg_r, lg_c, lg_x))
        row["register_host_arrays"] = timed(lambda: matrices.RegisteredArithmetization(*host_arrays))
        row["host_arrays_bytes"], row["csr_bytes"] = 3 * 32 * k, 8 * (m.rows + 1) + 36 * m.nnz
        if with_host_side:
            row["as_the_parent_commit_ms"] = round(row["matrix_evals_ms"] + row["register_host_arrays"]["wall_ms"], 1)
        points.append(row)
        print(json.dumps(row), flush=True)
        csr.free(), out.free()
    geo = np.zeros(4, dtype=np.uint32)
    assert L.snarkvm_hip_selftest_fr_arithmetize_geometry(1 << 20, 19, geo.ctypes.data) == 0
    return {"box": {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__},
            "geometry_at_2^20": dict(zip(("workgroups", "threads", "cap", "split_bits_of_2^19"), (int(x) for x in geo))), "points": points}


def markdown(res):
    def line(p, key, sub):
        return p[key][sub]

    out = ["# snarkvm_hip_fr_arithmetize / snarkvm_hip_fr_arith_register_csr", "",
           f"Tool: `{res['tool']}`.  Box: {res['box']['device']}, HIP {res['box']['hip']}, torch {res['box']['torch']}.", "", res["what"], "",
           "| lg K | rows | entries | arithmetize, 4 outputs (us) | 3 outputs (us) | register_csr (ms) | (a) register of host arrays (ms) | matrix_evals (ms) | (b) as the parent commit (ms) |",
           "|---|---|---|---|---|---|---|---|---|"]
    for p in res["points"]:
        out.append(f"| {p['lg_k']} | {p['rows']} | {p['nnz']} | {line(p, 'arithmetize_4_outputs', 'device_us')} | {line(p, 'arithmetize_3_outputs', 'device_us')} | "
                   f"{line(p, 'register_csr', 'wall_ms')} | {line(p, 'register_host_arrays', 'wall_ms')} | {p.get('matrix_evals_ms', 'not measured')} | "
                   f"{p.get('as_the_parent_commit_ms', 'not measured')} |")
    out += ["", "Device times: medians over the regions, per call, tables included.  Wall times: medians, the handle freed outside the clock.", ""]
    if res.get("variants"):
        out += ["## Kernel variants (device time per call, us; the bytes of every variant equal the committed build's)", "",
                "| build | " + " | ".join(f"2^{p['lg_k']}, 4 outputs | 2^{p['lg_k']}, 3 outputs" for p in res["points"]) + " |", "|---|" + "---|" * (2 * len(res["points"]))]
        for name, v in res["variants"].items():
            out.append(f"| {name} | " + " | ".join(f"{v[str(p['lg_k'])]['arithmetize_4_outputs']} | {v[str(p['lg_k'])]['arithmetize_3_outputs']}" for p in res["points"]) + " |")
        out += ["", res.get("verdict", ""), ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_arithmetize.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20 or args.runs < 5:
        raise SystemExit("bench_fr_arithmetize: at least 20 launches per region and 5 regions")
    if args.child:
        print("RESULT " + json.dumps(measure(args.runs, args.launches, False)))
        return
    variants = {}
    for spec in args.variant:  # before this process opens the GPU
        name, path = spec.split("=", 1)
        env = dict(os.environ, SNARKVM_HIP_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--launches", str(args.launches)], env=env,
                           capture_output=True, text=True, timeout=300)
        if r.returncode:
            raise SystemExit(f"bench_fr_arithmetize: the {name} child failed with status {r.returncode}\n{r.stdout}\n{r.stderr}")
        variants[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    res = {"tool": "tools/bench_fr_arithmetize.py",
           "what": "snarkvm_hip_fr_arithmetize on a resident CSR matrix (events around the enqueued calls, per call) and snarkvm_hip_fr_arith_register_csr (host wall "
                   "clock) vs snarkvm_hip_fr_arith_register of three finished host arrays (the same clock; the host's arithmetization is NOT counted) and vs "
                   "matrices.matrix_evals plus that registration (matrix_evals once); medians; matrices from synthetic.r1cs_like_matrix (an assumed distribution)"}
    res.update(measure(args.runs, args.launches, True))
    if variants:
        times = lambda points: {str(p["lg_k"]): {key: p[key]["device_us"] for key in ("arithmetize_4_outputs", "arithmetize_3_outputs")} for p in points}  # noqa: E731
        res["variants"] = {"committed": times(res["points"])}
        for name, v in variants.items():
            for p, q in zip(res["points"], v["points"]):
                if p["sha256"] != q["sha256"]:
                    raise SystemExit(f"bench_fr_arithmetize: the {name} build computes other bytes at 2^{p['lg_k']}")
            res["variants"][name] = times(v["points"])
        base, notes = res["variants"]["committed"], []
        for name in variants:
            ratios = {lg: round(res["variants"][name][lg]["arithmetize_4_outputs"] / base[lg]["arithmetize_4_outputs"], 3) for lg in base}
            wins = [lg for lg, r in ratios.items() if r < 1]
            notes.append(f"{name}: " + ", ".join(f"{r}x the committed time at 2^{lg}" for lg, r in ratios.items()) + " - "
                         + ("faster at every size" if len(wins) == len(ratios) else "not faster at every size: not kept" if wins else "slower or equal at every size: not kept"))
        res["verdict"] = "; ".join(notes) + "."
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
        f.write(markdown(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
