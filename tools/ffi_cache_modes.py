#!/usr/bin/env python3
"""The transfer_private-shaped call list through the reference's three symbols on host buffers (snarkvm_amd/proofs.py::replay_ffi), one
proof at a time, in the three modes of `snarkvm_msm`'s base cache - stateless (off), sampled 16 (SNARKVM_HIP_BASE_CACHE=16) and verified 16
(SNARKVM_HIP_BASE_CACHE=verified) - beside the resident path (device-resident operands, registered SRS, one scope per proof; without the G2
MSM, which the three-symbol rows do not count either).  Prints ONE JSON line: per-proof milliseconds inside the three symbols per row, and
for the verified row the bytes compared and the microseconds callers waited for their comparison per proof (snarkvm_hip_base_cache_stats).
Every row's results are checked against the resident replay.

    python tools/ffi_cache_modes.py [--proofs 16] [--warm 3] [--threads 4]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=16)
    ap.add_argument("--warm", type=int, default=3, help="untimed proofs per row first (a range is registered at its second sighting)")
    ap.add_argument("--threads", type=int, default=4, help="caller threads that issue the commitments of a round")
    args = ap.parse_args()

    import bench
    from snarkvm_amd import plugin, proofs

    salts = list(range(args.proofs))
    keys = proofs.ProverKeys(proofs.ProofShape())
    host = proofs.FfiProofHost(keys, args.threads)
    rows, results = {}, {}
    for name, tables, verified in (("stateless", 0, False), ("sampled_16", 16, False), ("verified_16", 16, True)):
        plugin.set_base_cache(tables, verified)
        for p in salts[: args.warm]:
            proofs.replay_ffi(host, p, None, {})
        plugin.base_cache_stats(reset=True)
        inside, got_all = [], []
        for p in salts:
            t, got = {}, []
            proofs.replay_ffi(host, p, got, t)
            inside.append((t["ntt"] + t["polymul"] + t["msm"]) * 1e3)
            got_all.append(got)
        st = plugin.base_cache_stats()
        n = len(salts)
        s = sorted(inside)
        rows[name] = {"ms_inside_the_three_symbols_per_proof": sum(inside) / n, "median_ms": s[n // 2], "min_ms": s[0], "max_ms": s[-1],
                      "msm_lookups_per_proof": st["lookups"] / n, "hits_per_proof": st["hits"] / n, "mismatches": st["mismatches"]}
        if verified:
            rows[name]["bytes_compared_per_proof"] = st["bytes_compared"] / n
            rows[name]["wait_us_per_proof"] = st["wait_us"] / n
        results[name] = got_all
    plugin.set_base_cache(0)
    host.close()
    keys.close()
    # the resident path without the G2 MSM (the like-for-like row of bench.py --ffi-only)
    keys0 = proofs.ProverKeys(proofs.ProofShape(lg_g2=0), tables=17, window_bits=15)
    dt, lat, got_res, _, _ = bench.proof1_run(keys0, 0, salts, async_msm=True, await_rounds=True, msm_in_stream=True)
    keys0.close()
    ls = sorted(x * 1e3 for x in lat)
    rows["resident"] = {"ms_per_proof": dt / len(salts) * 1e3, "median_ms": ls[len(ls) // 2], "min_ms": ls[0], "max_ms": ls[-1]}
    # checks: every FFI row's 14 G1 results == the resident replay's (the resident row has no G2 result)
    norm = [proofs.normalize_results(r)[:14] for r in got_res]
    for name, got in results.items():
        if [proofs.normalize_results(r)[:14] for r in got] != norm:
            raise SystemExit(f"ffi_cache_modes: row {name}: a result differs from the resident replay")
    v, sa = rows["verified_16"], rows["sampled_16"]
    print(json.dumps({"what": "ms per transfer_private-shaped proof inside snarkvm_ntt / snarkvm_polymul / snarkvm_msm on host buffers, by base-cache mode",
                      "proofs": len(salts), "caller_threads": args.threads, "rows": rows,
                      "verified_over_sampled": v["ms_inside_the_three_symbols_per_proof"] / sa["ms_inside_the_three_symbols_per_proof"],
                      "checks": "every row's 14 G1 results of every proof == the resident replay", "unix_time": int(time.time())}))


if __name__ == "__main__":
    main()
