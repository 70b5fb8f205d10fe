"""The verified mode of `snarkvm_msm`'s opt-in base cache (SNARKVM_HIP_BASE_CACHE=verified / snarkvm_hip_set_base_cache_verified):
every byte of every hit is compared with the host shadow taken at registration, so the result always follows the bytes passed
in, whatever the caller did to its vector in place.  Every scenario runs in a child process of its own (the cache and the
device set are process state) and checks every result against the oracle on the bytes as they are at call time; the cache's
own counters (snarkvm_hip_base_cache_stats) prove that the calls meant to be hits were hits."""
import os
import subprocess
import sys

import pytest

from tests import util

pytestmark = pytest.mark.gpu

PRELUDE = r'''
import ctypes, sys, threading
import numpy as np
sys.path.insert(0, %r)
from oracle import cpu as oracle
from snarkvm_amd import _lib, plugin, synthetic
from tests import util
L = _lib.lib()
stats = plugin.base_cache_stats
def check(b, s):
    got = oracle.g1_to_affine(plugin.msm(b, s))
    assert util.affine_equal(got, oracle.g1_to_affine(oracle.g1_msm(b, s))), "result != oracle"
def delta(s0):
    s1 = stats()
    return {k: s1[k] - s0[k] for k in ("lookups", "hits", "registrations", "mismatches", "bytes_compared")}
gen = util.g1_generator_affine()
''' % util.ROOT


def _run(body, env_extra=None, timeout=900):
    env = dict(os.environ)
    env.pop("SNARKVM_HIP_BASE_CACHE", None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, "-c", PRELUDE + body + '\nprint("SCENARIO_OK")\n'], capture_output=True, text=True, env=env,
                       timeout=timeout, cwd=util.ROOT)
    assert "SCENARIO_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_in_place_change_at_an_unsampled_position_is_caught():
    """The transparency sequence of the sampled mode, in verified mode from the environment; then bases[8191] - a position the
    sampled mode never reads - is changed in place on the SAME array: the next call gives the changed content's result."""
    _run(r'''
assert stats()["tables"] == 4 and stats()["verified"] == 1
n = 20000
bases = oracle.g1_gen_bases(gen, 3, n)
sc = synthetic.random_fr_integers(n, 2468)
check(bases[:9000], sc[:9000])          # first sighting
check(bases[:9000], sc[:9000])          # second sighting: registered
check(bases[:9000], sc[:9000])          # hit
check(bases[100:5100], sc[:5000])       # hit with an offset
check(bases[1:1100], sc[:1099])         # short slice
check(bases, sc)                        # bigger range supersedes the first one
check(bases[4096:12000], sc[:7904])     # sub-slice of a range not registered yet: stateless
check(bases, sc)                        # registered
check(bases[4096:12000], sc[:7904])     # hit
check(bases, sc)                        # hit
s = stats()
assert s["hits"] == 5 and s["registrations"] == 2 and s["mismatches"] == 0, s
bases[8192] = bases[1]
check(bases, sc)                        # caught
check(bases, sc)                        # registered again
check(bases, sc)                        # hit
s0 = stats()
assert s0["mismatches"] == 1 and s0["hits"] == 6 and s0["registrations"] == 3, s0
bases[8191] = bases[2]                  # in place, same array, a position the sampled mode never compares
check(bases, sc)
d = delta(s0)
assert d["mismatches"] == 1 and d["hits"] == 0, d
s1 = stats()
check(bases, sc)                        # second sighting of the changed range: registered from this call's memory
check(bases, sc)
check(bases[37:12345], sc[:12308])
d = delta(s1)
assert d["registrations"] == 1 and d["hits"] == 2 and d["mismatches"] == 0, d
assert d["bytes_compared"] == (n + 12308) * 97, d
''', {"SNARKVM_HIP_BASE_CACHE": "verified:4"})


def test_padding_bytes_are_never_compared():
    _run(r'''
plugin.set_base_cache(16, verified=True)
n = 20000
bases = oracle.g1_gen_bases(gen, 3, n)
sc = synthetic.random_fr_integers(n, 77)
check(bases, sc)
check(bases, sc)
s0 = stats()
raw = bases.view(np.uint8).reshape(n, 104)
raw[::97, 97:104] = 0xA5                # Rust's 7 padding bytes only (may be uninitialised there)
check(bases, sc)
check(bases[500:9000], sc[:8500])
d = delta(s0)
assert d["hits"] == 2 and d["mismatches"] == 0, d
assert d["bytes_compared"] == (n + 8500) * 97, d
''')


def test_whole_content_replaced_at_the_same_address():
    _run(r'''
plugin.set_base_cache(16, verified=True)
n = 20000
bases = oracle.g1_gen_bases(gen, 3, n)
other = oracle.g1_gen_bases(gen, 60001, n)
sc = synthetic.random_fr_integers(n, 99)
addr = bases.ctypes.data
check(bases, sc)
check(bases, sc)
check(bases, sc)
s0 = stats()
assert s0["hits"] == 1 and s0["registrations"] == 1, s0
bases[:] = other
assert bases.ctypes.data == addr
check(bases, sc)
check(bases[3000:7000], sc[:4000])     # the dropped entry is gone: not registered, stateless
d = delta(s0)
assert d["mismatches"] == 1 and d["hits"] == 0, d
''')


def test_change_outside_the_slice_is_not_a_miss_until_a_slice_covers_it():
    _run(r'''
plugin.set_base_cache(16, verified=True)
n = 20000
bases = oracle.g1_gen_bases(gen, 3, n)
sc = synthetic.random_fr_integers(n, 1234)
check(bases, sc)
check(bases, sc)
s0 = stats()
bases[15000] = bases[3]                 # inside the cached range, outside the next slice
check(bases[:9000], sc[:9000])
d = delta(s0)
assert d["hits"] == 1 and d["mismatches"] == 0 and d["bytes_compared"] == 9000 * 97, d
check(bases[10000:16000], sc[:6000])    # covers the changed point
d = delta(s0)
assert d["hits"] == 1 and d["mismatches"] == 1, d
''')


def test_concurrent_callers_a_change_affects_only_its_own_caller():
    """Eight threads call slices of one registered vector at the same moment (the coalescer fuses their tickets); before each
    round one point inside one thread's slice is changed: that thread's result follows the change, the others' are hits."""
    _run(r'''
plugin.set_base_cache(16, verified=True)
T, m = 8, 6000
n = T * m
bases = oracle.g1_gen_bases(gen, 11, n)
sc_all = synthetic.random_fr_integers(n, 4242)
scs = [synthetic.random_fr_integers(m, 500 + t) for t in range(T)]
co = (ctypes.c_uint64 * 4)()
L.snarkvm_hip_coalescer_stats(None, 1)
for rnd in range(5):
    plugin.msm(bases, sc_all)           # (re)register the whole vector: hits, or first + second sighting after a drop
    plugin.msm(bases, sc_all)
    changed = None
    if rnd:
        changed = (rnd * 3) % T
        bases[changed * m + 1000 + rnd] = bases[rnd + 20]
    s0 = stats()
    res = [None] * T
    bar = threading.Barrier(T)
    def run(t):
        bar.wait()
        res[t] = plugin.msm(bases[t * m:(t + 1) * m], scs[t])
    th = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for x in th: x.start()
    for x in th: x.join()
    d = delta(s0)
    for t in range(T):
        want = oracle.g1_to_affine(oracle.g1_msm(bases[t * m:(t + 1) * m], scs[t]))
        assert util.affine_equal(oracle.g1_to_affine(res[t]), want), (rnd, t)
    assert d["mismatches"] == (1 if rnd else 0), (rnd, d)
    if not rnd:
        assert d["hits"] == T, d
L.snarkvm_hip_coalescer_stats(co, 0)
assert co[2] >= 2, "the eight callers were never fused: " + str(list(co))
''')


def test_whole_proofs_through_the_ffi_in_verified_mode():
    """replay_ffi for three salts with the verified cache: all 15 results against the oracle and the resident replay; the
    reference's call counts; every commitment of a warmed-up proof but a few is a hit; nothing mismatches."""
    _run(r'''
from oracle import proof_replay
from snarkvm_amd import kzg10, proofs
from snarkvm_amd.layout import G1_PROJECTIVE, G2_PROJECTIVE
shape = proofs.ProofShape(lg_r=12, lg_k=13, lg_g2=10)
keys = proofs.ProverKeys(shape, seed=31)
host = proofs.FfiProofHost(keys, threads=4)
ref = proofs.ProofWorkspace(keys)
plugin.set_base_cache(16, verified=True)
for i, salt in enumerate((0, 4, 1)):
    s0 = stats()
    got, serial, t = [], [], {}
    proofs.replay_ffi(host, salt, got, t)
    proofs.replay(ref, salt, serial)
    want = proof_replay.expected_results(keys.pool_host, keys.g1_host, keys.g2_host, keys.point, shape.lg_r, shape.lg_k, shape.lg_g2, shape.nmax, salt)
    assert len(got) == 15
    for j in range(14):
        assert util.affine_equal(kzg10.to_affine(np.frombuffer(got[j], dtype=G1_PROJECTIVE)), want[j]), (salt, j)
    assert oracle.g2_to_affine(np.frombuffer(got[14], dtype=G2_PROJECTIVE)).tobytes() == want[14].tobytes(), (salt, "g2")
    assert proofs.normalize_results(got) == proofs.normalize_results(serial), salt
    assert (t["ntt_calls"], t["polymul_calls"], t["msm_calls"]) == (20, 5, 14)
    d = delta(s0)
    assert d["mismatches"] == 0, (salt, d)
    if i:
        assert d["hits"] >= 10, (salt, d)
print("proof stats", stats())
plugin.set_base_cache(0)
host.close()
keys.close()
''', timeout=1200)


def test_two_logical_devices_chunked_hit_and_change():
    """SNARKVM_HIP_DEVICES=0,0: a 2^19-point slice is cut over both logical devices (registered replicas on each); it is a hit,
    and a change inside it is caught."""
    _run(r'''
assert L.snarkvm_hip_num_devices() == 2
n = (1 << 19) + 4096
m = 1 << 19
bases = oracle.g1_gen_bases(gen, 5, n)
sc = synthetic.random_fr_integers(n, 31337)
check(bases, sc)                        # first sighting: stateless
check(bases, sc)                        # registered on both devices
s0 = stats()
check(bases[1000:1000 + m], sc[:m])
d = delta(s0)
assert d["hits"] == 1 and d["mismatches"] == 0 and d["bytes_compared"] == m * 97, d
bases[1000 + 300001] = bases[7]
check(bases[1000:1000 + m], sc[:m])
d = delta(s0)
assert d["hits"] == 1 and d["mismatches"] == 1, d
''', {"SNARKVM_HIP_DEVICES": "0,0", "SNARKVM_HIP_BASE_CACHE": "verified"}, timeout=1200)
