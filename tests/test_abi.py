"""CPU-only checks of the drop-in boundary: the HIP library builds/loads and exports every symbol declared in
include/snarkvm_hip.h; argument validation that needs no device; the oracle is not reachable from the product."""
import ctypes
import os
import re

import numpy as np
import pytest

from snarkvm_amd import _lib
from tests import util


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(util.ROOT, "include", "snarkvm_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(snarkvm_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name


def _rust_width(t):
    """Width class of a Rust FFI type as written in sys.rs (the twin of tools/gen_bindings.py::width_class on the C side)."""
    t = t.strip()
    depth = 0
    while t.startswith("*"):
        t = re.sub(r"^\*(const|mut)\s+", "", t)
        depth += 1
    if depth:
        return ("ptr", depth)
    if t == "Error":
        return ("err",)
    if t in ("NTTInputOutputOrder", "NTTDirection", "NTTType"):
        return ("int", 4)  # #[repr(C)] enums
    return {"usize": ("int", 8), "i32": ("int", 4), "u32": ("int", 4), "u64": ("int", 8), "f64": ("f64",)}[t]


def test_rust_sys_matches_the_header():
    """rust/snarkvm-algorithms-hip/src/sys.rs against include/snarkvm_hip.h: every declared function present (and nothing else), the same number
    of arguments, the same width class per argument and for the result, pointer depth included; the three #[repr(C)] enums of lib.rs carry the
    header's discriminants; and the committed file is exactly what tools/gen_bindings.py yields today."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_bindings", os.path.join(util.ROOT, "tools", "gen_bindings.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    funcs, consts = gen.parse_header()
    c_side = {f["name"]: f for f in funcs}
    assert set(c_side) == set(_lib.SYMBOLS)  # the header parser sees what the ctypes table lists
    rust_dir = os.path.join(util.ROOT, "rust", "snarkvm-algorithms-hip", "src")
    sys_rs = open(os.path.join(rust_dir, "sys.rs")).read()
    block = sys_rs[sys_rs.index('extern "C" {') :]
    rust_side = {}
    for m in re.finditer(r"pub fn (\w+)\(([^)]*)\)\s*(?:->\s*([^;]+))?;", block):
        args = [a.split(":", 1) for a in m.group(2).split(",") if a.strip()]
        rust_side[m.group(1)] = ([(n.strip(), _rust_width(t)) for n, t in args], _rust_width(m.group(3)) if m.group(3) else ("void",))
    assert set(rust_side) == set(c_side), set(rust_side) ^ set(c_side)
    for name, f in c_side.items():
        r_args, r_ret = rust_side[name]
        assert len(r_args) == len(f["args"]), name
        for (rn, rw), (cn, ct) in zip(r_args, f["args"]):
            assert rw == gen.width_class(ct), (name, cn, rw, ct)
        assert r_ret == gen.width_class(f["ret"]), name
    lib_rs = open(os.path.join(rust_dir, "lib.rs")).read()
    assert "pub mod sys;" in lib_rs and 'extern "C"' not in lib_rs  # no second, hand-written declaration block
    for enum in ("NTTInputOutputOrder", "NTTDirection", "NTTType"):
        body = re.search(r"#\[repr\(C\)\][^{]*pub enum " + enum + r"\s*\{([^}]*)\}", lib_rs).group(1)
        for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", body):
            assert consts[k] == int(v), (enum, k)
    for k in ("SNARKVM_HIP_SCOPE_ASYNC_MSM", "SNARKVM_HIP_SCOPE_STABLE_INPUTS", "SNARKVM_HIP_SCOPE_MSM_IN_STREAM"):
        assert re.search(rf"pub const {k}: u32 = {consts[k]};", sys_rs), k
    # every sys:: item the hand-written wrappers (and INTEGRATION.md's sketches) name is a declared one
    used = set(re.findall(r"sys::(snarkvm_\w+)", lib_rs + open(os.path.join(util.ROOT, "INTEGRATION.md")).read())) - set(gen.OPAQUE)
    assert used and used <= set(c_side), used - set(c_side)
    assert sys_rs == gen.generate(), "sys.rs is stale: run python tools/gen_bindings.py"


def _gen():
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_bindings", os.path.join(util.ROOT, "tools", "gen_bindings.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_python_abi_table_matches_the_header():
    """snarkvm_amd/_abi.py is exactly what tools/gen_bindings.py yields today, and lists the header's functions in the header's order."""
    from snarkvm_amd import _abi

    gen = _gen()
    text = open(os.path.join(util.ROOT, "snarkvm_amd", "_abi.py")).read()
    assert text.startswith("# @generated") and "DO NOT EDIT" in text.splitlines()[0]
    assert text == gen.generate_py(), "_abi.py is stale: run python tools/gen_bindings.py"
    names = [f["name"] for f in gen.parse_header()[0]]
    assert [name for name, _, _ in _abi.FUNCTIONS] == names and _lib.SYMBOLS == names


def _ctypes_class(t):
    """Width class of a ctypes restype / argtypes entry, in the vocabulary of tools/gen_bindings.py::width_class (pointers without a depth)."""
    if t is None:
        return ("void",)
    if t is _lib.RustError:
        return ("err",)
    if t in (ctypes.c_void_p, ctypes.c_char_p):
        return ("ptr",)
    if t is ctypes.c_double:
        return ("f64",)
    assert t in (ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_long, ctypes.c_ulong), t
    return ("int", ctypes.sizeof(t))


def test_every_function_is_bound_as_the_header_declares():
    """The loaded library's functions against include/snarkvm_hip.h (the expectation is computed from the header, not read from _abi.py): argtypes
    of the declared length, every argument and the result in the declared width class; pointer arguments are exactly c_void_p."""
    gen = _gen()
    L = _lib.lib()
    funcs, _ = gen.parse_header()
    assert len(funcs) == len(_lib.SYMBOLS)
    for f in funcs:
        fn = getattr(L, f["name"])
        assert fn.argtypes is not None and len(fn.argtypes) == len(f["args"]), f["name"]
        for t, (an, ct) in zip(fn.argtypes, f["args"]):
            want = gen.width_class(ct)
            if want[0] == "ptr":
                assert t is ctypes.c_void_p, (f["name"], an, t)
            else:
                assert _ctypes_class(t) == want, (f["name"], an, t, want)
        want = gen.width_class(f["ret"])
        assert _ctypes_class(fn.restype) == (("ptr",) if want[0] == "ptr" else want), (f["name"], fn.restype, want)


def test_bare_ints_travel_at_the_declared_width():
    """A bare Python int given to a size_t parameter arrives whole (without argtypes ctypes passes it as a 32-bit C int), and bare ints and
    addresses give what the explicitly wrapped calls of the other tests give."""
    L = _lib.lib()
    big = (1 << 32) + 1
    assert L.snarkvm_hip_batch_lanes(big) == L.snarkvm_hip_batch_lanes(ctypes.c_size_t(big))
    if "SNARKVM_HIP_TUNING" not in os.environ:  # 8 lanes below 2^20 points, 3 from there on: cut to 32 bits, 2^32 + 1 would count as 1
        assert L.snarkvm_hip_batch_lanes(big) == L.snarkvm_hip_batch_lanes(1 << 20) != L.snarkvm_hip_batch_lanes(1)
    for n, wb, tables, tb in ((1 << 16, 0, 1, 0), (1 << 22, 0, 16, 0), (1 << 24, 22, 12, 22), (5000, 15, 17, 15)):
        bare, wrapped = (ctypes.c_uint32 * 10)(), (ctypes.c_uint32 * 10)()
        rc_bare = L.snarkvm_hip_selftest_msm_plan(n, wb, tables, tb, bare)
        rc_wrapped = L.snarkvm_hip_selftest_msm_plan(ctypes.c_size_t(n), ctypes.c_int(wb), ctypes.c_int(tables), ctypes.c_int(tb), wrapped)
        assert rc_bare == rc_wrapped and list(bare) == list(wrapped) and any(bare), (n, wb, tables, tb)
    # the single-polynomial copy of snarkvm_polymul (test_polymul_single_polynomial_longer_than_domain), addresses and counts as bare ints
    p = np.arange(9 * 4, dtype=np.uint64).reshape(9, 4) + 1
    out = np.full((16, 4), 7, dtype=np.uint64)
    pp = (ctypes.c_void_p * 1)(p.ctypes.data)
    for lg, plen in ((3, 9), (0, 2)):
        with pytest.raises(_lib.HipError) as e:
            _lib.check(L.snarkvm_polymul(out.ctypes.data, 1, pp, (ctypes.c_size_t * 1)(plen), 0, None, None, lg))
        assert e.value.code == 1 and (out == 7).all(), lg
    _lib.check(L.snarkvm_polymul(out.ctypes.data, 1, pp, (ctypes.c_size_t * 1)(8), 0, None, None, 3))
    assert np.array_equal(out[:8], p[:8]) and (out[8:] == 7).all()


def test_a_scalar_of_the_wrong_ctypes_class_is_refused():
    """A c_int where size_t is declared raises instead of travelling on (held in a variable: written in the call it would be a finding of
    test_call_sites_match_the_header)."""
    wrong = ctypes.c_int(5)
    with pytest.raises(ctypes.ArgumentError):
        _lib.lib().snarkvm_hip_batch_lanes(wrong)


def test_call_sites_match_the_header():
    """Every `.snarkvm_*(...)` call written in a .py file of the repository (read as text, nothing imported) passes the declared number of
    positional arguments, and every argument written as ctypes.c_X(...) has the class of its parameter: pointer parameters take c_void_p or
    c_char_p, c_size_t / c_uint64 are one class, c_int / c_int32 are one class."""
    import ast

    gen = _gen()
    decl = {f["name"]: [gen.width_class(ct) for _, ct in f["args"]] for f in gen.parse_header()[0]}
    wrappers = {"c_void_p": ("ptr",), "c_char_p": ("ptr",), "c_size_t": ("u", 8), "c_uint64": ("u", 8), "c_int": ("i", 4), "c_int32": ("i", 4),
                "c_uint32": ("u", 4), "c_double": ("f64",)}
    params = {"size_t": ("u", 8), "uint64_t": ("u", 8), "uint32_t": ("u", 4), "int": ("i", 4), "int32_t": ("i", 4), "double": ("f64",)}
    header_args = {f["name"]: f["args"] for f in gen.parse_header()[0]}
    seen, bad = 0, []
    for dirpath, dirnames, files in os.walk(util.ROOT):
        dirnames[:] = [d for d in dirnames if not d.startswith(".") and d not in ("__pycache__", "build")]
        for fname in files:
            if not fname.endswith(".py"):
                continue
            path = os.path.join(dirpath, fname)
            for node in ast.walk(ast.parse(open(path).read(), filename=path)):
                if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in decl):
                    continue
                if any(isinstance(a, ast.Starred) for a in node.args):
                    continue
                seen += 1
                where = (os.path.relpath(path, util.ROOT), node.lineno, node.func.attr)
                if len(node.args) != len(decl[node.func.attr]) or node.keywords:
                    bad.append(where + ("argument count",))
                    continue
                for a, (pname, (base, levels)) in zip(node.args, header_args[node.func.attr]):
                    if isinstance(a, ast.Call) and isinstance(a.func, ast.Attribute) and isinstance(a.func.value, ast.Name) and a.func.value.id == "ctypes" and a.func.attr.startswith("c_"):
                        want = ("ptr",) if levels else ("i", 4) if base in gen.ENUMS else params[base]
                        if wrappers.get(a.func.attr) != want:
                            bad.append(where + (pname, a.func.attr))
    assert not bad, bad
    assert seen >= 500, seen


def test_rust_error_layout():
    # sppark cuda::Error {code: i32, message: *mut c_char}: 16 bytes on x86-64
    assert ctypes.sizeof(_lib.RustError) == 16


def test_polymul_host_only_corner_cases():
    """snarkvm.cu:196-201: no inputs -> no-op success; exactly one polynomial -> plain copy (no device involved)."""
    from snarkvm_amd import plugin

    out = plugin.polymul(8, [], [])
    assert not out.any()
    p = np.arange(12, dtype=np.uint64).reshape(3, 4)
    out = plugin.polymul(8, [p], [])
    assert np.array_equal(out[:3], p) and not out[3:].any()


def test_polymul_single_polynomial_longer_than_domain():
    """`out` holds 2^lg elements: a single polynomial longer than that is rejected, not copied past the end of `out`
    (the caller's buffer here is large enough that an unchecked copy stays inside it and shows up as a change)"""
    p = np.arange(9 * 4, dtype=np.uint64).reshape(9, 4) + 1
    out = np.full((16, 4), 7, dtype=np.uint64)
    pp = (ctypes.c_void_p * 1)(p.ctypes.data)
    for lg, plen in ((3, 9), (0, 2)):
        pl = (ctypes.c_size_t * 1)(plen)
        with pytest.raises(_lib.HipError) as e:
            _lib.check(_lib.lib().snarkvm_polymul(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(1), pp, pl, ctypes.c_size_t(0), None, None, ctypes.c_uint32(lg)))
        assert e.value.code == 1 and (out == 7).all(), lg  # hipErrorInvalidValue
    pl = (ctypes.c_size_t * 1)(8)  # exactly the domain: copied
    _lib.check(_lib.lib().snarkvm_polymul(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(1), pp, pl, ctypes.c_size_t(0), None, None, ctypes.c_uint32(3)))
    assert np.array_equal(out[:8], p[:8]) and (out[8:] == 7).all()


def test_argument_validation_raises_before_ffi():
    from snarkvm_amd import plugin
    from snarkvm_amd.layout import G1_AFFINE

    with pytest.raises(ValueError):
        plugin.NTT(12, np.zeros((12, 4), dtype=np.uint64), 0, 0, 0)  # not a power of two (lib.rs:84-86)
    with pytest.raises(ValueError):
        plugin.msm(np.zeros(3, dtype=G1_AFFINE), np.zeros((4, 4), dtype=np.uint64))  # lib.rs:150-152


def test_no_gpu_means_loud_failure_not_fallback():
    """Without a device every compute entry point must fail loudly (the reference's caller owns the CPU fallback)."""
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    from snarkvm_amd import plugin

    with pytest.raises(_lib.HipError):
        plugin.NTT(8, np.zeros((8, 4), dtype=np.uint64), 0, 0, 0)
    from snarkvm_amd.layout import G1_AFFINE

    with pytest.raises(_lib.HipError):
        plugin.msm(np.zeros(4, dtype=G1_AFFINE), np.zeros((4, 4), dtype=np.uint64))


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under snarkvm_amd/ (Python or C++/HIP) or include/ may import, include,
    link or dlopen it; bench.py only inside its cpu_baseline leg; __graft_entry__ only in build()/smoke()."""
    pat_py = re.compile(r"^\s*(from\s+oracle\b|import\s+oracle\b)", re.M)
    pat_c = re.compile(r"#\s*include\s*[\"<][^\">]*oracle|liboracle|cpu_oracle")
    for top in ("snarkvm_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(util.ROOT, top)):
            for f in files:
                path = os.path.join(dirpath, f)
                if f.endswith(".py"):
                    assert not pat_py.search(open(path).read()), path
                elif f.endswith((".hip", ".h", ".hpp", ".cpp")):
                    assert not pat_c.search(open(path).read()), path
    bench = open(os.path.join(util.ROOT, "bench.py")).read()
    # every oracle import of bench.py sits inside a checking leg that runs after the timed region of its function
    markers = ("CPU baseline + oracle checks (rank 0, N = 1 only)", "# ---- checks (outside the timed regions)")
    for m in re.finditer(r"from oracle import", bench):
        func_start = bench.rfind("\ndef ", 0, m.start())
        body = bench[func_start : m.start()]
        if body.startswith("\ndef oracle_check_proof("):
            continue  # the checker of the proof-shaped legs: its CALL SITES are held to the same rule below
        assert any(k in body for k in markers), bench[m.start() - 200 : m.start() + 40]
        assert "time.perf_counter() - t0" in body  # the timed region of that function has ended before the import
    calls = [m for m in re.finditer(r"(?<!def )oracle_check_proof\(", bench)]
    assert calls
    for m in calls:
        func_start = bench.rfind("\ndef ", 0, m.start())
        body = bench[func_start : m.start()]
        assert "# ---- checks (outside the timed regions)" in body, bench[m.start() - 200 : m.start() + 40]
        assert "time.perf_counter() - t0" in body
    assert len(re.findall(r"from oracle import", bench)) >= 2
