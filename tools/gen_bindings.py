#!/usr/bin/env python3
"""Generates the two bindings of include/snarkvm_hip.h: rust/snarkvm-algorithms-hip/src/sys.rs, where every `snarkvm_*` declaration of the header
becomes one item of an `extern "C"` block (the reference's crate binds everything its library exports by hand, algorithms/cuda/src/lib.rs:42-69;
its build.rs compiles the device code, algorithms/cuda/build.rs:71-93 - here the library is prebuilt and the declarations are derived mechanically
so that they cannot drift from the header), and snarkvm_amd/_abi.py, the prototype table snarkvm_amd/_lib.py sets every ctypes restype / argtypes from.

    python tools/gen_bindings.py            # rewrite both
    python tools/gen_bindings.py --check    # exit 1 if a committed file differs from what the header yields

`parse_header` is also what tests/test_abi.py uses for the header side of its comparisons (the Rust side is parsed from the text of sys.rs by the
test itself; the Python side is read off the loaded library's functions).  Rust type map: size_t -> usize, int -> i32, uint32_t -> u32, int32_t -> i32, uint64_t -> u64, double -> f64, char -> c_char,
void -> c_void, `enum X` -> the #[repr(C)] enum X of lib.rs, RustError -> Error, the opaque handle structs -> zero-sized #[repr(C)] structs;
`const T *` -> *const T, `T *` -> *mut T, `T *const *` -> *const *mut T.  Python tags (snarkvm_amd/_lib.py maps them to ctypes): a pointer argument of any
depth, constness or pointee -> "ptr" (c_void_p: call sites pass addresses, byref(), arrays, handles and None alike), size_t -> "size", int and the
three enums -> "int", int32_t -> "i32", uint32_t -> "u32", uint64_t -> "u64", double -> "f64"; results: RustError -> "err", void -> "void",
`void *` -> "ptr", `const char *` -> "str".
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snarkvm_hip.h")
SYS_RS = os.path.join(ROOT, "rust", "snarkvm-algorithms-hip", "src", "sys.rs")
ABI_PY = os.path.join(ROOT, "snarkvm_amd", "_abi.py")

SCALARS = {"size_t": "usize", "int": "i32", "uint32_t": "u32", "int32_t": "i32", "uint64_t": "u64", "double": "f64", "char": "c_char", "void": "c_void"}
PY_TAGS = {"size_t": "size", "int": "int", "uint32_t": "u32", "int32_t": "i32", "uint64_t": "u64", "double": "f64"}
ENUMS = ("NTTInputOutputOrder", "NTTDirection", "NTTType")
OPAQUE = ("snarkvm_hip_bases_t", "snarkvm_hip_bases_g2_t", "snarkvm_hip_fr_matrix_t", "snarkvm_hip_fr_arith_t")
RUST_KEYWORDS = {"type", "in", "ref", "move", "fn", "box", "loop", "match", "mod", "use", "where", "impl", "self", "super", "trait", "yield"}


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def parse_ctype(tokens):
    """['const', 'void', '*', 'const', '*'] -> (base, [pointer levels, innermost first]) where a level is 'const' or 'mut' for the POINTEE it points at."""
    toks = [t for t in tokens if t != "enum"]
    base_const = False
    i = 0
    if toks[i] == "const":
        base_const = True
        i += 1
    base = toks[i]
    i += 1
    if i < len(toks) and toks[i] == "const":  # `T const`
        base_const = True
        i += 1
    levels = []  # constness of what each '*' points at
    pointee_const = base_const
    while i < len(toks):
        assert toks[i] == "*", tokens
        levels.append("const" if pointee_const else "mut")
        i += 1
        pointee_const = False
        if i < len(toks) and toks[i] == "const":  # the pointer itself is const: matters for the next level out
            pointee_const = True
            i += 1
    return base, levels


def parse_header(path=HEADER):
    """-> (functions, enum constants).  functions: [{'name', 'ret': (base, levels), 'args': [(name, (base, levels))]}] in header order."""
    text = strip_comments(open(path).read())
    consts = {}
    for m in re.finditer(r"enum\s*(\w*)\s*\{([^}]*)\}", text):
        for item in m.group(2).split(","):
            if "=" in item:
                k, v = item.split("=")
                consts[k.strip()] = int(v.strip(), 0)
    funcs = []
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(snarkvm_\w+)\s*\(([^)]*)\)\s*;", text):
        ret_tokens = re.findall(r"\w+|\*", m.group(1))
        args = []
        body = m.group(3).strip()
        if body and body != "void":
            for a in body.split(","):
                toks = re.findall(r"\w+|\*", a)
                name = toks[-1]
                args.append((name, parse_ctype(toks[:-1])))
        funcs.append({"name": m.group(2), "ret": parse_ctype(ret_tokens), "args": args})
    return funcs, consts


def rust_type(ct):
    base, levels = ct
    if base == "RustError":
        r = "Error"
    elif base in ENUMS or base in OPAQUE:
        r = base
    else:
        r = SCALARS[base]
    for lv in levels:
        r = f"*{lv} {r}"
    return r


def width_class(ct):
    """What the test compares across the two sides: ('ptr', depth) | ('int', bytes) | ('f64',) | ('err',) | ('void',)."""
    base, levels = ct
    if levels:
        return ("ptr", len(levels))
    if base == "RustError":
        return ("err",)
    if base == "void":
        return ("void",)
    if base in ENUMS:
        return ("int", 4)
    return {"size_t": ("int", 8), "int": ("int", 4), "uint32_t": ("int", 4), "int32_t": ("int", 4), "uint64_t": ("int", 8), "double": ("f64",)}[base]


def generate():
    funcs, consts = parse_header()
    out = []
    w = out.append
    w("// @generated by tools/gen_bindings.py from include/snarkvm_hip.h - DO NOT EDIT (tests/test_abi.py::test_rust_sys_matches_the_header fails on drift).")
    w("//! The raw C ABI of libsnarkvm_hip.so: every `snarkvm_*` function include/snarkvm_hip.h declares.  Part 1 = the three symbols of")
    w("//! `snarkvm-algorithms-cuda` (algorithms/cuda/src/lib.rs:42-69); the rest is the extension ABI (device memory, device-resident operands,")
    w("//! registered bases, scopes) and the test hooks.  The header's comments are the documentation of every item.")
    w("#![allow(non_camel_case_types, non_snake_case, clippy::too_many_arguments, clippy::missing_safety_doc)]")
    w("use super::{Error, NTTDirection, NTTInputOutputOrder, NTTType};")
    w("use core::ffi::{c_char, c_void};")
    w("")
    for name in OPAQUE:
        w("/// Opaque handle (the header's `typedef struct ... " + name + "`): only ever used behind a pointer.")
        w("#[repr(C)]")
        w(f"pub struct {name} {{")
        w("    _private: [u8; 0],")
        w("}")
    w("")
    for k, v in consts.items():
        if k.startswith("SNARKVM_HIP_"):
            w(f"pub const {k}: u32 = {v};")
    w("")
    w('extern "C" {')
    for f in funcs:
        args = ", ".join(f"{(n + '_') if n in RUST_KEYWORDS else n}: {rust_type(t)}" for n, t in f["args"])
        ret = "" if width_class(f["ret"]) == ("void",) else f" -> {rust_type(f['ret'])}"
        w(f"    pub fn {f['name']}({args}){ret};")
    w("}")
    return "\n".join(out) + "\n"


def py_tag(ct, result=False):
    base, levels = ct
    if levels:
        return "str" if result and base == "char" else "ptr"
    if base == "RustError":
        return "err"
    if base == "void":
        return "void"
    return "int" if base in ENUMS else PY_TAGS[base]


def generate_py():
    funcs, _ = parse_header()
    out = ["# @generated by tools/gen_bindings.py from include/snarkvm_hip.h - DO NOT EDIT (tests/test_abi.py::test_python_abi_table_matches_the_header fails on drift).",
           '"""The prototypes of libsnarkvm_hip.so as data: (name, result tag, argument tags) per function of include/snarkvm_hip.h, in header order.',
           'snarkvm_amd/_lib.py maps the tags to ctypes; the header\'s comments are the documentation of every function."""',
           "FUNCTIONS = ("]
    for f in funcs:
        args = "".join(f'"{py_tag(t)}", ' for _, t in f["args"]).rstrip()
        if len(f["args"]) > 1:
            args = args[:-1]
        out.append(f'    ("{f["name"]}", "{py_tag(f["ret"], result=True)}", ({args})),')
    out.append(")")
    return "\n".join(out) + "\n"


def main():
    outputs = [(SYS_RS, generate()), (ABI_PY, generate_py())]
    if "--check" in sys.argv:
        stale = [path for path, text in outputs if not os.path.exists(path) or open(path).read() != text]
        for path in stale:
            print(f"{path} is stale: run python tools/gen_bindings.py", file=sys.stderr)
        if stale:
            sys.exit(1)
        print("sys.rs and _abi.py are current")
        return
    for path, text in outputs:
        with open(path, "w") as fh:
            fh.write(text)
        print(f"wrote {path}: {len(parse_header()[0])} functions")


if __name__ == "__main__":
    main()
