"""ctypes loader of snarkvm_amd/lib/libsnarkvm_hip.so (the C ABI of include/snarkvm_hip.h).

There is deliberately no CPU fallback: if the HIP library is missing or a call fails, an exception is
raised (the reference's *caller* owns the CPU fallback, msm/variable_base/mod.rs:39-43).
"""
import ctypes
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SNARKVM_HIP_LIB") or os.path.join(_HERE, "lib", "libsnarkvm_hip.so")  # override: A/B experiments only

class RustError(ctypes.Structure):
    """sppark `cuda::Error` (algorithms/cuda/src/lib.rs:20): code 0 == success."""
    _fields_ = [("code", ctypes.c_int32), ("message", ctypes.c_void_p)]


class HipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"snarkvm_hip error {code}: {message}")
        self.code = code
        self.message = message


# every symbol include/snarkvm_hip.h declares, and the ctypes class of every tag of _abi.py (tools/gen_bindings.py documents the tags; pointer
# arguments are c_void_p so that addresses, byref(), arrays, handles and None all pass; a bare int then travels at the parameter's full width)
SYMBOLS = [name for name, _, _ in _abi.FUNCTIONS]
_CTYPES = {"ptr": ctypes.c_void_p, "size": ctypes.c_size_t, "int": ctypes.c_int, "i32": ctypes.c_int32, "u32": ctypes.c_uint32, "u64": ctypes.c_uint64,
           "f64": ctypes.c_double, "err": RustError, "void": None, "str": ctypes.c_char_p}

_lib = None
_libc = None


def lib():
    global _lib, _libc
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing - build it with `python -m snarkvm_amd.build` (hipcc, gfx950). "
                "snarkvm_amd has no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.
        # If torch is installed, load it first so that this library binds to the runtime that is already in the
        # process (same SONAME); two runtimes in one process leave the second one without visible GPUs.
        # SNARKVM_HIP_NO_TORCH=1: a torch-free host (tests/test_gpu_devmem.py proves a whole proof's call list that way): the library then binds to the
        # HIP runtime of /opt/rocm like any C++ / Rust caller's process does.
        if not os.environ.get("SNARKVM_HIP_NO_TORCH"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in _abi.FUNCTIONS:  # a symbol the library lacks raises AttributeError here
            fn = getattr(L, name)
            fn.restype = _CTYPES[res]
            fn.argtypes = [_CTYPES[t] for t in args]
        _libc = ctypes.CDLL(None)
        _libc.free.argtypes = [ctypes.c_void_p]
        _lib = L
    return _lib


def check(err):
    """Raise HipError for a non-zero RustError (and free its message, as Rust's Drop would)."""
    if err.code != 0:
        msg = ctypes.string_at(err.message).decode(errors="replace") if err.message else ""
        if err.message:
            _libc.free(err.message)
        raise HipError(err.code, msg)


def device_count():
    return lib().snarkvm_hip_device_count()
