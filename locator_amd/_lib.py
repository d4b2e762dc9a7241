"""ctypes binding of liblocator_hip.so (C ABI: include/locator_hip.h).

PyTorch is used only as plumbing (device memory, streams, graphs); every kernel on the hot
path comes from this library.  A missing library is a hard error — there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import os

# torch ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  It must be the
# one already resident when liblocator_hip.so is dlopen'ed, otherwise the library binds /opt/rocm's
# copy and the process ends up with two HIP runtimes that do not share devices, streams or memory.
import torch  # noqa: F401  (side effect: loads torch's libamdhip64 first)

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblocator_hip.so")


def use_library(path):
    """Measurement tools only (tools/rows_gemm_bench.py --lib): bind another build of the library, e.g. a timing
    ablation from `make -C locator_amd/csrc ablate A=1`.  Must be called before load()."""
    global LIB_PATH
    assert _lib is None, "library already loaded"
    LIB_PATH = path


# The structs and every entry point's (restype, argtypes) come from the headers under include/ (locator_amd/_abi.py): a new entry
# point needs its prototype in a header, a new header needs one line in _abi's table, and nothing here.
Dims, Layout, Tuning, Net, CbState = (_abi.STRUCTS[n] for n in ("loc_dims", "loc_layout", "loc_tuning", "loc_net",
                                                                "loc_cb_state"))
SIGNATURES = _abi.PROTOTYPES


class LocatorHipError(RuntimeError):
    pass


_lib = None


def load():
    """Load liblocator_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LocatorHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C locator_amd/csrc`.  locator_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _abi.ALL_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().loc_last_error().decode(errors="replace")
        raise LocatorHipError(f"{what} failed (code {rc}): {msg}")


def make_dims(K, H, L):
    d = Dims()
    check(load().loc_make_dims(int(K), int(H), int(L), C.byref(d)), "loc_make_dims")
    return d


def param_layout(d):
    lay = Layout()
    check(load().loc_param_layout(C.byref(d), C.byref(lay)), "loc_param_layout")
    return lay
