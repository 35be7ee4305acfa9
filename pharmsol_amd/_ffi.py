"""ctypes binding of ``libpmx_hip.so`` (the C ABI of ``include/pmx.h``).

The library is built in-tree by ``__graft_entry__.build()`` / ``make``.  If it is
missing this module raises: there is no Python or CPU fallback for the compute path.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# PMX_LIB: developer override for same-device A/B runs of two builds (tools/ab_build.sh)
LIB_PATH = os.environ.get("PMX_LIB") or os.path.join(_HERE, "lib", "libpmx_hip.so")
_lib = None

# every symbol include/pmx.h declares: (name, restype, argtypes), generated from the header (_pmx_h.py)
SYMBOLS = _abi.FUNCTIONS


def lib():
    """Load libpmx_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make`).  pharmsol_amd has no CPU fallback.")
        # PyTorch bundles its own libamdhip64 (same SONAME as /opt/rocm's).  If libpmx_hip.so were loaded
        # first, the process would end up with TWO HIP runtimes and torch would see no GPU; loading torch
        # first makes the dynamic loader hand torch's runtime to this library too, so device pointers and
        # streams are shared.  (Pure C/C++ clients link /opt/rocm's runtime and never meet torch.)
        try:
            import torch  # noqa: F401
        except ImportError:  # the C ABI itself does not need torch
            pass
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if L.pmx_abi_version() != _abi.PMX_ABI_VERSION:
            raise ImportError("libpmx_hip.so ABI version mismatch")
        for st in _abi.STRUCTS:
            if L.pmx_sizeof_struct(st.__name__.encode()) != C.sizeof(st):
                raise ImportError(f"{st.__name__} layout drift between libpmx_hip.so and pharmsol_amd/_pmx_h.py")
        _lib = L
    return _lib


class Owned:
    """Base of the objects that own a library handle: ``handle`` goes back through the library function that ``_destroy``
    names when the object is collected."""
    _destroy = ""
    handle = None

    def __del__(self):
        h = self.handle
        if h and _lib is not None:  # (module globals vanish at interpreter exit)
            getattr(_lib, self._destroy)(h)
            self.handle = None


def check(rc: int, allow_pair_failures: bool = False) -> int:
    if rc == _abi.PMX_OK or (allow_pair_failures and rc == _abi.PMX_ERR_PAIR_FAILED):
        return rc
    raise _abi.PmxError(rc, lib().pmx_last_error().decode())
