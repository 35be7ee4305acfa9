"""What the Python binding knows beyond ``include/pmx.h``: the header's constants and structs are re-exported from the
generated ``_pmx_h.py`` (``tools/gen_python_binding.py``); kept here are the name tables, ``PmxError`` and the
user-closure role names.

Shared by the product binding (``_ffi.py`` -> libpmx_hip.so) and by the test oracle's binding (``oracle/__init__.py`` ->
libpmx_oracle.so); it holds no compute.
"""
from __future__ import annotations

from . import _pmx_h
from ._pmx_h import *  # noqa: F401,F403


def _names(prefix: str) -> dict:
    """name -> id of the header's ``<prefix>*`` enumerators (lower-cased suffix), without CUSTOM and the *_COUNT sentinels."""
    return {k[len(prefix):].lower(): v for k, v in vars(_pmx_h).items()
            if k.startswith(prefix) and not k.endswith(("_CUSTOM", "_COUNT"))}


# AnalyticalKernel (pharmsol-dsl/src/analysis.rs:187-200) and the built-in diffeq bodies, name -> id
ANALYTICAL_KERNELS = _names("PMX_K_")
ODE_MODELS = _names("PMX_ODE_")

# AnalyticalKernel::required_parameter_names (analysis.rs:240-255)
KERNEL_PARAMETER_NAMES = {
    "one_compartment": ["ke"],
    "one_compartment_cl": ["cl", "v"],
    "one_compartment_cl_with_absorption": ["ka", "cl", "v"],
    "one_compartment_with_absorption": ["ka", "ke"],
    "two_compartments": ["ke", "kcp", "kpc"],
    "two_compartments_cl": ["cl", "q", "vc", "vp"],
    "two_compartments_cl_with_absorption": ["ka", "cl", "q", "vc", "vp"],
    "two_compartments_with_absorption": ["ke", "ka", "kcp", "kpc"],
    "three_compartments": ["k10", "k12", "k13", "k21", "k31"],
    "three_compartments_cl": ["cl", "q2", "q3", "vc", "v2", "v3"],
    "three_compartments_cl_with_absorption": ["ka", "cl", "q2", "q3", "vc", "v2", "v3"],
    "three_compartments_with_absorption": ["ka", "k10", "k12", "k13", "k21", "k31"],
}

# AnalyticalKernel::state_count (analysis.rs:259-270)
KERNEL_STATE_COUNT = {
    "one_compartment": 1,
    "one_compartment_cl": 1,
    "one_compartment_cl_with_absorption": 2,
    "one_compartment_with_absorption": 2,
    "two_compartments": 2,
    "two_compartments_cl": 2,
    "two_compartments_cl_with_absorption": 3,
    "two_compartments_with_absorption": 3,
    "three_compartments": 3,
    "three_compartments_cl": 3,
    "three_compartments_cl_with_absorption": 4,
    "three_compartments_with_absorption": 4,
}

ODE_STATE_COUNT = {"one_cmt_iv": 1, "one_cmt_oral": 2, "two_cmt_iv": 2, "two_cmt_oral": 3, "three_cmt_iv": 3,
                   "three_cmt_oral": 4, "one_cmt_mm": 1}
ODE_PARAM_COUNT = {"one_cmt_iv": 1, "one_cmt_oral": 2, "two_cmt_iv": 3, "two_cmt_oral": 4, "three_cmt_iv": 5,
                   "three_cmt_oral": 6, "one_cmt_mm": 3}

STATUS_NAMES = {
    PMX_OK: "OK",
    PMX_ERR_INVALID_ARGUMENT: "InvalidArgument",
    PMX_ERR_INPUT_OUT_OF_RANGE: "InputOutOfRange",
    PMX_ERR_OUTEQ_OUT_OF_RANGE: "OuteqOutOfRange",
    PMX_ERR_UNSUPPORTED: "Unsupported",
    PMX_ERR_NO_DEVICE: "NoDevice",
    PMX_ERR_HIP: "HipError",
    PMX_ERR_OUT_OF_MEMORY: "OutOfMemory",
    PMX_ERR_PAIR_FAILED: "PairFailed",
    PMX_ERR_ERROR_MODEL: "ErrorModelError",
}


class PmxError(RuntimeError):
    """A failed C-ABI call (the Python face of ``PharmsolError``, src/error/mod.rs:13-49)."""

    def __init__(self, status: int, message: str):
        self.status = status
        self.status_name = STATUS_NAMES.get(status, str(status))
        super().__init__(f"{self.status_name}: {message}")


# ---- user closures (pmx_model_create_user) ----------------------------------------------------------------------
USER_FUNCTION_BITS = {"pmx_dynamics": PMX_FN_DYNAMICS, "pmx_dynamics_bolus": PMX_FN_DYNAMICS_BOLUS, "pmx_outputs": PMX_FN_OUTPUTS, "pmx_init": PMX_FN_INIT,
                      "pmx_derive": PMX_FN_DERIVE, "pmx_route_lag": PMX_FN_ROUTE_LAG,
                      "pmx_route_bioavailability": PMX_FN_ROUTE_BIOAVAILABILITY, "pmx_seq_eq": PMX_FN_SEQ_EQ,
                      "pmx_eq": PMX_FN_EQ}


def user_functions_of(source: str) -> int:
    """PMX_FN_* mask of the ``PMX_DEVICE void pmx_<role>(`` definitions a source text holds."""
    import re

    mask = 0
    for name, bit in USER_FUNCTION_BITS.items():
        if re.search(r"PMX_DEVICE\s+void\s+" + name + r"\s*\(", source):
            mask |= bit
    return mask

# parameter names of the built-in diffeq bodies, in the order the bodies read them (include/pmx.h PMX_ODE_*)
ODE_PARAMETER_NAMES = {"one_cmt_iv": ["ke"], "one_cmt_oral": ["ka", "ke"], "two_cmt_iv": ["ke", "kcp", "kpc"],
                       "two_cmt_oral": ["ke", "ka", "kcp", "kpc"], "three_cmt_iv": ["k10", "k12", "k13", "k21", "k31"],
                       "three_cmt_oral": ["ka", "k10", "k12", "k13", "k21", "k31"], "one_cmt_mm": ["vmax", "km", "v"]}
