"""No GPU: mpcd_mpc_step_batch_box's place in the C ABI - the symbol is exported and bound, its argument struct has the
header's layout, the per-state flag has the header's value, and the first argument check answers without a device."""
import ctypes
import os
import re

from mpc_via_diffusion_model_amd import _native as N

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcd.h")


def test_symbol_is_exported_and_bound():
    assert "mpcd_mpc_step_batch_box" in N.EXPORTS
    fn = N.lib().mpcd_mpc_step_batch_box
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.c_void_p, ctypes.POINTER(N.BatchStepArgs), ctypes.POINTER(N.BatchEliteArgs),
                           ctypes.POINTER(N.BatchBoxArgs), ctypes.c_void_p]


def test_struct_layout_follows_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} mpcd_batch_box_args;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, sizes = [], []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, rest = decl.rsplit(" ", 1) if "," not in decl else decl.split(" ", 1)
        for name in rest.split(","):
            name = name.strip()
            names.append(name.lstrip("*"))
            sizes.append(8 if name.startswith("*") or ctype.strip() in ("double", "int64_t") else 4)
    assert names == ["box", "tol", "viol_host", "n_feasible_host", "elite_viol_host", "reserved", "reserved2"]
    assert names == [f for f, _ in N.BatchBoxArgs._fields_]
    assert sizes == [ctypes.sizeof(t) for _, t in N.BatchBoxArgs._fields_]
    assert [getattr(N.BatchBoxArgs, f).offset for f in names] == [0, 8, 16, 24, 32, 40, 44]
    assert ctypes.sizeof(N.BatchBoxArgs) == 48
    assert ctypes.sizeof(N.StateBox) == 24 * 8


def test_infeasible_flag_value():
    assert N.MPCD_STEP_INFEASIBLE == 16
    assert re.search(r"enum \{ MPCD_STEP_INFEASIBLE = 16 \};", open(HEADER).read())
    others = (N.MPCD_STEP_CLIPPED, N.MPCD_STEP_NAN_SAMPLES, N.MPCD_STEP_NONFINITE_WINNER, N.MPCD_STEP_F32X3_RERUN)
    assert all(N.MPCD_STEP_INFEASIBLE & f == 0 for f in others)


def test_null_arguments_are_einval():
    L = N.lib()
    a, e, b = N.BatchStepArgs(), N.BatchEliteArgs(), N.BatchBoxArgs()
    e.k = 1
    assert L.mpcd_mpc_step_batch_box(None, ctypes.byref(a), ctypes.byref(e), ctypes.byref(b), None) == -1
    assert b"null" in L.mpcd_last_error()
    assert L.mpcd_mpc_step_batch_box(None, ctypes.byref(a), None, ctypes.byref(b), None) == -1
    assert L.mpcd_mpc_step_batch_box(None, None, None, None, None) == -1
