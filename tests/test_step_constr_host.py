"""No GPU: the one-call control step with a constraint set (mpcd_mpc_step_constr, DiffusionMPC.mpc_step_constr) in the C
ABI and in Python - the symbol is exported and bound, the ctypes mirror of mpcd_step_constr_args has the header's field
order, offsets and size (a probe compiled against include/mpcd.h reports them), NULL arguments answer MPCD_EINVAL
without a device, and the method's refusals that need no device."""
import ctypes
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from mpc_via_diffusion_model_amd import Constraints, DiffusionMPC, MPCResult, systems
from mpc_via_diffusion_model_amd import _native as N
from mpc_via_diffusion_model_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcd.h")
FIELDS = ["con", "tol", "u_prev_host", "viol_local", "viols_all", "k", "reserved", "next_priors_out", "elites_host",
          "elite_viol_host", "viol_host", "n_feasible_host"]

PROBE = "#include <stddef.h>\n#include <stdio.h>\n#include \"mpcd.h\"\nint main(void)\n{\n" + \
    "    printf(\"sizeof %zu\\n\", sizeof(mpcd_step_constr_args));\n" + \
    "".join(f"    printf(\"{f} %zu\\n\", offsetof(mpcd_step_constr_args, {f}));\n" for f in FIELDS) + "    return 0;\n}\n"


def test_symbol_is_exported_and_bound():
    L = N.lib()
    assert "mpcd_mpc_step_constr" in N.EXPORTS
    fn = L.mpcd_mpc_step_constr
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.c_void_p, ctypes.POINTER(N.StepArgs), ctypes.POINTER(N.WarmStart),
                           ctypes.POINTER(N.StepConstrArgs), ctypes.POINTER(N.Best), ctypes.c_void_p, ctypes.c_void_p]
    text = open(HEADER).read()
    decl = re.sub(r"/\*.*?\*/", "", re.search(r"int mpcd_mpc_step_constr\(([^;]*)\);", text).group(1), flags=re.S)
    assert len(decl.split(",")) == 7
    assert re.search(r"MPCD_STEP_INFEASIBLE = 16\b", text) and N.MPCD_STEP_INFEASIBLE == 16


def test_args_have_the_header_field_order():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} mpcd_step_constr_args;", text).group(1)
    names = [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert names == FIELDS == [f for f, _ in N.StepConstrArgs._fields_]


def test_ctypes_struct_has_the_c_layout(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    # the header is C and C++; the toolchain the library is built with compiles the probe as plain host C++
    subprocess.run([B.hipcc(), "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(N.StepConstrArgs) == int(out.pop("sizeof")) == 88
    assert list(out) == FIELDS
    for f, off in out.items():
        assert getattr(N.StepConstrArgs, f).offset == int(off), f
    assert [getattr(N.StepConstrArgs, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 44, 48, 56, 64, 72, 80]


def test_null_arguments_are_einval():
    L = N.lib()
    a, w, e, best = N.StepArgs(), N.WarmStart(), N.StepConstrArgs(), N.Best()
    u = (ctypes.c_float * 4)()
    assert L.mpcd_mpc_step_constr(None, None, None, None, None, None, None) == -1
    assert b"null" in L.mpcd_last_error()
    assert L.mpcd_mpc_step_constr(None, ctypes.byref(a), ctypes.byref(w), ctypes.byref(e), ctypes.byref(best), u, None) == -1
    assert b"null" in L.mpcd_last_error()
    assert L.mpcd_mpc_step_constr(None, ctypes.byref(a), None, None, ctypes.byref(best), u, None) == -1


def test_result_carries_the_elite_violations_last():
    names = [f.name for f in dataclasses.fields(MPCResult)]
    assert names[-1] == "elite_violation" and MPCResult.__dataclass_fields__["elite_violation"].default is None
    assert names[-3:-1] == ["violation", "n_feasible"]


def test_python_refusals_without_a_device():
    plan = DiffusionMPC.__new__(DiffusionMPC)  # every refusal below comes before the first use of the device context
    sysm, x0 = systems.double_int2d(), np.zeros(4)
    con = Constraints(du_max=[0.5, None])
    box = ([None, None, -1.0, -1.0], [None, None, 1.0, 1.0])
    for bad in (box, None, {"state_box": box}):
        with pytest.raises(ValueError, match="Constraints"):
            plan.mpc_step_constr(x0, sysm, 12, bad)
    with pytest.raises(ValueError, match="n_x = 4"):
        plan.mpc_step_constr(x0, sysm, 12, Constraints(state_box=([0.0], [1.0])))
    for tol in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="viol_tol"):
            plan.mpc_step_constr(x0, sysm, 12, con, viol_tol=tol)
    for up in (np.zeros(3), np.zeros((1, 2)), 0.5):
        with pytest.raises(ValueError, match=r"u_prev must be \[2\]"):
            plan.mpc_step_constr(x0, sysm, 12, con, u_prev=up)
    with pytest.raises(ValueError, match="elites needs warm_start"):
        plan.mpc_step_constr(x0, sysm, 12, con, elites=4)

    class Comm:  # stands for a NativeComm of two ranks
        rank, size = 1, 2

    with pytest.raises(ValueError, match="single-rank"):
        plan.mpc_step_constr(x0, sysm, 12, con, warm_start=5, elites=4, comm=Comm())
    with pytest.raises(ValueError, match="clip_rule"):
        plan.mpc_step_constr(x0, sysm, 12, con, clip_rule="all")
