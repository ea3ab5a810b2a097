"""No GPU: the constraint set's place in the C ABI and in Python - mpcd_rollout_cost_constr and
mpcd_mpc_step_batch_constr are exported and bound, the ctypes mirrors of mpcd_constraints and mpcd_batch_constr_args have
the header's layout, the first argument checks answer without a device, and Constraints validates against a system."""
import ctypes
import os
import re

import numpy as np
import pytest

from mpc_via_diffusion_model_amd import Constraints
from mpc_via_diffusion_model_amd import _native as N

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcd.h")
INF = float("inf")


def _struct(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)  # comments first: they may hold braces
    return re.search(r"typedef struct \{([^}]*)\} " + name + ";", text).group(1)


def test_symbols_are_exported_and_bound():
    L = N.lib()
    assert "mpcd_rollout_cost_constr" in N.EXPORTS and "mpcd_mpc_step_batch_constr" in N.EXPORTS
    fn = L.mpcd_rollout_cost_constr
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    assert fn.argtypes[10] == ctypes.POINTER(N.ConstraintSet)
    fn = L.mpcd_mpc_step_batch_constr
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.c_void_p, ctypes.POINTER(N.BatchStepArgs), ctypes.POINTER(N.BatchEliteArgs),
                           ctypes.POINTER(N.BatchConstrArgs), ctypes.c_void_p]
    # the header declares both with the same number of parameters
    text = open(HEADER).read()
    for name, n in (("mpcd_rollout_cost_constr", 15), ("mpcd_mpc_step_batch_constr", 5)):
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"int " + name + r"\(([^;]*)\);", text).group(1), flags=re.S)
        assert len(decl.split(",")) == n, name


def test_constraints_layout_follows_the_header():
    text = open(HEADER).read()
    assert re.search(r"#define MPCD_MAX_CON_ROWS 8\b", text) and N.MPCD_MAX_CON_ROWS == 8
    decls = [" ".join(d.split()) for d in _struct("mpcd_constraints").split(";") if d.strip()]
    assert decls == ["mpcd_state_box box", "int32_t n_rows", "int32_t reserved", "double A[MPCD_MAX_CON_ROWS][12]",
                     "double C[MPCD_MAX_CON_ROWS][4]", "double b[MPCD_MAX_CON_ROWS]", "double du_max[4]"]
    names = ["box", "n_rows", "reserved", "A", "C", "b", "du_max"]
    assert names == [f for f, _ in N.ConstraintSet._fields_]
    sizes = [24 * 8, 4, 4, 8 * 12 * 8, 8 * 4 * 8, 8 * 8, 4 * 8]
    assert sizes == [ctypes.sizeof(t) for _, t in N.ConstraintSet._fields_]
    offs = [0, 192, 196, 200, 968, 1224, 1288]
    assert [getattr(N.ConstraintSet, f).offset for f in names] == offs
    assert ctypes.sizeof(N.ConstraintSet) == 1320
    # row-major [row][component], as the header's A[r][i]
    c = N.ConstraintSet()
    c.A[2][5] = 7.0
    c.C[3][1] = 9.0
    raw = np.frombuffer(bytes(c), dtype=np.float64)
    assert raw[200 // 8 + 2 * 12 + 5] == 7.0 and raw[968 // 8 + 3 * 4 + 1] == 9.0


def test_batch_args_layout_follows_the_header():
    names, sizes = [], []
    for decl in filter(None, (d.strip() for d in _struct("mpcd_batch_constr_args").split(";"))):
        ctype, rest = decl.rsplit(" ", 1) if "," not in decl else decl.split(" ", 1)
        for name in rest.split(","):
            name = name.strip()
            names.append(name.lstrip("*"))
            sizes.append(8 if name.startswith("*") or ctype.strip() in ("double", "int64_t") else 4)
    assert names == ["con", "tol", "u_prev_host", "viol_host", "n_feasible_host", "elite_viol_host", "reserved", "reserved2"]
    assert names == [f for f, _ in N.BatchConstrArgs._fields_]
    assert sizes == [ctypes.sizeof(t) for _, t in N.BatchConstrArgs._fields_]
    assert [getattr(N.BatchConstrArgs, f).offset for f in names] == [0, 8, 16, 24, 32, 40, 48, 52]
    assert ctypes.sizeof(N.BatchConstrArgs) == 56


def test_null_arguments_are_einval():
    L = N.lib()
    a, e, b = N.BatchStepArgs(), N.BatchEliteArgs(), N.BatchConstrArgs()
    e.k = 1
    assert L.mpcd_mpc_step_batch_constr(None, ctypes.byref(a), ctypes.byref(e), ctypes.byref(b), None) == -1
    assert b"null" in L.mpcd_last_error()
    assert L.mpcd_mpc_step_batch_constr(None, ctypes.byref(a), None, ctypes.byref(b), None) == -1
    assert L.mpcd_mpc_step_batch_constr(None, None, None, None, None) == -1
    sysd, con = N.SystemDesc(), N.ConstraintSet()
    assert L.mpcd_rollout_cost_constr(None, ctypes.byref(sysd), None, 1, None, None, None, 1, 4, None, ctypes.byref(con),
                                      None, None, None, None) == -1
    assert b"null" in L.mpcd_last_error()


def test_constraints_native_fills_the_struct():
    con = Constraints(state_box=([None, -1.0], None), rows=[([1.0, 0.5], None, 2.0), ([-1.0, 0.0], [0.25], INF)],
                      du_max=[0.75]).native(2, 1)
    assert con.n_rows == 2 and con.reserved == 0
    assert list(con.box.lo)[:3] == [-INF, -1.0, -INF] and all(v == INF for v in con.box.hi)
    assert list(con.A[0])[:3] == [1.0, 0.5, 0.0] and list(con.C[0]) == [0.0] * 4 and con.b[0] == 2.0
    assert list(con.A[1])[:2] == [-1.0, 0.0] and con.C[1][0] == 0.25 and con.b[1] == INF
    assert all(con.b[r] == INF for r in range(2, 8))
    assert list(con.du_max) == [0.75, INF, INF, INF]
    empty = Constraints().native(12, 4)
    assert empty.n_rows == 0 and all(v == INF for v in empty.du_max) and all(v == -INF for v in empty.box.lo)
    assert list(Constraints(du_max=[None, 0.0]).native(4, 2).du_max)[:2] == [INF, 0.0]


@pytest.mark.parametrize("kw, needle", [
    (dict(state_box=([0.0, 0.0], [1.0, -1.0])), "component 1"),
    (dict(state_box=([0.0], [1.0])), "n_x = 2"),
    (dict(rows=[([1.0, 0.0], None, 0.0)] * 9), "at most 8"),
    (dict(rows=[([1.0], None, 0.0)]), "row 0"),
    (dict(rows=[([1.0, 0.0], None, 0.0), ([1.0, 0.0], [1.0, 2.0], 0.0)]), "row 1"),
    (dict(rows=[([1.0, float("nan")], None, 0.0)]), "a[1]"),
    (dict(rows=[([1.0, 0.0], [INF], 0.0)]), "c[0]"),
    (dict(rows=[([1.0, 0.0], None, float("nan"))]), "row 0: b"),
    (dict(rows=[([1.0, 0.0], None, -INF)]), "row 0: b"),
    (dict(rows=[(1.0, None)]), "row 0"),
    (dict(du_max=[0.1, 0.2]), "n_u = 1"),
    (dict(du_max=[-0.1]), "du_max[0]"),
    (dict(du_max=[float("nan")]), "du_max[0]"),
])
def test_constraints_validation_names_the_entry(kw, needle):
    with pytest.raises(ValueError, match=re.escape(needle)):
        Constraints(**kw).native(2, 1)
