"""Host side of the state-constraint entry points (no GPU): the symbols are exported and bound, the binding's struct is
the header's, and a call without a context is refused before anything touches a device."""
import ctypes
import os
import re

from mpc_via_diffusion_model_amd import _native as nat

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpcd_rollout_cost_box", "mpcd_topk_feasible", "mpcd_control_step_picked")


def test_symbols_are_exported_and_bound():
    L = nat.lib()
    for name in NAMES:
        assert name in nat.EXPORTS and getattr(L, name).restype is ctypes.c_int
        assert getattr(L, name).argtypes == nat.EXPORTS[name][0]


def test_state_box_is_the_headers():
    text = open(os.path.join(ROOT, "include", "mpcd.h")).read()
    m = re.search(r"typedef struct \{ double lo\[(\d+)\], hi\[(\d+)\]; \} mpcd_state_box;", text)
    assert m and int(m.group(1)) == int(m.group(2)) == 12
    assert ctypes.sizeof(nat.StateBox) == 2 * 12 * 8
    assert nat.StateBox.lo.offset == 0 and nat.StateBox.hi.offset == 96
    for name, n_args in zip(NAMES, (14, 12, 18)):  # the prototypes' argument counts
        proto = re.search(r"\bint " + name + r"\((.*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S)
        assert proto and len(proto.group(1).split(",")) == n_args == len(nat.EXPORTS[name][0]), name


def test_null_context_is_refused():
    L = nat.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    sysd, box = nat.SystemDesc(), nat.StateBox()
    assert L.mpcd_rollout_cost_box(None, ctypes.byref(sysd), p, 1, p, p, p, 1, 4, p, ctypes.byref(box), p, p, None) == EINVAL
    assert L.mpcd_last_error()
    assert L.mpcd_topk_feasible(None, p, p, 1, 2, 1, 0.0, 0, p, None, None, None) == EINVAL
    assert L.mpcd_last_error()
    assert L.mpcd_control_step_picked(None, ctypes.byref(sysd), p, 1, p, 1, 4, p, 1, 0, p, p, p, 4, p, p, p, None) == EINVAL
    assert L.mpcd_last_error()
