"""Host side of the elite-set entry points (no GPU): the symbols are exported and bound, the header's constant is the
binding's, and a call without a context is refused before anything touches a device."""
import ctypes
import os
import re

from mpc_via_diffusion_model_amd import _native as nat

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_bound():
    L = nat.lib()
    for name in ("mpcd_topk", "mpcd_elite_priors", "mpcd_mpc_step_elite"):
        assert name in nat.EXPORTS and getattr(L, name).restype is ctypes.c_int


def test_max_elites_is_the_headers():
    text = open(os.path.join(ROOT, "include", "mpcd.h")).read()
    assert int(re.search(r"#define MPCD_MAX_ELITES (\d+)", text).group(1)) == nat.MPCD_MAX_ELITES == 64


def test_null_context_is_refused():
    L = nat.lib()
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.mpcd_topk(None, p, 1, 2, 1, 0, p, None) == EINVAL
    assert L.mpcd_last_error()
    assert L.mpcd_elite_priors(None, p, 1, 2, 8, p, 1, 0, 1, p, None) == EINVAL
    st, w, best = nat.StepArgs(), nat.WarmStart(), nat.Best()
    assert L.mpcd_mpc_step_elite(None, ctypes.byref(st), ctypes.byref(w), 1, None, None, ctypes.byref(best), p, None) == EINVAL
