"""No GPU: mpcd_mpc_step_batch_elite's place in the C ABI - the symbol is exported and bound, its argument struct has
the header's layout, and the first argument check answers without a device."""
import ctypes

from mpc_via_diffusion_model_amd import _native as N


def test_symbol_is_exported_and_bound():
    assert "mpcd_mpc_step_batch_elite" in N.EXPORTS
    fn = N.lib().mpcd_mpc_step_batch_elite
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.c_void_p, ctypes.POINTER(N.BatchStepArgs), ctypes.POINTER(N.BatchEliteArgs),
                           ctypes.c_void_p]


def test_struct_layout():
    assert ctypes.sizeof(N.BatchEliteArgs) == 24
    assert [(f, getattr(N.BatchEliteArgs, f).offset) for f, _ in N.BatchEliteArgs._fields_] == [
        ("k", 0), ("reserved", 4), ("priors", 8), ("elites_host", 16)]
    assert ctypes.sizeof(N.Best) == 16  # an elite entry


def test_null_context_is_einval():
    L = N.lib()
    a, e = N.BatchStepArgs(), N.BatchEliteArgs()
    e.k = 1
    assert L.mpcd_mpc_step_batch_elite(None, ctypes.byref(a), ctypes.byref(e), None) == -1
    assert b"null" in L.mpcd_last_error()
    assert L.mpcd_mpc_step_batch_elite(None, None, None, None) == -1
