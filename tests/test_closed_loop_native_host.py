"""mpcd_closed_loop on the host: the entry point is exported and bound, rejects null arguments, and the ctypes
struct has the C struct's layout (a probe compiled against include/mpcd.h reports it). No GPU needed."""
import ctypes
import os
import subprocess

from mpc_via_diffusion_model_amd import _native as N
from mpc_via_diffusion_model_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"mpcd_closed_loop_args": N.ClosedLoopArgs, "mpcd_sample_args": N.SampleArgs}

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mpcd.h"
#define F(S, m) printf(#S " " #m " %zu\n", offsetof(S, m))
int main(void)
{
    printf("mpcd_closed_loop_args sizeof %zu\n", sizeof(mpcd_closed_loop_args));
    printf("mpcd_sample_args sizeof %zu\n", sizeof(mpcd_sample_args));
    F(mpcd_closed_loop_args, sys); F(mpcd_closed_loop_args, ctx_min); F(mpcd_closed_loop_args, ctx_max);
    F(mpcd_closed_loop_args, act_min); F(mpcd_closed_loop_args, act_max); F(mpcd_closed_loop_args, sample);
    F(mpcd_closed_loop_args, n_states); F(mpcd_closed_loop_args, group); F(mpcd_closed_loop_args, iterations);
    F(mpcd_closed_loop_args, group_contexts); F(mpcd_closed_loop_args, noise_iters);
    F(mpcd_closed_loop_args, clip_rule); F(mpcd_closed_loop_args, select_first); F(mpcd_closed_loop_args, decimals);
    F(mpcd_closed_loop_args, warm_t_start); F(mpcd_closed_loop_args, x_dev); F(mpcd_closed_loop_args, x_hist);
    F(mpcd_closed_loop_args, u_hist); F(mpcd_closed_loop_args, cost_hist); F(mpcd_closed_loop_args, index_hist);
    F(mpcd_closed_loop_args, u_norm);
    return 0;
}
"""


def test_null_arguments_are_einval():
    L = N.lib()
    assert L.mpcd_closed_loop(None, None, None) == -1
    assert L.mpcd_last_error()
    a = N.ClosedLoopArgs()
    assert L.mpcd_closed_loop(None, ctypes.byref(a), None) == -1


def test_ctypes_struct_has_the_c_layout(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    # the header is C and C++; the toolchain the library is built with compiles the probe as plain host C++
    subprocess.run([B.hipcc(), "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = []
    for line in out.splitlines():
        struct, member, value = line.split()
        cls = STRUCTS[struct]
        if member == "sizeof":
            assert ctypes.sizeof(cls) == int(value), line
        else:
            assert getattr(cls, member).offset == int(value), line
            seen.append(member)
    assert seen == [f for f, _ in N.ClosedLoopArgs._fields_], "field order"
