"""Host-side cost of one cfg2 control step's Python path (GPU box): plan.mpc_step with the library's mpcd_mpc_step
replaced by a no-op (everything else real: argument block, device tensors, ctypes), and its pieces timed alone; the same
for mpc_step_constr (mpcd_mpc_step_constr) and for mpc_step_batch at 64 states x 64 candidates (mpcd_mpc_step_batch).
The three figures are also printed as one JSON line after "HOST_PATH ".

  python tools/host_path.py"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mpc_via_diffusion_model_amd import Constraints, DiffusionMPC, NetSpec, systems  # noqa: E402

cfg = bench.WORKLOADS["cfg2"]
torch.cuda.set_device(0)
spec = NetSpec("mlp", state_dim=cfg["d"], horizon=cfg["H"], context_dim=cfg["C"], dtype=cfg["dtype"])
plan = DiffusionMPC(spec, bench.synthetic_params(spec, seed=0), variance_schedule=cfg["schedule"], n_diffusion_steps=cfg["N"])
system = systems.get(cfg["system"])
x0s = np.random.default_rng(1).uniform(-1, 1, (400, system.n_x))
B = 4096
for i in range(5):
    plan.mpc_step(x0s[i], system, B, w=0.01, seed=2 + i)
torch.cuda.synchronize()


class NoStep:
    """the library with one entry point as a no-op returning MPCD_OK"""
    def __init__(self, lib, entry):
        self._l, self._entry = lib, entry

    def __getattr__(self, n):
        if n == self._entry:
            return lambda *a: 0
        return getattr(self._l, n)


def per_call(f, n=20000):
    for _ in range(200):
        f()
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    return (time.perf_counter() - t0) / n * 1e6


real = plan._lib
con = Constraints(([None] * system.n_x, [None] * system.n_x), du_max=[1.5] * system.n_u)
u_prev, xb = np.zeros(system.n_u), x0s[:64]
paths = {"mpc_step": ("mpcd_mpc_step", lambda: plan.mpc_step(x0s[0], system, B, w=0.01, seed=3)),
         "mpc_step_constr": ("mpcd_mpc_step_constr",
                             lambda: plan.mpc_step_constr(x0s[0], system, B, con, u_prev=u_prev, w=0.01, seed=3)),
         "mpc_step_batch": ("mpcd_mpc_step_batch", lambda: plan.mpc_step_batch(xb, system, 64, w=0.01, seed=3))}
us = {}
for name, (entry, call) in paths.items():
    call()  # the real call once: whatever the path sets up on its first use
    torch.cuda.synchronize()
    plan._lib = NoStep(real, entry)
    us[name] = per_call(call)
    plan._lib = real
    print(f"{name} Python path without the library call: {us[name]:.2f} us")
print("HOST_PATH " + json.dumps(us))
fl = ctypes.c_int32()
print(f"  ctypes call (mpcd_last_step_flags):          {per_call(lambda: real.mpcd_last_step_flags(plan._ctx, ctypes.byref(fl))):.2f} us")
print(f"  torch.empty x2 on the device:                {per_call(lambda: (torch.empty((B, 32, 2), device=plan.device), torch.empty(B, dtype=torch.float64, device=plan.device))):.2f} us")
print(f"  plan._stream():                              {per_call(plan._stream):.2f} us")
print(f"  plan._system_desc(system):                   {per_call(lambda: plan._system_desc(system)):.2f} us")
print(f"  np.empty + ascontiguousarray:                {per_call(lambda: (np.empty((32, 2), dtype=np.float32), np.ascontiguousarray(x0s[0], dtype=np.float64))):.2f} us")
t0 = time.perf_counter()
for i in range(200):
    plan.mpc_step(x0s[i % 400], system, B, w=0.01, seed=2 + i)
torch.cuda.synchronize()
print(f"full mpc_step: {(time.perf_counter() - t0) / 200 * 1e3:.4f} ms; sampler kernel {plan.sample_ms_mean(200):.4f} ms")
