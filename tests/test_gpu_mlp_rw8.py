"""The 8-wave resident-weight MLP sampler (layout "rw32x8", csrc/mlp_rw.hip: two waves per SIMD, 32 rows per
workgroup): the same sums in the same order as the 4-wave rw32 and the streaming 32x8 kernels, so every result is
compared bit for bit; plus the oracle, the shard property, the chain maxima, the form report and (on the CPU) the
register / scratch budget of every rw32x8 instantiation. Small shapes: what can go wrong is a ragged workgroup, state
carried across steps in registers and the waves without a tile, not the size."""
import glob
import os
import re
import shutil
import subprocess

import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec
from oracle import sampler as osam
from oracle import schedule as osch

from ._util import assert_traj_close, make_mlp
from .test_gpu_mlp import _ctx, _planner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpc_via_diffusion_model_amd")
LLVM = "/opt/rocm/lib/llvm/bin"
C, N = 4, 100


def _under(layouts, run):
    from mpc_via_diffusion_model_amd.planner import force_mlp_layout
    outs = {}
    try:
        for lay in layouts:
            force_mlp_layout(lay)
            outs[lay] = run()
            torch.cuda.synchronize()
    finally:
        force_mlp_layout("auto")
    return outs


def _assert_same(outs, what):
    new = outs["rw32x8"]
    assert torch.isfinite(new).all(), what
    for lay in ("rw32", "32x8"):
        assert torch.equal(new, outs[lay]), f"rw32x8 differs from {lay} ({what}): max |d| {float((new - outs[lay]).abs().max()):.3e}"


# B = 17: one full workgroup plus one candidate. H*d = 32: the final layer has two n-tiles, waves 2-3 idle there.
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,mode", [(17, 32, "ddpm_nwo_chain"), (100, 16, "ddpm"), (40, 64, "ddpm"), (33, 32, "ddim_cfg"),
                                      (48, 32, "ddim"), (17, 32, "ddpm_noise")])
def test_rw32x8_bit_identical_to_rw32_and_32x8(B, H, mode):
    d = 2
    net = make_mlp(d, H, C, seed=5)
    plan = _planner(net, d, H, C, N, cfg=mode != "ddim", dtype="f32x3")
    ctx = _ctx(B, C, True)
    noise = torch.randn(N + 1, B, H, d, generator=torch.Generator().manual_seed(11))

    def run():
        if mode == "ddpm_nwo_chain":
            return plan.run_CFG(ctx, None, 0.01, n_samples=B, horizon=H, return_chain=True,
                                n_diffusion_steps_without_noise=5, seed=3)
        if mode == "ddpm":
            return plan.run_CFG(ctx, None, 0.01, n_samples=B, horizon=H, seed=3)
        if mode == "ddpm_noise":  # caller-supplied noise: the DDPM_XN instantiation
            return plan.run_CFG(ctx, None, 0.01, n_samples=B, horizon=H, return_chain=True, noise=noise)
        return plan.sample_trajectories(ctx, B, H, seed=3, sample_fn=mode)

    _assert_same(_under(("32x8", "rw32", "rw32x8"), run), f"{mode}, B={B}, H={H}")


@pytest.mark.gpu
def test_rw32x8_eps_both_branches_bit_identical():
    B, H, d = 40, 32, 2
    net = make_mlp(d, H, C, seed=12)
    plan = _planner(net, d, H, C, N, dtype="f32x3")
    x = torch.randn(B, H, d, generator=torch.Generator().manual_seed(1))
    ctx = _ctx(B, C, True)
    outs = _under(("32x8", "rw32", "rw32x8"), lambda: torch.stack(plan.eps(x, 37, ctx)))
    _assert_same(outs, "plan.eps, both branches")
    assert not torch.equal(outs["rw32x8"][0], outs["rw32x8"][1])


@pytest.mark.gpu
def test_rw32x8_matches_oracle_at_the_cfg1_shape():
    B, H, d, n = 64, 16, 2, 50
    net = make_mlp(d, H, C)
    plan = _planner(net, d, H, C, n, dtype="f32x3")
    ctx = _ctx(B, C, True)
    noise = torch.randn(n + 1, B, H, d, generator=torch.Generator().manual_seed(11))
    ref = osam.ddpm_cfg(net, osch.buffers("exponential", n), ctx.expand(B, C), 0.01, B, H, 0, noise=noise, return_chain=True)
    got = _under(("rw32x8",), lambda: plan.run_CFG(ctx, None, 0.01, n_samples=B, horizon=H, return_chain=True,
                                                    n_diffusion_steps_without_noise=0, noise=noise))["rw32x8"]
    assert_traj_close(got, ref, what="ddpm chain, layout rw32x8, B=64")


@pytest.mark.gpu
def test_rw32x8_shard_property_and_chain_maxima():
    B, H, d = 48, 32, 2
    net = make_mlp(d, H, C)
    plan = _planner(net, d, H, C, N, dtype="f32x3")
    ctx = _ctx(B, C, True)
    outs = _under(("rw32x8",), lambda: (plan.sample_trajectories(ctx, B, H, seed=123),
                                        plan.sample_trajectories(ctx, 16, H, seed=123, global_offset=32)))
    full, part = outs["rw32x8"]
    assert torch.equal(part, full[32:])

    # the call pattern of test_chain_absmax_every_mlp_layout (tests/test_gpu_rollout.py)
    d, H, n, B = 2, 16, 25, 45
    net = make_mlp(d, H, C, seed=7)
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), n_diffusion_steps=n)
    ctx = torch.rand(1, C, generator=torch.Generator().manual_seed(9)) * 2 - 1

    def run():
        am = torch.empty(B, dtype=torch.float32, device="cuda")
        chain = plan.sample_trajectories(ctx, B, H, seed=4, return_chain=True, absmax_out=am)
        return am, chain

    outs = _under(("rw32", "rw32x8"), run)
    am8, chain8 = outs["rw32x8"]
    assert torch.equal(am8, outs["rw32"][0])
    assert torch.equal(am8, chain8.abs().amax(dim=(0, 2, 3)))


@pytest.mark.gpu
def test_rw32x8_form_and_layout_range():
    from mpc_via_diffusion_model_amd import _native as nat
    from mpc_via_diffusion_model_amd.planner import force_mlp_layout
    d, H = 2, 32
    plan = _planner(make_mlp(d, H, C), d, H, C, N, dtype="f32x3")
    force_mlp_layout("rw32x8")
    try:
        form = plan.mlp_form(4096)
        assert form["layout"] == "rw32x8" and form["rows_per_workgroup"] == 32 and form["kernel"] == "x3", form
        assert plan.mlp_layout(4096) == "rw32x8"
        assert nat.lib().mpcd_mlp_force_layout(6) != 0, "layout 6 does not exist"
        assert plan.mlp_form(4096)["layout"] == "rw32x8", "a refused layout number changes nothing"
    finally:
        force_mlp_layout("auto")


def _rw_code_object_notes(tmp_path):
    """llvm-readelf --notes of the gfx950 code object that holds mlp_rw.hip's kernels: the built library's (build()
    compiled it with the library's flags), or, without a built library, a device-only compile with the same flags."""
    readelf, objdump = os.path.join(LLVM, "llvm-readelf"), os.path.join(LLVM, "llvm-objdump")
    if not (os.path.exists(readelf) and os.path.exists(objdump)):
        pytest.skip("the ROCm LLVM tools are not present")
    lib = os.path.join(PKG, "libmpcd.so")
    if os.path.exists(lib):
        so = tmp_path / "libmpcd.so"
        shutil.copy(lib, so)
        subprocess.run([objdump, "--offloading", str(so)], cwd=tmp_path, check=True, capture_output=True)
        cos = sorted(glob.glob(str(tmp_path / "libmpcd.so.*gfx950")))
    else:
        from mpc_via_diffusion_model_amd import build as b
        co = tmp_path / "mlp_rw.co"
        subprocess.run([b.hipcc()] + b.FLAGS + b.SOURCE_FLAGS.get("mlp_rw.hip", []) +
                       ["--cuda-device-only", "-c", os.path.join(b.CSRC, "mlp_rw.hip"), "-o", str(co)],
                       check=True, capture_output=True)
        cos = [str(co)]
    assert cos, "no gfx950 code object"
    return "\n".join(subprocess.run([readelf, "--notes", c], check=True, capture_output=True, text=True).stdout for c in cos)


def test_rw32x8_build_metadata_no_scratch_no_spills(tmp_path):
    """Resource counts (not instructions) from the code-object metadata of every rw32x8 kernel: 3 widths x 6 sampler
    modes x with / without context. Two waves per SIMD leave a wave 256 registers; scratch or a spill in the step loop
    is a performance bug the results would not show."""
    notes = _rw_code_object_notes(tmp_path)
    kernels = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        blk = ".agpr_count:" + blk
        f = {k: v for k, v in re.findall(r"\.(\w+):\s+(\S+)", blk)}
        # mlp_rw_kernel<D0, SMODE, CTX, 32, 8>: Itanium mangling of the template arguments
        if re.search(r"mlp_rw_kernelILi\d+ELi\d+ELb[01]ELi32ELi8EE", f.get("name", "")) and not f["name"].endswith(".kd"):
            kernels[f["name"]] = f
    assert len(kernels) == 36, f"{len(kernels)} rw32x8 kernels in the code object (3 x 6 x 2 expected)"
    for name, f in kernels.items():
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])
        assert int(f["vgpr_spill_count"]) == 0, (name, f["vgpr_spill_count"])
        assert int(f["vgpr_count"]) <= 256, (name, f["vgpr_count"])
        assert int(f["group_segment_fixed_size"]) <= 160 * 1024, (name, f["group_segment_fixed_size"])
        assert int(f["max_flat_workgroup_size"]) == 512, (name, f["max_flat_workgroup_size"])
