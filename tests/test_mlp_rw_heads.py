"""CPU check of the layer heads of the 8-wave resident-weight MLP sampler (csrc/mlp_rw.hip, the bench's cfg2 kernel
mlp_rw_kernel<64, DDPM_CFG, ctx, 32, 8>), read from its gfx950 code with tools/mlp_heads.py: what a wave issues
between the barrier that opens a layer and the layer's first MFMA stands on the critical path 14 times per denoise
step, so no wait there may be wider than the data that MFMA needs. The code is the built library's (build() compiled
it with the library's flags), or, without a built library, a device-only compile with the same flags, as in
tests/test_gpu_mlp_rw8.py. Nothing runs on a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "mpc_via_diffusion_model_amd", "libmpcd.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    import mlp_heads as mh
    tmp = str(tmp_path_factory.mktemp("heads"))
    if os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        lines = mh.library_lines(LIB, tmp)
    else:
        lines = open(mh.compile_asm(os.path.join(tmp, "mlp_rw.s"))).read().splitlines()
    return mh.Loop(mh.kernel_body(lines))


@pytest.fixture(scope="module")
def heads(loop):
    import mlp_heads as mh
    hs = mh.heads(loop)
    print(mh.report(loop))
    return hs


def test_fourteen_barriers_per_step(loop, heads):
    assert loop.barriers_per_step() == (14, 14)
    with_mfma = [h for h in heads if h["mfma"]]
    assert len({h["barrier"] for h in with_mfma}) == 14, "every barrier of the step opens a layer with an MFMA"


def test_no_scalar_load_at_a_head(heads):
    """A scalar load returns out of order: any wait behind it is lgkmcnt(0), the LDS reads read ahead included."""
    bad = [(h["barrier"], h["sload"]) for h in heads if h["mfma"] and (h["sload"] or h["lgkm_scalar"])]
    assert not bad, f"scalar loads between a barrier and the first MFMA behind it (barrier, loads): {bad}"


def test_first_mfma_never_waits_for_every_lds_read(heads):
    """LDS reads complete in order: lgkmcnt(0) in front of the first MFMA is a wait for the k-chunks read ahead too."""
    bad = [h["barrier"] for h in heads if h["mfma"] and h["lgkmcnt"] == 0]
    assert not bad, f"lgkmcnt(0) in front of the first MFMA behind the barriers at {bad}"
    assert all(h["lgkmcnt"] is not None for h in heads if h["mfma"]), "every head reads its operands behind the barrier"


def test_vmcnt_zero_only_for_the_youngest_load(heads):
    """vmcnt(0) in front of a first MFMA drains the fragments prefetched for later layers, unless the fragment the MFMA
    reads is the youngest load issued."""
    bad = [(h["barrier"], h["youngest_load"]) for h in heads if h["mfma"] and h["vmcnt"] == 0 and not h["youngest_feeds_mfma"]]
    assert not bad, f"vmcnt(0) drains younger loads at the heads behind (barrier, youngest load): {bad}"


def test_scan_reads_a_head():
    """The scan on a hand-written loop: one barrier, a scalar load and an uncounted wait at the head."""
    import mlp_heads as mh
    asm = ["k:", ".LBB0_1:", "  s_barrier", "  s_load_dword s0, s[2:3], 0x0", "  ds_read_b128 v[0:3], v9",
           "  ds_read_b128 v[4:7], v9 offset:64", "  buffer_load_dwordx4 v[20:23], v8, s[4:7], 0 offen",
           "  s_waitcnt vmcnt(0) lgkmcnt(0)", "  v_mfma_f32_16x16x32_bf16 v[10:13], v[20:23], v[0:3], v[10:13]",
           "  s_cbranch_scc1 .LBB0_1", "  s_endpgm", ".Lfunc_end0:"]
    loop = mh.Loop(mh.kernel_body(asm, "k"))
    assert loop.barriers_per_step() == (1, 1)
    (h,) = mh.heads(loop)
    assert (h["ds_read"], h["vload"], h["sload"], h["lgkmcnt"], h["vmcnt"], h["lgkm_scalar"], h["youngest_feeds_mfma"]) == \
        (2, 1, 1, 0, 0, True, True)
