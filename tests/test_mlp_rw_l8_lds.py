"""CPU check that Linear 8 of the 8-wave resident-weight MLP sampler (csrc/mlp_rw.hip, the bench's cfg2 kernel) no
longer loads its own weights while it runs: its trailing k-chunks are read from LDS, the others are issued in Linear 7's
slots and waited for in front of Linear 8's barrier. Read from the gfx950 code with tools/mlp_heads.py segments(), from
the built library or a device-only compile as tests/test_mlp_rw_heads.py does. Nothing runs on a GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "mpc_via_diffusion_model_amd", "libmpcd.so")
LLVM = "/opt/rocm/lib/llvm/bin"
W8P = 4  # k-chunks of Linear 8 the parent issued before the layer's barrier; the other 8 - W8P inside the layer


@pytest.fixture(scope="module")
def segs(tmp_path_factory):
    import mlp_heads as mh
    tmp = str(tmp_path_factory.mktemp("l8"))
    if os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        lines = mh.library_lines(LIB, tmp)
    else:
        lines = open(mh.compile_asm(os.path.join(tmp, "mlp_rw.s"))).read().splitlines()
    loop = mh.Loop(mh.kernel_body(lines))
    print(mh.segment_report(loop))
    return mh.segments(loop)


def _parent_l8_loads():
    """Linear 8's row of the parent's table (profiles/rw8_l8_lds_parent.txt, written by tools/mlp_heads.py)."""
    rows = open(os.path.join(ROOT, "profiles", "rw8_l8_lds_parent.txt")).read().split("segment  barrier@")[1].splitlines()[1:]
    seg, _, vload, mfma = (int(v) for v in rows[8].split()[:4])
    assert (seg, mfma) == (8, 48)
    return vload


def test_linear8_segment_loads_only_the_next_layers_fragments(segs):
    assert len(segs) == 14 and [s["mfma"] for s in segs[5:9]] == [48] * 4, [s["mfma"] for s in segs]
    l9, l10 = 6, 12  # Linear 9: 2 k-chunks x 3 planes of one n-tile; Linear 10: 4 k-chunks x 3 planes
    assert segs[8]["vload"] == l9 + l10, segs[8]
    assert segs[8]["vload"] == _parent_l8_loads() - 3 * (8 - W8P)


def test_no_vector_memory_wait_in_front_of_k_chunks_1_to_7(segs):
    bad = [w for w in segs[8]["vm_waits"] if 6 <= w[0] < 48]
    assert not bad, f"s_waitcnt vmcnt inside Linear 8 as (MFMAs before it, count, loads before it): {bad}"


def test_segments_on_a_snippet():
    """The scan on a hand-written loop of two segments: loads and vmcnt waits are counted per segment, and a wait is
    placed by the MFMAs issued before it."""
    import mlp_heads as mh
    mf = "  v_mfma_f32_16x16x32_bf16 v[10:13], v[20:23], v[0:3], v[10:13]"
    ld = "  buffer_load_dwordx4 v[20:23], v8, s[4:7], 0 offen"
    asm = ["k:", ".LBB0_1:", "  s_barrier", ld, ld, "  s_waitcnt vmcnt(1)", mf, "  s_waitcnt vmcnt(0) lgkmcnt(0)", mf,
           "  s_barrier", "  s_cbranch_scc0 .LBB0_2", mf, ld, "  s_waitcnt lgkmcnt(2)", ".LBB0_2:", "  s_cbranch_scc1 .LBB0_1",
           "  s_endpgm", ".Lfunc_end0:"]
    a, b = mh.segments(mh.Loop(mh.kernel_body(asm, "k")))
    assert (a["vload"], a["mfma"], a["vm_waits"]) == (2, 2, [(0, 1, 2), (1, 0, 2)])
    assert (b["vload"], b["mfma"], b["vm_waits"]) == (1, 1, []), "the path with the MFMA, not the branch round it"
    assert re.search(r"^\s+0\s+\d+\s+2\s+2\s+\(0,1,2\) \(1,0,2\)$", mh.segment_report(mh.Loop(mh.kernel_body(asm, "k"))), re.M)
