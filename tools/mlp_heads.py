"""Layer heads of the resident-weight MLP sampler, read from its gfx950 assembly (static; nothing is run).

  python tools/mlp_heads.py [libmpcd.so | mlp_rw.s | objdump -d text]
                                              # without a file: cross-compiles csrc/mlp_rw.hip with the build's flags

A head is what a wave issues between the barrier that opens a layer and that layer's first MFMA: it stands on the
critical path 14 times per denoise step. For the step loop of mlp_rw_kernel<64, DDPM_CFG, ctx, 32, 8> (the bench's
cfg2 kernel) this follows the control flow from every s_barrier to the first MFMA it can reach (a path that reaches
the next barrier first belongs to waves without a tile in that layer) and prints, per head: LDS reads, vector loads,
scalar loads and VALU instructions issued, the waits met, the counts in force at the first MFMA, and whether the
youngest vector load before it (in program text, around the loop's back edge) is the fragment that MFMA reads.
The compiler lays the step out as more s_barrier instructions than a wave executes (waves 4-7 get a path of their own
through the 32-wide layers); barriers_per_step() counts them along the paths. tests/test_mlp_rw_heads.py asserts on
both.

A second table (segments()) lists, per barrier-to-barrier segment of a step, the vector loads and MFMAs issued and
every s_waitcnt vmcnt with its count and the MFMAs in front of it: a fragment load or a vector-memory wait inside a
layer shows there (tests/test_mlp_rw_l8_lds.py: Linear 8 has neither for its own weights).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGSHIP = r"mlp_rw_kernelILi64ELi0ELb1ELi32ELi8EE"  # <D0 = 64, MODE_DDPM_CFG, CTX, 32 rows, 8 waves>

_LABEL = re.compile(r"^([.\w$]+):")
_REGS = re.compile(r"\b([va])(?:\[(\d+):(\d+)\]|(\d+))")


def compile_asm(out):
    """csrc/mlp_rw.hip -> gfx950 assembly, device only, with the library's flags."""
    sys.path.insert(0, ROOT)
    from mpc_via_diffusion_model_amd import build as b
    subprocess.run([b.hipcc()] + b.FLAGS + b.SOURCE_FLAGS.get("mlp_rw.hip", []) +
                   ["--cuda-device-only", "-S", os.path.join(b.CSRC, "mlp_rw.hip"), "-o", out],
                   check=True, capture_output=True)
    return out


_OD_HEAD = re.compile(r"^([0-9a-f]+) <(\S+)>:")
_OD_INST = re.compile(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$")


def _objdump_body(lines, name):
    """kernel_body for `llvm-objdump -d` text: branch targets (<symbol+0xOFF>) become labels."""
    start = base = None
    for i, ln in enumerate(lines):
        m = _OD_HEAD.match(ln)
        if m and re.search(name, m.group(2)):
            start, base = i, int(m.group(1), 16)
            break
    if start is None:
        raise ValueError(f"no kernel matching {name}")
    insts, targets = [], set()
    for ln in lines[start + 1:]:
        if _OD_HEAD.match(ln):
            break
        m = _OD_INST.match(ln)
        if not m:
            continue
        text, off = m.group(1), int(m.group(2), 16) - base
        if text.startswith(("s_cbranch", "s_branch")):
            t = re.search(r"\+0x([0-9a-f]+)>", m.group(3))
            tgt = int(t.group(1), 16) if t else 0
            targets.add(tgt)
            text = f"{text.split()[0]} L{tgt:x}"
        insts.append((off, text))
    body = []
    for off, text in insts:
        if off in targets:
            body.append(("label", f"L{off:x}"))
        body.append(("inst", text))
    return body


def kernel_body(lines, name=FLAGSHIP):
    """[(kind, text)] of one kernel, kind 'label' or 'inst', comments and directives dropped. lines: hipcc -S
    assembly, or llvm-objdump -d of the code object."""
    if any(_OD_HEAD.match(ln) for ln in lines[:2000]):
        return _objdump_body(lines, name)
    start = None
    for i, ln in enumerate(lines):
        m = _LABEL.match(ln)
        if m and re.search(name, m.group(1)) and not m.group(1).endswith(".kd"):
            start = i
            break
    if start is None:
        raise ValueError(f"no kernel matching {name}")
    body = []
    for ln in lines[start + 1:]:
        s = ln.split(";")[0].strip()
        if not s:
            continue
        m = _LABEL.match(s)
        if m:
            if m.group(1).startswith(".Lfunc_end"):
                break
            body.append(("label", m.group(1)))
        elif not s.startswith("."):
            body.append(("inst", s))
    return body


def _is_branch(t):
    return t.startswith(("s_cbranch", "s_branch"))


class Loop:
    """The step loop (the backward branch that spans the most barriers, the kernel's end not inside its span) as
    instructions with successors. The back edge leads to the loop's first instruction; a branch out of the loop's text
    ends that path (a conditional one falls through)."""

    def __init__(self, body):
        at = {t: i for i, (k, t) in enumerate(body) if k == "label"}
        best = (0, 0, 0)
        for i, (k, t) in enumerate(body):
            if k != "inst" or not _is_branch(t):
                continue
            j = at.get(t.split()[-1])
            if j is None or j > i:
                continue
            n = sum(1 for kk, tt in body[j:i] if kk == "inst" and tt.startswith("s_barrier"))
            if any(kk == "inst" and tt.startswith("s_endpgm") for kk, tt in body[j:i]):
                continue  # the kernel's end laid out inside a backward branch's span: not the step loop
            if n > best[0]:
                best = (n, j, i)
        n, j, i = best
        if n == 0:
            raise ValueError("no loop with a barrier")
        self.inst, label_at = [], {}
        for k, t in body[j:i + 1]:
            if k == "label":
                label_at[t] = len(self.inst)
            else:
                self.inst.append(t)
        last = len(self.inst) - 1
        self.succ = []
        for k, t in enumerate(self.inst):
            s = []
            if _is_branch(t):
                tgt = label_at.get(t.split()[-1])
                if k == last:
                    s.append(0)
                elif tgt is not None:
                    s.append(tgt)
                if t.startswith("s_cbranch") and k < last:
                    s.append(k + 1)
            elif k < last:
                s.append(k + 1)
            self.succ.append(s)

    def barriers_per_step(self):
        """(fewest, most) barriers on a path from the loop's first instruction to its back edge."""
        n = len(self.inst)
        lo, hi, state = [None] * n, [None] * n, [0] * n  # state: 0 new, 1 on the walk's stack, 2 done
        stack = [(0, 0)]
        while stack:  # depth first, values in post-order; an edge to a node on the stack closes an inner loop: skipped
            k, e = stack.pop()
            nx = self.succ[k] if k != n - 1 else []
            if e == 0:
                state[k] = 1
            if e < len(nx):
                stack.append((k, e + 1))
                if state[nx[e]] == 0:
                    stack.append((nx[e], 0))
                continue
            own = 1 if self.inst[k].startswith("s_barrier") else 0
            done = [s for s in nx if state[s] == 2 and lo[s] is not None]
            if k == n - 1:
                lo[k] = hi[k] = own
            elif done:
                lo[k], hi[k] = own + min(lo[s] for s in done), own + max(hi[s] for s in done)
            state[k] = 2
        return lo[0], hi[0]


def _regset(operand):
    out = set()
    for f, lo, hi, one in _REGS.findall(operand):
        if one:
            out.add((f, int(one)))
        else:
            out.update((f, r) for r in range(int(lo), int(hi) + 1))
    return out


def _is_vload(t):
    return t.startswith(("buffer_load", "global_load", "flat_load", "scratch_load"))


def _is_sload(t):
    return t.startswith(("s_load", "s_buffer_load"))


def _wait(t):
    """{'vmcnt': n, 'lgkmcnt': n} of an s_waitcnt (a counter not named is not waited on)."""
    return {k: int(v) for k, v in re.findall(r"(vmcnt|lgkmcnt)\((\d+)\)", t)}


def heads(loop):
    """One dict per (barrier, first MFMA reachable from it), in program order of the barriers. Each instruction is
    walked once per barrier, so where paths rejoin in front of the MFMA the counts are those of one of them.
    lgkmcnt: the count of the last wait that had LDS reads or scalar loads of this head to wait for (the barrier's own
    wait left none outstanding); None: the MFMA waits for none. vmcnt: the smallest count waited for since the barrier."""
    inst, out = loop.inst, []
    for b in [i for i, t in enumerate(inst) if t.startswith("s_barrier")]:
        seen = set()
        stack = [(s, dict(ds_read=0, vload=0, sload=0, valu=0, branch=0, waits=[], lg_out=0, sl_out=0, lgkmcnt=None,
                          lgkm_scalar=False, vmcnt=None)) for s in loop.succ[b]]
        idle = False
        while stack:
            k, h = stack.pop()
            while True:
                if k in seen:
                    break
                seen.add(k)
                t = inst[k]
                if t.startswith("s_barrier"):
                    idle = True
                    break
                if t.startswith("v_mfma"):
                    ops = [o.strip() for o in t.split(None, 1)[1].split(",")]
                    srcs = _regset(ops[1]) | _regset(ops[2])
                    j, young = k - 1, None
                    for _ in range(len(inst)):
                        if _is_vload(inst[j % len(inst)]):
                            young = inst[j % len(inst)]
                            break
                        j -= 1
                    h = dict(h, barrier=b, mfma_at=k, mfma=t, youngest_load=young,
                             youngest_feeds_mfma=bool(young) and bool(_regset(young.split(None, 1)[1].split(",")[0]) & srcs))
                    out.append(h)
                    break
                if t.startswith(("ds_read", "ds_write")):
                    h["ds_read"] += t.startswith("ds_read")
                    h["lg_out"] += 1
                elif _is_sload(t):
                    h["sload"] += 1
                    h["lg_out"] += 1
                    h["sl_out"] += 1
                elif _is_vload(t):
                    h["vload"] += 1
                elif t.startswith("s_waitcnt"):
                    w = _wait(t)
                    h["waits"] = h["waits"] + [w]
                    if "lgkmcnt" in w and h["lg_out"] > w["lgkmcnt"]:
                        h["lgkmcnt"], h["lgkm_scalar"], h["lg_out"] = w["lgkmcnt"], h["sl_out"] > 0, w["lgkmcnt"]
                        if w["lgkmcnt"] == 0:
                            h["sl_out"] = 0
                    if "vmcnt" in w:
                        h["vmcnt"] = w["vmcnt"] if h["vmcnt"] is None else min(h["vmcnt"], w["vmcnt"])
                elif t.startswith("v_"):
                    h["valu"] += 1
                nx = loop.succ[k]
                if _is_branch(t):
                    h["branch"] += 1
                if not nx:
                    break
                for s in nx[1:]:
                    stack.append((s, dict(h)))
                k = nx[0]
        if idle:
            out.append(dict(barrier=b, mfma=None))
    return out


def segments(loop):
    """One dict per barrier-to-barrier segment of a step, in the order a wave with a tile in every layer runs them
    (segment k is Linear k's, the last one the final layer's and the update's): from the loop's first instruction to the
    first barrier, then from each barrier along the path with the most MFMAs to the next barrier (the other paths are
    those of waves without a tile). Per segment: vload, the vector loads issued; mfma, the MFMAs; vm_waits, every
    s_waitcnt with a vmcnt in the segment as (MFMAs issued before it, its count, vector loads issued in the segment
    before it)."""
    inst = loop.inst

    def walk(starts):
        best, ends = {}, []  # an instruction is walked again only by a path that brings more MFMAs to it
        stack = [(s, dict(vload=0, mfma=0, vm_waits=[])) for s in starts]
        while stack:
            k, g = stack.pop()
            while True:
                t = inst[k]
                if t.startswith("s_barrier"):
                    ends.append((k, g))
                    break
                if best.get(k, -1) >= g["mfma"] or g["mfma"] > len(inst):  # the bound: an inner loop with MFMAs
                    break
                best[k] = g["mfma"]
                if _is_vload(t):
                    g["vload"] += 1
                elif t.startswith("v_mfma"):
                    g["mfma"] += 1
                elif t.startswith("s_waitcnt") and "vmcnt" in _wait(t):
                    g["vm_waits"] = g["vm_waits"] + [(g["mfma"], _wait(t)["vmcnt"], g["vload"])]
                nx = loop.succ[k]
                if not nx:
                    break
                for s in nx[1:]:
                    stack.append((s, dict(g)))
                k = nx[0]
        return max(ends, key=lambda e: e[1]["mfma"]) if ends else None

    first = walk([0])
    out, b = [], first[0] if first else None
    while b is not None and b not in [s["barrier"] for s in out]:
        end = walk(loop.succ[b])  # the last segment runs round the back edge to the step's first barrier
        if end is None:
            break
        nb, g = end
        out.append(dict(g, barrier=b))
        b = nb
    return out


def segment_report(loop):
    rows = ["segment  barrier@  vload  mfma  vmcnt waits as (MFMAs before it, count, loads of the segment before it)"]
    for k, g in enumerate(segments(loop)):
        rows.append(f"{k:7d}  {g['barrier']:8d}  {g['vload']:5d}  {g['mfma']:4d}  " + " ".join(f"({m},{c},{v})" for m, c, v in g["vm_waits"]))
    return "\n".join(rows)


def report(loop):
    hs = heads(loop)
    lo, hi = loop.barriers_per_step()
    rows = [f"step loop: {len(loop.inst)} instructions, {lo}..{hi} barriers per step on a path "
            f"({sum(t.startswith('s_barrier') for t in loop.inst)} in text), {sum(_is_vload(t) for t in loop.inst)} vector loads, "
            f"{sum(t.startswith('v_mfma') for t in loop.inst)} MFMAs in text",
            "barrier@  mfma@  ds_read  vload  sload  valu  branch  at first MFMA         youngest load feeds it  waits since the barrier"]
    for h in hs:
        if h["mfma"] is None:
            rows.append(f"{h['barrier']:8d}  (a path reaches the next barrier without an MFMA: waves with no tile)")
            continue
        w = " ".join("/".join(f"{k[0]}{v}" for k, v in sorted(x.items())) for x in h["waits"])
        cnt = f"vmcnt({h['vmcnt']}) lgkmcnt({h['lgkmcnt']})".replace("(None)", "(-)")
        rows.append(f"{h['barrier']:8d}  {h['mfma_at']:5d}  {h['ds_read']:7d}  {h['vload']:5d}  {h['sload']:5d}  {h['valu']:4d}  "
                    f"{h['branch']:6d}  {cnt:21s} {str(h['youngest_feeds_mfma']):23s} {w}")
    return "\n".join(rows)


def library_lines(so, tmp):
    """Disassembly (llvm-objdump -d) of the gfx950 code object of a built libmpcd.so that holds the kernel."""
    import glob
    import shutil
    objdump = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-objdump")
    cp = os.path.join(tmp, "libmpcd.so")
    shutil.copy(so, cp)
    subprocess.run([objdump, "--offloading", cp], cwd=tmp, check=True, capture_output=True)
    for co in sorted(glob.glob(cp + ".*gfx950")):
        syms = subprocess.run([objdump, "-t", co], check=True, capture_output=True, text=True).stdout
        if re.search(FLAGSHIP, syms):
            return subprocess.run([objdump, "-d", co], check=True, capture_output=True, text=True).stdout.splitlines()
    raise ValueError(f"no gfx950 code object with {FLAGSHIP} in {so}")


def main():
    if len(sys.argv) > 1 and sys.argv[1].endswith(".so"):
        with tempfile.TemporaryDirectory() as d:
            lines = library_lines(sys.argv[1], d)
    elif len(sys.argv) > 1:
        lines = open(sys.argv[1]).read().splitlines()
    else:
        with tempfile.TemporaryDirectory() as d:
            lines = open(compile_asm(os.path.join(d, "mlp_rw.s"))).read().splitlines()
    loop = Loop(kernel_body(lines))
    print(report(loop))
    print(segment_report(loop))


if __name__ == "__main__":
    main()
