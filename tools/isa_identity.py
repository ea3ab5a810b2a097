#!/usr/bin/env python3
"""Is the device code of a refactor the parent's, instruction for instruction? (CPU only, no GPU.)

    git archive <parent> mpc_via_diffusion_model_amd/csrc include | tar -x -C /tmp/parent
    python tools/isa_identity.py /tmp/parent --work /tmp/isa [-o profiles/<name>.txt] [--rename REGEX=REPL] [files.hip ...]

Compiles each translation unit of both trees device-only to assembly with build.py's FLAGS and SOURCE_FLAGS, once as
the product and once with -DMPCD_PROF_LAYERS, splits the text per function symbol (instantiation order may differ:
basic-block labels lose their function index, comments are dropped), and compares, per symbol, the instruction text
together with the .amdhsa_* block and the kernel's metadata entry (registers, AGPRs, scratch, LDS). Exit status 1 if
anything differs.
"""
import argparse
import concurrent.futures as cf
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_via_diffusion_model_amd import build as B  # noqa: E402

DEFAULT = ["mlp_rw.hip", "mlp_x3.hip", "mlp_h2.hip", "mlp_sampler.hip", "mpcd_api.hip"]
LABEL = re.compile(r"(\.L)?(BB|func_begin|func_end|tmp)\d+(_?)")
BEGIN = re.compile(r"^\t\.(?:globl|protected)\t(\S+)\s*; -- Begin function")  # .protected: kernels with external linkage
STOP = re.compile(r"^\t(\.section\t\.text|\.text|\.type\t\S+,@object|\.amdgpu_metadata)")


def assemble(csrc, src, out, defines):
    cmd = [B.hipcc()] + B.FLAGS + B.SOURCE_FLAGS.get(src, []) + defines + ["--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr}")


def functions(path, rename=()):
    """symbol -> normalised text: the function, its kernel descriptor directives, its metadata entry.
    rename: (regex, replacement) pairs applied to the whole text first (a symbol whose mangled name changed)"""
    fn, cur = {}, None
    text = open(path).read()
    for pat, repl in rename:
        text = re.sub(pat, repl, text)
    lines = text.split("\n")
    meta = lines.index("\t.amdgpu_metadata") if "\t.amdgpu_metadata" in lines else len(lines)
    for ln in lines[:meta]:
        m = BEGIN.match(ln)
        if m:
            cur = fn.setdefault(m.group(1), [])
        elif STOP.match(ln):
            cur = None
        code = ln.split(";")[0].strip()  # comments (loop notes, implicit-defs, register statistics) are not code
        if cur is not None and code:
            cur.append(" ".join(LABEL.sub(r"\1\2\3", code).split()))
    entry = None
    for ln in lines[meta:]:
        if ln.startswith("  - ."):  # the next kernel's entry
            entry = []
        elif not ln.startswith("    "):
            entry = None
        if entry is not None:
            entry.append(ln)
            m = re.match(r"    \.name:\s+(\S+)", ln)
            if m:
                fn[m.group(1)].append(entry)  # filled as the entry's remaining lines arrive
    return {k: "\n".join(x if isinstance(x, str) else "\n".join(x) for x in v) for k, v in fn.items()}


def digest(fn):
    return hashlib.sha256("\n".join(k + "\n" + fn[k] for k in sorted(fn)).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", help="root of the parent commit's tree")
    ap.add_argument("files", nargs="*", default=DEFAULT)
    ap.add_argument("--work", required=True, help="directory for the assembly files (kept; a side is reused if present)")
    ap.add_argument("--reuse", action="store_true", help="do not recompile assembly files that exist")
    ap.add_argument("-o", "--out")
    ap.add_argument("-j", type=int, default=4)
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="rewrite the parent's assembly text before it is split (renamed symbols); repeatable")
    a = ap.parse_args()
    sides = {"parent": os.path.join(a.parent, "mpc_via_diffusion_model_amd", "csrc"), "new": B.CSRC}
    variants = {"product": [], "MPCD_PROF_LAYERS": ["-DMPCD_PROF_LAYERS"]}
    jobs = []
    for side, csrc in sides.items():
        for var, defs in variants.items():
            d = os.path.join(a.work, f"{side}_{var}")
            os.makedirs(d, exist_ok=True)
            for f in a.files:
                out = os.path.join(d, f.replace(".hip", ".s"))
                if not (a.reuse and os.path.exists(out)):
                    jobs.append((csrc, f, out, defs))
    with cf.ThreadPoolExecutor(max_workers=a.j) as ex:
        list(ex.map(lambda j: assemble(*j), jobs))
    rep, bad = [f"device code per function symbol, {B.ARCH}: parent vs new ({' '.join(B.FLAGS)} + SOURCE_FLAGS)"], 0
    for var in variants:
        rep.append(f"\n[{var}]")
        for f in a.files:
            p, n = (functions(os.path.join(a.work, f"{s}_{var}", f.replace(".hip", ".s")),
                              [r.split("=", 1) for r in a.rename] if s == "parent" else ()) for s in sides)
            same = sum(1 for k in p if k in n and p[k] == n[k])
            diff = sorted(k for k in set(p) | set(n) if p.get(k) != n.get(k))
            bad += len(diff)
            rep.append(f"{f}: functions parent {len(p)} new {len(n)} identical {same}\n  sha256 parent {digest(p)}\n  sha256 new    {digest(n)}")
            rep += [f"  DIFFERS: {k}" + ("" if k in p and k in n else " (one side only)") for k in diff]
    rep.append("\nresult: " + ("IDENTICAL" if not bad else f"{bad} functions differ"))
    text = "\n".join(rep) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
