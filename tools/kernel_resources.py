#!/usr/bin/env python3
"""Before / after table of the register, scratch, LDS and occupancy figures of the kernels of two trees.

Compile the kernels of two trees with the library's flags plus the resource remarks, device only (no GPU needed):

    hipcc <build.py FLAGS + SOURCE_FLAGS> --cuda-device-only -Rpass-analysis=kernel-resource-usage \\
          -c mpc_via_diffusion_model_amd/csrc/mlp_rw.hip -o /dev/null 2> before/rw.txt      (and mlp_x3.hip, ...)

    python tools/kernel_resources.py before/ after/ > profiles/<name>.txt

Every kernel of both sets is listed; a kernel whose scratch is not 0, or whose occupancy / scratch / LDS differs
between the two, is marked and the exit status is 1."""
import glob
import os
import re
import subprocess
import sys

FIELDS = (("SGPRs", "TotalSGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("scratch", "ScratchSize [bytes/lane]"),
          ("occ", "Occupancy [waves/SIMD]"), ("LDS", "LDS Size [bytes/block]"))


def parse(folder):
    out = {}
    for path in sorted(glob.glob(os.path.join(folder, "*.txt"))):
        name = None
        for line in open(path, errors="replace"):
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                out[name] = {}
                continue
            m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
            if m and name:
                out[name][m.group(1).strip()] = int(m.group(2))
    return out


def short(mangled):
    """mlp_rw_kernel<32, 16, true, 32, 8> from the Itanium name"""
    m = re.search(r"(mlp_\w+?_kernel)I(.*?)EEv", mangled)
    if not m:
        try:
            full = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip() or mangled
            return re.sub(r"\(\w+\)$", "", re.sub(r"^void |\(anonymous namespace\)::", "", full))  # kernel<arguments>
        except OSError:
            return mangled
    args = re.findall(r"L([ib])(\d+)E", m.group(2))
    return f"{m.group(1)}<{', '.join(('true' if v == '1' else 'false') if t == 'b' else v for t, v in args)}>"


def main():
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    if any("mlp_" in k for k in set(before) | set(after)):
        print("template arguments: mlp_rw_kernel / mlp_x3_kernel <H*d, sampler mode, context, rows, waves>")
    print("dynamic LDS is sized at launch (the static figure is 0); b = before, a = after\n")
    print(f"{'kernel':46s} " + " ".join(f"{h + ' b':>9s} {h + ' a':>9s}" for h, _ in FIELDS))
    changed = fresh = 0
    for k in sorted(set(before) | set(after), key=short):
        b, a = before.get(k), after.get(k)
        cells, marks = [], []
        for h, f in FIELDS:
            vb, va = (b or {}).get(f), (a or {}).get(f)
            cells.append(f"{'-' if vb is None else vb:>9} {'-' if va is None else va:>9}")
            if b and a and h in ("scratch", "occ", "LDS") and vb != va:
                marks.append(f"{h} changed")
            if h == "scratch" and va and not b:
                marks.append("new kernel with scratch")
            elif h == "scratch" and va and va == vb:
                marks.append("scratch as before")
        changed += any("changed" in m for m in marks)
        fresh += any("new kernel" in m for m in marks)
        print(f"{short(k):46s} " + " ".join(cells) + ("  <-- " + ", ".join(marks) if marks else ""))
    print(f"\n{len(after)} kernels after, {len(before)} before; {changed} existing kernels with a changed scratch / "
          f"occupancy / LDS, {fresh} new kernels with scratch")
    return 1 if changed or fresh else 0


if __name__ == "__main__":
    sys.exit(main())
