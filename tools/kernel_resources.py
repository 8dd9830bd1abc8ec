#!/usr/bin/env python3
"""Registers / scratch / static LDS of the compiled kernels, from the code object's metadata
(llvm-readelf --notes gwinferno_amd/_lib/gwi_kernels.hsaco).  Usage: python tools/kernel_resources.py [substring ...]

The timing tools import kernel_resources(pattern) for the table at the end of their reports."""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _metadata(hsaco):
    """(mangled name, VGPRs, SGPRs, static LDS bytes, scratch bytes) of every kernel of the code object; nothing where it or llvm-readelf
    is missing."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    if not readelf or not os.path.exists(hsaco):
        return []
    notes = subprocess.run([readelf, "--notes", hsaco], capture_output=True, text=True).stdout
    rows = []
    for k in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        g = lambda key: re.search(rf"\.{key}:\s+(\S+)", k).group(1)  # noqa: E731
        rows.append((g("name"), int(g("vgpr_count")), int(g("sgpr_count")), int(g("group_segment_fixed_size")), int(g("private_segment_fixed_size"))))
    return rows


def _label(mangled):
    """The kernel's own name without its namespaces and arguments, and its template arguments if it has any: ``moment_cov_kernel``, ``<8>``;
    ``hist_merge_kernel``, ``<true>``; ``cond_tile_kernel``, ``<4, false>``."""
    at, name = re.match(r"_ZN?|", mangled).end(), mangled
    while True:
        n = re.match(r"\d+", mangled[at:])
        if not n:
            break
        at += n.end() + int(n.group())
        name = mangled[at - int(n.group()):at]
    t = re.match(r"I((?:L[bi]\d+E)+)", mangled[at:])
    args = [d if kind == "i" else ("false", "true")[int(d)] for kind, d in re.findall(r"L([bi])(\d+)E", t.group(1))] if t else []
    return name, "<" + ", ".join(args) + ">" if args else ""


def kernel_resources(pattern, hsaco=None):
    """Sorted rows ``(kernel, VGPRs, SGPRs, static LDS bytes, scratch bytes)`` of the kernels whose name (``_label``) matches the regular
    expression ``pattern`` in full, templated ones with their argument (``moment_cov_kernel<8>``).  ``hsaco``: the code object beside the
    engine's library unless given."""
    if hsaco is None:
        sys.path.insert(0, ROOT)
        from gwinferno_amd import _native

        hsaco = os.path.join(os.path.dirname(_native.LIB_PATH), "gwi_kernels.hsaco")
    rows = []
    for mangled, *counts in _metadata(hsaco):
        name, template = _label(mangled)
        if re.fullmatch(pattern, name):
            rows.append((name + template, *counts))
    return sorted(rows)


def main():
    rows = _metadata(os.path.join(ROOT, "gwinferno_amd", "_lib", "gwi_kernels.hsaco"))
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.splitlines()
    want = sys.argv[1:]
    print(f"{'vgpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>6}  kernel")
    for (raw, v, s, lds, sc), name in zip(rows, names):
        name = name.replace("void gwi::", "").replace("(gwi::KArgs)", "").replace("(gwi::TailArgs)", "")
        if not want or any(w in name for w in want):
            print(f"{v:5d} {s:5d} {sc:8d} {lds:6d}  {name}")


if __name__ == "__main__":
    main()
