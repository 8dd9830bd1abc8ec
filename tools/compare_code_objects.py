#!/usr/bin/env python3
"""Do two gfx950 code objects hold the same device code?      python tools/compare_code_objects.py OLD NEW

The check a refactor of device code has to pass: every kernel keeps its instructions.  Two builds of the SAME source are not
byte-identical on this toolchain -- a symbol's name changes from one compilation to the next, and with it the name tables
.dynsym, .dynstr, .hash, .gnu.hash and .strtab -- so the files are compared by what they mean instead:

  * the disassembly, symbol by symbol and in order, without raw bytes, addresses and the trailing `//` comments;
  * the per-kernel metadata out of the notes (register counts, LDS, scratch, kernarg size, spills, ...);
  * the bytes of .text, .rodata and .note.

OLD and NEW are raw code objects (gwi_kernels.hsaco) or host libraries / objects that carry an offload bundle in .hip_fatbin
(libgwi_engine.so), whose gfx950 entry is taken out first.  Prints one line per comparison and, where the disassembly differs,
the first differing symbol with its first differing line; exits 1 on any difference."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SECTIONS = (".text", ".rodata", ".note")
KERNEL_KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size",
               ".kernarg_segment_align", ".wavefront_size", ".max_flat_workgroup_size", ".sgpr_spill_count", ".vgpr_spill_count", ".uses_dynamic_stack")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], capture_output=True, text=True, check=True).stdout


def sections_of(path):
    return set(re.findall(r"^\s*\[\s*\d+\]\s+(\S+)", tool("llvm-readelf", "-S", "-W", path), re.M))


def code_object(path, tmp, tag):
    """The raw code object behind `path`: the file itself, or the gfx950 entry of its offload bundle."""
    if ".hip_fatbin" not in sections_of(path):
        return path
    bundle, out = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".hsaco")
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + bundle, path)
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + out)
    return out


def symbols(path):
    """[(symbol, [instruction lines])] in the order of the file."""
    out = []
    for raw in tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", path).splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:", raw)
        if m:
            out.append((m.group(1), []))
        elif out:
            text = raw.split("//", 1)[0].strip()
            if text:
                out[-1][1].append(text)
    return out


def metadata(notes):
    """{kernel: {key: value}} out of the notes' amdhsa.kernels list."""
    entries, inside = [], False
    for raw in notes.splitlines():
        if not raw.startswith(" "):
            inside = raw.startswith("amdhsa.kernels:")
            continue
        m = re.match(r"^  (- |  )(\.\w+):\s*(.*)$", raw) if inside else None  # a kernel's own keys; those of its .args are indented further
        if not m:
            continue
        if m.group(1) == "- ":
            entries.append({})
        entries[-1][m.group(2)] = m.group(3)
    return {e[".name"]: {k: e.get(k) for k in KERNEL_KEYS} for e in entries}


def dump(path, section, tmp, tag):
    out = os.path.join(tmp, tag + section.replace(".", "_"))
    tool("llvm-objcopy", "--dump-section", section + "=" + out, path)
    with open(out, "rb") as f:
        return f.read()


def compare(old, new):
    differs = False

    def report(what, same, detail=""):
        nonlocal differs
        differs |= not same
        print(f"{what}: {'identical' if same else 'DIFFERENT'}{detail}")

    with tempfile.TemporaryDirectory(prefix="gwi_cmp_") as tmp:
        old, new = code_object(old, tmp, "old"), code_object(new, tmp, "new")
        a, b = symbols(old), symbols(new)
        first = next((n for n, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        report("disassembly", first is None, f" ({len(a)} code symbols, {sum(len(s[1]) for s in a)} lines)" if first is None else "")
        if first is not None:
            if first >= min(len(a), len(b)):
                print(f"  {len(a)} against {len(b)} symbols; the first without a partner: {(a + b)[first if len(a) > len(b) else len(a) + first][0]}")
            elif a[first][0] != b[first][0]:
                print(f"  symbol {first}: {a[first][0]} against {b[first][0]}")
            else:
                x, y = a[first][1], b[first][1]
                at = next((n for n, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                print(f"  first differing symbol: {a[first][0]} ({len(x)} against {len(y)} instructions), at instruction {at}:")
                print(f"    old: {x[at] if at < len(x) else '(end)'}\n    new: {y[at] if at < len(y) else '(end)'}")
                print(f"  {sum(p != q for p, q in zip(a, b))} of {len(a)} symbols differ")
        na, nb = tool("llvm-readelf", "--notes", old), tool("llvm-readelf", "--notes", new)
        ma, mb = metadata(na), metadata(nb)
        bad = [k for k in ma if ma[k] != mb.get(k)] + [k for k in mb if k not in ma]
        report("per-kernel metadata", not bad and len(ma) > 0, f" ({len(ma)} kernels)" if not bad else "")
        for k in bad[:1]:
            print(f"  first differing kernel: {k}")
            print("    " + ", ".join(f"{key} {ma.get(k, {}).get(key)} -> {mb.get(k, {}).get(key)}" for key in KERNEL_KEYS if ma.get(k, {}).get(key) != mb.get(k, {}).get(key)))
        report("whole notes text", na == nb)
        for s in SECTIONS:
            x, y = dump(old, s, tmp, "old"), dump(new, s, tmp, "new")
            at = next((n for n, (p, q) in enumerate(zip(x, y)) if p != q), None if len(x) == len(y) else min(len(x), len(y)))
            report(f"{s} bytes", at is None, f" ({len(x)})" if at is None else f" ({len(x)} against {len(y)} bytes, first at offset {at})")
    return differs


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(1 if compare(sys.argv[1], sys.argv[2]) else 0)
