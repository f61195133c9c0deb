#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the library, kernel by kernel.

    python tools/device_code_diff.py A/libchronoclust_hip.so B/libchronoclust_hip.so [--renamed A_SYMBOL=B_SYMBOL ...]

A change that only moves host code must leave every kernel as it was.  For each library the gfx950 code object is taken
out of the .hip_fatbin section, disassembled, and cut into symbols; the per-kernel metadata (registers, LDS, scratch,
arguments) is read from the notes.  Three things differ legitimately between two builds of the same kernels and are
normalised: the __hip_cuid_* symbol (derived from the source path: ignored), addresses (host functions in another order
change the order of template instantiation and so the layout: the "// address: encoding" comments are dropped and the
comparison is per symbol, without the padding (s_nop, zeros) behind a kernel's last instruction - the last kernel of the section is
padded to its end, and which kernel that is follows the order), and the 32-bit literals of the s_add_u32 / s_addc_u32 pair
behind an s_getpc_b64 (the PC-relative address of a global).  --renamed: a kernel of A that B holds under another symbol (a template that gained a parameter changes the mangled name
of its instances): A's symbol takes B's name before the comparison.  Prints the counts and every symbol that differs; exit
status 1 on a difference."""
import os
import re
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, capture_output=True, text=True).stdout


def code_object(lib, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, tag + ".copy"))
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co)
    return co


def kernels_text(co):
    """symbol -> its instructions, one string (comments dropped, PC-relative literals masked)"""
    out, name, pc = {}, None, 0
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name is None or not line.startswith("\t"):
            continue
        ins = re.sub(r"\s+", " ", line.split("//")[0].strip())
        if ins.startswith("s_getpc_b64"):
            pc = 2
        elif pc and ins.startswith(("s_add_u32", "s_addc_u32")):
            ins = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <pcrel>", ins)
            pc -= 1
        else:
            pc = 0
        out[name].append(ins)
    for body in out.values():  # (padding behind a kernel's last instruction: it belongs to the layout)
        while body and body[-1] in ("s_nop 0", "..."):
            body.pop()
    return {k: "\n".join(v) for k, v in out.items()}


def kernels_meta(co):
    """kernel name -> its block of the amdhsa.kernels metadata (registers, LDS, scratch, arguments, ...)"""
    text = tool("llvm-readelf", "--notes", co)
    text = text[text.index("amdhsa.kernels:"):]
    text = text[:re.search(r"^amdhsa\.(target|version)", text, re.M).start()]
    out = {}
    for block in re.split(r"^  - (?=\.)", text, flags=re.M)[1:]:
        out[re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)] = block
    return out


def function_symbols(co):
    return sum(1 for line in tool("llvm-readelf", "-s", co).splitlines() if " FUNC " in line)


def main():
    args, renamed = sys.argv[1:], {}
    while "--renamed" in args:
        i = args.index("--renamed")
        old, new = args[i + 1].split("=")
        renamed[old] = new
        del args[i:i + 2]
    if len(args) != 2:
        sys.exit(__doc__)
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        cos = [code_object(lib, tmp, tag) for lib, tag in zip(args, "ab")]
        for what, read in (("instructions", kernels_text), ("metadata", kernels_meta)):
            a, b = read(cos[0]), read(cos[1])
            for old, new in sorted(renamed.items()):
                for suffix in ("", ".kd"):
                    if old + suffix in a:
                        a[new + suffix] = a.pop(old + suffix).replace(old, new)
                        print("  %s: A's %s compared as %s" % (what, old + suffix, new + suffix))
            print("%s: %d kernel symbols in A, %d in B" % (what, len(a), len(b)))
            for name in sorted(set(a) ^ set(b)):
                print("  only in %s: %s" % ("A" if name in a else "B", name))
                differ += 1
            for name in sorted(set(a) & set(b)):
                if a[name] != b[name]:
                    print("  %s differ: %s" % (what, name))
                    differ += 1
        print("function symbols of the code objects: %d in A, %d in B" % tuple(function_symbols(c) for c in cos))
    print("device code differs in %d places" % differ if differ else "device code identical, kernel by kernel")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
