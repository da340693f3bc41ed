#!/usr/bin/env python3
"""Which kernels of two builds of libgptq_mi355x.so differ?  (CPU only: no GPU is touched.  tools/isa_same.py compares two hipcc -S outputs of ONE translation
unit; this one compares whole built libraries, every code object.)

    python tools/isa_same_lib.py PARENT.so HEAD.so [--expect SUBSTR ...] > profiles/NAME.log

Both libraries are unbundled with the ROCm LLVM tools (as tests/test_kernel_resources.py does), every gfx950 code object is disassembled, and the
instruction text of every kernel (mnemonic + operands; the address / encoding comment of each line is dropped, so that a kernel that merely moved inside
its code object compares equal) is compared by symbol, together with its metadata (registers, LDS, scratch, kernarg bytes).  Prints the counts, every
kernel that was added / removed / changed with its old and new resources, and -- with --expect -- fails (exit 1) when a changed kernel's name contains none
of the given substrings or a substring matches no changed kernel."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size")


def kernels(so):
    """name -> (sha1 of the instruction text, instruction count, {metadata})"""
    objcopy, bundler, readelf, objdump = (os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"))
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([objcopy, f"--dump-section=.hip_fatbin={fat}", so, os.path.join(d, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, a in enumerate(starts):
            part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"co{i}.o")
            open(part, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            r = subprocess.run([bundler, "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            meta = {}
            for ent in re.split(r"\n  - ", subprocess.run([readelf, "--notes", co], capture_output=True, text=True).stdout):
                nm = re.search(r"\.name:\s+(\S+)", ent)
                if nm:
                    meta[nm.group(1)] = {k: int(m.group(1)) for k in META if (m := re.search(rf"\.{k}:\s+(\d+)", ent))}
            cur, text = None, {}
            for line in subprocess.run([objdump, "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    cur = m.group(1)
                    text[cur] = []
                elif cur and line.startswith("\t"):
                    text[cur].append(re.sub(r"\s*//.*$", "", line).strip())
            for name, ins in text.items():
                if name in meta:
                    out[name] = (hashlib.sha1("\n".join(ins).encode()).hexdigest(), len(ins), meta[name])
    return out


def demangle(names):
    import shutil
    tool = next((t for t in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if not tool or not names:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    d = r.stdout.splitlines() if r.returncode == 0 and len(r.stdout.splitlines()) == len(names) else list(names)
    return dict(zip(names, d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("head")
    ap.add_argument("--expect", nargs="*", default=None, help="substrings of the (demangled) names of the kernels that may -- and must -- change")
    a = ap.parse_args()
    P, H = kernels(a.parent), kernels(a.head)
    added, removed = sorted(set(H) - set(P)), sorted(set(P) - set(H))
    changed = sorted(n for n in set(P) & set(H) if P[n][0] != H[n][0])
    meta_only = sorted(n for n in set(P) & set(H) if P[n][0] == H[n][0] and P[n][2] != H[n][2])
    dm = demangle(added + removed + changed + meta_only)
    print(f"kernels: parent {len(P)}, head {len(H)}; added {len(added)}, removed {len(removed)}, instruction text changed {len(changed)}, "
          f"metadata only changed {len(meta_only)}, identical {len(set(P) & set(H)) - len(changed) - len(meta_only)}")
    for n in added:
        print(f"ADDED    {dm[n]}  {H[n][1]} instructions  {H[n][2]}")
    for n in removed:
        print(f"REMOVED  {dm[n]}  {P[n][1]} instructions  {P[n][2]}")
    for n in changed:
        print(f"CHANGED  {dm[n]}\n    parent  {P[n][1]} instructions  {P[n][2]}\n    head    {H[n][1]} instructions  {H[n][2]}")
    for n in meta_only:
        print(f"METADATA {dm[n]}\n    parent  {P[n][2]}\n    head    {H[n][2]}")
    if a.expect is not None:
        touched = [dm[n] for n in added + removed + changed + meta_only]
        stray = [t for t in touched if not any(e in t for e in a.expect)]
        missing = [e for e in a.expect if not any(e in t for t in touched)]
        print(f"expected to change: {a.expect}; outside that set: {stray or 'none'}; expected but unchanged: {missing or 'none'}")
        if stray or missing:
            sys.exit(1)


if __name__ == "__main__":
    main()
