#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, symbol by symbol (no GPU needed).

    python tools/kernel_diff.py OLD NEW [--match SUBSTRING ...] [--list-identical]
    python tools/kernel_diff.py --list BUILD [--match SUBSTRING ...]      the counts of one build's kernels, for kernels whose names changed

OLD / NEW: a library (libdrmnet_hip.so), an object file, or a directory of objects (csrc/_obj).  Every device code object inside them is
disassembled with the ROCm llvm-objdump; a kernel is IDENTICAL when its whole instruction text (mnemonics, registers, immediates, branch
offsets) is the same on both sides; the padding between its last instruction and the next symbol is not part of it.  For a kernel that differs: instructions on each side, and VGPRs, AGPRs, scratch bytes and the waves
per SIMD the register count allows, from the code object's metadata.  Exit status 1 when anything differs or exists on one side only.
"""
from __future__ import annotations

import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def llvm(tool: str) -> str:
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "llvm", "bin", tool)):
            return os.path.join(root, "llvm", "bin", tool)
    return tool


def code_objects(path: str, tmp: str):
    """paths of the amdgcn ELF images inside a host object / library (its .hip_fatbin bundles), or the file itself if it is one"""
    files = [path]
    if os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith((".o", ".so", ".co", ".hsaco")))
    out = []
    for f in files:
        fb = os.path.join(tmp, f"fb{len(out)}.bin")
        r = subprocess.run([llvm("llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", f, fb + ".copy"], capture_output=True)
        if os.path.exists(fb + ".copy"):
            os.remove(fb + ".copy")
        if r.returncode != 0 or not os.path.exists(fb):
            out.append(f)  # (a bare code object)
            continue
        d = open(fb, "rb").read()
        os.remove(fb)
        for m in re.finditer(re.escape(MAGIC), d):
            base = m.start()
            (n,) = struct.unpack_from("<Q", d, base + 24)
            o = base + 32
            for _ in range(n):
                off, size, ln = struct.unpack_from("<QQQ", d, o)
                tid = d[o + 24:o + 24 + ln].decode()
                o += 24 + ln
                if "amdgcn" in tid and size:
                    co = os.path.join(tmp, f"co{len(out)}.elf")
                    open(co, "wb").write(d[base + off:base + off + size])
                    out.append(co)
    return out


def kernels(path: str):
    """{symbol: (instruction lines, metadata dict)} of every kernel in the build at `path`"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(path, tmp):
            meta = {}
            notes = subprocess.run([llvm("llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
            for blk in re.split(r"\n  - (?=\.agpr_count|\.args)", notes):
                nm = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M)
                if nm:
                    meta[nm.group(1)] = {k: int(v) for k, v in re.findall(r"^\s+\.(vgpr_count|agpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", blk, re.M)}
            dis = subprocess.run([llvm("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True).stdout
            sym = None
            for line in dis.splitlines():
                m = re.match(r"^<(.+)>:$", line)
                if m:
                    sym = m.group(1)
                    if sym in meta:
                        res[sym] = ([], meta[sym])
                    else:
                        sym = None
                elif sym and line.startswith("\t"):
                    res[sym][0].append(line.split("//")[0].strip())
    for ins, _ in res.values():
        # what follows a kernel's last instruction is the section's padding up to the next symbol's alignment (s_nop, or zero bytes that
        # objdump prints as "..."): it belongs to the layout, which moves when a kernel is added after this one, not to the kernel
        while ins and ins[-1] in ("s_nop 0", "..."):
            ins.pop()
    return res


def waves(m) -> int:
    regs = (m.get("vgpr_count", 0) + 3) // 4 * 4 + m.get("agpr_count", 0)  # unified file: 512 per lane and SIMD, granule 8
    return min(8, 512 // max(8, (regs + 7) // 8 * 8))


def counts(ins, m) -> str:
    return (f"{len(ins)} instructions, {m.get('vgpr_count', 0)} VGPRs, {m.get('agpr_count', 0)} AGPRs, {m.get('sgpr_count', 0)} SGPRs, "
            f"{m.get('private_segment_fixed_size', 0)} B scratch, {waves(m)} waves/SIMD by registers")


def demangle(names):
    for tool in (llvm("llvm-cxxfilt"), "c++filt"):  # (whichever is installed; the mangled names otherwise)
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
        except FileNotFoundError:
            continue
        out = r.stdout.splitlines() if r.returncode == 0 else []
        if len(out) == len(names):
            return dict(zip(names, out))
    return {n: n for n in names}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old", nargs="?")
    ap.add_argument("new", nargs="?")
    ap.add_argument("--list", metavar="BUILD", help="print the counts of every kernel of this one build instead of comparing two")
    ap.add_argument("--match", action="append", default=[], help="only kernels whose demangled name contains this (repeatable)")
    ap.add_argument("--list-identical", action="store_true", help="print the identical kernels too, not only their count")
    a = ap.parse_args()
    if a.list:
        ks = kernels(a.list)
        for sym, name in demangle(sorted(ks)).items():
            if not a.match or any(s in name for s in a.match):
                print(f"{counts(*ks[sym])}  {name}")
        return 0
    if not a.old or not a.new:
        ap.error("OLD and NEW, or --list BUILD")
    ko, kn = kernels(a.old), kernels(a.new)
    names = demangle(sorted(set(ko) | set(kn)))
    same = diff = 0
    for sym, name in names.items():
        if a.match and not any(s in name for s in a.match):
            continue
        if sym not in ko or sym not in kn:
            print(f"ONLY IN {'NEW' if sym in kn else 'OLD'}  {name}")
            diff += 1
        elif ko[sym][0] == kn[sym][0]:
            same += 1
            if a.list_identical:
                print(f"identical  {name}")
        else:
            diff += 1
            print(f"DIFFERENT  {name}")
            for tag, (ins, m) in (("old", ko[sym]), ("new", kn[sym])):
                print(f"    {tag}: {counts(ins, m)}")
    print(f"{same} identical, {diff} different")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
