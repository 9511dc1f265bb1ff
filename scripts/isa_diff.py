#!/usr/bin/env python3
"""Compare the gfx950 code of named kernels between two builds of libsdfr.so.

    scripts/isa_diff.py OLD.so NEW.so [kernel-name-substring ...]

For every kernel whose demangled name contains one of the substrings (default: the
render's field / gather kernels) it compares the disassembled body and the kernel
descriptor's register, scratch and LDS sizes, and prints one line per kernel; with
--report NAME it also prints those sizes for kernels found only in NEW.so (e.g. a new
instantiation).  --rename OLD=NEW compares the kernel named OLD in OLD.so with the one
named NEW in NEW.so (full demangled names: a kernel that became a template instantiation
keeps its code under another symbol).  Exit status 1 when a compared kernel differs or is
missing.

CPU only: binutils c++filt and llvm-objcopy / llvm-objdump / llvm-readelf of the ROCm LLVM
($ROCM_PATH/llvm/bin, default /opt/rocm).
"""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
DEFAULT = ["field_r_kernel<sdfr::NgpNet>", "field_r_kernel<sdfr::FcNet>",
           "field_p_kernel<sdfr::SirenNet>", "field_merge_kernel", "ngp_encode_kernel"]
META = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_objects(so, tmp):
    """The gfx950 ELF of every translation unit in the library's .hip_fatbin."""
    fb = os.path.join(tmp, "fatbin")
    run(os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fb)
    data = open(fb, "rb").read()
    out, pos = [], data.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", data, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple:
                path = os.path.join(tmp, f"co{len(out)}_{os.path.basename(so)}.elf")
                open(path, "wb").write(data[pos + off:pos + off + size])
                out.append(path)
        pos = data.find(MAGIC, pos + 1)
    return out


def kernels(so, tmp):
    """demangled name -> (body lines without addresses, metadata dict)."""
    res = {}
    for co in code_objects(so, tmp):
        notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
        meta = {}
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            blk = ".agpr_count:" + blk
            sym = re.search(r"\.symbol:\s+'?([\w.$]+?)\.kd'?\s", blk)
            if sym:
                meta[sym.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                                      for k in META if re.search(rf"\.{k}:\s+(\d+)", blk)}
        dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn",
                  "--no-leading-addr", co)
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]* ?<([\w.$]+)>:$", line)
            if m:
                cur = m.group(1) if m.group(1) in meta else None
                if cur:
                    res[cur] = ([], meta[cur])
            elif cur and line.strip():
                # branch targets are printed with absolute addresses: keep the mnemonic
                # and operands, drop the "// 0000..." address comments
                res[cur][0].append(re.sub(r"\s*//.*$", "", line.strip()))
    # the s_nop fill between a kernel's last s_endpgm and the next symbol's alignment is
    # not code: it moves with the symbol order (a kernel that becomes a template
    # instantiation is emitted elsewhere in its section)
    for body, _ in res.values():
        while body and body[-1] in ("s_nop 0", "...") and "s_endpgm" in body:
            body.pop()
    names = run("c++filt", *res.keys()).splitlines() if res else []
    return {d: res[m] for m, d in zip(res.keys(), names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("names", nargs="*")
    ap.add_argument("--report", action="append", default=[])
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ko, kn = kernels(a.old, tmp), kernels(a.new, tmp)
    renamed = set()
    for pair in a.rename:
        old, new = pair.split("=", 1)
        if old in ko and new in kn and old not in kn:
            kn[old] = kn.pop(new)
            renamed.add(old)
            print(f"RENAMED   {old} -> {new}")
    bad = 0
    for sub in a.names or DEFAULT:
        hits = sorted(k for k in ko if sub in k)
        if not hits:
            print(f"MISSING   {sub}: not in {a.old}")
            bad += 1
        for k in hits:
            if k not in kn:
                print(f"MISSING   {k}: not in {a.new}")
                bad += 1
                continue
            same_body, same_meta = ko[k][0] == kn[k][0], ko[k][1] == kn[k][1]
            print(f"{'IDENTICAL' if same_body and same_meta else 'DIFFERENT'} {k}: "
                  f"{len(kn[k][0])} instructions, {kn[k][1]}")
            if not same_meta:
                print(f"          old descriptor: {ko[k][1]}")
            bad += not (same_body and same_meta)
    for sub in a.report:
        for k in sorted(k for k in kn if sub in k and k not in ko):
            print(f"NEW       {k}: {len(kn[k][0])} instructions, {kn[k][1]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
