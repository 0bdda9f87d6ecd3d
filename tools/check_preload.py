#!/usr/bin/env python3
"""Kernarg preload length of every kernel of the BUILT library: how many dwords of the kernarg segment gfx950 delivers in user SGPRs
at wave launch (the Makefile's KERNARG_PRELOAD; csrc/decode_kernels.cuh, "kernel entry").  Unbundles the gfx950 code objects like
check_scratch.py and reads the kernel descriptors: the length is bits 6:0 of the 16-bit field at byte 58 of each <kernel>.kd symbol
(the AMDGPU metadata notes do not carry it).  usage: check_preload.py [path/to/lib.so] [--all]
Lists the decode-frame kernels (--all: every kernel) with the dword count of their leading arguments; exit code 1 if a frame kernel's
preload length differs from it.  tests/test_kernarg_preload.py runs it."""
import os, re, struct, subprocess, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_scratch

# the kernels one single-stream decode frame launches
FRAME_KERNELS = ("gemv_kernel", "attn_pred_kernel", "attn_decode_kernel", "sample_pred_wave_kernel", "sample_talker_wave_kernel",
                 "frame_begin_kernel", "embed_sum_kernel")
MAX_DWORDS = 14            # 16 user SGPRs minus the kernarg segment pointer


def descriptors(blob):
    """(mangled name, preload length) of every kernel descriptor of one ELF64 code object"""
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    out = []
    for name, typ, flags, addr, off, size, link, info, align, entsize in secs:
        if typ != 2:            # SHT_SYMTAB
            continue
        str_off = secs[link][4]
        for i in range(size // entsize):
            st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", blob, off + i * entsize)
            end = blob.index(b"\0", str_off + st_name)
            sym = blob[str_off + st_name:end].decode()
            if not sym.endswith(".kd") or st_shndx == 0 or st_shndx >= shnum:
                continue
            sec = secs[st_shndx]
            field, = struct.unpack_from("<H", blob, sec[4] + st_value - sec[3] + 58)
            out.append((sym[:-3], field & 0x7F))
    return out


def kernels(path):
    """[(demangled signature, preload length)] over every gfx950 code object embedded in the library"""
    ds = [d for blob in check_scratch.code_objects(path) for d in descriptors(blob)]
    names = subprocess.run(["c++filt"], input="\n".join(n for n, _ in ds), capture_output=True, text=True).stdout.split("\n")
    return [(n.replace("(anonymous namespace)::", ""), length) for n, (_, length) in zip(names, ds)]


def split_args(sig):
    """the parameter types of a demangled function signature"""
    depth, start, args = 0, None, []
    body = sig[:sig.rindex(")")]
    # the parameter list opens at the last '(' of nesting depth 0 counted from the right
    for i in range(len(body) - 1, -1, -1):
        c = body[i]
        depth += c in ")>"
        depth -= c in "(<"
        if depth < 0:
            start = i
            break
    depth, cur = 0, ""
    for c in body[start + 1:]:
        if c == "," and depth == 0:
            args.append(cur.strip()); cur = ""
            continue
        depth += c in "(<"
        depth -= c in ")>"
        cur += c
    if cur.strip():
        args.append(cur.strip())
    return args


def leading_dwords(sig):
    """dwords of the leading run of plain pointers and 32-bit scalars of a kernel's argument list (a pointer is 8-byte aligned: a hole
    in front of it counts); the run ends at the first other type or at the first argument that no longer fits into MAX_DWORDS"""
    n = 0
    for a in split_args(sig):
        if a.endswith("*"):
            end = (n + 1) // 2 * 2 + 2
        elif a in ("int", "float", "unsigned int"):
            end = n + 1
        else:
            break
        if end > MAX_DWORDS:
            break
        n = end
    return n


def frame_kernels(path):
    """[(signature, family, preload length, leading dwords)] of the decode-frame kernels"""
    out = []
    for sig, length in kernels(path):
        m = re.match(r"void fq3::(\w+)<", sig)
        if m and m.group(1) in FRAME_KERNELS:
            out.append((sig, m.group(1), length, leading_dwords(sig)))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = args[0] if args else os.path.join(root, "faster-qwen3-tts_amd", "lib", "libfq3hip.so")
    short = lambda s: re.sub(r"\(.*", "", s.replace("fq3::", "").replace("unsigned short", "bf16").replace("void ", ""))[:80]
    if "--all" in sys.argv:
        for sig, length in kernels(path):
            print(f"{short(sig):80s} preload={length:2d}")
    rows = frame_kernels(path)
    bad = 0
    for sig, fam, length, lead in rows:
        ok = length == lead and 0 < lead <= MAX_DWORDS
        bad += not ok
        print(f"{short(sig):80s} preload={length:2d} leading={lead:2d}{'' if ok else '   MISMATCH'}")
    print(f"{len(rows)} decode-frame kernels, {bad} whose preload length is not the dword count of their leading arguments")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
