#!/usr/bin/env python3
"""Do two builds of libaarmvs.so hold the same gfx950 kernels?  python tools/isa_same.py A.so B.so

For every kernel (a function symbol NAME with a descriptor symbol NAME.kd) in the gfx950 code
objects of both libraries, the raw bytes of the function and of its 64-byte kernel descriptor are
compared.  Only these: a code object's notes, symbol order and the padding between functions
follow the translation unit a kernel is built in, not the kernel.  For the same reason the
descriptor's bytes 16-23 are left out: they hold the distance from the descriptor to the
function's entry, which is layout.  Prints the kernels found in one library only, the kernels
whose bytes differ and the number of identical ones; exit status 0 only if the sets are equal
and nothing differs."""
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "aa-rmvsnet_amd"))
from aarmvs import isa  # noqa: E402


def kernels(lib):
    """{name: function bytes + descriptor bytes (without the entry offset)} over all code objects"""
    out = {}
    for co in isa.code_objects(lib):
        shoff, = struct.unpack_from("<Q", co, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", co, 0x3A)
        # (type, addr, offset, size, link) of every section
        secs = [struct.unpack_from("<4xI8xQQQI", co, shoff + i * shentsize) for i in range(shnum)]
        syms = {}
        for typ, _, off, size, link in secs:
            if typ != 2:   # SHT_SYMTAB
                continue
            stroff = secs[link][2]
            for p in range(off, off + size, 24):
                name, _, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", co, p)
                end = co.index(b"\0", stroff + name)
                if 0 < shndx < shnum:
                    start = secs[shndx][2] + value - secs[shndx][1]
                    syms[co[stroff + name:end].decode()] = co[start:start + ssize]
        for name, kd in syms.items():
            if name.endswith(".kd") and name[:-3] in syms:
                assert name[:-3] not in out, f"{lib}: two kernels named {name[:-3]}"
                out[name[:-3]] = syms[name[:-3]] + kd[:16] + kd[24:]
    return out


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    for lib, only in ((a, ka.keys() - kb.keys()), (b, kb.keys() - ka.keys())):
        for n in sorted(only):
            print(f"only in {lib}: {n}")
    differ = sorted(n for n in ka.keys() & kb.keys() if ka[n] != kb[n])
    for n in differ:
        print(f"differs: {n} ({len(ka[n])} / {len(kb[n])} bytes)")
    same = len(ka.keys() & kb.keys()) - len(differ)
    print(f"{len(ka)} kernels in {a}, {len(kb)} in {b}: {same} identical, {len(differ)} differ, "
          f"{len(ka.keys() ^ kb.keys())} in one library only")
    return 0 if same and ka.keys() == kb.keys() and not differ else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
