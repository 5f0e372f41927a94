#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libfiunet_hip.so byte for byte.

    python tools/kernel_code_compare.py A.so B.so

For each library: every code object bundled for hipv4-amdgcn-amd-amdhsa--gfx950 in its .hip_fatbin section (one bundle
per translation unit) is taken apart and every kernel (a function symbol `name` with a kernel descriptor `name.kd`) is
listed with the bytes of its function.  Reported, and answered with exit status 1:

  * kernels that only one library has;
  * kernels a library has more than once (compiled into two units);
  * kernels whose bytes differ.

Whole functions are compared, as encoded: a refactor that only moves code between translation units leaves every one of
them unchanged.  Needs nothing but the two files (the ELF and bundle headers are read here).
"""
from __future__ import annotations

import struct
import sys
from collections import Counter

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
STT_FUNC, STT_OBJECT = 2, 1


class Elf:
    """The little of a 64-bit little-endian ELF image this tool needs: sections by name, the symbol table."""

    def __init__(self, data: bytes, what: str):
        if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
            raise ValueError(f"{what}: not a 64-bit little-endian ELF image")
        self.data = data
        shoff, = struct.unpack_from("<Q", data, 0x28)
        shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
        self.sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
        # (name, type, flags, addr, offset, size, link, info, addralign, entsize)
        strtab = self.sections[shstrndx]
        self.names = [self._str(strtab, s[0]) for s in self.sections]

    def _str(self, strtab, off: int) -> str:
        start = strtab[4] + off
        return self.data[start:self.data.index(b"\0", start)].decode()

    def section(self, name: str) -> bytes:
        s = self.sections[self.names.index(name)]
        return self.data[s[4]:s[4] + s[5]]

    def symbols(self):
        """-> (name, type, section index, value, size) of every entry of .symtab"""
        if ".symtab" not in self.names:
            return
        s = self.sections[self.names.index(".symtab")]
        strtab = self.sections[s[6]]
        for off in range(s[4], s[4] + s[5], 24):
            name, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", self.data, off)
            yield self._str(strtab, name), info & 15, shndx, value, size

    def bytes_at(self, shndx: int, value: int, size: int) -> bytes:
        s = self.sections[shndx]
        start = s[4] + value - s[3]
        return self.data[start:start + size]


def code_objects(fatbin: bytes, what: str):
    """The gfx950 code objects of a .hip_fatbin section: its bundles follow each other, each padded to a page."""
    pos, found = fatbin.find(BUNDLE_MAGIC), []
    if pos < 0:
        raise ValueError(f"{what}: no offload bundle in .hip_fatbin (a compressed bundle is not read)")
    while pos >= 0:
        n, = struct.unpack_from("<Q", fatbin, pos + len(BUNDLE_MAGIC))
        at = pos + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, at)
            triple = fatbin[at + 24:at + 24 + tlen].decode()
            at += 24 + tlen
            if triple == TARGET and size:
                found.append(fatbin[pos + off:pos + off + size])
        pos = fatbin.find(BUNDLE_MAGIC, at)
    return found


def kernels(path: str):
    """-> ([(kernel name, bytes of its function)] over every gfx950 code object of the library, number of code objects)"""
    with open(path, "rb") as f:
        lib = Elf(f.read(), path)
    if ".hip_fatbin" not in lib.names:
        raise ValueError(f"{path}: no .hip_fatbin section")
    objs = code_objects(lib.section(".hip_fatbin"), path)
    out = []
    for k, blob in enumerate(objs):
        co = Elf(blob, f"{path}: code object {k}")
        syms = list(co.symbols())
        descriptors = {name[:-3] for name, typ, *_ in syms if typ == STT_OBJECT and name.endswith(".kd")}
        for name, typ, shndx, value, size in syms:
            if typ == STT_FUNC and name in descriptors:
                out.append((name, co.bytes_at(shndx, value, size)))
    return out, len(objs)


def compare(path_a: str, path_b: str, out=sys.stdout) -> int:
    problems = 0
    tables = []
    for path in (path_a, path_b):
        ks, nobj = kernels(path)
        print(f"{path}: {len(ks)} kernels in {nobj} gfx950 code object(s), {sum(len(b) for _, b in ks)} bytes", file=out)
        if not ks:
            print(f"  no kernel found in {path}", file=out)
            problems += 1
        for name, count in sorted(Counter(n for n, _ in ks).items()):
            if count > 1:
                print(f"  {path}: {count} copies of {name}", file=out)
                problems += 1
        tables.append(dict(ks))
    a, b = tables
    for name in sorted(a.keys() - b.keys()):
        print(f"  only in {path_a}: {name}", file=out)
        problems += 1
    for name in sorted(b.keys() - a.keys()):
        print(f"  only in {path_b}: {name}", file=out)
        problems += 1
    for name in sorted(a.keys() & b.keys()):
        if a[name] != b[name]:
            first = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
            print(f"  differs: {name} ({len(a[name])} / {len(b[name])} bytes, first difference at byte {first})", file=out)
            problems += 1
    print("identical kernel code" if not problems else f"{problems} difference(s)", file=out)
    return 1 if problems else 0


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    return compare(argv[1], argv[2])


if __name__ == "__main__":
    sys.exit(main(sys.argv))
