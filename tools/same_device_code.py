#!/usr/bin/env python3
"""Do two builds hold the same gfx950 machine code?  For a move-only change of the kernel sources.

    python tools/same_device_code.py PARENT/build/obj NEW/build/obj

For every unit (`NAME.o`) present in both object directories: the gfx950 code object is unbundled from the object's
`.hip_fatbin` section (clang-offload-bundler of the ROCm LLVM directory), `.text` and `.rodata` are compared byte for byte
and the defined function / object symbols (kernels, their descriptors, device functions and tables) by name and size;
the unit id `__hip_cuid_*`, a hash of the compile, is ignored.  One line per unit with the section sizes; exit status 1 on
any difference.  Section bytes and symbol tables only: nothing is disassembled.
"""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def bundler() -> str:
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (os.path.join(rocm, "llvm", "bin", "clang-offload-bundler"), shutil.which("clang-offload-bundler")):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit("clang-offload-bundler not found (set ROCM_PATH)")


class Elf:
    """Sections and the symbol table of a little-endian ELF64 image."""

    def __init__(self, data: bytes):
        if data[:6] != b"\x7fELF\x02\x01":
            raise ValueError("not a little-endian ELF64 image")
        self.data = data
        shoff, = struct.unpack_from("<Q", data, 0x28)
        shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
        # (name offset, type, offset, size, link, entsize) of every section header
        self.sh = []
        for i in range(shnum):
            name, typ, _, _, off, size, link, _, _, entsize = struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize)
            self.sh.append((name, typ, off, size, link, entsize))
        strs = self.sh[shstrndx]
        self.names = [self._str(strs[2], s[0]) for s in self.sh]

    def _str(self, table_off: int, off: int) -> str:
        end = self.data.index(b"\0", table_off + off)
        return self.data[table_off + off:end].decode()

    def section(self, name: str) -> bytes:
        if name not in self.names:
            return b""
        _, typ, off, size, _, _ = self.sh[self.names.index(name)]
        return b"" if typ == 8 else self.data[off:off + size]       # 8: SHT_NOBITS

    def symbols(self) -> dict:
        """name -> (type, size) of the defined FUNC / OBJECT symbols of .symtab."""
        out = {}
        for _, typ, off, size, link, entsize in self.sh:
            if typ != 2:        # SHT_SYMTAB
                continue
            stroff = self.sh[link][2]
            for k in range(size // entsize):
                name, info, _, shndx, _, ssize = struct.unpack_from("<IBBHQQ", self.data, off + k * entsize)
                if shndx == 0 or (info & 15) not in (1, 2):      # undefined; neither STT_OBJECT nor STT_FUNC
                    continue
                n = self._str(stroff, name)
                if not n.startswith("__hip_cuid_"):
                    out[n] = ("object" if (info & 15) == 1 else "func", ssize)
        return out


def code_object(obj_path: str, tmp: str):
    """The gfx950 code object of a unit, or None for a unit of host code only."""
    with open(obj_path, "rb") as f:
        fat = Elf(f.read()).section(".hip_fatbin")
    if not fat:
        return None
    src, dst = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
    with open(src, "wb") as f:
        f.write(fat)
    subprocess.run([bundler(), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={src}", f"--output={dst}"], check=True)
    with open(dst, "rb") as f:
        return Elf(f.read())


def main(argv) -> int:
    if len(argv) != 3:
        raise SystemExit(__doc__)
    a_dir, b_dir = argv[1], argv[2]
    units = sorted(f for f in os.listdir(a_dir) if f.endswith(".o") and os.path.exists(os.path.join(b_dir, f)))
    if not units:
        raise SystemExit("no unit is present in both directories")
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            a, b = code_object(os.path.join(a_dir, u), tmp), code_object(os.path.join(b_dir, u), tmp)
            if a is None or b is None:
                bad += a is not b
                print(f"{u[:-2]:<16} " + ("no device code" if a is b else "DIFFERENT: device code in one build only"))
                continue
            notes = []
            for sec in (".text", ".rodata"):
                if a.section(sec) != b.section(sec):
                    notes.append(f"{sec} differs ({len(a.section(sec))} / {len(b.section(sec))} bytes)")
            sa, sb = a.symbols(), b.symbols()
            for n in sorted(set(sa) | set(sb)):
                if sa.get(n) != sb.get(n):
                    notes.append(f"symbol {n}: {sa.get(n)} / {sb.get(n)}")
            bad += bool(notes)
            print(f"{u[:-2]:<16} .text {len(a.section('.text')):>8}  .rodata {len(a.section('.rodata')):>6}  symbols {len(sa):>4}  "
                  + ("identical" if not notes else "DIFFERENT"))
            for n in notes[:20]:
                print("    " + n)
            if len(notes) > 20:
                print(f"    ... and {len(notes) - 20} more")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
