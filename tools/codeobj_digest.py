"""One digest per gfx950 code object of a built library, over every ELF section but the five that carry clang's per-compile
``__hip_cuid_<hash>`` symbol (it changes with the object path, not with the code): two libraries print the same list exactly
when their device code is the same, section by section.  A host-only change must leave the list as it was.

    python tools/codeobj_digest.py [libtsm_hip.so] [other.so ...]
"""
import hashlib
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from workoutdetector_amd.codeobj import _gfx950_elfs  # noqa: E402

SKIPPED = ('.dynsym', '.dynstr', '.strtab', '.hash', '.gnu.hash')


def sections(elf: bytes):
    """[(name, bytes)] of a 64-bit little-endian ELF, in section order (SHT_NOBITS sections have no bytes)."""
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from('<HHH', elf, 0x3A)
    heads = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + k * shentsize) for k in range(shnum)]
    names = elf[heads[shstrndx][4]:heads[shstrndx][4] + heads[shstrndx][5]]
    out = []
    for h in heads:
        name = names[h[0]:names.index(b'\0', h[0])].decode()
        out.append((name, b'' if h[1] == 8 else elf[h[4]:h[4] + h[5]]))
    return out


def digests(lib_path: str):
    out = []
    for elf in _gfx950_elfs(lib_path):
        h = hashlib.sha256()
        for name, data in sections(elf):
            if name not in SKIPPED:
                h.update(name.encode() + b'\0' + struct.pack('<Q', len(data)) + data)
        out.append(h.hexdigest()[:16])
    return out


if __name__ == '__main__':
    from workoutdetector_amd.build import LIB_PATH
    for path in sys.argv[1:] or [LIB_PATH]:
        print(path)
        for i, d in enumerate(digests(path)):
            print(f'  object {i}: {d}')
