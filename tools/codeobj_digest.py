"""Digests of the gfx950 device code of a built library: the check that a change to the kernel sources left the code objects
as they were (a device helper is accepted only if they did).

An OBJECT digest is a function of the device code and its metadata only: every ELF section (``.text``, ``.rodata``, ``.note``
and the other program data) except the name tables, ``.symtab`` and ``.dynamic``, plus the symbol table as a sorted list of
(name, value, size, info).  clang's per-compile ``__hip_cuid_<hash>`` symbol is left out of that list: it changes with the
object path, not with the code, and its varying length moves the string tables, one word of ``.dynamic`` (the string-table
size) and one of ``.symtab`` -- the sections skipped here.

    python tools/codeobj_digest.py [lib.so ...]             one digest per code object (one per translation unit)
    python tools/codeobj_digest.py --kernels [lib.so]       one line per kernel: code size, sha of its bytes in .text, and the
                                                            figures of workoutdetector_amd.codeobj (vgpr, agpr, sgpr, vgpr / sgpr
                                                            spills, scratch, fixed LDS)
    python tools/codeobj_digest.py a.so b.so                only what differs between the two: the kernels (both lines) and the
                                                            objects whose digest differs; exit status 1 if anything does
"""
import hashlib
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from workoutdetector_amd.codeobj import _gfx950_elfs, kernel_metadata  # noqa: E402

SKIPPED = ('.dynsym', '.dynstr', '.strtab', '.hash', '.gnu.hash', '.symtab', '.dynamic')
FIGURES = (('vgpr', '.vgpr_count'), ('agpr', '.agpr_count'), ('sgpr', '.sgpr_count'), ('vspill', '.vgpr_spill_count'),
           ('sspill', '.sgpr_spill_count'), ('scratch', '.private_segment_fixed_size'), ('lds', '.group_segment_fixed_size'))


def _headers(elf: bytes):
    """[(name, section header)] of a 64-bit little-endian ELF, in section order."""
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from('<HHH', elf, 0x3A)
    heads = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + k * shentsize) for k in range(shnum)]
    names = elf[heads[shstrndx][4]:heads[shstrndx][4] + heads[shstrndx][5]]
    return [(names[h[0]:names.index(b'\0', h[0])].decode(), h) for h in heads]


def sections(elf: bytes):
    """[(name, bytes)] in section order (SHT_NOBITS sections have no bytes)."""
    return [(name, b'' if h[1] == 8 else elf[h[4]:h[4] + h[5]]) for name, h in _headers(elf)]


def symbols(elf: bytes):
    """Sorted [(name, value, size, info)] of ``.symtab``, without the ``__hip_cuid_*`` entry."""
    heads = _headers(elf)
    out = []
    for name, h in heads:
        if name != '.symtab':
            continue
        strtab = heads[h[6]][1]                                  # sh_link: its string table
        strs = elf[strtab[4]:strtab[4] + strtab[5]]
        for pos in range(h[4], h[4] + h[5], 24):
            st_name, info, _other, _shndx, value, size = struct.unpack_from('<IBBHQQ', elf, pos)
            sym = strs[st_name:strs.index(b'\0', st_name)].decode()
            if not sym.startswith('__hip_cuid_'):
                out.append((sym, value, size, info))
    return sorted(out)


def digest(elf: bytes) -> str:
    h = hashlib.sha256()
    for name, data in sections(elf):
        if name not in SKIPPED:
            h.update(name.encode() + b'\0' + struct.pack('<Q', len(data)) + data)
    h.update(repr(symbols(elf)).encode())
    return h.hexdigest()[:16]


def digests(lib_path: str):
    return [digest(elf) for elf in _gfx950_elfs(lib_path)]


def kernels(lib_path: str):
    """{demangled kernel name: 'size sha figures' line} of every kernel of the library."""
    code = {}
    for elf in _gfx950_elfs(lib_path):
        text = dict(_headers(elf))['.text']
        for sym, value, size, info in symbols(elf):
            if info & 0xF == 2:                                  # STT_FUNC
                start = text[4] + value - text[3]                # file offset of an address inside .text
                code[sym] = (size, hashlib.sha256(elf[start:start + size]).hexdigest()[:16])
    out = {}
    for name, r in kernel_metadata(lib_path).items():
        size, sha = code[r['.name']]
        out[name] = f'{size:>7} {sha} ' + ' '.join(f'{label}={r[key]}' for label, key in FIGURES)
    return out


if __name__ == '__main__':
    from workoutdetector_amd.build import LIB_PATH
    args = [a for a in sys.argv[1:] if a != '--kernels']
    if len(args) == 2:
        (a, b), differs = [kernels(path) for path in args], 0
        for name in sorted(set(a) | set(b)):
            if a.get(name) != b.get(name):
                differs += 1
                print(f'{name}\n  < {a.get(name, "(absent)")}\n  > {b.get(name, "(absent)")}')
        da, db = digests(args[0]), digests(args[1])
        objects = [i for i in range(max(len(da), len(db))) if da[i:i + 1] != db[i:i + 1]]
        for i in objects:
            print(f'object {i}: {"".join(da[i:i + 1]) or "(absent)"} != {"".join(db[i:i + 1]) or "(absent)"}')
        print(f'{differs} of {len(set(a) | set(b))} kernels and {len(objects)} of {max(len(da), len(db))} objects differ')
        sys.exit(1 if differs or objects else 0)
    for path in args or [LIB_PATH]:
        print(path)
        if '--kernels' in sys.argv:
            for name, line in sorted(kernels(path).items()):
                print(f'  {line}  {name}')
        else:
            for i, d in enumerate(digests(path)):
                print(f'  object {i}: {d}')
