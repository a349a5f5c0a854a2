#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds kernel by kernel (for changes that only move code).

    hipcc --offload-arch=gfx950 --cuda-device-only -cuid=<fixed> -O3 -std=c++17 -fPIC -c x.hip -o <dir>/x.o
    python tools/gemm_codeobj_diff.py <parent dir> <new dir>

For every *.o in both directories: sha256 of the files; if they differ, the code object is taken out
of the offload bundle (clang-offload-bundler) and every kernel's machine code (its FUNC symbol's
bytes) and kernel descriptor (the 64-byte <kernel>.kd: VGPRs, SGPRs, LDS, scratch, hence occupancy)
are compared by symbol name, as are the device variables.  Exit status 1 if a kernel that both
builds have differs, or if the new build has a kernel the parent lacks.
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

BUNDLER = os.path.join(os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin"), "clang-offload-bundler")


def code_object(path):
    with tempfile.NamedTemporaryFile(suffix=".co") as t:
        subprocess.run([BUNDLER, "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + path, "--output=" + t.name], check=True)
        return open(t.name, "rb").read()


def symbols(elf):
    """{name: (type, bytes or size, address)} of the defined FUNC and OBJECT symbols of an ELF64 image"""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for name_, type_, _, _, off, size, link, _, _, entsize in secs:
        if type_ != 2:   # SHT_SYMTAB
            continue
        stroff = secs[link][4]
        for i in range(size // entsize):
            st_name, info, _, shndx, value, st_size = struct.unpack_from("<IBBHQQ", elf, off + i * entsize)
            kind = info & 15
            if kind not in (1, 2) or shndx == 0 or shndx >= shnum:   # OBJECT, FUNC; defined
                continue
            name = elf[stroff + st_name:elf.index(b"\0", stroff + st_name)].decode()
            _, stype, _, saddr, soff, _, _, _, _, _ = secs[shndx]
            body = st_size if stype == 8 else elf[soff + value - saddr:soff + value - saddr + st_size]   # 8: NOBITS
            if name.endswith(".kd"):   # kernel_code_entry_byte_offset: where the code lies, not what it is
                body = body[:16] + bytes(8) + body[24:]
            out[name] = ("FUNC" if kind == 2 else "OBJECT", body, value)
    return out


def descriptor(kd):
    """the resource fields of a kernel descriptor (LLVM AMDGPU usage, code object v3+)"""
    lds, scratch = struct.unpack_from("<II", kd, 0)
    rsrc1, = struct.unpack_from("<I", kd, 48)
    rsrc3, = struct.unpack_from("<I", kd, 44)
    return "vgpr_gran=%d sgpr_gran=%d accum_offset=%d lds=%d scratch=%d" % (
        rsrc1 & 63, (rsrc1 >> 6) & 15, ((rsrc3 & 63) + 1) * 4, lds, scratch)


def main(parent, new):
    bad = False
    for name in sorted(f for f in os.listdir(parent) if f.endswith(".o")):
        a, b = (open(os.path.join(d, name), "rb").read() for d in (parent, new))
        ha, hb = hashlib.sha256(a).hexdigest(), hashlib.sha256(b).hexdigest()
        if ha == hb:
            print("%-20s identical  %s" % (name, ha[:16]))
            continue
        sa, sb = symbols(code_object(os.path.join(parent, name))), symbols(code_object(os.path.join(new, name)))
        kernels = [k for k, v in sa.items() if v[0] == "FUNC"]
        kernels.sort(key=lambda k: sa[k][2])   # emission order
        same = [k for k in kernels if k in sb and sb[k][1] == sa[k][1] and sb[k + ".kd"][1] == sa[k + ".kd"][1]]
        differ = [k for k in kernels if k in sb and k not in same]
        gone = [k for k in sa if k not in sb and not k.endswith(".kd")]
        added = [k for k in sb if k not in sa and not k.endswith(".kd")]
        order = sorted((k for k in kernels if k in sb), key=lambda k: sb[k][2]) != [k for k in kernels if k in sb]
        print("%-20s differs    %s -> %s" % (name, ha[:16], hb[:16]))
        print("    kernels in both: %d, machine code and descriptor identical: %d%s" % (
            len(same) + len(differ), len(same), ", emitted in another order" if order else ""))
        for k in differ:
            print("    DIFFERS  %s\n      parent %s\n      new    %s" % (k, descriptor(sa[k + ".kd"][1]), descriptor(sb[k + ".kd"][1])))
        for k in gone:
            print("    only in parent: %s %s" % (sa[k][0], k))
        for k in added:
            print("    only in new:    %s %s" % (sb[k][0], k))
        others = [k for k, v in sa.items() if v[0] == "OBJECT" and not k.endswith(".kd") and k in sb and sb[k][1] != v[1]]
        for k in others:
            print("    DIFFERS  variable %s" % k)
        bad = bad or differ or others or any(sb[k][0] == "FUNC" for k in added)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
