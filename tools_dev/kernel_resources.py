"""Per-kernel resource usage of a built library, read from its gfx950 code objects (no GPU needed):
    python tools_dev/kernel_resources.py <libscpose_hip.so> [name substring ...]
One line per kernel: VGPRs, AGPRs, SGPRs, scratch bytes per lane, static LDS bytes, code bytes, demangled name.
(profiles/refactor_m32p_resource_usage.txt is this table for conv_m32_kernel / conv_m32p_kernel, two builds side by side.)"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path, arch="gfx950"):
    """the device ELF images of every offload bundle in the file.  Uncompressed bundles only (what csrc/Makefile builds):
    a compressed bundle (--offload-compress, magic CCOB) is not unpacked, and table() refuses a file that yields no code object"""
    data = open(path, "rb").read()
    pos = data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if arch in triple and size:
                yield data[pos + off:pos + off + size]
        pos = data.find(MAGIC, pos + 1)


def kernels_of(elf):
    """{mangled name: dict(vgpr, agpr, sgpr, scratch, lds, code)} of one code object"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(elf)
        f.flush()
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], text=True)
        syms = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-s", "--wide", f.name], text=True)
    size = {}
    for line in syms.splitlines():
        w = line.split()
        if len(w) >= 8 and w[3] == "FUNC":
            size[w[7]] = int(w[2], 0)
    out, cur = {}, None
    keys = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".private_segment_fixed_size": "scratch",
            ".group_segment_fixed_size": "lds"}
    for line in notes.splitlines():
        m = re.match(r"^  - (\.\w+):", line)   # a new entry of amdhsa.kernels (its argument lists are indented deeper)
        if m:
            cur = {}
        m = re.match(r"^  [ -] (\.\w+):\s*(\S+)", line)
        if cur is None or not m:
            continue
        if m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2), 0)
        elif m.group(1) == ".name":
            cur["code"] = size.get(m.group(2), -1)
            out[m.group(2)] = cur
    return out


def table(path, filters=()):
    rows = {}
    for elf in code_objects(path):
        rows.update(kernels_of(elf))
    if not rows:
        raise SystemExit("%s: no uncompressed gfx950 code object found (compressed offload bundles are not supported)" % path)
    names = sorted(rows)
    filt = os.path.join(LLVM, "llvm-cxxfilt")   # beside llvm-readelf where the ROCm install ships it, else binutils' from PATH
    plain = subprocess.check_output([filt if os.path.exists(filt) else "c++filt"], input="\n".join(names), text=True).splitlines()
    res = {}
    for mangled, name in zip(names, plain):
        name = re.sub(r"^void ", "", name)
        if name.endswith(")"):   # drop the argument list: the parenthesis that closes at the end ("(anonymous namespace)" stays)
            depth, i = 0, len(name)
            while i > 0:
                i -= 1
                depth += (name[i] == ")") - (name[i] == "(")
                if depth == 0:
                    break
            name = name[:i]
        if not filters or any(f in name for f in filters):
            res[name] = rows[mangled]
    return res


COLS = ("vgpr", "agpr", "sgpr", "scratch", "lds", "code")

if __name__ == "__main__":
    t = table(sys.argv[1], sys.argv[2:])
    print("%5s %5s %5s %7s %6s %7s  kernel" % COLS)
    for name in sorted(t):
        print("%5d %5d %5d %7d %6d %7d  %s" % (tuple(t[name][c] for c in COLS) + (name,)))
