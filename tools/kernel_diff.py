"""Compare the gfx950 kernels of two builds of liba5x.so, kernel by kernel.

    python tools/kernel_diff.py OLD.so NEW.so

The code objects are taken out of the libraries' .hip_fatbin bundles (one bundle per
translation unit).  Per kernel symbol: equal / DIFFERENT (symbol size from llvm-readelf -s and
the llvm-objdump -d text without addresses and encodings), the instruction counts, and the
VGPR, SGPR, scratch, spill and LDS figures of the code object metadata, old -> new where they
differ.  It only diffs.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def tool(name, *args):
    exe = os.path.join(LLVM, name)
    if not os.path.exists(exe):
        exe = shutil.which(name) or exe
    return subprocess.run([exe, *args], check=True, capture_output=True, text=True).stdout


def code_objects(lib, arch, tmp):
    """The arch code object of every bundle in the library, written under tmp."""
    data = open(lib, "rb").read()
    out = []
    for n, m in enumerate(re.finditer(re.escape(MAGIC), data)):
        base = m.start()
        pos = base + len(MAGIC)
        count = int.from_bytes(data[pos:pos + 8], "little")
        pos += 8
        for _ in range(count):
            off, size, tlen = (int.from_bytes(data[pos + 8 * k:pos + 8 * k + 8], "little") for k in range(3))
            triple = data[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if triple.endswith(arch) and size:
                path = os.path.join(tmp, "%s.%d.co" % (os.path.basename(lib), n))
                with open(path, "wb") as f:
                    f.write(data[base + off:base + off + size])
                out.append(path)
    return out


def kernels(co):
    """name -> dict(size, text, meta) for every kernel of a code object."""
    meta = {}
    cur = None
    for line in tool("llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'")
        if key == "agpr_count":  # the first field of a kernel's record
            cur = {}
        if cur is None:
            continue
        if key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
                   "vgpr_spill_count", "sgpr_spill_count"):
            cur[key] = int(val)
        elif key == "name":
            cur["name"] = val
        elif key == "wavefront_size":  # the last field of a kernel's record
            if "name" in cur:
                meta[cur["name"]] = cur
            cur = None
    sizes = {}
    for line in tool("llvm-readelf", "-s", "-W", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            sizes[f[7]] = int(f[2])
    text = {}
    name = None
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line.strip())
        if m:
            name = m.group(1)
            text[name] = []
        elif name and line.strip():
            text[name].append(re.sub(r"\s*//.*$", "", line).strip())
    return {k: {"size": sizes.get(k, 0), "text": text.get(k, []), "meta": v} for k, v in meta.items()}


def load(lib, arch, tmp):
    out = {}
    for co in code_objects(lib, arch, tmp):
        out.update(kernels(co))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    arch = os.environ.get("A5X_OFFLOAD_ARCH", "gfx950")
    with tempfile.TemporaryDirectory() as tmp:
        old, new = load(sys.argv[1], arch, tmp), load(sys.argv[2], arch, tmp)
    fields = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("scratch", "private_segment_fixed_size"),
              ("vspill", "vgpr_spill_count"), ("sspill", "sgpr_spill_count"), ("lds", "group_segment_fixed_size"))
    ndiff = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%-9s %s" % ("only-old" if name in old else "only-new", name))
            ndiff += 1
            continue
        a, b = old[name], new[name]
        same = a["size"] == b["size"] and a["text"] == b["text"]
        ndiff += not same
        cols = ["insts %d" % len(a["text"]) if same else "insts %d -> %d" % (len(a["text"]), len(b["text"]))]
        for label, key in fields:
            x, y = a["meta"].get(key, 0), b["meta"].get(key, 0)
            cols.append("%s %d" % (label, x) if x == y else "%s %d -> %d" % (label, x, y))
        print("%-9s %s  %s" % ("equal" if same else "DIFFERENT", name, "  ".join(cols)))
    print("%d kernels, %d different" % (len(set(old) | set(new)), ndiff))


if __name__ == "__main__":
    main()
