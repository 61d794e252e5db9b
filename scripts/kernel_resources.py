#!/usr/bin/env python3
"""Register / scratch / LDS figures of every kernel in the gfx950 code objects of two builds' object files, side by
side (no GPU needed): the amdhsa metadata notes and the kernel symbol sizes.

    python scripts/kernel_resources.py PARENT_OBJ_DIR THIS_OBJ_DIR [name.o ...] > profiles/<tag>_kernel_resources.txt

The object directories are pychemkin_amd/_lib/obj of the two builds (same flags, same source lists).  Exit status 1
if a kernel present in both builds differs in any figure."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FIELDS = (".sgpr_count", ".vgpr_count", ".agpr_count", ".private_segment_fixed_size", ".sgpr_spill_count",
          ".vgpr_spill_count", ".group_segment_fixed_size")


def code_object(obj, tmp):
    fat = os.path.join(tmp, "fat.bin")
    co = os.path.join(tmp, "dev.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "x.o")], check=True,
                   capture_output=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}", f"--output={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
    return co


def kernels(obj):
    """{demangled kernel name: (sgpr, vgpr, agpr, scratch, sgpr spills, vgpr spills, static LDS, code bytes)}"""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
        syms = subprocess.run([f"{LLVM}/llvm-readelf", "-sW", co], capture_output=True, text=True, check=True).stdout
    size = {}
    for line in syms.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC":
            size[p[7]] = int(p[2], 0)
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        vals = tuple(int(re.search(re.escape(f) + r":\s+(\d+)", blk).group(1)) for f in FIELDS)
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip()
        dem = re.sub(r"^void ", "", dem)
        dem = re.sub(r"\(anonymous namespace\)::|ckmi::", "", dem)
        dem = re.sub(r"\)\(.*$|\(.*$", "", dem) if not dem.startswith("(") else dem
        out[dem] = vals + (size.get(name, 0),)
    return out


def main():
    a_dir, b_dir = sys.argv[1:3]
    names = sys.argv[3:] or sorted(f for f in os.listdir(b_dir) if f.endswith(".o"))
    print("# SGPRs / VGPRs / AGPRs / scratch bytes per lane / SGPR spills / VGPR spills / static LDS bytes / code bytes of")
    print("# every kernel, parent -> this tree: the amdhsa metadata and the kernel symbol sizes of the gfx950 code objects")
    print("# inside the two builds' own objects (same flags, same source lists).")
    moved = 0
    for f in names:
        try:
            a, b = kernels(os.path.join(a_dir, f)), kernels(os.path.join(b_dir, f))
        except subprocess.CalledProcessError:
            continue  # a host-only object: no device code
        print(f"## {f}: {len(a)} kernels -> {len(b)} kernels")
        for k in sorted(set(a) | set(b)):
            fa = " / ".join(map(str, a[k])) if k in a else "(new)"
            fb = " / ".join(map(str, b[k])) if k in b else "(gone)"
            tag = "same" if a.get(k) == b.get(k) else ("NEW" if k not in a else ("GONE" if k not in b else "CHANGED"))
            moved += tag in ("CHANGED", "GONE")
            print(f"{k:<60} {fa}  ->  {fb}  {tag}")
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
