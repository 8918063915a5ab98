"""Registers, scratch and static LDS of every kernel in a build's object files,
read from the gfx950 code objects' metadata (no GPU needed):

    python scripts/kernel_resources.py [objdir] > profiles/<name>.txt

objdir defaults to ponyc_amd/build/libgpuactor. One line per kernel:
object, kernel (demangled), VGPRs, AGPRs, SGPRs, scratch bytes, static LDS
bytes. A name past MAX_NAME characters (library templates) is cut and ends in
a hash of the whole name. Two builds' outputs diff line by line (a kernel a change must not touch
has to come out identical)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
ARCH = os.environ.get("PONYC_AMD_ARCH", "gfx950")
KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size"]
MAX_NAME = 96     # longer kernel names are cut (they run to kilobytes each)


def kernels(obj: str, tmp: str):
    # the device code objects are a bundle in the host object's .hip_fatbin section
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    # (with an output file of its own: objcopy otherwise rewrites its input)
    r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj,
                        os.path.join(tmp, "copy.o")], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(fat):
        return []
    r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                        f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}", f"--input={fat}", f"--output={co}"],
                       capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
        return []
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co],
                           capture_output=True, text=True, check=True).stdout
    # amdhsa.kernels: a list item per kernel ("  - .key: v", then "    .key: v";
    # its arguments' items are indented deeper)
    items, cur = [], None
    for line in notes.splitlines():
        m = re.match(r"^(  - | {4})(\.\w+):\s*(\S*)", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
            items.append(cur)
        if cur is not None:
            cur[m.group(2)] = m.group(3)
    return [(k[".name"], [int(k.get(key, 0)) for key in KEYS]) for k in items
            if ".name" in k and ".vgpr_count" in k]


def main():
    objdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "ponyc_amd", "build", "libgpuactor")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(os.listdir(objdir)):
            if f.endswith(".o"):
                rows += [(f, n, v) for n, v in kernels(os.path.join(objdir, f), tmp)]
    names = [n for _, n, _ in rows]
    import shutil
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    dem = names
    if filt and names:
        dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True,
                             check=True).stdout.splitlines()
    print("# object kernel vgpr agpr sgpr scratch_bytes static_lds_bytes")
    for (f, _, v), d in sorted(zip(rows, dem), key=lambda x: (x[0][0], x[1])):
        d = d.replace(" ", "")
        if len(d) > MAX_NAME:       # library templates (hipcub): the head and a hash of the whole name
            d = d[:MAX_NAME - 14] + "..#" + hashlib.sha1(d.encode()).hexdigest()[:12]
        print(f, d, *v)


if __name__ == "__main__":
    main()
