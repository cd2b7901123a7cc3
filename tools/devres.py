"""Device-only compile of csrc/*.hip, or of the sources named with --src (same flags as the
extension build), and a resource report (VGPRs, AGPRs, SGPRs, spills, private segment, LDS,
code size) for kernels whose name matches a pattern.
Usage: python tools/devres.py PATTERN [--src FILE.hip ...] [-DFLAG=V ...]"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigrad_amd.ops import build as B

LLVM = os.path.join(B.ROCM, "lib", "llvm", "bin")
pat, rest = sys.argv[1], sys.argv[2:]
srcs, extra = [], []
while rest:
    a = rest.pop(0)
    if a == "--src":
        while rest and not rest[0].startswith("-"):
            srcs.append(os.path.join(B.CSRC, os.path.basename(rest.pop(0))))
    else:
        extra.append(a)
srcs = srcs or [s for s in B.sources() if s.endswith(".hip")]
tmp = tempfile.mkdtemp(prefix="devres")
for src in srcs:
    co, elf = os.path.join(tmp, "devres.co"), os.path.join(tmp, "devres.elf")
    cmd = B._compile_cmd(src)
    cmd[cmd.index("-o") + 1] = co
    cmd = [c for c in cmd if c != "-c"] + ["--cuda-device-only"] + extra
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                    "--input=" + co, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--output=" + elf], check=True)
    run = lambda *a: subprocess.run(a, capture_output=True, text=True, check=True).stdout
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", elf)
    size = {f[7]: f[2] for f in (ln.split() for ln in
                                 run(os.path.join(LLVM, "llvm-readelf"), "-s", "-W", elf).splitlines())
            if len(f) >= 8 and f[3] == "FUNC"}
    for blk in notes.split("  - .agpr_count")[1:]:
        blk = ".agpr_count" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if not re.search(pat, name):
            continue
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, None])[1]
        print(os.path.basename(src), name[:90], "vgpr", g("vgpr_count"), "agpr", g("agpr_count"),
              "sgpr", g("sgpr_count"), "spill", g("vgpr_spill_count"), g("sgpr_spill_count"),
              "priv", g("private_segment_fixed_size"), "lds", g("group_segment_fixed_size"),
              "size", size.get(name))
