"""Register table of a HIP source file's gfx950 kernels, from the assembly metadata (no GPU needed):
  hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only FILE.hip -o FILE.s && python tools/kernel_regs.py FILE.s
One line per kernel: demangled name, VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, static LDS bytes, scratch bytes."""
import re
import subprocess
import sys

text = open(sys.argv[1]).read()
rows = []
for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
    blk = ".agpr_count:" + blk

    def f(key):
        m = re.search(r"\." + key + r":\s*(\S+)", blk)
        return m.group(1) if m else "?"

    rows.append((f("name"), f("vgpr_count"), f("agpr_count"), f("sgpr_count"), f("vgpr_spill_count"), f("sgpr_spill_count"),
                 f("group_segment_fixed_size"), f("private_segment_fixed_size")))
names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
print("kernel | vgpr | agpr | sgpr | vgpr_spill | sgpr_spill | lds_bytes | scratch_bytes")
for r, n in sorted(zip(rows, names), key=lambda t: t[1]):
    print(" | ".join((re.sub(r"^void |\(.*$", "", n),) + r[1:]))
