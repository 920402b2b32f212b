"""Register / LDS / occupancy table of the stiffness kernels as compiled for gfx950
(-Rpass-analysis=kernel-resource-usage).  usage: python tools/kernel_resources.py [extra hipcc flags]"""
import os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-munsafe-fp-atomics",
       "-fno-gpu-rdc", *sys.argv[1:], "-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null",
       os.path.join(ROOT, "pmg-dolfinx_amd", "csrc", "laplacian.hip")]
out = subprocess.run(cmd, capture_output=True, text=True).stderr
cur, rows = None, {}
for line in out.splitlines():
    m = re.search(r"remark: (.*?) \[-Rpass", line)
    if not m:
        continue
    k, _, v = m.group(1).partition(": ")
    if k == "Function Name":
        cur = v
        rows[cur] = {}
    elif cur:
        rows[cur][k.strip()] = v.strip()
GEO = {"0": "stored", "1": "affine", "2": "recomputed"}  # GEO_* of stiffness_layer.hpp
print("| kernel | VGPRs | SGPRs | spills V/S | scratch B/lane | LDS bytes | waves/SIMD (registers) |")
print("|---|---|---|---|---|---|---|")
table = []
for name, r in rows.items():
    m = re.search(r"stiffness_column_kernelILi(\d)ELi(\d)ELb(\d)", name)
    if m:
        label = f"stiffness_column_kernel<{m.group(1)}, {GEO[m.group(2)]}, nt={m.group(3)}>"
    else:
        m = re.search(r"stiffness_restrict_kernelILi(\d)ELi(\d)ELi(\d)ELb(\d)", name)
        if not m:
            continue
        label = f"stiffness_restrict_kernel<{m.group(1)}, {m.group(2)}, {GEO[m.group(3)]}, nt={m.group(4)}>"
    table.append(f"| {label} | {r.get('VGPRs')} | {r.get('TotalSGPRs')} | "
                 f"{r.get('VGPRs Spill')}/{r.get('SGPRs Spill')} | {r.get('ScratchSize [bytes/lane]')} | "
                 f"{r.get('LDS Size [bytes/block]')} | {r.get('Occupancy [waves/SIMD]')} |")
print("\n".join(sorted(table)))
