"""Register / LDS / occupancy table of the stiffness kernels as compiled for gfx950
(-Rpass-analysis=kernel-resource-usage).  usage: python tools/kernel_resources.py [extra hipcc flags]

``resource_rows(source)`` gives the same remarks for any source file of csrc/ (tools/cell_form.py reads the cell-form
kernel's through it)."""
import os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resource_rows(source="laplacian.hip", extra_flags=()):
    """{mangled kernel name: {remark key: value}} of one source file of pmg-dolfinx_amd/csrc, built as build() does."""
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
           "-shared", "-munsafe-fp-atomics", "-fno-gpu-rdc", *extra_flags, "-Rpass-analysis=kernel-resource-usage",
           "-o", "/dev/null", os.path.join(ROOT, "pmg-dolfinx_amd", "csrc", source)]
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
    return rows


HEADER = ("| kernel | VGPRs | SGPRs | spills V/S | scratch B/lane | LDS bytes | waves/SIMD (registers) |\n"
          "|---|---|---|---|---|---|---|")


def table_row(label, r):
    return (f"| {label} | {r.get('VGPRs')} | {r.get('TotalSGPRs')} | "
            f"{r.get('VGPRs Spill')}/{r.get('SGPRs Spill')} | {r.get('ScratchSize [bytes/lane]')} | "
            f"{r.get('LDS Size [bytes/block]')} | {r.get('Occupancy [waves/SIMD]')} |")


def main():
    rows = resource_rows("laplacian.hip", sys.argv[1:])
    GEO = {"0": "stored", "1": "affine", "2": "recomputed"}  # GEO_* of stiffness_layer.hpp
    print(HEADER)
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
        table.append(table_row(label, r))
    print("\n".join(sorted(table)))


if __name__ == "__main__":
    main()
