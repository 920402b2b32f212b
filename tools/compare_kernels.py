"""Compare two gfx950 assembly listings kernel by kernel, by demangled name.

The listings come from hipcc with the flags of build() plus `--cuda-device-only -S` on the same source file of two
commits.  Per kernel: whether the instruction text agrees (comments and debug directives dropped, the function index
inside local branch labels left out), whether the `.amdhsa_kernel` resource block agrees, and the registers, scratch,
LDS and occupancy of both sides.

--rename 'REGEX=REPLACEMENT' (repeatable) rewrites the demangled names of both listings before they are matched, for a
change that adds a template parameter: --rename 'patch_kernel<(\d)=patch_kernel<double, \1' lets the parent's
prolong_patch_kernel<2, 3> meet the result's prolong_patch_kernel<double, 2, 3>.

usage: python tools/compare_kernels.py PARENT.s RESULT.s [--markdown] [--only SUBSTRING] [--rename REGEX=REPLACEMENT]"""
import re
import shutil
import subprocess
import sys


def demangle(names):
    try:
        tool = (shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
                or shutil.which("llvm-cxxfilt", path="/opt/rocm/lib/llvm/bin") or "c++filt")
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        # "void (anonymous namespace)::kernel<4, true>(double const*, ...)" -> "kernel<4, true>"
        short = [re.sub(r"^void ", "", o).replace("(anonymous namespace)::", "").rsplit("(", 1)[0] for o in out]
        return dict(zip(names, short))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """{name: (instruction lines, resource block lines, summary dict)}"""
    lines = open(path).read().splitlines()
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    found = {}
    for name in names:
        i = next(j for j, ln in enumerate(lines) if ln.startswith(name + ":")) + 1
        text, block, info = [], [], {}
        while not lines[i].strip().startswith(".amdhsa_kernel "):  # the function body
            s = lines[i].split(";")[0].strip()
            if s and not s.startswith((".loc", ".file", ".cfi", ".p2align", ".section")):
                text.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
            i += 1
        i += 1  # (the .amdhsa_kernel line carries the name only)
        while not lines[i].strip().startswith(".end_amdhsa_kernel"):  # its resource block
            block.append(lines[i].strip())
            i += 1
        while i < len(lines) and "-- Begin function" not in lines[i]:  # the summary comments behind it
            m = re.match(r";\s*(Occupancy|ScratchSize|NumVgprs|NumAgprs|TotalNumSgprs|LDSByteSize):\s*(\d+)",
                         lines[i].strip())
            if m:
                info[m.group(1)] = int(m.group(2))
            i += 1
        found[name] = (text, block, info)
    return found


def by_name(found, renames):
    """The kernels of one listing under their demangled, renamed names (the mangled one added where two collide)."""
    short = demangle(sorted(found))
    out = {}
    for mangled, kernel in found.items():
        name = short[mangled]
        for pattern, replacement in renames:
            name = re.sub(pattern, replacement, name)
        out[name + " " + mangled if name in out else name] = kernel
    return out


def main():
    argv = sys.argv[1:]
    markdown = "--markdown" in argv
    only, renames, args = "", [], []
    while argv:
        a = argv.pop(0)
        if a == "--only":
            only = argv.pop(0)
        elif a == "--rename":
            renames.append(argv.pop(0).split("=", 1))
        elif not a.startswith("--"):
            args.append(a)
    a, b = by_name(kernels(args[0]), renames), by_name(kernels(args[1]), renames)
    print(f"kernels: {len(a)} parent, {len(b)} result, {len(set(a) & set(b))} in both")
    for n in sorted(set(a) ^ set(b)):
        print(("only in parent: " if n in a else "only in result: ") + n)
    head = ["kernel", "text", "resources", "instructions", "VGPRs", "AGPRs", "SGPRs", "scratch", "LDS", "waves/SIMD"]
    if markdown:
        print("| " + " | ".join(head) + " |\n|" + "---|" * len(head))
    same = 0
    for n in sorted(set(a) & set(b)):
        if only not in n:
            continue
        (ta, ba, ia), (tb, bb, ib) = a[n], b[n]
        pair = lambda k: str(ia.get(k)) if ia.get(k) == ib.get(k) else f"{ia.get(k)} -> {ib.get(k)}"  # noqa: E731
        row = [n, "equal" if ta == tb else "differs", "equal" if ba == bb else "differs",
               str(len(ta)) if len(ta) == len(tb) else f"{len(ta)} -> {len(tb)}", pair("NumVgprs"), pair("NumAgprs"),
               pair("TotalNumSgprs"), pair("ScratchSize"), pair("LDSByteSize"), pair("Occupancy")]
        same += ta == tb and ba == bb
        print("| " + " | ".join(row) + " |" if markdown else "  ".join(row))
    print(f"{same} kernels with equal text and equal resource block")


if __name__ == "__main__":
    main()
