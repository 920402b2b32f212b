"""Generate tests/golden/mt_uniform_golden.json: the start vector of the AMG set-up's power method,
``std::uniform_real_distribution<double>(0.5, 1.0)`` drawn from ``std::mt19937_64(12345)``
(``csrc/amg.hip``, ``lambda_max_jacobi``), as the C++ standard library of the build compiler produces it.

Run once (``python tests/golden/make_mt_uniform_fixture.py``, needs a C++ compiler as ``$CXX`` or ``c++``).  The
fixture is data: single draws by index, printed with 17 significant digits, and the running sum of the first
100 000.  ``oracle.amg_oracle.mt_uniform_half_one`` -- a pure-Python MT19937-64 -- must reproduce them bit for
bit (tests/test_amg_oracle.py)."""
import json
import os
import subprocess
import tempfile

COUNT = 100000
INDICES = [0, 1, 2, 3, 4, 311, 312, 313, 623, 624, 4095, 4096, 9260, 99999]  # both sides of the state refills

SRC = r"""
#include <cstdio>
#include <random>
int main(int argc, char** argv)
{
  std::mt19937_64 gen(12345);
  std::uniform_real_distribution<double> U(0.5, 1.0);
  double sum = 0.0;
  for (int i = 0; i < %d; ++i)
  {
    const double v = U(gen);
    sum += v;
    for (int k = 1; k < argc; ++k)
      if (std::atoi(argv[k]) == i)
        std::printf("%%d %%.17g\n", i, v);
  }
  std::printf("sum %%.17g\n", sum);
}
""" % COUNT

with tempfile.TemporaryDirectory() as tmp:
    src, exe = os.path.join(tmp, "draws.cpp"), os.path.join(tmp, "draws")
    with open(src, "w") as f:
        f.write(SRC)
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-o", exe, src])
    lines = subprocess.check_output([exe] + [str(i) for i in INDICES], text=True).split("\n")

values, total = {}, None
for line in lines:
    if line.startswith("sum"):
        total = line.split()[1]
    elif line:
        values[line.split()[0]] = line.split()[1]
out = {"source": "std::mt19937_64(12345) through std::uniform_real_distribution<double>(0.5, 1.0), libstdc++",
       "count": COUNT, "values": values, "sum": total}
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mt_uniform_golden.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", path)
