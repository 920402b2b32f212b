"""Time the patched transfers of a hierarchy alone (default: config 2, 64^3, p = 1, 2, 4), per degree pair.
--fp32 times the float entry points on float tensors, the same way.
usage: python tools/time_transfers.py [--n 64] [--orders 1,2,4] [--fp32]"""
import argparse
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import pmg_dolfinx_amd as pm

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--orders", default="1,2,4")
ap.add_argument("--fp32", action="store_true")
a = ap.parse_args()
H = pm.PoissonHierarchy(a.n, tuple(int(p) for p in a.orders.split(",")), cheb_its=3)


def timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for i, ip in enumerate(H.interpolators):
    uc, uf = H.new_vector(i), H.new_vector(i + 1)
    uc.data.normal_()
    uf.data.normal_()
    if a.fp32:
        c32, f32 = uc.data.float(), uf.data.float()
        prolong, restrict = (lambda: ip.interpolate_add_fp32(c32, f32)), (lambda: ip.reverse_interpolate_fp32(f32, c32))
    else:
        prolong, restrict = (lambda: ip.interpolate_add(uc, uf)), (lambda: ip.reverse_interpolate(uf, uc))
    pc, pf = H.orders[i], H.orders[i + 1]
    print(f"lib={os.environ.get('PMG_AMD_LIB', 'default')} {'fp32' if a.fp32 else 'fp64'} n={a.n} p{pc}->p{pf}: "
          f"prolong+add {timed(prolong):7.1f} us   restrict {timed(restrict):7.1f} us")
