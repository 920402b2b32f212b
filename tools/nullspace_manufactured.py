"""The manufactured pure-Neumann problem of `pmg_main --neumann`, restated on the CPU (no GPU needed):
u = cos(pi x) cos(pi y) cos(pi z) on the unit box, kappa = 2, no Dirichlet dof; load = lumped mass times
-div(kappa grad u), made compatible by removing its mean; solved with the projected Jacobi-CG of
tests/nullspace_reference.py on the oracle's operator; the largest nodal error after removing the lumped-mass mean from
the solution and from the nodal values of u.  tests/test_gpu_nullspace_drivers.py holds the printed value as a constant.

    python tools/nullspace_manufactured.py --n 8 --degree 4
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def restated_error(n, P, rtol=1e-8, kappa=2.0):
    import nullspace_reference as ns
    from oracle import pmg_oracle as po

    mesh = po.BoxMesh(n)
    A = po.Laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, np.zeros(mesh.ndofs(P), np.int8))
    c = mesh.dof_coordinates(P)
    u = np.cos(np.pi * c[:, 0]) * np.cos(np.pi * c[:, 1]) * np.cos(np.pi * c[:, 2])
    # lumped mass (GLL collocation): w3 |det J| summed over the cells of a dof
    mass = np.bincount(A.dofmap.ravel(), weights=(A.w3[None, :] * A.detJ.reshape(A.ncells, -1)).ravel(),
                       minlength=A.ndofs)
    b = ns.remove_mean(kappa * mass * (3.0 * np.pi**2 * u))
    dinv = A.diag_inverse()
    x, its = ns.pcg_nullspace(A.apply, lambda r: dinv * r, b, np.zeros_like(b), rtol, 5000)
    err = np.abs(ns.remove_mean(x, mass) - ns.remove_mean(u, mass)).max()
    return err, its, abs(mass.sum() - 1.0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--rtol", type=float, default=1e-8)
    a = ap.parse_args()
    err, its, vol = restated_error(a.n, a.degree, a.rtol)
    print(f"n = {a.n}, degree {a.degree}, rtol {a.rtol:g}: {its} Jacobi-CG iterations, "
          f"max nodal error = {err:.6e} (|sum(mass) - 1| = {vol:.1e})")
