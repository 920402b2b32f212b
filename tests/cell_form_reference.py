"""Numpy reference for the per-cell bilinear form (tests/test_cell_form_abi.py, tests/test_gpu_cell_form.py,
tests/test_gpu_adjoint.py), written from the weak form, not from the stored tensor.  Per cell c and quadrature point q

    term_q = w_q / |det J| * (adj(J)^T gradref v) . K_c (adj(J)^T gradref u)      [ x kq[dof(c, q)] ]

with J[d, r] = d x_d / d xi_r of the coordinate element of degree g (tests/curved_geometry_reference.py: its table is
pinned there), adj(J) = det(J) J^-1 through numpy.linalg -- nothing of the library's or the oracle's adjugate code --
and gradref by the oracle's 1-D derivative table.  e_c = sum_q term_q [ x kappa_c ]; S_c = sum_q |term_q| [ x kappa_c ]
is the scale every comparison of the form is made on."""
import numpy as np

import curved_geometry_reference as cr
import tensor_coefficient_reference as tr
from oracle import pmg_oracle as po


def jitter(x):
    """A deterministic "random" displacement of every point, boundary included, by up to 0.03 per axis: the same for a
    vertex whichever rank or cell evaluates it, and far below the smallest cell width used (1/5)."""
    x = np.asarray(x, dtype=np.float64)
    ph = np.array([0.3, 1.1, 2.3])
    return x + 0.03 * np.sin(37.0 * x[:, [1, 2, 0]] + 23.0 * x[:, [2, 0, 1]] + 11.0 * x + ph)


def gradref(P, dofmap, x):
    """[ncells, nq, 3]: the three reference derivatives of the cell's polynomial at its GLL points."""
    nd = P + 1
    xi, _ = po.gll_points_weights(nd)
    D = po.lagrange_deriv_matrix(xi)
    xe = np.asarray(x)[np.asarray(dofmap).reshape(-1, nd**3)].reshape(-1, nd, nd, nd)
    g0 = np.einsum("qi,cijk->cqjk", D, xe)
    g1 = np.einsum("qj,cijk->ciqk", D, xe)
    g2 = np.einsum("qk,cijk->cijq", D, xe)
    return np.stack([g0, g1, g2], axis=-1).reshape(-1, nd**3, 3)


def point_terms(P, dofmap, xgeom, geom_dofmap, u, v, g=1, marker=None, kq=None, T=None):
    """[ncells, nq]: the form's term at every point, without kappa.  ``marker``: marked dofs of u and v read as zero;
    ``kq``: nodal coefficient [ndofs]; ``T``: per-cell tensor [ncells, 6]."""
    dm = np.asarray(dofmap).reshape(-1, (P + 1) ** 3)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if marker is not None:
        m = np.asarray(marker).astype(bool)
        u, v = np.where(m, 0.0, u), np.where(m, 0.0, v)
    _, w3 = cr.tables(P, g)
    J = cr.jacobians(P, g, xgeom, geom_dofmap)  # [c, q, d, r]
    det = np.linalg.det(J)
    adj = det[..., None, None] * np.linalg.inv(J)  # [c, q, r, d]
    pu = np.einsum("cqrd,cqr->cqd", adj, gradref(P, dm, u))
    pv = np.einsum("cqrd,cqr->cqd", adj, gradref(P, dm, v))
    if T is not None:
        pu = np.einsum("cde,cqe->cqd", tr.full(T), pu)
    s = w3[None, :] / np.abs(det)
    if kq is not None:
        s = s * np.asarray(kq)[dm]
    return s * (pv * pu).sum(axis=-1)


def cell_form(P, dofmap, xgeom, geom_dofmap, u, v, g=1, kappa=None, marker=None, kq=None, T=None):
    """(e [ncells], S [ncells]): the form and its scale, times kappa[c] when ``kappa`` is given."""
    t = point_terms(P, dofmap, xgeom, geom_dofmap, u, v, g, marker, kq, T)
    e, S = t.sum(axis=1), np.abs(t).sum(axis=1)
    if kappa is not None:
        k = np.broadcast_to(np.asarray(kappa, dtype=np.float64), e.shape)
        e, S = k * e, k * S
    return e, S
