"""Numpy reference for the coefficient gradients of the form (tests/test_form_gradients_abi.py,
tests/test_gpu_form_gradients.py), written from the weak form like tests/cell_form_reference.py and with its helpers:
J[d, r] of the coordinate element from tests/curved_geometry_reference.py, adj(J) = det(J) J^-1 and det through
numpy.linalg, the reference gradients by the oracle's 1-D derivative table.  At the point q of cell c

    pu = adj(J)^T gradref u,  pv = adj(J)^T gradref v,  s = w_q / |det J|,  t = pv . T_c pu

    d_kappa[c]     = sum_q s kq_q t
    d_field[n]     = sum over the points (c, q) on dof n of the listed cells of  kappa_c s t
    d_tensor[c][k] = kappa_c sum_q s kq_q m_k,   m = (pv_x pu_x, pv_x pu_y + pv_y pu_x, ..., pv_z pu_z)
    d_sigma[c]     = sum_q w_q |det J| u_q v_q

Every output comes with its scale S: the same sum taken over the magnitudes of its terms.  For the per-cell outputs a
term is a point's, as in tests/cell_form_reference.py: a cell sums (P + 1)^3 >= 8 of them.  A dof inside a cell gets ONE
point's term in d_field, so there the sum that rounds is the point's own dot product t = sum_d pv_d (T_c pu)_d, whose
computed value is off by up to a few eps sum_d |pv_d (T_c pu)_d| however small |t| itself comes out; d_field's terms are
therefore the dot product's three summands, kappa_c s pv_d (T_c pu)_d, at every point on the dof."""
import numpy as np

import cell_form_reference as cf
import curved_geometry_reference as cr
import tensor_coefficient_reference as tr

NAMES = ("kappa", "field", "tensor", "sigma")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # (xx, xy, xz, yy, yz, zz)

jitter = cf.jitter


def form_gradients(P, dofmap, xgeom, geom_dofmap, u, v, kappa, g=1, marker=None, kq=None, T=None, listed=None,
                   ndofs=None):
    """{name: (value, S)} for the four outputs.  ``marker``: marked dofs of u and v read as zero; ``kq`` [ndofs] and
    ``T`` [ncells, 6]: the coefficients that are set (None: 1 and the identity); ``listed`` [ncells] bool: the cells
    d_field sums over (None: all)."""
    dm = np.asarray(dofmap).reshape(-1, (P + 1) ** 3)
    nc = dm.shape[0]
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if marker is not None:
        m = np.asarray(marker).astype(bool)
        u, v = np.where(m, 0.0, u), np.where(m, 0.0, v)
    kappa = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (nc,))
    _, w3 = cr.tables(P, g)
    J = cr.jacobians(P, g, xgeom, geom_dofmap)  # [c, q, d, r]
    det = np.linalg.det(J)
    adj = det[..., None, None] * np.linalg.inv(J)  # [c, q, r, d]
    pu = np.einsum("cqrd,cqr->cqd", adj, cf.gradref(P, dm, u))
    pv = np.einsum("cqrd,cqr->cqd", adj, cf.gradref(P, dm, v))
    Tpu = pu if T is None else np.einsum("cde,cqe->cqd", tr.full(T), pu)
    s = w3[None, :] / np.abs(det)
    kqq = np.ones(dm.shape) if kq is None else np.asarray(kq, dtype=np.float64)[dm]
    out = {}
    tk = s * kqq * (pv * Tpu).sum(axis=-1)
    out["kappa"] = (tk.sum(axis=1), np.abs(tk).sum(axis=1))
    tf = kappa[:, None] * s * (pv * Tpu).sum(axis=-1)
    if listed is not None:
        tf = tf * np.asarray(listed).astype(bool)[:, None]
    n = int(dm.max()) + 1 if ndofs is None else ndofs
    val, S = np.zeros(n), np.zeros(n)
    np.add.at(val, dm.ravel(), tf.ravel())
    tf_abs = kappa[:, None] * s * np.abs(pv * Tpu).sum(axis=-1)
    if listed is not None:
        tf_abs = tf_abs * np.asarray(listed).astype(bool)[:, None]
    np.add.at(S, dm.ravel(), tf_abs.ravel())
    out["field"] = (val, S)
    mk = np.stack([pv[..., i] * pu[..., j] + (pv[..., j] * pu[..., i] if i != j else 0.0) for i, j in PAIRS], axis=-1)
    tt = (kappa[:, None] * s * kqq)[..., None] * mk  # [c, q, 6]
    out["tensor"] = (tt.sum(axis=1), np.abs(tt).sum(axis=1))
    ts = w3[None, :] * np.abs(det) * u[dm] * v[dm]
    out["sigma"] = (ts.sum(axis=1), np.abs(ts).sum(axis=1))
    return out
