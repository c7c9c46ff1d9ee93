"""Per-cell cross moments of two level vectors (include/hmg.h: hmg_cell_pair_moments), stated twice on the CPU; the bilinear
counterpart of tests/_cell_moments_form.py, whose geometry, interpolants and random vectors it reuses.

  S_vw(c) = 1/2 int_c (grad v (x) grad w + grad w (x) grad v)                      symmetric (d, d) per cell

  reference_form   from the oracle's reference matrices: q_ab = v_c . (A^(a,b) w_c), symmetrised in (a, b), then
                   S = |J| Jinv sym(q) Jinv^T; with them the mean gradients m_v, m_w of _cell_moments_form.reference_form
  element_form     no shared code: the P1 gradients of v and w on every fine element T of every cell,
                   S = sum_T |T| sym(grad v_T (x) grad w_T)

and for u = xi_v.x + v, z = xi_w.x + w:  S_uz = S_vw + |c| sym(xi_v xi_w^T + xi_v m_w^T + m_v xi_w^T)  (with_xi).
The scale of an error is sqrt(max |G_v| max |G_w|) (Cauchy-Schwarz), so that a small cross term does not inflate it (scale)."""
import math

import numpy as np

import _cell_moments_form as F


def sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def reference_form(O, implicit, level, v, w, diffusion_terms=None):
    """mean_v (Ne, d), mean_w (Ne, d), pair (Ne, d, d) of the (nf, Ne) level vectors v and w"""
    base, ref = implicit.base, implicit.reference.levels[level - 1]
    dim = base.dim
    K = diffusion_terms if diffusion_terms is not None else O.build_local_diffusion_operators(ref)
    d = O.partial_derivatives_functionals(ref)                       # (nf, dim)
    _, Jinv, det = O.cell_geometry(base)
    q = np.empty((dim, dim, v.shape[1]))
    for a in range(dim):
        for b in range(dim):
            q[a, b] = np.einsum("ie,ie->e", v, K[a][b] @ w)
    q = 0.5 * (q + q.transpose(1, 0, 2))
    mv = np.einsum("eka,ae->ek", Jinv, d.T @ v) / F.ref_volume(dim)
    mw = np.einsum("eka,ae->ek", Jinv, d.T @ w) / F.ref_volume(dim)
    pair = det[:, None, None] * np.einsum("eka,abe,elb->ekl", Jinv, q, Jinv)
    return mv, mw, pair


def element_gradients(implicit, level, v):
    """P1 gradient (Ne, nt, d) of v on every fine element, and the elements' volumes (Ne, nt)"""
    base, ref = implicit.base, implicit.reference.levels[level - 1]
    dim = base.dim
    P = base.nodes[base.elements]                                    # (Ne, d+1, d)
    E = P[:, 1:, :] - P[:, :1, :]
    X = P[:, :1, :] + np.einsum("na,eac->enc", ref.nodes, E)        # (Ne, nf, d): physical fine nodes
    T = ref.elements
    XT = X[:, T, :]
    D = XT[:, :, 1:, :] - XT[:, :, :1, :]                            # rows x_i - x_0
    VT = v.T[:, T]
    dv = VT[:, :, 1:] - VT[:, :, :1]
    grad = np.linalg.solve(D, dv[..., None])[..., 0]                 # D grad = dv
    return grad, np.abs(np.linalg.det(D)) / math.factorial(dim)


def element_form(O, implicit, level, v, w):
    """the same from explicit fine-element P1 gradients"""
    gv, volT = element_gradients(implicit, level, v)
    gw, _ = element_gradients(implicit, level, w)
    vol = volT.sum(axis=1)
    mv = np.einsum("et,etk->ek", volT, gv) / vol[:, None]
    mw = np.einsum("et,etk->ek", volT, gw) / vol[:, None]
    return mv, mw, sym(np.einsum("et,etk,etl->ekl", volT, gv, gw))


def with_xi(mv, mw, pair, vol, xi_v, xi_w):
    """the pair moment of u = xi_v.x + v and z = xi_w.x + w from the quantities of v and w (xi None: 0)"""
    d = mv.shape[1]
    xv = np.zeros(d) if xi_v is None else np.asarray(xi_v, dtype=np.float64)
    xw = np.zeros(d) if xi_w is None else np.asarray(xi_w, dtype=np.float64)
    t = np.outer(xv, xw)[None] + xv[None, :, None] * mw[:, None, :] + mv[:, :, None] * xw[None, None, :]
    return pair + vol[:, None, None] * sym(t)


def scale(gram_v, gram_w):
    return math.sqrt(np.abs(gram_v).max() * np.abs(gram_w).max())
