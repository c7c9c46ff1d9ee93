"""Per-cell gradient moments of a level vector (include/hmg.h: hmg_cell_moments), stated twice on the CPU.

Cell c has the affine map x = p0 + J x^; with Jinv = J^-T (oracle.cell_geometry) d_k v = sum_a Jinv[k,a] d^_a v.

  reference_form   from the oracle's reference matrices: l_a = d_a . v_c with d = partial_derivatives_functionals(ref), and
                   q_ab = v_c . (A^(a,b) v_c) with A = build_local_diffusion_operators(ref) (an operator's `diffusion_terms`);
                   m_v = Jinv l / |ref|, G_v = |J| Jinv q Jinv^T
  element_form     no shared code: the P1 gradient of v on every fine element T of every cell from the node coordinates,
                   m_v = sum_T |T| grad v_T / |c|, G_v = sum_T |T| grad v_T (x) grad v_T

and for u = xi.x + v:  m_u = xi + m_v,  G_u = |c| (xi xi^T + xi m_v^T + m_v xi^T) + G_v  (with_xi)."""
import math

import numpy as np


def ref_volume(dim):
    return 1.0 / math.factorial(dim)


def cell_volumes(O, base):
    _, _, det = O.cell_geometry(base)
    return det * ref_volume(base.dim)


def reference_form(O, implicit, level, v, diffusion_terms=None):
    """mean (Ne, d), gram (Ne, d, d) of the (nf, Ne) level vector v"""
    base, ref = implicit.base, implicit.reference.levels[level - 1]
    dim = base.dim
    K = diffusion_terms if diffusion_terms is not None else O.build_local_diffusion_operators(ref)
    d = O.partial_derivatives_functionals(ref)                       # (nf, dim)
    _, Jinv, det = O.cell_geometry(base)
    l = d.T @ v                                                      # (dim, Ne)
    q = np.empty((dim, dim, v.shape[1]))
    for a in range(dim):
        for b in range(dim):
            q[a, b] = np.einsum("ie,ie->e", v, K[a][b] @ v)
    mean = np.einsum("eka,ae->ek", Jinv, l) / ref_volume(dim)
    gram = det[:, None, None] * np.einsum("eka,abe,elb->ekl", Jinv, q, Jinv)
    return mean, gram


def element_form(O, implicit, level, v):
    """the same from explicit fine-element P1 gradients"""
    base, ref = implicit.base, implicit.reference.levels[level - 1]
    dim = base.dim
    P = base.nodes[base.elements]                                    # (Ne, d+1, d)
    E = P[:, 1:, :] - P[:, :1, :]                                    # rows p_a - p_0
    X = P[:, :1, :] + np.einsum("na,eac->enc", ref.nodes, E)        # (Ne, nf, d): physical fine nodes
    T = ref.elements                                                 # (nt, d+1)
    XT = X[:, T, :]                                                  # (Ne, nt, d+1, d)
    D = XT[:, :, 1:, :] - XT[:, :, :1, :]                            # (Ne, nt, d, d): rows x_i - x_0
    VT = v.T[:, T]                                                   # (Ne, nt, d+1)
    dv = VT[:, :, 1:] - VT[:, :, :1]                                 # (Ne, nt, d)
    grad = np.linalg.solve(D, dv[..., None])[..., 0]                 # D grad = dv
    volT = np.abs(np.linalg.det(D)) / math.factorial(dim)            # (Ne, nt)
    vol = volT.sum(axis=1)
    mean = np.einsum("et,etk->ek", volT, grad) / vol[:, None]
    gram = np.einsum("et,etk,etl->ekl", volT, grad, grad)
    return mean, gram


def with_xi(mean_v, gram_v, vol, xi):
    """moments of u = xi.x + v from those of v"""
    xi = np.asarray(xi, dtype=np.float64)
    mu = mean_v + xi[None, :]
    cross = xi[None, :, None] * mean_v[:, None, :] + mean_v[:, :, None] * xi[None, None, :]
    gu = gram_v + vol[:, None, None] * (np.outer(xi, xi)[None] + cross)
    return mu, gu


def linear_interpolant(O, implicit, level, g):
    """the nodal interpolant of x -> g.x as an (nf, Ne) level vector"""
    X = implicit.construct_full_grid(level)                          # (Ne, nf, d)
    return np.asfortranarray((X @ np.asarray(g, dtype=np.float64)).T)


def consistent_random(O, implicit, level, rng):
    """a random vector made consistent: every copy of a shared node holds the same value (the interface sum of random copies)"""
    v = np.asfortranarray(rng.standard_normal((implicit.nf(level), implicit.base.nelements())))
    O.broadcast_interfaces(v, implicit, level)
    return v


def cell_energy(O, base, A, v):
    """v_c . (K_c v_c) per cell from the oracle's operator (lambda = 0 wanted by the caller)"""
    y = np.zeros_like(v, order="F")
    O.mul(1.0, base, A, v, y)
    return np.einsum("ie,ie->e", v, y)
