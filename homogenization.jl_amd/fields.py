"""
What one does with a corrector once it is solved, from two per-cell quantities (api.cell_moments, include/hmg.h:
hmg_cell_moments): the mean gradient `mean` (Ne, d) and the Gram tensor of the gradient `gram` (Ne, d, d) of u = xi.x + v over
every coarse cell.  Plain numpy on those arrays; nothing here touches a level vector or the device.

`cond` is the conductivity per cell as `L2PlusDivAGrad` takes it: (Ne, d), the diagonals of diagonal tensors, or (Ne, d, d), full
symmetric tensors.  No counterpart in the reference.
"""
from __future__ import annotations

import math

import numpy as np


def _cond(cond, ne, d):
    s = np.asarray(cond, dtype=np.float64)
    if s.shape not in ((ne, d), (ne, d, d)):
        raise ValueError(f"cond must have shape ({ne}, {d}) or ({ne}, {d}, {d}), not {s.shape}")
    return s


def cell_volumes(base, ncells=None):
    """|c| of the first `ncells` cells of a base mesh (api.Mesh: elements 1-based)."""
    els = np.asarray(base.elements)[:ncells] - 1
    p = np.asarray(base.nodes, dtype=np.float64)[els]                 # (Ne, d+1, d)
    d = p.shape[2]
    return np.abs(np.linalg.det(p[:, 1:, :] - p[:, :1, :])) / math.factorial(d)


def mean_flux(cond, mean):
    """sigma_c m(c): the mean flux of every cell, (Ne, d)."""
    mean = np.asarray(mean, dtype=np.float64)
    s = _cond(cond, *mean.shape)
    return s * mean if s.ndim == 2 else np.einsum("ekl,el->ek", s, mean)


def energy(cond, gram):
    """sigma_c : G(c) = int_c grad u . sigma grad u: the energy dissipated in every cell, (Ne,)."""
    gram = np.asarray(gram, dtype=np.float64)
    s = _cond(cond, gram.shape[0], gram.shape[1])
    return np.einsum("ek,ekk->e", s, gram) if s.ndim == 2 else np.einsum("ekl,ekl->e", s, gram)


def flux_row(base, cond, mean, ncells=None):
    """Flux form of the row Sigma xi of the homogenized tensor over the first `ncells` cells (default: all that `mean` covers):
    sum_c |c| sigma_c m_u(c) / sum_c |c|, with m_u the mean gradient of u = xi.x + v."""
    mean = np.asarray(mean, dtype=np.float64)
    n = mean.shape[0] if ncells is None else int(ncells)
    vol = cell_volumes(base, n)
    flux = mean_flux(np.asarray(cond)[:n], mean[:n])
    return (vol[:, None] * flux).sum(axis=0) / vol.sum()


def phase_moments(labels, volumes, mean, gram):
    """First and second moments of the gradient field per phase: {label: {"volume": |phase|, "mean": <grad u> (d),
    "second": <grad u (x) grad u> (d, d)}}, the averages volume-weighted over the cells that carry the label."""
    labels = np.asarray(labels)
    vol = np.asarray(volumes, dtype=np.float64)
    mean = np.asarray(mean, dtype=np.float64)
    gram = np.asarray(gram, dtype=np.float64)
    if not (labels.shape == vol.shape == (mean.shape[0],) and gram.shape[0] == mean.shape[0]):
        raise ValueError("labels, volumes, mean and gram must describe the same cells")
    out = {}
    for lab in np.unique(labels):
        sel = labels == lab
        v = vol[sel].sum()
        out[lab.item() if hasattr(lab, "item") else lab] = {
            "volume": float(v),
            "mean": (vol[sel, None] * mean[sel]).sum(axis=0) / v,
            "second": gram[sel].sum(axis=0) / v,          # (gram is already the integral over the cell)
        }
    return out


def sensitivity(gram, diagonal=False):
    """d(energy) / d(sigma_c) of the plain Dirichlet cell problem (lambda = 0, driver.dirichlet_homogenization), energy =
    sum_c sigma_c : G_u(c) at the minimiser: G_u(c) itself, entry (k, l) for the tensor entry sigma_kl taken as an independent
    variable; diagonal=True: its diagonal (Ne, d), for a `cond` of diagonals.  Exact because the energy is stationary in v.
    Not the gradient of the screened multi-step drivers' value, which is no energy minimum."""
    gram = np.asarray(gram, dtype=np.float64)
    return np.ascontiguousarray(np.einsum("ekk->ek", gram)) if diagonal else gram
