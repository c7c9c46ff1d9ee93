"""
What one does with a corrector once it is solved, from two per-cell quantities (api.cell_moments, include/hmg.h:
hmg_cell_moments): the mean gradient `mean` (Ne, d) and the Gram tensor of the gradient `gram` (Ne, d, d) of u = xi.x + v over
every coarse cell -- and, for two correctors, from their symmetrised cross moment `pair` (Ne, d, d) (api.cell_pair_moments:
pair_energy, tensor_sensitivity) -- and, for the pass over the fine elements (api.cell_extrema), the forms to give it and what
its extrema and counts mean (energy_form, flux_form, exceedance_volume, concentration) and what its histograms say
(api.cell_histogram: histogram_volume, histogram_quantile, histogram_tail) -- and, for point samples (api.sample,
api.sample_raster), the flux and the energy density at every point (sample_flux, sample_energy_density, line_points).  Plain numpy on those arrays; nothing here touches a level vector or the device.

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


def _corners(base, cells):
    """Corner positions (n, d + 1, d) of some cells of a base mesh: api.Mesh.cell_corners, which unwraps the cells of a torus; a
    mesh-like object without it has no period."""
    if hasattr(base, "cell_corners"):
        return np.asarray(base.cell_corners(cells), dtype=np.float64)
    return np.asarray(base.nodes, dtype=np.float64)[np.asarray(base.elements)[cells] - 1]


def cell_volumes(base, ncells=None):
    """|c| of the first `ncells` cells of a base mesh (api.Mesh: elements 1-based)."""
    p = _corners(base, slice(None, ncells))                          # (Ne, d+1, d)
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


def pair_energy(cond, pair):
    """sigma_c : S(c) = int_c grad u . sigma grad z for the symmetrised cross moment S of two fields (api.cell_pair_moments): the
    per-cell energy density of an entry of the homogenized tensor, Sigma_kl |Omega| = sum_c sigma_c : S_{u_k u_l}(c), (Ne,).  Not
    a dissipation: for two different fields it has either sign."""
    pair = np.asarray(pair, dtype=np.float64)
    if pair.ndim != 3 or pair.shape[1] != pair.shape[2]:
        raise ValueError(f"pair must have shape (Ne, d, d), not {pair.shape}")
    s = _cond(cond, pair.shape[0], pair.shape[1])
    return np.einsum("ek,ekk->e", s, pair) if s.ndim == 2 else np.einsum("ekl,ekl->e", s, pair)


def tensor_sensitivity(pairs, diagonal=False):
    """d(Sigma_kl |Omega|) / d(sigma_c,mn) of the plain Dirichlet cell problem (lambda = 0, driver.dirichlet_homogenization_tensor)
    as entry [k, l, c, m, n] of a (d, d, Ne, d, d) array: `pairs` itself, pairs[k, l, c] = S_{u_k u_l}(c), the cross moment of
    the correctors u_k = e_k.x + v_k.  The entries of sigma_c are taken as independent variables: moving a symmetric off-diagonal
    pair sigma_mn = sigma_nm together gives 2 S_mn.  diagonal=True: the diagonals, [k, l, c, m] of (d, d, Ne, d), for a `cond` of
    diagonals.  Exact because Sigma_kl |Omega| = a(u_k, u_l) and BOTH correctors are stationary: the first-order change of
    either corrector is a test function, against which the other's residual vanishes.  It does not hold where a corrector is not
    the solution of that problem: an unconverged solve, or the screened multi-step drivers, whose value is no such bilinear
    form at a solution."""
    pairs = np.asarray(pairs, dtype=np.float64)
    if pairs.ndim != 5 or not (pairs.shape[0] == pairs.shape[1] == pairs.shape[3] == pairs.shape[4]):
        raise ValueError(f"pairs must have shape (d, d, Ne, d, d), not {pairs.shape}")
    return np.ascontiguousarray(np.einsum("klcmm->klcm", pairs)) if diagonal else pairs


def _full(cond, what="cond"):
    s = np.asarray(cond, dtype=np.float64)
    if s.ndim == 2:
        out = np.zeros(s.shape + (s.shape[1],))
        i = np.arange(s.shape[1])
        out[:, i, i] = s
        return out
    if s.ndim != 3 or s.shape[1] != s.shape[2]:
        raise ValueError(f"{what} must have shape (Ne, d) or (Ne, d, d), not {s.shape}")
    return s


def energy_form(cond):
    """The form of api.cell_extrema whose q is the energy density grad u . sigma_c grad u: Q = sigma_c (symmetrised), (Ne, d, d)."""
    s = _full(cond)
    return 0.5 * (s + np.swapaxes(s, 1, 2))


def flux_form(cond):
    """The form whose q is the squared flux |sigma_c grad u|^2: Q = sigma_c^T sigma_c, (Ne, d, d), exactly symmetric."""
    s = _full(cond)
    q = np.einsum("emk,eml->ekl", s, s)
    return 0.5 * (q + np.swapaxes(q, 1, 2))


def exceedance_volume(counts, volumes, nel):
    """Volume of every cell on which q exceeds each threshold: counts |c| / nel, (Ne, nthr) -- the fine elements of a cell all
    have the volume |c| / nel, nel = api.fine_elements(implicit, level)."""
    counts = np.asarray(counts, dtype=np.float64)
    vol = np.asarray(volumes, dtype=np.float64)
    if counts.ndim != 2 or vol.shape != (counts.shape[0],):
        raise ValueError("counts must be (Ne, nthr) and volumes (Ne,)")
    if nel <= 0:
        raise ValueError("nel must be positive")
    return counts * (vol[:, None] / float(nel))


def concentration(qmax, mean_density):
    """Peak over mean: qmax (Ne,) over a mean density -- a number (the homogenized energy density, say) or one per cell."""
    return np.asarray(qmax, dtype=np.float64) / np.asarray(mean_density, dtype=np.float64)


# ---- histograms over the fine elements (api.cell_histogram): counts (Ne, nbins), nbins = nreg + 3 -- column 0 below the first
# edge, columns 1 .. nreg between the edges, column nreg + 1 from the last edge up, the last column NaN ---------------------------
def histogram_volume(counts, volumes, nel, labels=None):
    """Volume per bin over all cells: sum_c counts[c, b] |c| / nel, (nbins,) -- the fine elements of a cell all have the volume
    |c| / nel, nel = api.fine_elements(implicit, level); the entries sum to the volume of the cells.  With `labels` (Ne,): one such
    row per label, {label: (nbins,)} over the cells that carry it (the convention of phase_moments); the rows add up to the row
    without labels."""
    counts = np.asarray(counts)
    vol = np.asarray(volumes, dtype=np.float64)
    if counts.ndim != 2 or vol.shape != (counts.shape[0],):
        raise ValueError("counts must be (Ne, nbins) and volumes (Ne,)")
    if nel <= 0:
        raise ValueError("nel must be positive")
    w = vol / float(nel)
    if labels is None:
        return w @ counts.astype(np.float64)
    labels = np.asarray(labels)
    if labels.shape != vol.shape:
        raise ValueError("labels must be (Ne,)")
    out = {}
    for lab in np.unique(labels):
        sel = labels == lab
        out[lab.item() if hasattr(lab, "item") else lab] = w[sel] @ counts[sel].astype(np.float64)
    return out


def histogram_quantile(volume_per_bin, edges, p):
    """The interval (lo, hi) of the bin that contains the p-quantile of q, 0 <= p <= 1, by volume: the first bin at which the
    cumulated volume reaches p times the total.  An interval, not an interpolated number: within a bin nothing is known.  The
    bin below the first edge is (-inf, E_0), the one from the last edge up (E_nreg, inf).  volume_per_bin is histogram_volume's
    row, (len(edges) + 2,); a NaN bin behind it must be empty (a NaN has no place in an order)."""
    vol = np.asarray(volume_per_bin, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    n = edges.shape[0] + 1
    if vol.ndim != 1 or vol.shape[0] not in (n, n + 1):
        raise ValueError(f"volume_per_bin must have {n} entries (or {n + 1} with the NaN bin) for {edges.shape[0]} edges")
    if vol.shape[0] == n + 1 and vol[n] != 0.0:
        raise ValueError("the NaN bin is not empty: no quantiles")
    if not 0.0 <= p <= 1.0:
        raise ValueError("p must lie in [0, 1]")
    vol = vol[:n]
    if (vol < 0.0).any() or not vol.sum() > 0.0:
        raise ValueError("volume_per_bin must be non-negative and not all zero")
    cum = np.cumsum(vol)
    b = int(np.searchsorted(cum, p * cum[-1], side="left"))
    b = min(b, n - 1)
    while vol[b] == 0.0:                                              # (p = 0: the first bin that holds something)
        b += 1
    bounds = np.concatenate(([-np.inf], edges, [np.inf]))
    return float(bounds[b]), float(bounds[b + 1])


def histogram_tail(counts):
    """Elements at or above each edge: (Ne, nreg + 1) int64, column i = the number of fine elements with q >= E_i (the NaN bin
    takes no part).  Column i equals api.cell_extrema's count for the threshold nextafter(E_i, -inf)."""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] < 4:
        raise ValueError("counts must be (Ne, nbins) with nbins >= 4")
    return np.ascontiguousarray(np.cumsum(counts[:, -2:0:-1].astype(np.int64), axis=1)[:, ::-1])


# ---- point samples (api.sample, api.sample_raster): the flux and the energy density of u at every point --------------------
def sample_flux(cond, cell, gradient):
    """sigma_cell grad u at every sampled point: cond (Ne, d) or (Ne, d, d), cell (...) as api.sample / sample_raster return it,
    gradient (..., d); the result has gradient's shape and is NaN where cell < 0."""
    cell = np.asarray(cell)
    g = np.asarray(gradient, dtype=np.float64)
    if g.shape[:-1] != cell.shape:
        raise ValueError(f"gradient {g.shape} does not fit cell {cell.shape}")
    s = _full(cond)
    if s.shape[1] != g.shape[-1]:
        raise ValueError(f"cond is for dimension {s.shape[1]}, the gradients have {g.shape[-1]} components")
    ok = cell >= 0
    out = np.einsum("...kl,...l->...k", s[np.where(ok, cell, 0)], g)
    out[~ok] = np.nan
    return out


def sample_energy_density(cond, cell, gradient):
    """grad u . sigma_cell grad u at every sampled point, cell's shape; NaN where cell < 0."""
    g = np.asarray(gradient, dtype=np.float64)
    return np.einsum("...k,...k->...", g, sample_flux(cond, cell, g))


def line_points(p0, p1, n):
    """n points from p0 to p1, both ends included, (n, d): a line profile for api.sample."""
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    if p0.shape != p1.shape or p0.ndim != 1:
        raise ValueError("p0 and p1 must be points of one dimension")
    if n < 2:
        raise ValueError("a line takes at least its two ends")
    t = np.linspace(0.0, 1.0, int(n))[:, None]
    return (1.0 - t) * p0 + t * p1


def element_points(implicit, level, cells, nodes):
    """Physical coordinates of named vertices of fine elements: cells (n,) coarse cell ids, nodes (n, d + 1) 0-based hierarchical
    node ids of `level` (api.cell_extrema_where's where_max / where_min, api.locate's nodes) -> (n, d + 1, d).  Formed from the
    base mesh's corners of those cells and the level's reference positions of those vertices only -- never the whole fine grid.
    A vertex id of -1 (a cell without a location: NaN extrema) gives NaN."""
    base = implicit.base
    d = base.dim
    cells = np.asarray(cells, dtype=np.int64).reshape(-1)
    nodes = np.asarray(nodes, dtype=np.int64)
    if nodes.ndim != 2 or nodes.shape[0] != cells.shape[0]:
        raise ValueError(f"nodes {nodes.shape} does not fit {cells.shape[0]} cells")
    nf = implicit.nf(level)
    if cells.size and (cells.min() < 0 or cells.max() >= implicit.ncells()):
        raise ValueError("a cell id is not a current cell of the grid")
    if nodes.size and (nodes.min() < -1 or nodes.max() >= nf):
        raise ValueError(f"a node id is not a node of level {level}")
    m = 2 ** (level - 1)
    h2s = implicit.table_i32("hier2slot", level)
    ijk = implicit.table_i32("slot_ijk", level).reshape(-1, 3)
    ok = nodes >= 0
    ref = ijk[h2s[np.where(ok, nodes, 0)]][..., :d].astype(np.float64) / m        # (n, d + 1, d) reference coordinates
    X = _corners(base, cells)                                                            # (n, d + 1, d) corners
    J = X[:, 1:, :] - X[:, :1, :]
    out = X[:, :1, :] + np.einsum("nva,nac->nvc", ref, J)
    out[~ok] = np.nan
    return out


def element_centroids(implicit, level, cells, nodes):
    """The centroids of those elements, (n, d): interior points of the elements (api.locate finds the element again)."""
    return element_points(implicit, level, cells, nodes).mean(axis=1)


def hot_spots(qmax, where_max, implicit, level, k=10):
    """The k cells with the highest qmax (api.cell_extrema_where), highest first, equal values by ascending cell id, NaN last:
    (cells (k,) int64, values (k,), centroids (k, d) of the elements that hold them)."""
    q = np.asarray(qmax, dtype=np.float64).reshape(-1)
    w = np.asarray(where_max)
    if w.ndim != 2 or w.shape[0] != q.shape[0]:
        raise ValueError(f"where_max {w.shape} does not fit {q.shape[0]} cells")
    key = np.where(np.isnan(q), -np.inf, q)
    order = np.lexsort((np.arange(q.shape[0]), np.isnan(q), -key))[:max(int(k), 0)]
    return order.astype(np.int64), q[order], element_centroids(implicit, level, order, w[order])
