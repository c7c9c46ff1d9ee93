"""Per-cell extrema and exceedance counts of a quadratic form of the fine-element gradients (include/hmg.h: hmg_cell_extrema),
stated on the CPU without any code of the library.

For every coarse cell c and every fine element T of it, from the PHYSICAL coordinates of the fine nodes
(implicit.construct_full_grid) and the reference's element list (ref.elements): the P1 gradient of v on T by a solve per
element, then

    q_T = (xi + grad v_T) . Q_c (xi + grad v_T)          Q_c symmetric, None: the identity; xi None: 0

and per cell max_T q_T, min_T q_T and the number of T with q_T > threshold_j.

The geometry the library's kernel rests on is stated here as a function too (kuhn_elements): with the reference nodes scaled by
m = 2^(level-1), every fine element is {p, p + pi1, p + pi1 + pi2, p + s} for a permutation pi of the basis a, b, c (2D: a, b),
s = a + b + c, p its lexicographically lowest vertex."""
import itertools

import numpy as np

BASIS = {3: np.array([(0, 0, 1), (0, 1, -1), (1, -1, 0)]), 2: np.array([(0, 1), (1, -1)])}


def perturbed_cube(O, dim, n, amplitude=0.12, seed=5):
    """hypercube(dim, n) with every node moved by up to `amplitude` of the lattice spacing: no two cells congruent, J full"""
    base = O.hypercube(dim, n)
    rng = np.random.default_rng(seed)
    nodes = base.nodes + amplitude * (base.nodes.max() - base.nodes.min()) / n * rng.uniform(-1.0, 1.0, base.nodes.shape)
    return O.Mesh(np.ascontiguousarray(nodes), base.elements.copy())


def element_gradients(O, implicit, level, v):
    """grad v on every fine element: (Ne, nt, d)"""
    ref = implicit.reference.levels[level - 1]
    X = implicit.construct_full_grid(level)                          # (Ne, nf, d): physical fine nodes
    T = ref.elements                                                 # (nt, d+1)
    XT = X[:, T, :]
    D = XT[:, :, 1:, :] - XT[:, :, :1, :]                            # rows x_i - x_0
    VT = v.T[:, T]
    dv = VT[:, :, 1:] - VT[:, :, :1]
    return np.linalg.solve(D, dv[..., None])[..., 0]


def element_values(grad, xi=None, form=None):
    """q_T, (Ne, nt), from element_gradients' result"""
    g = grad if xi is None else grad + np.asarray(xi, dtype=np.float64)[None, None, :]
    if form is None:
        return np.einsum("etk,etk->et", g, g)
    return np.einsum("etk,ekl,etl->et", g, np.asarray(form, dtype=np.float64), g)


def extrema(q, thresholds=()):
    """qmax (Ne,), qmin (Ne,), counts (Ne, nthr) of the element values q (Ne, nt)"""
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    counts = np.stack([(q > t).sum(axis=1) for t in thr], axis=1) if thr.size else np.zeros((q.shape[0], 0), dtype=np.int64)
    return q.max(axis=1), q.min(axis=1), counts.astype(np.int64)


def gap_thresholds(q, quantiles=(0.10, 0.50, 0.90, 0.99)):
    """one threshold per quantile of all element values: the midpoint of the widest gap between neighbouring values within
    a window of positions around the quantile (a hundredth of the values, 200 at most) -- as far from any value as the data
    allow there"""
    s = np.sort(q.ravel())
    window = min(200, max(2, s.size // 100))
    out = []
    for p in quantiles:
        k = int(round(p * (s.size - 1)))
        lo, hi = max(k - window, 0), min(k + window, s.size - 1)
        gaps = np.diff(s[lo:hi + 1])
        i = lo + int(np.argmax(gaps))
        out.append(0.5 * (s[i] + s[i + 1]))
    return np.array(out)


def margin(q, thresholds):
    """the smallest distance of an element value from a threshold, relative to the largest value"""
    return min(np.abs(q - t).min() for t in thresholds) / np.abs(q).max()


def kuhn_elements(ref_nodes, level):
    """the geometry claim: the Kuhn simplices of the lattice of the scaled reference nodes, as a set of sorted node tuples"""
    dim = ref_nodes.shape[1]
    m = 2 ** (level - 1)
    P = np.rint(np.asarray(ref_nodes) * m).astype(np.int64)
    assert np.abs(P - np.asarray(ref_nodes) * m).max() < 1e-9
    index = {tuple(p): i for i, p in enumerate(P)}
    out = set()
    for p in P:
        for perm in itertools.permutations(range(dim)):
            cur, nodes = p.copy(), [index[tuple(p)]]
            for b in perm:
                cur = cur + BASIS[dim][b]
                if tuple(cur) not in index:
                    break
                nodes.append(index[tuple(cur)])
            else:
                out.add(tuple(sorted(nodes)))
    return out


def fine_elements(dim, level):
    return 2 ** (dim * (level - 1))
