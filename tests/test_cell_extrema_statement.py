"""The CPU statement of the per-cell extrema (tests/_cell_extrema_form.py) pinned: what the GPU tests compare against is right.
  - a linear field has the same q on every fine element: (xi + g) . Q (xi + g);
  - the volume mean of q_T over a cell is sigma_c : G_u(c) / |c| of the per-cell moments' own statement
    (_cell_moments_form.element_form), all fine elements of a cell having the same volume;
  - the element count is 2^(dim (level - 1)), and the elements are the Kuhn simplices of the scaled lattice (the geometry the
    library's kernel rests on)."""
import numpy as np
import pytest

import _cell_extrema_form as X
import _cell_moments_form as F
import _tensor_sigma_form as T

CASES = [(2, 2), (2, 3), (2, 4), (3, 2), (3, 3), (3, 4)]
_cache = {}


@pytest.fixture(scope="module")
def shapes(oracle):
    def get(dim, level):
        if dim not in _cache:
            base = X.perturbed_cube(oracle, dim, 2)
            _cache[dim] = (base, oracle.ImplicitFineGrid.create(base, 4))
        return _cache[dim]
    yield get
    _cache.clear()


@pytest.mark.parametrize("dim,level", CASES)
def test_linear_field_has_one_value(oracle, shapes, dim, level):
    base, implicit = shapes(dim, level)
    rng = np.random.default_rng(level)
    g, xi = rng.standard_normal(dim), rng.standard_normal(dim)
    Q = T.random_spd(rng, base.nelements(), dim)
    v = F.linear_interpolant(oracle, implicit, level, g)
    q = X.element_values(X.element_gradients(oracle, implicit, level, v), xi, Q)
    want = np.einsum("k,ekl,l->e", xi + g, Q, xi + g)
    assert np.abs(q - want[:, None]).max() <= 1e-11 * np.abs(want).max()
    qmax, qmin, counts = X.extrema(q, [0.5 * want.min(), 2.0 * want.max()])
    np.testing.assert_allclose(qmax, want, rtol=1e-11)
    np.testing.assert_allclose(qmin, want, rtol=1e-11)
    assert (counts[:, 0] == X.fine_elements(dim, level)).all() and (counts[:, 1] == 0).all()


@pytest.mark.parametrize("dim,level", CASES)
def test_mean_of_the_element_values_is_the_moment(oracle, shapes, dim, level):
    base, implicit = shapes(dim, level)
    rng = np.random.default_rng(10 + level)
    v = F.consistent_random(oracle, implicit, level, rng)
    xi = rng.standard_normal(dim)
    sig = T.random_spd(rng, base.nelements(), dim)
    q = X.element_values(X.element_gradients(oracle, implicit, level, v), xi, sig)
    assert q.shape == (base.nelements(), X.fine_elements(dim, level))
    vol = F.cell_volumes(oracle, base)
    _, gu = F.with_xi(*F.element_form(oracle, implicit, level, v), vol, xi)
    want = np.einsum("ekl,ekl->e", sig, gu) / vol
    assert np.abs(q.mean(axis=1) - want).max() <= 1e-11 * np.abs(want).max()
    # an indefinite form and the identity go the same way
    Q = sig - np.einsum("ekk->e", sig)[:, None, None] / dim * np.eye(dim)[None]
    assert (np.linalg.eigvalsh(Q)[:, 0] < 0.0).all() and (np.linalg.eigvalsh(Q)[:, -1] > 0.0).all()
    q2 = X.element_values(X.element_gradients(oracle, implicit, level, v), xi, Q)
    want2 = np.einsum("ekl,ekl->e", Q, gu) / vol
    assert np.abs(q2.mean(axis=1) - want2).max() <= 1e-11 * np.abs(np.einsum("ekl,ekl->e", sig, gu) / vol).max()
    q3 = X.element_values(X.element_gradients(oracle, implicit, level, v), None, None)
    gv = F.element_form(oracle, implicit, level, v)[1]
    np.testing.assert_allclose(q3.mean(axis=1), np.einsum("ekk->e", gv) / vol, rtol=1e-11)


@pytest.mark.parametrize("dim,level", CASES)
def test_the_elements_are_the_kuhn_simplices(oracle, shapes, dim, level):
    _, implicit = shapes(dim, level)
    ref = implicit.reference.levels[level - 1]
    listed = {tuple(sorted(int(i) for i in t)) for t in ref.elements}
    assert len(listed) == ref.elements.shape[0] == X.fine_elements(dim, level)
    assert X.kuhn_elements(ref.nodes, level) == listed


def test_thresholds_sit_in_gaps():
    rng = np.random.default_rng(0)
    q = rng.random((7, 500)) ** 2
    thr = X.gap_thresholds(q)
    assert thr.shape == (4,) and (np.diff(thr) > 0).all()
    assert X.margin(q, thr) > 1e-9
    _, _, counts = X.extrema(q, thr)
    frac = counts.sum(axis=0) / q.size
    np.testing.assert_allclose(frac, [0.90, 0.50, 0.10, 0.01], atol=0.06)
