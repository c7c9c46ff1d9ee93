"""Pins the yardstick of the per-cell pair moments (tests/_cell_pair_moments_form.py): two independent statements against each
other on Delaunay meshes in 2D and 3D and on a cube, and the identities the quantity must have -- S_vv = G_v, S_vw = S_wv,
polarisation, and the xi formula against the forms applied to the interpolants of xi.x + v.  No library code runs here.
Errors are relative to sqrt(max |G_v| max |G_w|)."""
import numpy as np
import pytest

import _cell_moments_form as F
import _cell_pair_moments_form as P
import _meshes

CASES = ["delaunay2", "delaunay3", "cube"]
BOUND = 1e-12          # the bound of tests/test_cell_moments_statement.py for the same two statements of one vector
_cache = {}


def build(O, name):
    if name == "delaunay2":
        return _meshes.delaunay_mesh(O, 2, 14, 3), 4
    if name == "delaunay3":
        return _meshes.delaunay_mesh(O, 3, 12, 4), 3
    return O.hypercube(3, 2), 3


@pytest.fixture(scope="module")
def shapes(oracle):
    """per mesh: base, implicit grid, level, two consistent random vectors and the reference form of (v, v), (w, w), (v, w)"""
    def get(name):
        O = oracle
        if name not in _cache:
            base, level = build(O, name)
            implicit = O.ImplicitFineGrid.create(base, level)
            rng = np.random.default_rng(31)
            v, w = F.consistent_random(O, implicit, level, rng), F.consistent_random(O, implicit, level, rng)
            gv, gw = F.reference_form(O, implicit, level, v)[1], F.reference_form(O, implicit, level, w)[1]
            _cache[name] = (base, implicit, level, v, w, gv, gw, P.reference_form(O, implicit, level, v, w))
        return _cache[name]
    yield get
    _cache.clear()


@pytest.mark.parametrize("name", CASES)
def test_reference_form_against_fine_element_gradients(oracle, shapes, name):
    base, implicit, level, v, w, gv, gw, (mv, mw, pair) = shapes(name)
    mv2, mw2, pair2 = P.element_form(oracle, implicit, level, v, w)
    sc = P.scale(gv, gw)
    e = np.abs(pair - pair2).max() / sc
    em = max(np.abs(mv - mv2).max() / np.abs(mv2).max(), np.abs(mw - mw2).max() / np.abs(mw2).max())
    print(f"{name}: pair {e:.2e}, means {em:.2e}")
    assert e <= BOUND and em <= BOUND


@pytest.mark.parametrize("name", CASES)
def test_same_vector_gives_the_gram_tensor(oracle, shapes, name):
    base, implicit, level, v, w, gv, gw, _ = shapes(name)
    for form in (P.reference_form, P.element_form):
        e = np.abs(form(oracle, implicit, level, v, v)[2] - gv).max() / np.abs(gv).max()
        print(f"{name} {form.__name__}: S_vv - G_v {e:.2e}")
        assert e <= BOUND


@pytest.mark.parametrize("name", CASES)
def test_symmetric_in_the_two_vectors_and_in_the_two_indices(oracle, shapes, name):
    base, implicit, level, v, w, gv, gw, (mv, mw, pair) = shapes(name)
    sc = P.scale(gv, gw)
    for form in (P.reference_form, P.element_form):
        a, b = form(oracle, implicit, level, v, w)[2], form(oracle, implicit, level, w, v)[2]
        e1 = np.abs(a - b).max() / sc
        e2 = np.abs(a - np.swapaxes(a, 1, 2)).max() / sc
        print(f"{name} {form.__name__}: S_vw - S_wv {e1:.2e}, S - S^T {e2:.2e}")
        assert e1 <= BOUND and e2 <= BOUND


@pytest.mark.parametrize("name", CASES)
def test_polarisation_identity(oracle, shapes, name):
    base, implicit, level, v, w, gv, gw, (mv, mw, pair) = shapes(name)
    gs = F.reference_form(oracle, implicit, level, np.asfortranarray(v + w))[1]
    e = np.abs(pair - 0.5 * (gs - gv - gw)).max() / P.scale(gv, gw)
    print(f"{name}: S_vw - (G_(v+w) - G_v - G_w) / 2 {e:.2e}")
    assert e <= BOUND


@pytest.mark.parametrize("name", CASES)
def test_xi_formula_against_the_interpolants(oracle, shapes, name):
    O = oracle
    base, implicit, level, v, w, gv, gw, (mv, mw, pair) = shapes(name)
    vol = F.cell_volumes(O, base)
    xv, xw = np.array([0.6, -0.3, 0.5])[:base.dim], np.array([-0.2, 0.9, 0.4])[:base.dim]
    for a, b in ((xv, xw), (xv, None), (None, xw)):
        u = v if a is None else np.asfortranarray(v + F.linear_interpolant(O, implicit, level, a))
        z = w if b is None else np.asfortranarray(w + F.linear_interpolant(O, implicit, level, b))
        got = P.with_xi(mv, mw, pair, vol, a, b)
        sc = P.scale(F.reference_form(O, implicit, level, u)[1], F.reference_form(O, implicit, level, z)[1])
        for form in (P.reference_form, P.element_form):
            e = np.abs(got - form(O, implicit, level, u, z)[2]).max() / sc
            print(f"{name} {form.__name__} xi_v {a is not None} xi_w {b is not None}: {e:.2e}")
            assert e <= BOUND
