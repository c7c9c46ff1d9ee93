"""Pins the yardstick of the per-cell gradient moments (tests/_cell_moments_form.py): known answers, the oracle's operator, two
independent statements against each other, and the two identities the feature is for -- energy form = flux form of the
homogenized row, and G_u as the exact sensitivity of the energy -- on a converged oracle solve.  No library code runs here."""
import numpy as np
import pytest

import _cell_moments_form as F

CASES = [(3, 2, 3), (2, 3, 4)]          # dim, n, grids


def setup(O, dim, n, grids):
    base = O.hypercube(dim, n)
    implicit = O.ImplicitFineGrid.create(base, grids)
    return base, implicit


@pytest.mark.parametrize("dim,n,grids", CASES)
def test_linear_field_has_its_gradient_and_its_gram(oracle, dim, n, grids):
    O = oracle
    base, implicit = setup(O, dim, n, grids)
    g = np.array([0.7, -1.3, 0.45])[:dim]
    vol = F.cell_volumes(O, base)
    for level in range(2, grids + 1):
        v = F.linear_interpolant(O, implicit, level, g)
        for form in (F.reference_form, F.element_form):
            mean, gram = form(O, implicit, level, v)
            e1 = np.abs(mean - g[None, :]).max()
            want = vol[:, None, None] * np.outer(g, g)[None]
            e2 = np.abs(gram - want).max() / np.abs(want).max()
            print(form.__name__, level, e1, e2)
            assert e1 <= 1e-12 and e2 <= 1e-12          # (measured 3e-15, 5e-14)


@pytest.mark.parametrize("dim,n,grids", CASES)
def test_diagonal_contraction_is_the_oracles_cell_energy(oracle, dim, n, grids):
    O = oracle
    base, implicit = setup(O, dim, n, grids)
    rng = np.random.default_rng(5)
    sig = np.ascontiguousarray(rng.choice([1.0, 9.0], size=(base.nelements(), dim)))
    constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(base))
    ref = implicit.reference.levels[-1]
    A = O.L2PlusDivAGrad(O.build_local_diffusion_operators(ref), O.mass_matrix(ref), constraint, 0.0, sig)
    v = F.consistent_random(O, implicit, grids, rng)
    _, gram = F.reference_form(O, implicit, grids, v, A.diffusion_terms)
    got = np.einsum("ek,ekk->e", sig, gram)
    want = F.cell_energy(O, base, A, v)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("sigma:G vs v.(K v)", err)
    assert err <= 1e-12                                 # (measured 3e-16)


@pytest.mark.parametrize("dim,n,grids", CASES)
def test_reference_form_against_fine_element_gradients(oracle, dim, n, grids):
    O = oracle
    base, implicit = setup(O, dim, n, grids)
    rng = np.random.default_rng(6)
    v = F.consistent_random(O, implicit, grids, rng)
    m1, g1 = F.reference_form(O, implicit, grids, v)
    m2, g2 = F.element_form(O, implicit, grids, v)
    e1 = np.abs(m1 - m2).max() / np.abs(m2).max()
    e2 = np.abs(g1 - g2).max() / np.abs(g2).max()
    print("mean", e1, "gram", e2)
    assert e1 <= 1e-12 and e2 <= 1e-12                  # (measured 1.4e-15)


def dirichlet_solve(O, base, implicit, grids, sig, xi, cycles=60):
    """converged lambda = 0 solve of a(v, w) = -int sigma xi . grad w by oracle V-cycles; returns v and the relative residual"""
    constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(base))
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), constraint, 0.0, sig)
           for l in implicit.reference.levels]
    states = [O.LevelState.create(base.nelements(), implicit.nf(i + 1)) for i in range(grids)]
    top = states[-1]
    dphis = O.partial_derivatives_functionals(implicit.reference.levels[-1])
    O.rhs_axi_grad_v(top.b, dphis, implicit, sig, xi)
    base_level = O.make_base_level(base, sig, 0.0)

    def rnorm():
        O.local_residual(implicit, ops[-1], top, grids)
        r = top.r.copy(order="F")
        O.broadcast_interfaces(r, implicit, grids)
        O.zero_out_all_but_one(r, implicit, grids)
        return float(np.linalg.norm(r))

    r0 = rnorm()
    for _ in range(cycles):
        O.vcycle(implicit, base_level, ops, states, grids, 3)
    return top.x.copy(order="F"), rnorm() / r0


def forms(O, base, implicit, grids, sig, xi):
    v, res = dirichlet_solve(O, base, implicit, grids, sig, xi)
    vol = F.cell_volumes(O, base)
    mv, gv = F.reference_form(O, implicit, grids, v)
    mu, gu = F.with_xi(mv, gv, vol, xi)
    energy = float(np.einsum("ek,ekk->e", sig, gu).sum())
    flux = (vol[:, None] * sig * mu).sum(axis=0)
    return energy, flux, gu, res


def test_energy_form_is_flux_form_and_gram_is_the_sensitivity(oracle):
    O = oracle
    dim, n, grids = 2, 3, 3
    base, implicit = setup(O, dim, n, grids)
    rng = np.random.default_rng(2)
    sig = np.ascontiguousarray(rng.choice([1.0, 9.0], size=(base.nelements(), dim)))
    xi = np.array([0.6, 0.8])
    energy, flux, gu, res = forms(O, base, implicit, grids, sig, xi)
    print("residual", res, "energy", energy, "xi.flux", float(xi @ flux))
    assert res <= 1e-12
    assert abs(energy - xi @ flux) <= 1e-10 * abs(energy)
    c, eps = 7, 1e-4
    e = []
    for s in (+1.0, -1.0):
        sp = sig.copy()
        sp[c, 0] += s * eps
        e.append(forms(O, base, implicit, grids, sp, xi)[0])
    fd = (e[0] - e[1]) / (2 * eps)
    err = abs(fd - gu[c, 0, 0]) / abs(gu[c, 0, 0])
    print("central difference", fd, "G_u,11", gu[c, 0, 0], err)
    assert err <= 1e-8                                   # (measured 4e-11)
