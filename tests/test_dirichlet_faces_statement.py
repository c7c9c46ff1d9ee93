"""The yardsticks of tests/_dirichlet_faces_form.py against each other, on the CPU and without the library: the closure rule in
numpy against the oracle's constraint maps, the oracle's V-cycle under a constraint on chosen faces against the global matrix
form, and -- by sparse direct solves on the global form -- what the mixed ("uniaxial") cell problem computes."""
import numpy as np
import pytest

from _dirichlet_faces_form import (FaceSetForm, block_boundary_faces, closure, default_faces, interior_faces, oracle_base_level,
                                   oracle_constraint, plane_faces)


def sides(m, axis):
    x = m.nodes[:, axis]
    return np.concatenate([plane_faces(m.nodes, m.elements, axis, x.min()), plane_faces(m.nodes, m.elements, axis, x.max())])


def mask_of(O, m, cons):
    """per-cell bitmask from the oracle's (element, local id) lists: faces, edges, nodes"""
    nface, nedge = (4, 6) if m.dim == 3 else (0, 3)
    mask = np.zeros(m.nelements(), dtype=np.int64)
    for smap, shift in ((cons.faces, 0), (cons.edges, nface), (cons.nodes, nface + nedge)):
        if len(smap):
            np.bitwise_or.at(mask, smap.element, 1 << (shift + smap.local_id))
    return mask


@pytest.mark.parametrize("dim,n", [(3, 2), (2, 4), (3, 1)])
def test_closure_in_numpy_is_the_oracles(oracle, dim, n):
    O = oracle
    m = O.hypercube(dim, n)
    dflt = default_faces(m.elements)
    dmask, con = closure(m.elements, dflt, m.nnodes())
    np.testing.assert_array_equal(dmask, mask_of(O, m, O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(m))))
    np.testing.assert_array_equal(np.flatnonzero(~con), O.list_interior_nodes(m))
    sets = [interior_faces(m.elements), sides(m, 0), np.zeros((0, dim), dtype=np.int64)]
    if n > 1:
        sets += [plane_faces(m.nodes, m.elements, 0, m.nodes[:, 0].min() + n // 2), block_boundary_faces(m.nodes, m.elements, n // 2)]
    for faces in sets:
        dmask, con = closure(m.elements, faces, m.nnodes())
        np.testing.assert_array_equal(dmask, mask_of(O, m, oracle_constraint(O, m, faces)))
        assert con.sum() == np.unique(faces).size
    # a face whose nodes are all constrained but which was not chosen carries no face bit
    if dim == 3 and n == 1:
        dmask, con = closure(m.elements, interior_faces(m.elements), m.nnodes())
        assert con.all() and all(bin(int(d) & 0xF).count("1") == 2 for d in dmask)


def custom_set(m, dim, n, which):
    if which == "mid-plane and two sides":
        return np.concatenate([plane_faces(m.nodes, m.elements, 0, m.nodes[:, 0].min() + n // 2), sides(m, dim - 1)])
    return block_boundary_faces(m.nodes, m.elements, 2)


@pytest.mark.parametrize("dim,n,grids,which", [(3, 2, 3, "mid-plane and two sides"), (2, 4, 4, "blocks")])
def test_oracle_vcycle_with_a_face_set_equals_the_global_form(oracle, dim, n, grids, which):
    """The oracle's vcycle! with the constraint on chosen faces -- an internal plane among them -- and a BaseLevel on the set's free
    nodes, against the global matrix form whose constrained nodes are found by geometry.  x: 1e-11, r: 1e-10, the bounds of
    tests/test_oracle_reference_kats.py::test_vcycle_equals_its_global_matrix_form."""
    O = oracle
    lam, steps = 1.0, 3
    rng = np.random.default_rng(11)
    base = O.hypercube(dim, n)
    faces = custom_set(base, dim, n, which)
    sgrid = np.where(rng.random((n,) * dim + (dim,)) < 0.5, 1.0, 9.0)
    cond = O.conductivity_per_element(base, sgrid, (0.0,) * dim)
    implicit = O.ImplicitFineGrid.create(base, grids)
    constraint = oracle_constraint(O, base, faces)
    base_level = oracle_base_level(O, base, cond, lam, faces)
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(m), O.mass_matrix(m), constraint, lam, cond)
           for m in implicit.reference.levels]
    states = [O.LevelState.create(base.nelements(), implicit.nf(i + 1)) for i in range(grids)]
    top = states[-1]
    top.x[...] = rng.random(top.x.shape)
    O.broadcast_interfaces(top.x, implicit, grids)
    O.apply_constraint(top.x, grids, constraint, implicit)
    O.local_rhs(top.b, implicit)
    G = FaceSetForm(O, base, sgrid, lam, implicit, grids, dim, faces)
    gx = G.gather(top.x, grids - 1)
    assert not gx[~G.inner[-1]].any() and np.count_nonzero(gx[G.inner[-1]]) == G.inner[-1].sum()   # same constrained nodes
    gb = G.gather_sum(top.b, grids - 1)
    for cycle in range(2):
        O.vcycle(implicit, base_level, ops, states, grids, steps)
        gx, gr = G.vcycle(grids - 1, gx, gb, steps)
        ox, orr = G.gather(top.x, grids - 1), G.gather(top.r, grids - 1)
        assert np.abs(ox - gx).max() <= 1e-11 * np.abs(gx).max(), (cycle, np.abs(ox - gx).max())
        assert np.abs(orr - gr).max() <= 1e-10 * max(np.abs(gr).max(), 1e-300), (cycle, np.abs(orr - gr).max())


def energy_diagonal(O, base, sgrid, grids, k, faces):
    """e_k . Sigma e_k of the cell problem with v = 0 on `faces`, natural elsewhere, by a sparse direct solve on the refined mesh:
    with F(w) = -int sigma e_k . grad w and a(v, v) = F(v), int sigma grad u . grad u = int sigma_kk - F(v)."""
    import scipy.sparse.linalg as spla
    dim = base.dim
    cond = O.conductivity_per_element(base, sgrid, (0.0,) * dim)
    implicit = O.ImplicitFineGrid.create(base, grids)
    G = FaceSetForm(O, base, sgrid, 0.0, implicit, grids, dim, faces)
    b = np.zeros((implicit.nf(grids), base.nelements()), order="F")
    O.rhs_axi_grad_v(b, O.partial_derivatives_functionals(implicit.reference.levels[-1]), implicit, cond, np.eye(dim)[k])
    F = G.gather_sum(b, grids - 1)
    idx = np.flatnonzero(G.inner[-1])
    v = np.zeros_like(F)
    v[idx] = spla.spsolve(G.A[-1][idx][:, idx].tocsc(), F[idx])
    _, _, det = O.cell_geometry(base)
    vol = np.abs(det) / (6.0 if dim == 3 else 2.0)
    return float((vol * cond[:, k]).sum() - F @ v) / float(vol.sum())


@pytest.mark.parametrize("dim,n,grids,bound", [(2, 4, 3, 7.7e-15), (3, 3, 2, 1.5e-14)])
def test_uniaxial_conditions_are_exact_for_a_laminate(oracle, dim, n, grids, bound):
    """Layers normal to e_1, the potential fixed on the two faces normal to e_k, the others insulated: u_k is piecewise linear,
    so the P1 solution is exact -- the harmonic mean of sigma_11 over the layers for k = 1, the arithmetic mean of sigma_kk for
    the others.  Measured here (relative error of the worst direction, direct solve): 2D 7.65e-16, 3D 1.50e-15 -- rounding;
    asserted: ten times that, 7.7e-15 and 1.5e-14."""
    O = oracle
    base = O.hypercube(dim, n)
    layers = np.array([1.0, 9.0, 3.0, 0.5][:n])[:, None] * np.array([1.0, 2.0, 0.25][:dim])[None, :]   # sigma_kk per layer
    sgrid = np.broadcast_to(layers.reshape((n,) + (1,) * (dim - 1) + (dim,)), (n,) * dim + (dim,)).copy()
    worst = 0.0
    for k in range(dim):
        got = energy_diagonal(O, base, sgrid, grids, k, sides(base, k))
        want = n / (1.0 / layers[:, 0]).sum() if k == 0 else layers[:, k].mean()
        worst = max(worst, abs(got - want) / want)
    print(f"laminate, {dim}D: relative error {worst:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("dim,n,grids", [(2, 4, 3), (3, 2, 3)])
def test_uniaxial_diagonal_is_below_the_all_faces_dirichlet_diagonal(oracle, dim, n, grids):
    """A smaller constrained set gives a larger space and a lower energy minimum."""
    O = oracle
    rng = np.random.default_rng(5)
    base = O.hypercube(dim, n)
    sgrid = np.where(rng.random((n,) * dim + (dim,)) < 0.5, 1.0, 9.0)
    for k in range(dim):
        uni = energy_diagonal(O, base, sgrid, grids, k, sides(base, k))
        full = energy_diagonal(O, base, sgrid, grids, k, default_faces(base.elements))
        assert uni <= full * (1.0 + 1e-13) and uni < full                # (strictly, on a checkerboard)
