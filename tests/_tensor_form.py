"""The homogenized TENSOR from one run, stated with the oracle's primitives and numpy.

The correctors are linear in the direction, so d corrector solves (one per unit vector e_i) are enough; the off-diagonal entries
follow from cross integrals of the correctors.  With v_k^i the corrector of e_i at outer step k, b^i = rhs_a.e_i.grad(v) and all
sums over the first `nint` cells (as in integrate_first_term / integrate_terms):

    Mq(v; w) = sum_c |J_c| sum_i w_i (M v)_i          Lq(v; s) = sum_c |J_c| sum_i v_i s_i

    step 0     I_0^{ij} = 1/2 [Lq(v_0^i; b^j) + Lq(v_0^j; b^i)] + Mq(v_0^i; v_0^j)
    step k>=1  I_k^{ij} = Mq(v_k^i; v_k^j) + 1/2 [Mq(v_k^j; v_{k-1}^i) + Mq(v_k^i; v_{k-1}^j)]
    Sigma = sum_k 2^k I_k / area_k

For i = j these are integrate_first_term and integrate_terms, which is what the cycle loop stops on; xi' Sigma xi is what
oracle.checkerboard_homogenization(xi=xi) returns once both have converged.  The radii and the shrink schedule do not depend on
the direction, so all directions share the outer loop.  The loop below is oracle.checkerboard_homogenization's, direction by
direction inside each outer step.
"""
import numpy as np

from oracle import oracle as O


def pair_mass(v, w, det, nsubset, mass):
    """Mq(v; w)"""
    run = np.einsum("ie,ie->e", w[:, :nsubset], mass @ v[:, :nsubset])
    return float(np.sum(run * det[:nsubset]))


def pair_load(v, s, det, nsubset):
    """Lq(v; s)"""
    run = np.einsum("ie,ie->e", v[:, :nsubset], s[:, :nsubset])
    return float(np.sum(run * det[:nsubset]))


def polarised(scalar_of_xi, dim):
    """The symmetric tensor from d (d + 1) / 2 scalar runs: S_ii = q(e_i), S_ij = q((e_i + e_j) / sqrt 2) - (S_ii + S_jj) / 2."""
    S = np.zeros((dim, dim))
    E = np.eye(dim)
    for i in range(dim):
        S[i, i] = scalar_of_xi(E[i])
    for i in range(dim):
        for j in range(i + 1, dim):
            S[i, j] = S[j, i] = scalar_of_xi((E[i] + E[j]) / np.sqrt(2.0)) - 0.5 * (S[i, i] + S[j, j])
    return S


def checkerboard_homogenization_tensor(n=4, dim=2, refinements=2, smoothing_steps_=3, tolerance=1e-4, seed=0,
                                       sigma_values=(1.0, 9.0), max_cycles=1000, x0=None, sigma_grid=None):
    """-> (Sigma, history); history rows (k, direction, cycle, rnorm, Sigma_ii so far, |change|)"""
    rng = np.random.default_rng(seed)
    lam = 1.0
    Sigma = np.zeros((dim, dim))
    box_radius = O.compute_box_radius(0, n)
    boundary_layer = O.compute_boundary_layer(lam, n)
    total_radius = box_radius + boundary_layer
    width = 2 * total_radius
    base = O.order_nodes_and_elements_by_magnitude(O.hypercube(dim, width, origin=(-float(total_radius),) * dim))
    if sigma_grid is None:
        sigma_grid = np.where(rng.random((width,) * dim + (dim,)) < 0.5, sigma_values[0], sigma_values[1])
    cond = O.conductivity_per_element(base, sigma_grid, (total_radius + 1.0,) * dim)
    total_grids = refinements + 1
    implicit = O.ImplicitFineGrid.create(base, total_grids)
    constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(base))
    diff_terms = [O.build_local_diffusion_operators(m) for m in implicit.reference.levels]
    mass_terms = [O.mass_matrix(m) for m in implicit.reference.levels]
    mass = mass_terms[-1]
    ops = [O.L2PlusDivAGrad(d, m, constraint, lam, cond) for d, m in zip(diff_terms, mass_terms)]
    states = [O.LevelState.create(base.nelements(), implicit.nf(i + 1)) for i in range(total_grids)]
    top = states[-1]
    if x0 is None:
        x0 = rng.random(top.x.shape)
    dphis = O.partial_derivatives_functionals(implicit.reference.levels[-1])
    E = np.eye(dim)
    V = [None] * dim          # v_k^i
    Vprev = [None] * dim      # v_{k-1}^i with the constraint of step k
    history = []
    for k in range(n + 1):
        base_level = O.make_base_level(base, cond, lam)
        _, _, det = O.cell_geometry(base)
        nint = O.find_elements_in_radius(base, box_radius)
        area = O.integrate_area(mass, implicit, nint)
        for d in range(dim):
            if k == 0:
                top.x[...] = x0
                O.broadcast_interfaces(top.x, implicit, total_grids)
                O.apply_constraint(top.x, total_grids, constraint, implicit)
                O.rhs_axi_grad_v(top.b, dphis, implicit, cond, E[d])
            else:
                top.x[...] = Vprev[d]
                O.next_rhs(top.b, top.x, implicit, mass, lam)
            dsig, dsig_prev = 0.0, 0.0
            for i in range(1, max_cycles + 1):
                O.vcycle(implicit, base_level, ops, states, total_grids, smoothing_steps_)
                if k == 0:
                    integral = O.integrate_first_term(top.x, dphis, implicit, nint, mass, cond, E[d])
                else:
                    integral = O.integrate_terms(top.x, Vprev[d], implicit, nint, mass)
                dsig = 2.0 ** k * integral / area
                O.zero_out_all_but_one(top.r, implicit, total_grids)
                history.append((k, d, i, float(np.linalg.norm(top.r)), Sigma[d, d] + dsig, abs(dsig - dsig_prev)))
                if abs(dsig - dsig_prev) < tolerance:
                    break
                dsig_prev = dsig
            Sigma[d, d] += dsig
            V[d] = top.x.copy(order="F")
        for i in range(dim):                             # the off-diagonal increments, from the pair forms
            for j in range(i + 1, dim):
                if k == 0:
                    bi, bj = np.zeros_like(top.b), np.zeros_like(top.b)
                    O.rhs_axi_grad_v(bi, dphis, implicit, cond, E[i])
                    O.rhs_axi_grad_v(bj, dphis, implicit, cond, E[j])
                    integral = 0.5 * (pair_load(V[i], bj, det, nint) + pair_load(V[j], bi, det, nint)) + \
                        pair_mass(V[i], V[j], det, nint, mass)
                else:
                    integral = pair_mass(V[i], V[j], det, nint, mass) + \
                        0.5 * (pair_mass(V[j], Vprev[i], det, nint, mass) + pair_mass(V[i], Vprev[j], det, nint, mass))
                Sigma[i, j] += 2.0 ** k * integral / area
                Sigma[j, i] = Sigma[i, j]
        lam /= 2
        box_radius = O.compute_box_radius(k + 1, n)
        boundary_layer = O.compute_boundary_layer(lam, n)
        if box_radius + boundary_layer > total_radius:
            break
        total_radius = box_radius + boundary_layer
        nn_keep = O.find_nodes_in_radius(base, total_radius)
        ne_keep = O.find_elements_in_radius(base, total_radius)
        base = O.Mesh(base.nodes[:nn_keep], np.ascontiguousarray(base.elements[:ne_keep]))
        cond = np.ascontiguousarray(cond[:ne_keep])
        constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(base))
        states = [O.LevelState(*(np.asfortranarray(a[:, :ne_keep]) for a in (s.x, s.b, s.r, s.p, s.Ap))) for s in states]
        top = states[-1]
        implicit = O.ImplicitFineGrid(total_grids, implicit.reference, O.interfaces(base), base)
        for d in range(dim):
            Vprev[d] = np.asfortranarray(V[d][:, :ne_keep])
            O.apply_constraint(Vprev[d], total_grids, constraint, implicit)
        ops = [O.L2PlusDivAGrad(d, m, constraint, lam, cond) for d, m in zip(diff_terms, mass_terms)]
    return Sigma, history
