"""The CPU statements of the Chebyshev-Jacobi smoother (tests/_cheb_smoother_form.py) that the device is held against
(tests/test_gpu_cheb_smoother.py): the cell-local one and the global one agree, the bound formed from the oracle's operator tables
holds against the largest eigenvalue of D^-1 A on the free nodes, the smoother converges at high contrast with the default ratio,
and the tail that drops the last apply leaves the same x.  For tests/test_gpu_cheb_smoother_cross.py: the statement over full
tensors is the oracle's on the rotated mesh, the bound follows the Dirichlet face set (by more than 1 % between the default set
and none; exactly 0 on a level without a free entry), and the two statements agree under a chosen set.  No GPU."""
import numpy as np
import pytest

from _cheb_smoother_form import (CONVERGENCE_FACTOR, CONVERGENCE_PIN, DEFAULT_RATIO, SAFETY, ChebGlobalForm, bounds_local,
                                 inverse_diagonals, residual_history_cheb, smoothing_steps_cheb, vcycle_cheb)
from _fcg_form import local_problem
from _pcg_smoother_form import convergence_case, residual_history


def _field(rng, n, dim, contrast, isotropic=False):
    pick = rng.random((n,) * dim + (1 if isotropic else dim,)) < 0.5
    return np.where(np.broadcast_to(pick, (n,) * dim + (dim,)), 1.0, float(contrast))


def _start(O, rng, implicit, constraint, states, grids):
    top = states[-1]
    top.x[...] = rng.random(top.x.shape)
    O.broadcast_interfaces(top.x, implicit, grids)
    O.apply_constraint(top.x, grids, constraint, implicit)
    O.local_rhs(top.b, implicit)
    return top


@pytest.mark.parametrize("dim,n,grids,lam,contrast", [(3, 2, 3, 0.7, 100), (2, 4, 4, 1.0, 100), (3, 2, 4, 1.0, 9)])
def test_cell_local_statement_equals_the_global_form(oracle, dim, n, grids, lam, contrast):
    """The smoother alone (one, two and three steps on the top level: x, r) and x, r after one, two and three V-cycles of three
    smoothing steps, both statements with the cell-local statement's bounds: 1e-11 relative, the bound
    tests/test_pcg_smoother_statement.py holds its pair to."""
    O = oracle
    rng = np.random.default_rng(11)
    sgrid = _field(rng, n, dim, contrast)
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, sgrid)
    base_level = O.make_base_level(base, cond, lam)
    top = _start(O, rng, implicit, constraint, states, grids)
    dinvs = inverse_diagonals(O, implicit, ops, grids)
    his = bounds_local(O, implicit, ops, grids, dinvs)
    G = ChebGlobalForm(O, base, sgrid, lam, implicit, grids, dim).set_interval(his)
    x0 = top.x.copy(order="F")
    gx0, gb = G.gather(x0, grids - 1), G.gather_sum(top.b, grids - 1)
    for steps in (1, 2, 3):
        top.x[...] = x0
        smoothing_steps_cheb(O, steps, implicit, ops[-1], top, grids, dinvs[-1], his[-1] / DEFAULT_RATIO, his[-1])
        gx, gr = G.smooth(grids - 1, gx0, gb, steps)
        ex = np.abs(G.gather(top.x, grids - 1) - gx).max() / np.abs(gx).max()
        er = np.abs(G.gather(top.r, grids - 1) - gr).max() / np.abs(gr).max()
        print(f"smoother, {steps} steps: x {ex:.2e}  r {er:.2e}")
        assert ex <= 1e-11 and er <= 1e-11, (steps, ex, er)
    top.x[...] = x0
    gx = gx0
    for cycle in range(3):
        vcycle_cheb(O, implicit, base_level, ops, states, grids, 3, dinvs, his)
        gx, gr = G.vcycle(grids - 1, gx, gb, 3)
        ex = np.abs(G.gather(top.x, grids - 1) - gx).max() / np.abs(gx).max()
        er = np.abs(G.gather(top.r, grids - 1) - gr).max() / max(np.abs(gr).max(), 1e-300)
        print(f"cycle {cycle + 1}: x {ex:.2e}  r {er:.2e}")
        assert ex <= 1e-11 and er <= 1e-11, (cycle, ex, er)


def _perturbed_problem(O, grids, lam, sgrid):
    """3D n = 2 with the inner nodes of the base mesh moved: every cell has its own geometry"""
    base = O.hypercube(3, 2)
    rng = np.random.default_rng(2)
    inner = O.list_interior_nodes(base)
    base.nodes[inner] += 0.08 * (rng.random((len(inner), 3)) - 0.5)
    cond = O.conductivity_per_element(O.hypercube(3, 2), sgrid, (0.0,) * 3)
    implicit = O.ImplicitFineGrid.create(base, grids)
    constraint = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(base))
    ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(m), O.mass_matrix(m), constraint, lam, cond)
           for m in implicit.reference.levels]
    return base, cond, implicit, ops


def _assembled(O, base, implicit, ops, k):
    """The assembled matrix of level k and its free nodes from the cell-local operator alone: unit-vector probes would cost Nf
    applies, so it is assembled from the oracle's tables -- global ids from the coordinates of the repeated nodes."""
    import scipy.sparse as sp
    A = ops[k - 1]
    dim = base.dim
    _, Jinv, det = O.cell_geometry(base)
    P = np.einsum("eki,ek,ekj->eij", Jinv, A.sigmas, Jinv)
    nf, ne = A.mass.shape[0], base.nelements()
    pts = np.round(implicit.construct_full_grid(k).reshape(-1, dim) * 2 ** 20).astype(np.int64)
    _, gid = np.unique(pts, axis=0, return_inverse=True)
    gid = np.asarray(gid).reshape(ne, nf)
    n = int(gid.max()) + 1
    M = sp.csr_matrix((n, n))
    for c in range(ne):
        loc = (A.lam * det[c]) * A.mass
        for a in range(dim):
            for b in range(dim):
                loc = loc + (det[c] * P[c, a, b]) * A.diffusion_terms[a][b]
        loc = loc.tocoo()
        M = M + sp.csr_matrix((loc.data, (gid[c][loc.row], gid[c][loc.col])), shape=(n, n))
    ones = np.ones((nf, ne), order="F")
    O.apply_constraint(ones, k, A.constraint, implicit)
    free = np.zeros(n, dtype=bool)
    free[gid.T.reshape(-1, order="F")[ones.reshape(-1, order="F") == 1.0]] = True
    return M.tocsr(), free


def _lambda_max(M, free):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    idx = np.flatnonzero(free)
    A = M[idx][:, idx]
    s = sp.diags(1.0 / np.sqrt(A.diagonal()))
    return float(spla.eigsh((s @ A @ s).tocsc(), k=1, which="LA", tol=1e-10, return_eigenvectors=False)[0])


@pytest.mark.parametrize("name", ["convergence_case", "isotropic_lam0", "isotropic_lam1", "2d_n8", "perturbed"])
def test_the_bound_holds(oracle, name):
    """lambda_hi >= lambda_max(D^-1 A) on the free nodes (Lanczos) on every level >= 2, lambda_hi / 1.02 >= the assembled matrix's own
    Gershgorin bound (|sum_c a^c_ij| <= sum_c |a^c_ij|), and lambda_hi <= 1.02 (dim + 1) -- observed under the default Dirichlet set
    of these meshes, not a property of the bound (test_the_bound_follows_the_face_set)."""
    O = oracle
    if name == "perturbed":
        grids, dim = 3, 3
        sgrid = _field(np.random.default_rng(4), 2, 3, 100)
        base, cond, implicit, ops = _perturbed_problem(O, grids, 0.3, sgrid)
        G = None
    else:
        if name == "convergence_case":
            base, cond, implicit, constraint, ops, states, _, _, sgrid = convergence_case(O)
            dim, n, grids, lam = 3, 4, 4, 0.0
        else:
            dim, n, grids, lam, iso = {"isotropic_lam0": (3, 4, 4, 0.0, True), "isotropic_lam1": (3, 4, 4, 1.0, True),
                                       "2d_n8": (2, 8, 5, 0.0, False)}[name]
            sgrid = _field(np.random.default_rng(3), n, dim, 100, iso)
            base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, sgrid)
        G = ChebGlobalForm(O, base, sgrid, lam, implicit, grids, dim)
    dinvs = inverse_diagonals(O, implicit, ops, grids)
    his = bounds_local(O, implicit, ops, grids, dinvs)
    for k in range(2, grids + 1):
        if G is not None:
            true, gersh = G.lambda_max(k - 1), G.gershgorin(k - 1)
        else:
            M, free = _assembled(O, base, implicit, ops, k)
            true = _lambda_max(M, free)
            d = np.where(free, 1.0 / np.where(free, M.diagonal(), 1.0), 0.0)
            gersh = float((d * np.asarray(abs(M).sum(axis=1)).reshape(-1)).max())
        print(f"{name} level {k}: lambda_max {true:.4f}  Gershgorin {gersh:.4f}  lambda_hi {his[k - 1]:.4f}")
        assert his[k - 1] >= true, (k, his[k - 1], true)
        assert his[k - 1] / SAFETY >= gersh * (1.0 - 1e-12), (k, his[k - 1], gersh)
        assert his[k - 1] <= SAFETY * (dim + 1) * (1.0 + 1e-12), (k, his[k - 1])


def test_convergence_pin(oracle):
    """convergence_case with the default ratio: the last-six factor of the 14 residual norms within the statement's own measured
    value + 0.03 (the margin test_convergence_at_contrast_100 gives kind 1), the residual after 14 cycles below the CG smoother's."""
    O = oracle
    case = convergence_case(O)
    rs = residual_history_cheb(O, case)
    factor = (rs[13] / rs[7]) ** (1.0 / 6.0)
    cg = residual_history(O, case, "cg")
    print(f"chebyshev, ratio {DEFAULT_RATIO:g}: factor {factor:.4f}  residuals {rs[0]:.3e} ... {rs[13]:.3e}  (cg: {cg[13]:.3e})")
    assert abs(factor - CONVERGENCE_FACTOR) <= 2e-3, factor          # the pin is the statement's own number
    assert factor <= CONVERGENCE_PIN
    assert rs[13] < cg[13]


@pytest.mark.parametrize("steps", [1, 2, 3])
def test_the_dead_tail_leaves_the_same_x(oracle, steps):
    """DeadXp (no apply for the last step) and ScratchP against Full: x bit for bit; ScratchP's r as well."""
    O = oracle
    dim, n, grids, lam = 3, 2, 3, 0.7
    rng = np.random.default_rng(6)
    base, cond, implicit, constraint, ops, states = local_problem(O, dim, n, grids, lam, _field(rng, n, dim, 100))
    top = _start(O, rng, implicit, constraint, states, grids)
    dinvs = inverse_diagonals(O, implicit, ops, grids)
    hi = bounds_local(O, implicit, ops, grids, dinvs)[-1]
    x0 = top.x.copy(order="F")
    out = {}
    for tail in ("full", "scratch_p", "dead_xp"):
        top.x[...] = x0
        smoothing_steps_cheb(O, steps, implicit, ops[-1], top, grids, dinvs[-1], hi / DEFAULT_RATIO, hi, tail=tail)
        out[tail] = (top.x.copy(), top.r.copy())
    assert np.array_equal(out["full"][0], out["dead_xp"][0])
    assert np.array_equal(out["full"][0], out["scratch_p"][0])
    assert np.array_equal(out["full"][1], out["scratch_p"][1])
    assert not np.array_equal(out["full"][0], x0)


# ---- full tensors, chosen faces ------------------------------------------------------------------------------------------------
def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("dim,n,grids", [(3, 2, 3), (2, 4, 4)])
def test_tensor_statement_is_the_oracle_on_the_rotated_mesh(oracle, dim, n, grids):
    """The statement over tests/_tensor_sigma_form.py's TensorOp with sigma = Q D Q^T in every cell (contrast 100) against the same
    statement over the oracle's own diagonal operator on the mesh x -> Q^T x (tests/test_tensor_sigma_statement.py's pair): the
    bound of every level, x and r of one, two and three smoothing steps and of three V-cycles, 1e-12 relative."""
    from test_tensor_sigma_statement import rotated_pair
    O = oracle
    prob, (mr, cond, implicit, constraint, ops, states, base_level), Q, D, x0, b0 = rotated_pair(O, dim, n, grids)
    dinvs, odinvs = inverse_diagonals(O, prob.implicit, prob.ops, grids), inverse_diagonals(O, implicit, ops, grids)
    his, ohis = bounds_local(O, prob.implicit, prob.ops, grids, dinvs), bounds_local(O, implicit, ops, grids, odinvs)
    for k in range(2, grids + 1):
        print(f"level {k}: bound {his[k - 1]:.12f}, on the rotated mesh {ohis[k - 1]:.12f}")
        assert abs(his[k - 1] - ohis[k - 1]) <= 1e-12 * ohis[k - 1]
        assert _rel(dinvs[k - 1], odinvs[k - 1]) <= 1e-12
    top, otop = prob.states[-1], states[-1]
    for steps in (1, 2, 3):
        prob.start(x0, b0)
        otop.x[...] = top.x
        otop.b[...] = b0
        smoothing_steps_cheb(O, steps, prob.implicit, prob.ops[-1], top, grids, dinvs[-1], his[-1] / DEFAULT_RATIO, his[-1])
        smoothing_steps_cheb(O, steps, implicit, ops[-1], otop, grids, odinvs[-1], ohis[-1] / DEFAULT_RATIO, ohis[-1])
        ex, er, ep = _rel(top.x, otop.x), _rel(top.r, otop.r), _rel(top.p, otop.p)
        print(f"{steps} steps: x {ex:.2e}  r {er:.2e}  p {ep:.2e}")
        assert ex <= 1e-12 and er <= 1e-12 and ep <= 1e-12, (steps, ex, er, ep)
    prob.start(x0, b0)
    otop.x[...] = top.x
    for cycle in range(3):
        vcycle_cheb(O, prob.implicit, prob.base_level, prob.ops, prob.states, grids, 3, dinvs, his)
        vcycle_cheb(O, implicit, base_level, ops, states, grids, 3, odinvs, ohis)
        ex, er = _rel(top.x, otop.x), _rel(top.r, otop.r)
        print(f"cycle {cycle + 1}: x {ex:.2e}  r {er:.2e}")
        assert ex <= 1e-12 and er <= 1e-12, (cycle, ex, er)


# lambda_hi_local per level >= 2 of _cheb_smoother_form.FACE_SET_CASES under its three face sets, to the digits it was first computed to
_FACE_SET_BOUNDS = {3: {"default": (2.8804, 3.0454, 3.0456), "empty": (3.1850, 3.1858, 3.1860), "every": (0.0, 3.0454, 3.0456)},
                    2: {"default": (2.2043, 2.2074, 2.2076, 2.2076), "empty": (6.2666, 6.3592, 6.3828, 6.3887),
                        "every": (0.0, 2.2074, 2.2076, 2.2076)}}


@pytest.fixture(scope="module")
def face_set_cases(oracle):
    from _cheb_smoother_form import FaceSetCase
    return {dim: FaceSetCase(oracle, dim) for dim in (3, 2)}


@pytest.mark.parametrize("dim", [3, 2])
def test_the_bound_follows_the_face_set(face_set_cases, dim):
    """What lets tests/test_gpu_cheb_smoother_cross.py fail on a bound left over from another mask: between the default set and
    the lifted constraint the bound of at least one level moves by more than 1 % (the device is held to 1e-11), in both dimensions;
    with every face of every cell constrained level 2 has no free entry and its bound is exactly 0.  The ceiling 1.02 (dim + 1) is
    a property of the default set on these meshes: in 2D the lifted constraint exceeds it."""
    c = face_set_cases[dim]
    his = {name: c.under(faces)[3][1:] for name, faces in c.sets.items()}
    for name, hi in his.items():
        print(f"{dim}D, {name}: " + " / ".join(f"{h:.4f}" for h in hi))
        assert np.abs(np.array(hi) - np.array(_FACE_SET_BOUNDS[dim][name])).max() <= 1e-4, (name, hi)
    move = max(abs(a - b) / min(a, b) for a, b in zip(his["default"], his["empty"]))
    print(f"{dim}D: default against empty, largest relative move {move:.3f}")
    assert move > 0.01
    assert his["every"][0] == 0.0 and all(h > 0.0 for h in his["every"][1:])
    assert not c.under(c.sets["every"])[2][1].any()
    assert all(h <= SAFETY * (dim + 1) for h in his["default"])
    if dim == 2:
        assert max(his["empty"]) > SAFETY * (dim + 1)


@pytest.mark.parametrize("which", ["empty", "mid"])
@pytest.mark.parametrize("dim", [3, 2])
def test_both_statements_agree_under_a_chosen_face_set(face_set_cases, dim, which):
    """The cell-local statement under the oracle's constraint of the set against the global form whose constrained nodes come from
    the set by geometry, with the constraint lifted and with an internal plane: the smoother (one to three steps) and three V-cycles
    of three steps, both with the cell-local statement's bounds, 1e-11 as test_cell_local_statement_equals_the_global_form."""
    from _cheb_smoother_form import ChebFaceSetForm
    from _dirichlet_faces_form import mid_plane_and_sides, oracle_base_level
    c = face_set_cases[dim]
    O, grids = c.O, c.levels
    faces = c.sets["empty"] if which == "empty" else mid_plane_and_sides(O.hypercube(dim, 2))
    cons, ops, dinvs, his = c.under(faces)
    G = ChebFaceSetForm(O, c.mesh, None, c.lam, c.impl, grids, dim, faces, cond=c.sig).set_interval(his)
    states = [O.LevelState.create(c.mesh.nelements(), c.impl.nf(i + 1)) for i in range(grids)]
    top = states[-1]
    rng = np.random.default_rng(31)
    x0 = np.asfortranarray(rng.random(top.x.shape))
    O.broadcast_interfaces(x0, c.impl, grids)
    O.apply_constraint(x0, grids, cons, c.impl)
    top.b[...] = rng.standard_normal(top.x.shape)
    gx0, gb = G.gather(x0, grids - 1), G.gather_sum(top.b, grids - 1)
    for steps in (1, 2, 3):
        top.x[...] = x0
        smoothing_steps_cheb(O, steps, c.impl, ops[-1], top, grids, dinvs[-1], his[-1] / DEFAULT_RATIO, his[-1])
        gx, gr = G.smooth(grids - 1, gx0, gb, steps)
        ex, er = _rel(G.gather(top.x, grids - 1), gx), _rel(G.gather(top.r, grids - 1), gr)
        print(f"smoother, {steps} steps: x {ex:.2e}  r {er:.2e}")
        assert ex <= 1e-11 and er <= 1e-11, (steps, ex, er)
    top.x[...] = x0
    gx = gx0
    base_level = oracle_base_level(O, c.mesh, c.sig, c.lam, faces)
    for cycle in range(3):
        vcycle_cheb(O, c.impl, base_level, ops, states, grids, 3, dinvs, his)
        gx, gr = G.vcycle(grids - 1, gx, gb, 3)
        ex, er = _rel(G.gather(top.x, grids - 1), gx), _rel(G.gather(top.r, grids - 1), gr)
        print(f"cycle {cycle + 1}: x {ex:.2e}  r {er:.2e}")
        assert ex <= 1e-11 and er <= 1e-11, (cycle, ex, er)
