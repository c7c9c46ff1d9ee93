"""
The Chebyshev-Jacobi smoother where its bound has to follow something: the Dirichlet faces the caller chooses, full tensors per
cell, long smoothings, a level without a free entry, coefficients that are not finite.  lambda_hi = 1.02 max(dinv o interface-summed
|row sums|) depends on the operator, on the mask (k_dinv_finish writes dinv = 0 on constrained entries, so their rows leave the
maximum) and on the domain; a bound left over from another mask is too small, and the polynomial then amplifies the top of the
spectrum.  tests/test_cheb_smoother_statement.py holds the evidence that these tests can fail: between the default set and the
lifted constraint the bound moves by 10 % in 3D and by 190 % in 2D, against the 1e-11 asked here.

The two cases are _cheb_smoother_form.FACE_SET_CASES: hypercube(3, 2), 48 cells, levels 2-4, and hypercube(2, 2), 8 cells, levels
2-5, sigma in {1, 100}, lambda 0.7, the nodes moved by 0.2.  Tolerances are the project's: the bound 1e-11, x, r, p of a smoother
1e-10, x 1e-9 and r 1e-8 after V-cycles.  No test here asserts the ceiling 1.02 (dim + 1): it does not hold once the constraint is
lifted.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver
from homogenization_jl_amd._lib import HmgError

import _tensor_sigma_form as T
from _cheb_smoother_form import (DEFAULT_RATIO, FACE_SET_CASES, ChebFaceSetForm, bounds_local, face_sets, inverse_diagonals,
                                 lambda_hi_local, smoothing_steps_cheb, vcycle_cheb)
from _dirichlet_faces_form import default_faces, one_based, oracle_base_level, oracle_constraint
from test_gpu_dirichlet_faces import Case, mid_plane_and_sides
from test_gpu_pcg_smoother import Problem, _cube, ctx, relerr  # noqa: F401

pytestmark = pytest.mark.gpu

LAM = 0.7


def _case(O, ctx, dim, smoother="chebyshev"):
    """(Case under the default set named face by face, the face sets chosen on the lattice)"""
    seed, levels = FACE_SET_CASES[dim]
    m = O.hypercube(dim, 2)
    sets = dict(face_sets(m), mid=mid_plane_and_sides(m))
    return Case(O, ctx, m, levels, sets["default"], lam=LAM, seed=seed, perturb=0.2, smoother=smoother, values=(1.0, 100.0)), sets


def _put(c, faces):
    """the set on the device (None: the default one, by the call's own default) and on the oracle"""
    c.g.set_dirichlet_faces(None if faces is None else one_based(faces))
    c.faces = default_faces(c.mesh.elements) if faces is None else faces
    c.cons = oracle_constraint(c.O, c.mesh, c.faces)
    c._ops = {}


def _statement(c):
    """(inverse diagonals, bounds) of the case under its current set: entry l - 1 for level l"""
    dinvs = inverse_diagonals(c.O, c.impl, c.ops(), c.levels)
    return dinvs, bounds_local(c.O, c.impl, c.ops(), c.levels, dinvs)


def _check_smoother(ctx, c, lev, steps, dinv, hi, A=None, op=None, g=None):
    """hmg_smooth against the statement run with the STATEMENT's bound: x, r, p 1e-10; "cheb_applies" rises by `steps`"""
    O = c.O
    g, A, op = g or c.g, A or c.A, op or c.op(lev)
    st = c.state(lev)
    dst = hmg.LevelState(g, lev)
    dst.x.from_host(st.x)
    dst.b.from_host(st.b)
    a0 = ctx.counter("cheb_applies")
    smoothing_steps_cheb(O, steps, c.impl, op, st, lev, dinv, hi / DEFAULT_RATIO, hi)
    hmg.smoothing_steps(steps, g, A, dst, lev)
    assert ctx.counter("cheb_applies") == a0 + steps
    ex, er, ep = relerr(dst.x.to_host(), st.x), relerr(dst.r.to_host(), st.r), relerr(dst.p.to_host(), st.p)
    print(f"level {lev}, {steps} steps: x {ex:.2e}  r {er:.2e}  p {ep:.2e}")
    dst.close()
    assert ex <= 1e-10 and er <= 1e-10 and ep <= 1e-10, (lev, steps, ex, er, ep)


@pytest.mark.parametrize("dim", [3, 2])
def test_bound_and_smoother_follow_the_face_set(oracle, ctx, dim):
    """One grid, set_smoother("chebyshev") first and the bounds of every level queried, so that they are cached; then an internal
    plane with two outer sides, the empty list, None.  After each setter: hmg_grid_smoother_bounds of every level >= 2 is the
    statement's under the same constraint (1e-11), the inverse diagonal has the statement's zeros, "smoother_bound_builds" has risen
    by exactly levels - 1 and a second query forms nothing, and hmg_smooth with one, two and three steps on every level is the
    statement's with the statement's own bound.  After None the bounds are the bits of the first query."""
    c, sets = _case(oracle, ctx, dim)
    levels = c.levels
    try:
        n0 = ctx.counter("smoother_bound_builds")
        first = [hmg.smoother_bounds(c.g, lev) for lev in range(2, levels + 1)]
        assert ctx.counter("smoother_bound_builds") == n0 + levels - 1
        seen = [first]
        for name, faces in (("mid", sets["mid"]), ("empty", sets["empty"]), ("None", None)):
            _put(c, faces)
            dinvs, his = _statement(c)
            n0 = ctx.counter("smoother_bound_builds")
            got = [hmg.smoother_bounds(c.g, lev) for lev in range(2, levels + 1)]
            assert ctx.counter("smoother_bound_builds") == n0 + levels - 1, name
            assert got == [hmg.smoother_bounds(c.g, lev) for lev in range(2, levels + 1)]
            assert ctx.counter("smoother_bound_builds") == n0 + levels - 1, name
            for lev, (lo, hi) in zip(range(2, levels + 1), got):
                want = his[lev - 1]
                print(f"{name}, level {lev}: lambda_hi {hi:.12f}, statement {want:.12f}, relative difference {abs(hi - want) / want:.2e}")
                assert abs(hi - want) <= 1e-11 * want, (name, lev, hi, want)
                assert lo == hi / DEFAULT_RATIO
                d = hmg.smoother_diag(c.g, lev)
                np.testing.assert_array_equal(d.to_host() == 0.0, dinvs[lev - 1] == 0.0, err_msg=f"{name}, level {lev}")
                d.close()
            assert ctx.counter("smoother_bound_builds") == n0 + levels - 1, name
            for lev in range(2, levels + 1):
                for steps in (1, 2, 3):
                    _check_smoother(ctx, c, lev, steps, dinvs[lev - 1], his[lev - 1])
            seen.append(got)
        assert seen[3] == first                                          # back on the default set: the bits of the first query
        assert seen[1] != first and seen[2] != first and seen[1] != seen[2]
    finally:
        c.close()


@pytest.mark.parametrize("which", ["empty", "mid"])
@pytest.mark.parametrize("dim", [3, 2])
def test_vcycles_under_a_chosen_face_set(oracle, ctx, dim, which):
    """Three hmg_vcycle's (3 / 2 steps) with the constraint lifted and with an internal plane, on a grid whose bounds were formed
    under the default set first: x 1e-9 and r 1e-8 against the cell-local statement and against the global form whose constrained
    nodes come from the set by geometry; "cheb_applies" per cycle as tests/test_gpu_cheb_smoother.py counts them."""
    O = oracle
    c, sets = _case(O, ctx, dim)
    levels = c.levels
    try:
        stale = [hmg.smoother_bounds(c.g, lev) for lev in range(2, levels + 1)]
        _put(c, sets[which])
        dinvs, his = _statement(c)
        G = ChebFaceSetForm(O, c.mesh, None, LAM, c.impl, levels, dim, c.faces, cond=c.sig).set_interval(his)
        sts = [O.LevelState.create(c.mesh.nelements(), c.impl.nf(i + 1)) for i in range(levels)]
        sts[-1] = c.state(levels)
        top = sts[-1]
        gx, gb = G.gather(top.x, levels - 1), G.gather_sum(top.b, levels - 1)
        dsts = [hmg.LevelState(c.g, i + 1) for i in range(levels)]
        dsts[-1].x.from_host(top.x)
        dsts[-1].b.from_host(top.b)
        base, dbase = oracle_base_level(O, c.mesh, c.sig, LAM, c.faces), hmg.BaseLevel(c.g)
        for cyc in range(3):
            a0 = ctx.counter("cheb_applies")
            hmg.vcycle(c.g, dbase, [c.A] * levels, dsts, levels, 3)
            # the top level's pre-smoother 3 - 1 applies, its post-smoother 3; every level between 2 and the top 2 - 1 and 2 - 1
            assert ctx.counter("cheb_applies") - a0 == (3 - 1) + 3 + 2 * (levels - 2)
            vcycle_cheb(O, c.impl, base, c.ops(), sts, levels, 3, dinvs, his)
            gx, gr = G.vcycle(levels - 1, gx, gb, 3)
            dx, dr = dsts[-1].x.to_host(), dsts[-1].r.to_host()
            eg, egr = relerr(G.gather(dx, levels - 1), gx), relerr(G.gather(dr, levels - 1), gr)
            el, elr = relerr(dx, top.x), relerr(dr, top.r)
            print(f"{which} cycle {cyc + 1}: global x {eg:.2e} r {egr:.2e}  cell-local x {el:.2e} r {elr:.2e}")
            assert eg <= 1e-9 and egr <= 1e-8 and el <= 1e-9 and elr <= 1e-8, (cyc, eg, egr, el, elr)
        assert [hmg.smoother_bounds(c.g, lev) for lev in range(2, levels + 1)] != stale
        for s in dsts:
            s.close()
    finally:
        c.close()


def test_given_bounds_stay_given(oracle, ctx):
    """With lambda_hi given for every level a face change and a set_lambda form nothing: "smoother_bound_builds" is unchanged and
    hmg_grid_smoother_bounds returns the caller's numbers."""
    c, sets = _case(oracle, ctx, 3)
    levels = c.levels
    try:
        his = [0.0] + [3.5 + 0.25 * lev for lev in range(2, levels + 1)]
        c.g.set_smoother("chebyshev", lambda_hi=his, ratio=16.0)
        n0 = ctx.counter("smoother_bound_builds")
        given = [(h / 16.0, h) for h in his[1:]]
        assert [hmg.smoother_bounds(c.g, lev) for lev in range(2, levels + 1)] == given
        d0 = hmg.smoother_diag(c.g, levels).to_host()
        for faces in (sets["mid"], sets["empty"], None):
            _put(c, faces)
            assert [hmg.smoother_bounds(c.g, lev) for lev in range(2, levels + 1)] == given
        c.A.lam = LAM + 0.25                                             # hmg_grid_set_lambda
        assert [hmg.smoother_bounds(c.g, lev) for lev in range(2, levels + 1)] == given
        d1 = hmg.smoother_diag(c.g, levels).to_host()
        assert not np.array_equal(d0, d1)                                # (the inverse diagonal was formed again, the bound was not)
        st = hmg.LevelState(c.g, levels)
        st.b.rand(4)
        hmg.smoothing_steps(3, c.g, c.A, st, levels)
        assert np.isfinite(st.x.to_host()).all()
        st.close()
        assert ctx.counter("smoother_bound_builds") == n0
    finally:
        c.close()


class _TensorCase:
    """tests/_tensor_sigma_form.py's Problem on a perturbed mesh, with the members _check_smoother reads"""

    def __init__(self, O, dim, seed, sig=None):
        self.O = O
        levels = FACE_SET_CASES[dim][1]
        rng = np.random.default_rng(seed)
        base = O.hypercube(dim, 2)
        base.nodes = base.nodes + 0.2 * (rng.random(base.nodes.shape) - 0.5)
        self.sig = T.random_spd(rng, base.nelements(), dim) if sig is None else sig
        self.prob = T.Problem(O, base, levels, LAM, self.sig)
        self.rng, self.impl, self.levels, self.mesh = rng, self.prob.implicit, levels, base

    def state(self, lev):
        O, p = self.O, self.prob
        st = O.LevelState.create(self.mesh.nelements(), self.impl.nf(lev))
        st.x[...] = p.rand(self.rng, lev)
        O.broadcast_interfaces(st.x, self.impl, lev)
        O.apply_constraint(st.x, lev, p.constraint, self.impl)
        st.b[...] = p.rand(self.rng, lev)
        return st

    def device(self, ctx, sig=None):
        g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(self.mesh.nodes, self.mesh.elements + 1), self.levels)
        g.set_smoother("chebyshev")
        return g, hmg.L2PlusDivAGrad(g, LAM, self.sig if sig is None else sig)


@pytest.mark.parametrize("dim", [3, 2])
def test_full_tensors(oracle, ctx, dim):
    """One random symmetric positive definite tensor per cell, eigenvalues 1 .. 100, on the perturbed meshes of the two cases:
    the bound of every level (1e-11), hmg_smooth with one to three steps on every level (1e-10) and two V-cycles (x 1e-9, r 1e-8)
    against the statement over the tensor operator, which tests/test_cheb_smoother_statement.py ties to the oracle."""
    O = oracle
    c = _TensorCase(O, dim, 50 + dim)
    p, levels = c.prob, c.levels
    g, A = c.device(ctx)
    try:
        dinvs = inverse_diagonals(O, c.impl, p.ops, levels)
        his = bounds_local(O, c.impl, p.ops, levels, dinvs)
        for lev in range(2, levels + 1):
            hi = hmg.smoother_bounds(g, lev)[1]
            print(f"level {lev}: lambda_hi {hi:.12f}, statement {his[lev - 1]:.12f}")
            assert abs(hi - his[lev - 1]) <= 1e-11 * his[lev - 1], (lev, hi, his[lev - 1])
            for steps in (1, 2, 3):
                _check_smoother(ctx, c, lev, steps, dinvs[lev - 1], his[lev - 1], A=A, op=p.ops[lev - 1], g=g)
        rng = np.random.default_rng(6)
        p.start(p.rand(rng, levels), p.rand(rng, levels))
        dst = [hmg.LevelState(g, i + 1) for i in range(levels)]
        dst[-1].x.from_host(p.states[-1].x)
        dst[-1].b.from_host(p.states[-1].b)
        bl = hmg.BaseLevel(g)
        for cyc in range(2):
            vcycle_cheb(O, c.impl, p.base_level, p.ops, p.states, levels, 3, dinvs, his)
            hmg.vcycle(g, bl, [A] * levels, dst, levels, 3)
            ex, er = relerr(dst[-1].x.to_host(), p.states[-1].x), relerr(dst[-1].r.to_host(), p.states[-1].r)
            print(f"cycle {cyc + 1}: x {ex:.2e}  r {er:.2e}")
            assert ex <= 1e-9 and er <= 1e-8, (cyc, ex, er)
        for s in dst:
            s.close()
    finally:
        g.close()


@pytest.mark.parametrize("dim", [3, 2])
def test_diagonal_tensors_give_the_bits_of_the_diagonal_entry(oracle, ctx, dim):
    """A diagonal field given as full tensors against hmg_grid_set_operator on the same numbers: the bounds of every level and x,
    r after two V-cycles, bit for bit."""
    O = oracle
    levels = FACE_SET_CASES[dim][1]
    rng = np.random.default_rng(60 + dim)
    diag = rng.choice([1.0, 100.0], size=(O.hypercube(dim, 2).nelements(), dim))
    full = np.zeros(diag.shape + (dim,))
    full[:, np.arange(dim), np.arange(dim)] = diag
    c = _TensorCase(O, dim, 60 + dim, sig=full)
    out = []
    for sig in (full, diag):
        g, A = c.device(ctx, sig=sig)
        bounds = [hmg.smoother_bounds(g, lev) for lev in range(2, levels + 1)]
        dst = [hmg.LevelState(g, i + 1) for i in range(levels)]
        dst[-1].x.rand(3)
        dst[-1].b.rand(4)
        hmg.broadcast_interfaces(dst[-1].x, g, levels)
        hmg.apply_constraint(dst[-1].x, levels, g)
        bl = hmg.BaseLevel(g)
        for _ in range(2):
            hmg.vcycle(g, bl, [A] * levels, dst, levels, 3)
        out.append((bounds, dst[-1].x.to_host(), dst[-1].r.to_host()))
        for s in dst:
            s.close()
        g.close()
    assert out[0][0] == out[1][0]
    assert np.isfinite(out[0][1]).all() and np.abs(out[0][1]).max() > 0
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize("dim,lev", [(3, 3), (2, 4)])
def test_long_smoothings(oracle, ctx, dim, lev):
    """hmg_smooth with 5 and 8 steps -- the coefficient recurrence (ChebCoef, the c1 / c2 kernel arguments) past the three steps a
    V-cycle asks for -- against the statement: x, r, p 1e-10, "cheb_applies" + 5 and + 8."""
    c, sets = _case(oracle, ctx, dim)
    try:
        dinv = inverse_diagonals(c.O, c.impl, c.ops(), c.levels)[lev - 1]
        hi = lambda_hi_local(c.O, c.impl, c.op(lev), lev, dinv)
        for steps in (5, 8):
            _check_smoother(ctx, c, lev, steps, dinv, hi)
    finally:
        c.close()


@pytest.mark.parametrize("dim", [3, 2])
def test_a_level_without_a_free_entry(oracle, ctx, dim):
    """Every face of every cell constrained: level 2 (vertices and edge midpoints) has no free entry, its inverse diagonal is 0
    everywhere and the statement's bound is exactly 0 (tests/test_cheb_smoother_statement.py).  None of the three smoothers
    works there, and this test pins what each does, as it is: "cg" and "jacobi" raise nothing and return x that is not finite --
    their first step divides 0 by 0 --, from hmg_smooth on level 2 and from a V-cycle through it; "chebyshev" refuses, with "the
    bound of this level is not a positive number", wherever the level's bound would be formed: the bounds query, the diagonal
    query, hmg_smooth, hmg_vcycle.  Its levels above 2 have the statement's bounds."""
    O = oracle
    for smoother in ("cg", "jacobi", "chebyshev"):
        c, sets = _case(O, ctx, dim, smoother=smoother)
        levels = c.levels
        try:
            _put(c, sets["every"])
            st = hmg.LevelState(c.g, 2)
            st.x.rand(3)
            hmg.apply_constraint(st.x, 2, c.g)
            assert not st.x.to_host().any()                              # (every entry of the level is constrained)
            st.b.rand(4)
            dsts = [hmg.LevelState(c.g, i + 1) for i in range(levels)]
            dsts[-1].b.rand(4)
            bl = hmg.BaseLevel(c.g)
            if smoother == "chebyshev":
                dinvs, his = _statement(c)
                assert his[1] == 0.0
                for call in (lambda: hmg.smoother_bounds(c.g, 2), lambda: hmg.smoother_diag(c.g, 2),
                             lambda: hmg.smoothing_steps(3, c.g, c.A, st, 2),
                             lambda: hmg.vcycle(c.g, bl, [c.A] * levels, dsts, levels, 3)):
                    with pytest.raises(HmgError, match="the bound of this level is not a positive number"):
                        call()
                for lev in range(3, levels + 1):
                    hi = hmg.smoother_bounds(c.g, lev)[1]
                    assert abs(hi - his[lev - 1]) <= 1e-11 * his[lev - 1], (lev, hi, his[lev - 1])
            else:
                if smoother == "jacobi":
                    assert not hmg.smoother_diag(c.g, 2).to_host().any()
                hmg.smoothing_steps(3, c.g, c.A, st, 2)
                assert not np.isfinite(st.x.to_host()).all()
                for _ in range(2):
                    hmg.vcycle(c.g, bl, [c.A] * levels, dsts, levels, 3)
                assert not np.isfinite(dsts[-1].x.to_host()).all()
            st.close()
            for s in dsts:
                s.close()
        finally:
            c.close()


def test_block_driver_with_blocks_of_one_cube(ctx):
    """driver.block_homogenization_tensor(2, 1, smoother="chebyshev"): the block boundaries are the cubes' faces, the faces between
    the simplices of one cube stay free, so every level has free entries and a positive bound -- the driver runs, and every block's
    tensor is what dirichlet_homogenization_tensor gives on that cube's two triangles as a mesh of their own, to 1e-8 of the largest
    entry (both solver-limited, tolerance 1e-12; the yardstick of test_block_tensors_equal_the_blocks_run_alone).  One conductivity
    per triangle: with one per cube every block is a uniform medium, its corrector is zero and no cycle runs.  (The "cg" run of this
    driver call is no yardstick: level 2 has one free node per cube, CG ends there before its steps do, and the next step's 0 / 0
    leaves a tensor that is not finite.)"""
    cond = np.random.default_rng(5).choice([1.0, 9.0], size=(8, 2))
    kw = dict(ctx=ctx, tolerance=1e-12, smoother="chebyshev")
    out = driver.block_homogenization_tensor(2, 1, hmg.Tri64, 2, cond=cond, fields=True, **kw)
    T_, F_ = out["tensor"], out["tensor_flux"]
    print(f"cycles {out['cycles']}")
    assert min(out["cycles"]) > 0                                        # (a live case: both correctors are solved for)
    assert T_.shape == (2, 2, 2, 2) and np.isfinite(T_).all() and np.isfinite(F_).all()
    assert np.array_equal(T_, np.swapaxes(T_, -1, -2))
    worst = 0.0
    for idx in np.ndindex(2, 2):
        cells = np.flatnonzero((out["block_of_cell"] == np.array(idx)).all(axis=1))
        assert cells.size == 2
        # (the two triangles of a square change places under the half turn that maps the square to itself and leaves tensors alone)
        alone = driver.dirichlet_homogenization_tensor(1, hmg.Tri64, 2, cond=cond[cells], **kw)
        worst = max(worst, np.abs(T_[idx] - alone["tensor"]).max() / np.abs(alone["tensor"]).max(),
                    np.abs(F_[idx] - alone["tensor_flux"]).max() / np.abs(alone["tensor_flux"]).max())
    print(f"largest relative difference over the blocks {worst:.3e}")
    assert worst <= 1e-8


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_coefficients_that_are_not_finite(oracle, ctx, bad):
    """hmg_grid_set_operator_tensor refuses an entry that is not finite; hmg_grid_set_operator (diagonal tensors) and
    hmg_grid_set_lambda pass one on to the device.  There the bound must not come back finite: the fold of k_cheb_max,
    k_cheb_max_fold and block_max keeps a NaN, and the host refuses the level with "not a positive number".  One cell of 48 holds
    the bad value."""
    O = oracle
    m = _cube(O, 3, 2, perturb=0.2, seed=7)
    rng = np.random.default_rng(7)
    sig = rng.choice([1.0, 100.0], size=(48, 3))
    g = hmg.ImplicitFineGrid(ctx, hmg.Mesh(m.nodes, m.elements + 1), 4)
    g.set_smoother("chebyshev")
    try:
        full = T.random_spd(rng, 48, 3)
        full[29, 1, 1] = bad
        with pytest.raises(HmgError, match="sigma of cell 29 is not finite"):
            hmg.L2PlusDivAGrad(g, LAM, full)
        good = hmg.L2PlusDivAGrad(g, LAM, sig)
        hi = hmg.smoother_bounds(g, 3)[1]
        assert np.isfinite(hi) and hi > 0.0
        spoilt = sig.copy()
        spoilt[29, 1] = bad
        hmg.L2PlusDivAGrad(g, LAM, spoilt)
        for lev in (2, 3, 4):
            with pytest.raises(HmgError, match="not a positive number"):
                hmg.smoother_bounds(g, lev)
        good._bind()
        assert hmg.smoother_bounds(g, 3)[1] == hi
        good.lam = bad                                                   # hmg_grid_set_lambda
        for lev in (2, 3, 4):
            with pytest.raises(HmgError, match="not a positive number"):
                hmg.smoother_bounds(g, lev)
        good.lam = LAM
        assert hmg.smoother_bounds(g, 3)[1] == hi
    finally:
        g.close()
