"""
Option "lazy_r": the last launch of hmg_vcycle / hmg_fcg_step on the top level finishes x only (k_cg_x_tail) and leaves the r-update
r_3 = r_2 - alpha_2 (A p_2 + face partner) as a record on the grid.  The record is settled -- the eager launch, late -- by the first
call that is handed r or Ap, and dropped where nobody can have read r: the next V-cycle on the same vectors, a copy or a fill over
r, the destruction of r.  A caller that does read r after a cycle is remembered: its next cycle runs the eager tail (and only notes
whether r is read again), so it never pays for the split twice; one cycle whose r goes unread brings the x-only tail back -- which is
why the cases below look at the SECOND of two V-cycles.  Everything a caller can observe (x, r, every value derived from them, the allocation count) must be what
lazy_r = 0 gives, to the last bit.  Grids: 2^3 cubes x 6 tetrahedra = 48 cells, checkerboard of contrast 9, seeded x0 and b.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib, driver

# ---- which ABI functions take a level vector, and where this file puts a pending r or Ap in front of each -------------------------
# (CPU part: a function added to include/hmg.h with an hmg_vec argument and no entry here fails test_every_vector_entry_has_a_case)
READERS = {}          # name of the case -> (ABI functions it goes through, callable(P, st) -> tuple of arrays / numbers)
ELSEWHERE = {
    "hmg_vcycle": "test_forms_match_the_eager_tail, test_a_run_of_vcycles_never_forms_r",
    "hmg_fcg_start": "test_flexible_cg_never_forms_r", "hmg_fcg_step": "test_flexible_cg_never_forms_r",
    "hmg_fcg_residual_norm": "test_flexible_cg_never_forms_r",
    "hmg_vec_wrap": "test_eager_fallbacks", "hmg_vec_create": "every case (LevelState)",
    "hmg_level_tune_placement": "test_things_under_the_record",
    # level-1 vectors only (hmg_objects.hpp check_vec refuses another level): the record lives on a top level >= 2
    "hmg_gather_base": "level 1 only", "hmg_scatter_base": "level 1 only", "hmg_coarse_solve": "level 1 only",
}


def reader(*abi):
    def deco(fn):
        READERS[fn.__name__] = (abi, fn)
        return fn
    return deco


def _vector_entries():
    text = (Path(__file__).resolve().parents[1] / "include" / "hmg.h").read_text()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = set()
    for m in re.finditer(r"\b(hmg_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bhmg_vec\s*\*", m.group(2)):
            names.add(m.group(1))
    return names


def test_every_vector_entry_has_a_case():
    names = _vector_entries()
    assert {"hmg_vec_download", "hmg_smooth", "hmg_cell_moments", "hmg_fcg_step"} <= names      # (the header was parsed)
    assert names <= set(_lib.SIGNATURES)                                                      # (... and bound)
    covered = set(ELSEWHERE)
    for abi, _ in READERS.values():
        covered |= set(abi)
    assert not names - covered, f"no pending-r case for {sorted(names - covered)}"


# ---- problems and runs --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


class Problem:
    def __init__(self, ctx, levels, width=2, cells=None):
        """cells: the grid is shrunk to that prefix of its cells (all nodes kept) -- 47 of 48 gives every level an odd number of
        entries (165, 969 and 6545 nodes per cell are odd), so flat pairs straddle columns and one thread finishes the last entry"""
        self.ctx, self.levels = ctx, levels
        self.base, self.cond, self.g, self.op = driver.checkerboard_problem(ctx, hmg.Tet64, width, levels, seed=17, lam=0.8)
        if cells is not None:
            self.g.shrink(cells, self.g.nnodes_base())
            assert self.g.ncells() == cells
        self.bl = hmg.BaseLevel(self.g)
        self.ops = [self.op] * levels

    def start(self):
        st = [hmg.LevelState(self.g, i + 1) for i in range(self.levels)]
        st[-1].x.rand(3)
        st[-1].b.rand(4)
        hmg.broadcast_interfaces(st[-1].x, self.g, self.levels)
        hmg.apply_constraint(st[-1].x, self.levels, self.g)
        return st

    def cycles(self, st, n=1, steps=3):
        for _ in range(n):
            hmg.vcycle(self.g, self.bl, self.ops, st, self.levels, steps, 2)

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def problems(ctx):
    made = {}

    def get(levels, cells=None):
        if (levels, cells) not in made:
            made[levels, cells] = Problem(ctx, levels, cells=cells)
        return made[levels, cells]
    yield get
    for p in made.values():
        p.close()


def _close(*states):
    for st in states:
        for s in st:
            if s is not None:
                s.close()


def _both(ctx, run):
    """run(lazy) with the option off, then on: the two results"""
    out = []
    try:
        for lazy in (0, 1):
            ctx.set_option("lazy_r", lazy)
            out.append(run(lazy))
    finally:
        ctx.set_option("lazy_r", 1)
    return out


def _equal(a, b, what=""):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        if isinstance(u, np.ndarray):
            assert u.shape == v.shape and np.array_equal(u, v, equal_nan=True), (what, i)
        else:
            assert u == v, (what, i, u, v)


# ---- 1. top levels and forms ----------------------------------------------------------------------------------------------------
FORMS = {"top3": (3, True, 2), "top2-nospare": (3, False, 1), "top2-steps": (2, True, 1)}     # steps, spare vector, lazy_top_form


@pytest.mark.gpu
@pytest.mark.parametrize("cells", [48, 47])
@pytest.mark.parametrize("levels", [6, 5, 4])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_forms_match_the_eager_tail(ctx, problems, levels, form, cells):
    """Two V-cycles from identical states with lazy_r = 1 and 0: x, r, norm_unique(r) and the allocation count are equal, and the
    x-only tail is what ran (Top3 with the spare vector, Top2 without it or with two steps).  On the whole grid and on the grid
    shrunk to 47 of its 48 cells: an odd number of entries, the last one finished by the tail branch of k_cg_x_tail<1|2> and, at
    the late read, of k_cg_rupdate_faces<0> with the step length from the grid's buffer."""
    P = problems(levels, None if cells == 48 else cells)
    assert (P.g.ld(levels) * P.g.ncells()) % 2 == cells % 2
    steps, spare, top_form = FORMS[form]
    keep = []

    def run(lazy):
        st = P.start()
        keep.append(st)
        P.cycles(st, 1, steps)
        allocs = ctx.counter("device_allocs")
        P.cycles(st, 1, steps)
        assert ctx.counter("device_allocs") == allocs
        assert ctx.counter("lazy_top_form") == top_form
        assert ctx.counter("lazy_r_form") == lazy
        x = st[-1].x.to_host()                       # (x is finished: reading it forms nothing)
        formed, by_read = ctx.counter("r_materialized"), ctx.counter("r_materialized_by_read")
        n = hmg.norm_unique(st[-1].r)
        assert ctx.counter("r_materialized") - formed == lazy and ctx.counter("r_materialized_by_read") - by_read == lazy
        return x, st[-1].r.to_host(), n, ctx.counter("device_allocs") - allocs

    try:
        P.g.reserve_spare(spare)
        eager, lazy = _both(ctx, run)
        assert np.isfinite(eager[2]) and eager[2] > 0.0
        _equal(eager, lazy, form)
    finally:
        P.g.reserve_spare(True)
        _close(*keep)


# ---- 2. every reader ------------------------------------------------------------------------------------------------------------
@reader("hmg_vec_download")
def download(P, st):
    return (st[-1].r.to_host(),)


@reader("hmg_vec_download")
def download_Ap(P, st):
    return (st[-1].Ap.to_host(),)


@reader("hmg_vec_copy")
def copy_from(P, st):
    t = st[-1].r.copy()
    try:
        return (t.to_host(),)
    finally:
        t.close()


@reader("hmg_vec_copy")
def copy_over_r(P, st):          # (every entry overwritten unread: the record is dropped)
    st[-1].r.copyto(st[-1].b)
    return ()


@reader("hmg_vec_copy")
def copy_over_Ap(P, st):         # (r still needs the old Ap: formed first)
    st[-1].Ap.copyto(st[-1].b)
    return ()


@reader("hmg_vec_fill")
def fill_r(P, st):
    st[-1].r.fill(2.0)
    return ()


@reader("hmg_vec_fill")
def fill_Ap(P, st):
    st[-1].Ap.fill(2.0)
    return ()


@reader("hmg_vec_upload")
def upload(P, st):
    st[-1].Ap.from_host(hmg.host_random(st[-1].Ap.shape, 21))
    return ()


@reader("hmg_vec_axpy")
def axpy_from_r(P, st):
    hmg.axpy(2.0, st[-1].r, st[-1].b)
    return (st[-1].b.to_host(),)


@reader("hmg_vec_axpy")
def axpy_into_r(P, st):
    hmg.axpy(0.5, st[-1].b, st[-1].r)
    return ()


@reader("hmg_vec_xpby")
def xpby_from_r(P, st):
    hmg.xpby(st[-1].r, 0.5, st[-1].b)
    return (st[-1].b.to_host(),)


@reader("hmg_vec_xpby")
def xpby_into_r(P, st):
    hmg.xpby(st[-1].b, 0.5, st[-1].r)
    return ()


@reader("hmg_vec_dot")
def dot(P, st):
    return (hmg.dot(st[-1].r, st[-1].r),)


@reader("hmg_vec_dot")
def dot_second(P, st):
    return (hmg.dot(st[-1].b, st[-1].Ap),)


@reader("hmg_vec_norm_unique")
def norm_unique(P, st):
    return (hmg.norm_unique(st[-1].r),)


@reader("hmg_vec_fill_random", "hmg_vec_dot")
def fill_random_elsewhere_then_dot(P, st):
    st[-1].b.rand(5)
    return (hmg.dot(st[-1].b, st[-1].r),)


@reader("hmg_vec_fill_random")
def fill_random_Ap(P, st):
    st[-1].Ap.rand(5)
    return ()


@reader("hmg_apply")
def apply_r(P, st):
    hmg.mul(1.0, P.g, P.op, st[-1].r, st[-1].b)
    return (st[-1].b.to_host(),)


@reader("hmg_apply_ex")
def apply_ex_r(P, st):
    hmg.apply_ex(-1.0, P.g, st[-1].r, st[-1].b, st[-1].p, constrain=True)
    return (st[-1].p.to_host(),)


@reader("hmg_residual")
def residual(P, st):
    hmg.local_residual(P.g, P.op, st[-1], P.levels)
    return ()


@reader("hmg_constraint")
def constraint(P, st):
    hmg.apply_constraint(st[-1].r, P.levels, P.g)
    return ()


@reader("hmg_interface_sum")
def interface_sum(P, st):
    hmg.broadcast_interfaces(st[-1].r, P.g, P.levels)
    return ()


@reader("hmg_zero_duplicates")
def zero_duplicates(P, st):
    hmg.zero_out_all_but_one(st[-1].r, P.g, P.levels)
    return ()


@reader("hmg_integrate")
def integrate(P, st):
    return (hmg.integrate_terms(st[-1].r, st[-1].x, P.g, P.g.ncells()), hmg.integrate_pair_load(st[-1].x, st[-1].r, P.g, P.g.ncells()))


@reader("hmg_cell_moments")
def cell_moments(P, st):
    return hmg.cell_moments(st[-1].r, P.g)


@reader("hmg_cell_pair_moments")
def cell_pair_moments(P, st):
    return (hmg.cell_pair_moments(st[-1].x, st[-1].r, P.g),)


@reader("hmg_cell_extrema")
def cell_extrema(P, st):
    return hmg.cell_extrema(st[-1].r, P.g)


@reader("hmg_restrict")
def restrict(P, st):
    hmg.restrict_to(st[-2].b, P.g, st[-1].r)
    return (st[-2].b.to_host(),)


@reader("hmg_prolong_add")
def prolong_add(P, st):
    hmg.interpolate_and_sum_to(st[-1].r, P.g, st[-2].x)
    return ()


@reader("hmg_rhs_axi_grad")
def rhs_axi_grad(P, st):
    hmg.rhs_axi_grad_v(st[-1].Ap, P.g, np.array([0.3, 0.2, -0.7]))
    return ()


@reader("hmg_local_rhs")
def local_rhs(P, st):
    hmg.local_rhs(st[-1].Ap, P.g)
    return ()


@reader("hmg_next_rhs")
def next_rhs(P, st):
    hmg.next_rhs(st[-1].b, st[-1].r, P.g)
    return (st[-1].b.to_host(),)


@reader("hmg_smooth")
def smooth(P, st):
    hmg.smoothing_steps(2, P.g, P.op, st[-1], P.levels)
    return (st[-1].x.to_host(), st[-1].p.to_host(), st[-1].Ap.to_host())


@reader("hmg_vcycle_up")
def vcycle_up(P, st):
    hmg.vcycle_up(P.g, P.ops, st, P.levels, 3)
    return (st[-1].x.to_host(),)


@reader("hmg_vcycle_down")
def vcycle_down(P, st):
    hmg.vcycle_down(P.g, P.ops, st, P.levels, 3)
    return (st[-1].x.to_host(), st[-2].b.to_host())


@reader("hmg_vec_device_ptr")
def device_ptr(P, st):
    assert st[-1].r.device_ptr() != 0
    return ()


@reader("hmg_vec_destroy")
def destroy_Ap(P, st):           # (a destroy never launches: the record keeps Ap's memory until r is formed, see LATE)
    st[-1].Ap.close()
    st[-1].Ap = hmg.DeviceMatrix(P.g, P.levels)
    return ()


@reader("hmg_vec_destroy")
def destroy_r(P, st):            # (nothing to compare r with afterwards: the new vector is zero in both runs)
    st[-1].r.close()
    st[-1].r = hmg.DeviceMatrix(P.g, P.levels)
    return ()


@reader("hmg_grid_smoother_diag")
def smoother_diag(P, st):        # (hmg_grid_set_smoother settles the record; the diagonal is then formed in the old Ap)
    P.g.set_smoother("jacobi")
    try:
        hmg.smoother_diag(P.g, P.levels, out=st[-1].Ap)
    finally:
        P.g.set_smoother("cg")
    return ()


LATE = {"destroy_Ap"}            # cases whose call leaves the record open: the read of r behind them settles it


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(READERS))
def test_every_reader_sees_the_eager_r(ctx, problems, case):
    """One lazy V-cycle (the second of two), then exactly one ABI function on r or Ap: its output, r and x afterwards equal the
    eager run's bit for bit, and the call formed r at most once."""
    P = problems(6)
    fn = READERS[case][1]
    keep = []

    def run(lazy):
        st = P.start()
        keep.append(st)
        P.cycles(st, 2)
        assert ctx.counter("lazy_r_form") == lazy and ctx.counter("lazy_top_form") == 2
        formed, dropped = ctx.counter("r_materialized"), ctx.counter("r_dropped")
        out = tuple(fn(P, st))
        settled = (ctx.counter("r_materialized") - formed) + (ctx.counter("r_dropped") - dropped)
        assert settled == (0 if case in LATE else lazy), "the call did not settle the record (or did so twice)"
        out += (st[-1].r.to_host(), st[-1].x.to_host())
        assert ctx.counter("r_materialized") - formed + ctx.counter("r_dropped") - dropped == lazy
        return out

    try:
        eager, lazy = _both(ctx, run)
        _equal(eager, lazy, case)
    finally:
        _close(*keep)


# ---- 3. drop paths --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_run_of_vcycles_never_forms_r(ctx, problems):
    P = problems(6)
    keep = []

    def run(lazy):
        st = P.start()
        keep.append(st)
        P.cycles(st, 2)
        formed, dropped = ctx.counter("r_materialized"), ctx.counter("r_dropped")
        P.cycles(st, 3)
        assert ctx.counter("r_materialized") == formed
        assert ctx.counter("r_dropped") - dropped == 3 * lazy
        return st[-1].r.to_host(), st[-1].x.to_host(), hmg.norm_unique(st[-1].r)

    try:
        _equal(*_both(ctx, run))
    finally:
        _close(*keep)


@pytest.mark.gpu
def test_a_caller_that_reads_r_pays_for_the_split_once(ctx, problems):
    """V-cycle, norm_unique(r), V-cycle, norm_unique(r), ...: the first read forms r late; from then on the tail is the eager one and
    the reads launch nothing.  Two cycles without a read: the first still eager, the second x-only again.  Same bits throughout."""
    P = problems(6)
    keep = []

    def run(lazy):
        st = P.start()
        keep.append(st)
        P.cycles(st, 2)                                  # (whatever the grid remembered: the second one defers)
        assert ctx.counter("lazy_r_form") == lazy
        out = []
        formed = ctx.counter("r_materialized")
        out.append(hmg.norm_unique(st[-1].r))
        assert ctx.counter("r_materialized") - formed == lazy
        for _ in range(2):
            P.cycles(st, 1)
            assert ctx.counter("lazy_r_form") == 0
            out.append(hmg.norm_unique(st[-1].r))
        assert ctx.counter("r_materialized") - formed == lazy
        P.cycles(st, 1)
        assert ctx.counter("lazy_r_form") == 0          # (the reader is forgotten when this cycle's r has gone unread ...)
        P.cycles(st, 1)
        assert ctx.counter("lazy_r_form") == lazy       # (... which the next cycle finds out)
        out += [st[-1].r.to_host(), st[-1].x.to_host()]
        return tuple(out)

    try:
        _equal(*_both(ctx, run))
    finally:
        _close(*keep)


@pytest.mark.gpu
def test_destroying_both_vectors_under_the_record_forms_nothing(ctx, problems):
    """hmg_vec_destroy of Ap, then of r, with a record open: no launch (the record keeps Ap's memory until r goes, then drops), and
    the grid goes on working with new vectors."""
    P = problems(6)
    st = P.start()
    try:
        P.cycles(st, 2)
        assert ctx.counter("lazy_r_form") == 1
        formed, dropped = ctx.counter("r_materialized"), ctx.counter("r_dropped")
        st[-1].Ap.close()
        st[-1].r.close()
        assert ctx.counter("r_materialized") == formed and ctx.counter("r_dropped") - dropped == 1
        st[-1].Ap = hmg.DeviceMatrix(P.g, P.levels)
        st[-1].r = hmg.DeviceMatrix(P.g, P.levels)
        P.cycles(st, 2)
        n = hmg.norm_unique(st[-1].r)
        assert np.isfinite(n) and n > 0.0
    finally:
        _close(st)


@pytest.mark.gpu
def test_flexible_cg_never_forms_r(ctx, problems):
    """hmg_fcg_start, two hmg_fcg_step: the V-cycle inside leaves r pending, the next step and hmg_fcg_residual_norm (a copy over r)
    drop it; iterate and residual norm do not depend on the option."""
    P = problems(6)
    keep = []

    def run(lazy):
        st = P.start()
        keep.append(st)
        x = st[-1].x.copy()
        b = st[-1].b.copy()
        keep.append([x, b])
        fcg = hmg.FlexibleCG(P.g, P.bl, P.ops, st, P.levels, steps=3)
        try:
            formed = ctx.counter("r_materialized")
            fcg.start(x, b)
            norms = []
            for _ in range(2):
                fcg.step()
                norms.append(fcg.residual_norm())
            assert ctx.counter("lazy_r_form") == lazy
            assert ctx.counter("r_materialized") == formed
            return (x.to_host(), fcg.vec("R")) + tuple(norms)
        finally:
            fcg.close()

    try:
        _equal(*_both(ctx, run))
    finally:
        _close(*keep)


# ---- 4. eager fall-backs --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("why", ["wrapped", "exposed", "jacobi", "chebyshev", "partitioned"])
def test_eager_fallbacks(ctx, problems, why):
    """Where the memory of r can be read behind the library's back, on a partitioned grid and with the Jacobi smoother the eager
    tail runs whatever the option says: lazy_r_form = 0, nothing is ever formed late, and the results are those of lazy_r = 0."""
    import torch
    levels = 6
    keep, tensors = [], []
    if why == "partitioned":
        from homogenization_jl_amd import dist as hdist
        prob = hdist.partitioned_checkerboard(ctx, 2, levels, 1, 0, seed=3, backend="rccl", synthetic_cut=True)
        P = Problem.__new__(Problem)
        P.ctx, P.levels, P.g, P.op, P.bl, P.ops = ctx, levels, prob.implicit, prob.op, prob.base_level(), [prob.op] * levels
    else:
        P = problems(levels)

    def run(lazy):
        st = P.start()
        keep.append(st)
        if why == "wrapped":
            t = torch.zeros(P.g.ld(levels) * P.g.ncells(), dtype=torch.float64, device="cuda:0")
            tensors.append(t)
            st[-1].r.close()
            st[-1].r = hmg.DeviceMatrix(P.g, levels, device_ptr=t.data_ptr())
        if why == "exposed":
            assert st[-1].r.device_ptr() != 0
        formed = ctx.counter("r_materialized")
        P.cycles(st, 2)
        assert ctx.counter("lazy_r_form") == 0
        out = ()
        if why == "wrapped":
            ctx.sync()
            out = (t.cpu().numpy().copy(),)           # the tensor's memory, no API read of r
        out += (st[-1].r.to_host(), st[-1].x.to_host(), hmg.norm_unique(st[-1].r))
        assert ctx.counter("r_materialized") == formed
        return out

    try:
        if why in ("jacobi", "chebyshev"):
            P.g.set_smoother(why)
        _equal(*_both(ctx, run), why)
    finally:
        if why in ("jacobi", "chebyshev"):
            P.g.set_smoother("cg")
        _close(*keep)
        if why == "partitioned":
            P.g.close()


# ---- 5. things under the record -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["set_operator", "tune_placement", "grid_destroy", "reserve_spare_off"])
def test_things_under_the_record(ctx, problems, what):
    """With a record open: a new operator (the record does not rest on it), the placement tuner (settles, then refills the
    vectors), the grid handle's destruction (the vectors keep the grid, and with it the record, alive) and the release of the spare
    vector."""
    P = Problem(ctx, 5) if what == "grid_destroy" else problems(5)
    keep = []

    def run(lazy):
        st = P.start()
        keep.append(st)
        P.cycles(st, 2)
        assert ctx.counter("lazy_r_form") == lazy
        if what == "set_operator":
            P.g.set_operator(2.0 * np.asarray(P.cond), 0.5)
            P.g.set_operator(P.cond, 0.8)
        elif what == "tune_placement":
            x = st[-1].x.copy()
            keep.append([x])
            formed = ctx.counter("r_materialized")
            hmg.tune_placement(P.g, P.ops, st, P.levels, steps=3, trials=2, extra=1)
            assert ctx.counter("r_materialized") - formed == lazy
            assert not st[-1].r.to_host().any() and not st[-1].x.to_host().any()
            return (x.to_host(),)
        elif what == "reserve_spare_off":
            P.g.reserve_spare(False)
            P.g.reserve_spare(True)
        elif what == "grid_destroy" and lazy:
            formed = ctx.counter("r_materialized")
            P.g._fin()                                            # hmg_grid_destroy: the handle's reference; the vectors hold the grid
            assert ctx.counter("r_materialized") == formed        # (a destroy never launches; the grid outlives r)
        return st[-1].r.to_host(), st[-1].x.to_host()

    try:
        _equal(*_both(ctx, run), what)
    finally:
        _close(*keep)
        if what == "grid_destroy":
            P.g.h = None


@pytest.mark.gpu
def test_shrink_under_the_record_and_forms_on_the_shrunk_grid(ctx):
    """hmg_grid_shrink settles the record on the cells it was opened for; afterwards the prefix of r is the eager one, and V-cycles on
    the shrunk grid (another cell count under the streaming kernels: 4^3 cubes cut to the ball of radius 1) match the eager tail."""
    P = Problem(ctx, 4, width=4)
    ne, nn = driver.find_elements_in_radius(P.base, 1.0), driver.find_nodes_in_radius(P.base, 1.0)
    assert 0 < ne < P.g.ncells()
    P.close()
    keep, grids = [], []

    def run(lazy):
        Q = Problem(ctx, 4, width=4)
        grids.append(Q)
        st = Q.start()
        keep.append(st)
        Q.cycles(st, 2)
        assert ctx.counter("lazy_r_form") == lazy
        formed, by_read = ctx.counter("r_materialized"), ctx.counter("r_materialized_by_read")
        Q.g.shrink(ne, nn)
        assert ctx.counter("r_materialized") - formed == lazy and ctx.counter("r_materialized_by_read") == by_read
        Q.bl = hmg.BaseLevel(Q.g)
        Q.cycles(st, 1)
        assert ctx.counter("lazy_r_form") == lazy         # (a setter that settles the record is not a reader: the next cycle defers)
        first = (st[-1].r.to_host(), st[-1].x.to_host())
        Q.cycles(st, 2)
        assert ctx.counter("lazy_r_form") == lazy
        return first + (st[-1].x.to_host(), st[-1].r.to_host(), hmg.norm_unique(st[-1].r))

    try:
        _equal(*_both(ctx, run))
    finally:
        _close(*keep)
        for Q in grids:
            Q.close()
