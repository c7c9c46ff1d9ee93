"""
Option "lazy_ap": where hmg_vcycle / hmg_fcg_step leave the top level's last r-update pending (option "lazy_r", three-update form), the
CG step in front of it runs in the dead form -- p_2.Ap_2 for the step length, no Ap stored, no interface sum -- and the record
rebuilds Ap = A p_2 by the eager tail's own launch when somebody reads r: beta_2 from the two doubles k_cg_x_tail saved next to the
step length, p_1 from the spare vector, the operator and the kernel choice as they stood.  So whatever changes one of those settles
the record first.  Everything a caller can observe must be what lazy_ap = 0 gives, and what lazy_r = 0 gives, to the last bit.
Grids: those of test_gpu_lazy_r.py -- 2^3 cubes x 6 tetrahedra = 48 cells, whole and shrunk to 47 cells (odd column tails), top
levels 4 (k_apply_small), 5 (k_apply_wave) and 6 (register-blocked k_apply), three smoothing steps.
"""
import ctypes

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import _lib, driver

pytestmark = pytest.mark.gpu

MODES = {"lazy_r=0": (0, 1), "lazy_ap=0": (1, 0), "on": (1, 1)}      # option lazy_r, option lazy_ap


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bank(ctx):
    """The context's scalar bank in a tensor the test can read: what a following hmg_smooth would find in it."""
    import torch
    t = torch.zeros(16, dtype=torch.float64, device="cuda:0")
    lib = _lib.load()
    _lib.check(lib.hmg_ctx_set_scalar_bank(ctx.h, ctypes.c_void_p(t.data_ptr())))

    def read():
        ctx.sync()
        return t.cpu().numpy().copy().view(np.uint64)
    yield read
    _lib.check(lib.hmg_ctx_set_scalar_bank(ctx.h, None))


class Problem:
    def __init__(self, ctx, levels, width=2, cells=None, tag=None):
        self.ctx, self.levels = ctx, levels
        self.base, self.cond, self.g, self.op = driver.checkerboard_problem(ctx, tag or hmg.Tet64, width, levels, seed=17, lam=0.8)
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


def _modes(ctx, run, modes=("lazy_r=0", "lazy_ap=0", "on")):
    """run(mode) under each pair of options: the results, in the order of `modes`"""
    out = []
    try:
        for m in modes:
            ctx.set_option("lazy_r", MODES[m][0])
            ctx.set_option("lazy_ap", MODES[m][1])
            out.append(run(m))
    finally:
        ctx.set_option("lazy_r", 1)
        ctx.set_option("lazy_ap", 1)
    return out


def _all_equal(results, what=""):
    for other in results[1:]:
        assert len(other) == len(results[0])
        for i, (u, v) in enumerate(zip(results[0], other)):
            if isinstance(u, np.ndarray):
                np.testing.assert_array_equal(u, v, err_msg=f"{what} [{i}]")
            else:
                assert u == v, (what, i, u, v)


def _counters(ctx, *names):
    return tuple(ctx.counter(n) for n in names)


# ---- 1. the read -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [48, 47])
@pytest.mark.parametrize("levels", [6, 5, 4])
def test_read_after_two_vcycles(ctx, bank, problems, levels, cells):
    """Two V-cycles, then x, norm_unique(r), r, Ap and the scalar bank: equal in the three modes.  With the option on the record has
    no stored Ap before the read and the read runs the apply again, once; nothing allocates."""
    P = problems(levels, None if cells == 48 else cells)
    keep = []

    def run(mode):
        lazy_r, lazy_ap = MODES[mode]
        st = P.start()
        keep.append(st)
        P.cycles(st, 1)
        allocs = ctx.counter("device_allocs")
        P.cycles(st, 1)
        assert ctx.counter("device_allocs") == allocs
        assert ctx.counter("lazy_top_form") == 2
        assert ctx.counter("lazy_r_form") == lazy_r
        assert ctx.counter("lazy_ap_form") == (1 if mode == "on" else 0)
        x = st[-1].x.to_host()                                     # (x is finished: reading it forms nothing)
        allocs = ctx.counter("device_allocs")                      # (a download takes a staging buffer: counted behind it)
        before = _counters(ctx, "ap_rebuilt", "r_materialized", "r_materialized_by_read")
        n = hmg.norm_unique(st[-1].r)
        after = _counters(ctx, "ap_rebuilt", "r_materialized", "r_materialized_by_read")
        assert ctx.counter("device_allocs") == allocs              # the read -- rebuild and r-update included -- allocates nothing
        assert after[0] - before[0] == (1 if mode == "on" else 0)
        assert after[1] - before[1] == lazy_r and after[2] - before[2] == lazy_r
        scal = bank()
        r, Ap = st[-1].r.to_host(), st[-1].Ap.to_host()
        assert _counters(ctx, "ap_rebuilt", "r_materialized") == after[:2]      # (settled: nothing more to form)
        return x, r, Ap, n, scal

    try:
        res = _modes(ctx, run)
        assert np.isfinite(res[0][3]) and res[0][3] > 0.0 and np.abs(res[0][2]).max() > 0.0
        _all_equal(res, f"levels {levels}, {cells} cells")
    finally:
        _close(*keep)


# ---- 2. a run of V-cycles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [6, 5, 4])
def test_a_run_of_vcycles_rebuilds_nothing(ctx, problems, levels):
    P = problems(levels)
    keep = []

    def run(mode):
        st = P.start()
        keep.append(st)
        P.cycles(st, 2)
        rebuilt, formed, dropped = _counters(ctx, "ap_rebuilt", "r_materialized", "r_dropped")
        for i in range(3):
            P.cycles(st, 1)
            assert ctx.counter("r_dropped") - dropped == (i + 1) * MODES[mode][0]
            assert ctx.counter("lazy_ap_form") == (1 if mode == "on" else 0)
        assert _counters(ctx, "ap_rebuilt", "r_materialized") == (rebuilt, formed)
        return (st[-1].x.to_host(),)

    try:
        _all_equal(_modes(ctx, run))
    finally:
        _close(*keep)


# ---- 3. setters under the record -----------------------------------------------------------------------------------------------------
def _tensor(cond):
    s = np.zeros((cond.shape[0], 3, 3))
    for a in range(3):
        s[:, a, a] = cond[:, a]
    s[:, 0, 1] = s[:, 1, 0] = 0.125
    s[:, 1, 2] = s[:, 2, 1] = -0.0625
    return s


def _some_faces(P):
    f = hmg.boundary_faces(P.base)
    return f[: len(f) // 2]


# name -> (what is called under the record, what brings the grid back; None: the change stays)
SETTERS = {
    "set_operator": (lambda P: P.g.set_operator(2.0 * np.asarray(P.cond), 0.5), lambda P: P.g.set_operator(P.cond, 0.8)),
    "set_operator_tensor": (lambda P: P.g.set_operator(_tensor(np.asarray(P.cond)), 0.8), lambda P: P.g.set_operator(P.cond, 0.8)),
    "set_lambda": (lambda P: P.g.set_lambda(0.3), lambda P: P.g.set_lambda(0.8)),
    "set_dirichlet_faces": (lambda P: P.g.set_dirichlet_faces(_some_faces(P)), lambda P: P.g.set_dirichlet_faces(None)),
    "shrink": (lambda P: P.g.shrink(P.g.ncells() - 3, P.g.nnodes_base()), None),      # (48 -> 45 -> 42 cells)
    "reserve_spare_off": (lambda P: P.g.reserve_spare(False), lambda P: P.g.reserve_spare(True)),
    "option_weight_cache": (lambda P: P.ctx.set_option("weight_cache", 0), lambda P: P.ctx.set_option("weight_cache", 1)),
    "option_lazy_ap": (lambda P: P.ctx.set_option("lazy_ap", 0), None),                 # (_modes and the run below set it again)
}


@pytest.mark.parametrize("what", sorted(SETTERS))
def test_setters_under_the_record(ctx, what):
    """With a record open that has no stored Ap: the setter settles it first (one rebuild, not a read), so r read back afterwards is
    the eager run's r under the old operator and options; and since a setter is not a reader, the next cycle defers again."""
    change, restore = SETTERS[what]
    keep, grids = [], []

    def run(mode):
        lazy_r, lazy_ap = MODES[mode]
        P = Problem(ctx, 6)
        grids.append(P)
        st = P.start()
        keep.append(st)
        P.cycles(st, 2)
        assert ctx.counter("lazy_ap_form") == (1 if mode == "on" else 0)
        before = _counters(ctx, "ap_rebuilt", "r_materialized_by_read")
        change(P)
        after = _counters(ctx, "ap_rebuilt", "r_materialized_by_read")
        assert after[0] - before[0] == (1 if mode == "on" else 0) and after[1] == before[1]
        if restore:
            restore(P)
        ctx.set_option("lazy_ap", lazy_ap)
        if what == "shrink":
            P.bl = hmg.BaseLevel(P.g)
        P.cycles(st, 1)
        assert ctx.counter("lazy_r_form") == lazy_r                 # (a setter that settles the record is not a reader)
        assert ctx.counter("lazy_ap_form") == (1 if mode == "on" else 0)
        change(P)                                                   # ... and the same again, with a read behind it
        assert ctx.counter("ap_rebuilt") - after[0] == (1 if mode == "on" else 0)
        out = (st[-1].r.to_host(), st[-1].Ap.to_host(), st[-1].x.to_host())
        assert ctx.counter("ap_rebuilt") - after[0] == (1 if mode == "on" else 0)
        if restore:
            restore(P)
        return out

    try:
        res = _modes(ctx, run)
        assert np.isfinite(res[0][0]).all() and np.abs(res[0][0]).max() > 0.0
        _all_equal(res, what)
    finally:
        ctx.set_option("weight_cache", 1)
        _close(*keep)
        for P in grids:
            P.close()


# ---- 4. the scalar bank between the V-cycle and the read -----------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [48, 47])
@pytest.mark.parametrize("levels", [6, 5, 4])
def test_scalar_bank_clobbered_before_the_read(ctx, problems, levels, cells):
    """hmg_smooth on a lower level with other vectors, and a V-cycle on another grid of the context, overwrite the slots beta_2 was
    read from (r.r of the last two steps): the rebuilt Ap is formed with the numbers saved on the grid."""
    P = problems(levels, None if cells == 48 else cells)
    Q = problems(5 if levels != 5 else 4)
    keep = []

    def run(mode):
        st, other = P.start(), Q.start()
        low = hmg.LevelState(P.g, levels - 1)
        keep.extend([st, other, [low]])
        low.x.rand(7)
        low.b.rand(8)
        P.cycles(st, 2)
        assert ctx.counter("lazy_ap_form") == (1 if mode == "on" else 0)
        rebuilt = ctx.counter("ap_rebuilt")
        hmg.smoothing_steps(3, P.g, P.op, low, levels - 1)
        Q.cycles(other, 1)
        assert ctx.counter("ap_rebuilt") == rebuilt
        n = hmg.norm_unique(st[-1].r)
        assert ctx.counter("ap_rebuilt") - rebuilt == (1 if mode == "on" else 0)
        return st[-1].r.to_host(), st[-1].Ap.to_host(), st[-1].x.to_host(), n

    try:
        _all_equal(_modes(ctx, run))
    finally:
        _close(*keep)


# ---- 5. destroy calls ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [6, 5, 4])
def test_ap_destroyed_under_the_record_then_r_is_read(ctx, problems, levels):
    """The record keeps the destroyed Ap's memory: it is the column the rebuild writes."""
    P = problems(levels)
    keep = []

    def run(mode):
        st = P.start()
        keep.append(st)
        P.cycles(st, 2)
        rebuilt = ctx.counter("ap_rebuilt")
        st[-1].Ap.close()
        assert ctx.counter("ap_rebuilt") == rebuilt                # (a destroy never launches)
        out = (st[-1].r.to_host(), hmg.norm_unique(st[-1].r), st[-1].x.to_host())
        assert ctx.counter("ap_rebuilt") - rebuilt == (1 if mode == "on" else 0)
        st[-1].Ap = hmg.DeviceMatrix(P.g, P.levels)
        P.cycles(st, 1)
        return out + (st[-1].x.to_host(),)

    try:
        _all_equal(_modes(ctx, run))
    finally:
        _close(*keep)


def test_both_vectors_destroyed_under_the_record(ctx, problems):
    P = problems(6)
    st = P.start()
    try:
        P.cycles(st, 2)
        assert ctx.counter("lazy_ap_form") == 1
        before = _counters(ctx, "ap_rebuilt", "r_materialized", "r_dropped")
        st[-1].Ap.close()
        st[-1].r.close()
        after = _counters(ctx, "ap_rebuilt", "r_materialized", "r_dropped")
        assert after[:2] == before[:2] and after[2] - before[2] == 1
        st[-1].Ap = hmg.DeviceMatrix(P.g, P.levels)
        st[-1].r = hmg.DeviceMatrix(P.g, P.levels)
        P.cycles(st, 2)
        n = hmg.norm_unique(st[-1].r)
        assert np.isfinite(n) and n > 0.0
    finally:
        _close(st)


def test_grid_closed_under_the_record(ctx):
    """hmg_grid_destroy hands the handle's reference back; the vectors keep the grid alive, and the record goes with r -- no launch."""
    P = Problem(ctx, 5)
    st = P.start()
    try:
        P.cycles(st, 2)
        assert ctx.counter("lazy_ap_form") == 1
        before = _counters(ctx, "ap_rebuilt", "r_materialized", "r_dropped")
        P.g._fin()
        assert _counters(ctx, "ap_rebuilt", "r_materialized", "r_dropped") == before
        _close(st)
        after = _counters(ctx, "ap_rebuilt", "r_materialized", "r_dropped")
        assert after[:2] == before[:2] and after[2] - before[2] == 1
        ctx.set_option("lazy_ap", 1)                               # (the context's list of open records no longer names the grid)
        ctx.sync()
    finally:
        P.g.h = None


# ---- 6. flexible CG ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [6, 5, 4])
def test_flexible_cg(ctx, problems, levels):
    P = problems(levels)
    keep = []

    def run(mode):
        st = P.start()
        keep.append(st)
        x, b = st[-1].x.copy(), st[-1].b.copy()
        keep.append([x, b])
        fcg = hmg.FlexibleCG(P.g, P.bl, P.ops, st, P.levels, steps=3)
        try:
            rebuilt, formed = _counters(ctx, "ap_rebuilt", "r_materialized")
            fcg.start(x, b)
            out = []
            for _ in range(3):
                fcg.step()
                assert ctx.counter("lazy_ap_form") == (1 if mode == "on" else 0)
                out.append(x.to_host())
            out.append(fcg.residual_norm())
            assert _counters(ctx, "ap_rebuilt", "r_materialized") == (rebuilt, formed)
            return tuple(out) + (fcg.vec("R"),)
        finally:
            fcg.close()

    try:
        _all_equal(_modes(ctx, run))
    finally:
        _close(*keep)


# ---- 7. the forms that keep the stored Ap --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["top2-nospare", "two-steps", "2d", "jacobi", "chebyshev", "synthetic-cut", "wrapped", "r-reader"])
def test_fallbacks_keep_todays_form(ctx, problems, why):
    """Without the spare vector (Top2), with two smoothing steps, in 2D, with the Jacobi smoother, on a partitioned grid, with a
    caller-owned r and for a caller that reads r after every cycle the last step stores Ap as before: lazy_ap_form = 0, nothing is
    ever rebuilt, and x, r are those of lazy_ap = 0."""
    import torch
    levels, steps = 6, 3
    keep, tensors = [], []
    own_ctx = None
    if why == "synthetic-cut":
        from homogenization_jl_amd import dist as hdist
        own_ctx = hmg.Context(0)                                   # (the exchange brings its own scalar bank)
        prob = hdist.partitioned_checkerboard(own_ctx, 2, levels, 1, 0, seed=3, backend="rccl", synthetic_cut=True)
        P = Problem.__new__(Problem)
        P.ctx, P.levels, P.g, P.op, P.bl, P.ops = own_ctx, levels, prob.implicit, prob.op, prob.base_level(), [prob.op] * levels
    elif why == "2d":
        levels = 5
        P = Problem(ctx, levels, tag=hmg.Tri64)
    else:
        P = problems(levels)
    c = P.ctx
    if why == "two-steps":
        steps = 2

    def run(mode):
        st = P.start()
        keep.append(st)
        if why == "wrapped":
            t = torch.zeros(P.g.ld(levels) * P.g.ncells(), dtype=torch.float64, device="cuda:0")
            tensors.append(t)
            st[-1].r.close()
            st[-1].r = hmg.DeviceMatrix(P.g, levels, device_ptr=t.data_ptr())
        rebuilt = c.counter("ap_rebuilt")
        P.cycles(st, 2, steps)
        if why == "r-reader":
            assert c.counter("lazy_ap_form") == (1 if mode == "on" else 0)
            first = hmg.norm_unique(st[-1].r)                       # (the one rebuild a reader pays for)
            assert c.counter("ap_rebuilt") - rebuilt == (1 if mode == "on" else 0)
            rebuilt = c.counter("ap_rebuilt")
            P.cycles(st, 1, steps)
            assert c.counter("lazy_r_form") == 0
        else:
            first = 0.0
        assert c.counter("lazy_ap_form") == 0
        if why in ("top2-nospare", "two-steps"):
            assert c.counter("lazy_top_form") == 1 and c.counter("lazy_r_form") == 1
        out = (first, st[-1].x.to_host(), st[-1].r.to_host(), hmg.norm_unique(st[-1].r))
        assert c.counter("ap_rebuilt") == rebuilt
        return out

    try:
        if why in ("jacobi", "chebyshev"):
            P.g.set_smoother(why)
        if why == "top2-nospare":
            P.g.reserve_spare(False)
        res = _modes(c, run, modes=("lazy_ap=0", "on"))
        assert np.isfinite(res[0][3]) and res[0][3] > 0.0
        _all_equal(res, why)
    finally:
        if why in ("jacobi", "chebyshev"):
            P.g.set_smoother("cg")
        if why == "top2-nospare":
            P.g.reserve_spare(True)
        _close(*keep)
        if why in ("synthetic-cut", "2d"):
            P.g.close()
        if own_ctx is not None:
            own_ctx.close()
