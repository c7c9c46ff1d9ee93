"""
Option "lazy_x": where hmg_vcycle leaves the top level's last r-update pending (options "lazy_r" / "lazy_ap"), the x-only tail that
remained is not launched either.  The grid notes that x lacks two (two-update form) or three CG updates, puts the ratios aside, and
the next hmg_vcycle on the same states forms x in the load phase of its first residual, which writes x and r in one pass.  Every other
call that is handed x, the direction or the residual the updates rest on, or changes what they rest on, runs the x-only tail first.
Everything a caller can observe must be what lazy_x = 0 gives, to the last bit.

Grids: one cube (6 cells) and 2^3 cubes (48 cells: shared faces, edges and nodes) x 6 tetrahedra.  Top level 6 (register-blocked
k_apply: the one family whose first residual carries the updates); top levels 5 (k_apply_wave) and 4 (k_apply_small) keep the eager
tail and must say so.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

pytestmark = pytest.mark.gpu

OPTIONS = ("lazy_x", "lazy_r", "lazy_ap", "lazy_top")
DEFAULTS = {"lazy_x": 1, "lazy_r": 1, "lazy_ap": 1, "lazy_top": 2}
COUNTERS = ("x_deferred", "x_settled", "x_settled_read")


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


class Problem:
    def __init__(self, ctx, levels, width=2):
        self.ctx, self.levels, self.width = ctx, levels, width
        self.base, self.cond, self.g, self.op = driver.checkerboard_problem(ctx, hmg.Tet64, width, levels, seed=17, lam=0.8)
        if width == 1:
            # (one cube: every level-1 node lies on the boundary.  Half of the boundary faces constrained leaves the level-1 system
            #  some unknowns; the mass term keeps the operator definite)
            faces = hmg.boundary_faces(self.base)
            self.g.set_dirichlet_faces(faces[: len(faces) // 2])
        self.bl = hmg.BaseLevel(self.g)
        self.ops = [self.op] * levels

    def start(self):
        st = [hmg.LevelState(self.g, i + 1) for i in range(self.levels)]
        st[-1].x.rand(3)
        st[-1].b.rand(4)
        hmg.broadcast_interfaces(st[-1].x, self.g, self.levels)
        hmg.apply_constraint(st[-1].x, self.levels, self.g)
        return st

    def cycles(self, st, n=1, steps=3, top=None):
        for _ in range(n):
            hmg.vcycle(self.g, self.bl, self.ops, st, top or self.levels, steps, 2)

    def forget(self):
        """The grid remembers whether the last V-cycle's x and r were read (x_reader, r_reader) and finishes them at once if so.  Two
        V-cycles nobody reads, on states that go unread too, clear both memories: the next V-cycle defers what the options allow."""
        st = self.start()
        self.cycles(st, 2)
        for s in st:
            s.close()

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def problems(ctx):
    made = {}

    def get(levels, width=2):
        if (levels, width) not in made:
            made[levels, width] = Problem(ctx, levels, width)
        return made[levels, width]
    yield get
    for p in made.values():
        p.close()


def _close(*states):
    for st in states:
        for s in st:
            if s is not None:
                s.close()


def _with(ctx, settings, run):
    """run() under each dict of options (missing ones at their defaults): the results, in order"""
    out = []
    try:
        for s in settings:
            for name in OPTIONS:
                ctx.set_option(name, s.get(name, DEFAULTS[name]))
            out.append(run(s.get("lazy_x", 1)))
    finally:
        for name in OPTIONS:
            ctx.set_option(name, DEFAULTS[name])
    return out


OFF_ON = ({"lazy_x": 0}, {"lazy_x": 1})


def _all_equal(results, what=""):
    for other in results[1:]:
        assert len(other) == len(results[0])
        for i, (u, v) in enumerate(zip(results[0], other)):
            if isinstance(u, np.ndarray):
                np.testing.assert_array_equal(u, v, err_msg=f"{what} [{i}]")
            else:
                assert u == v, (what, i, u, v)


def _counters(ctx, names=COUNTERS):
    return tuple(ctx.counter(n) for n in names)


def _observed(st):
    """every level's x, then the top level's r and its norm (r after its first read: the read forms it)"""
    xs = tuple(s.x.to_host() for s in st)
    n = hmg.norm_unique(st[-1].r)
    return xs + (st[-1].r.to_host(), n)


def _form(levels, steps, lazy_x):
    return (3 if steps == 3 else 2) if lazy_x and levels == 6 else 0


# ---- 1. runs of V-cycles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [3, 2])
@pytest.mark.parametrize("levels,width", [(6, 1), (6, 2), (5, 2), (4, 2)])
def test_vcycles_leave_the_same_bits(ctx, problems, levels, width, steps):
    """1, 2 and 3 V-cycles from the same x0 and b with 3 / 2 steps (three-update form) and 2 / 2 steps (two-update form).  Levels 5
    and 4 have no carrying residual: lazy_x_form = 0."""
    P = problems(levels, width)
    keep = []

    def run(lazy_x):
        out = []
        for n in (1, 2, 3):
            P.forget()
            st = P.start()
            keep.append(st)
            settled = ctx.counter("x_settled")
            P.cycles(st, n, steps)
            assert ctx.counter("lazy_top_form") == (2 if steps == 3 else 1)
            assert ctx.counter("lazy_x_form") == _form(levels, steps, lazy_x)
            assert ctx.counter("x_settled") == settled             # (cycles 2 .. n carried what cycle 1 .. n - 1 left)
            out.extend(_observed(st))
            assert ctx.counter("x_settled") - settled == (1 if _form(levels, steps, lazy_x) else 0)
        return tuple(out)

    try:
        res = _with(ctx, OFF_ON, run)
        assert [i for i, u in enumerate(res[0]) if not np.isfinite(u).all()] == [] and np.abs(res[0][levels - 1]).max() > 0.0
        _all_equal(res, f"levels {levels}, width {width}, steps {steps}")
    finally:
        _close(*keep)


@pytest.mark.parametrize("steps", [3, 2])
def test_later_cycles_launch_no_x_tail(ctx, problems, steps):
    """The x-only tail runs only where "x_settled" counts it: cycles 2 and 3 defer again and settle nothing."""
    P = problems(6)
    P.forget()
    st = P.start()
    try:
        P.cycles(st, 1, steps)
        assert ctx.counter("lazy_x_form") == _form(6, steps, 1)
        before = _counters(ctx)
        for i in (1, 2):
            P.cycles(st, 1, steps)
            now = _counters(ctx)
            assert now[0] - before[0] == i and now[1:] == before[1:], (i, before, now)
        st[-1].x.to_host()
        assert _counters(ctx) == (before[0] + 2, before[1] + 1, before[2] + 1)
    finally:
        _close(st)


# ---- 2. every path that settles ------------------------------------------------------------------------------------------------------
def _replace(st, name, P):
    getattr(st[-1], name).close()
    setattr(st[-1], name, hmg.DeviceMatrix(P.g, P.levels))


# name -> (the call made under the record, fresh grid needed)
SETTLERS = {
    "download": (lambda P, st: st[-1].x.to_host(), False),
    "norm": (lambda P, st: hmg.norm(st[-1].x), False),
    "dot": (lambda P, st: hmg.dot(st[-1].b, st[-1].x), False),
    "axpy_into_x": (lambda P, st: hmg.axpy(0.5, st[-1].b, st[-1].x), False),
    "fill_p": (lambda P, st: st[-1].p.fill(0.25), False),
    "smooth_top": (lambda P, st: hmg.smoothing_steps(3, P.g, P.op, st[-1], P.levels), False),
    "vcycle_below": (lambda P, st: P.cycles(st, 1, 3, top=P.levels - 1), False),
    "shrink": (lambda P, st: P.g.shrink(P.g.ncells() - 3, P.g.nnodes_base()), True),
    "set_operator": (lambda P, st: P.g.set_operator(2.0 * np.asarray(P.cond), 0.5), True),
    "tune_placement": (lambda P, st: hmg.tune_placement(P.g, P.ops, st, P.levels, steps=3, trials=1, extra=0), True),
    "destroy_p": (lambda P, st: _replace(st, "p", P), False),
}


@pytest.mark.parametrize("what", sorted(SETTLERS))
def test_settling_paths(ctx, problems, what):
    """After a deferred cycle, one call of each kind: the x-only tail runs once, before the call sees x, and x is the eager x."""
    call, fresh = SETTLERS[what]
    keep, grids = [], []

    def run(lazy_x):
        P = Problem(ctx, 6) if fresh else problems(6)
        if fresh:
            grids.append(P)
        P.forget()
        st = P.start()
        keep.append(st)
        P.cycles(st, 2)
        assert ctx.counter("lazy_x_form") == (3 if lazy_x else 0)
        settled = ctx.counter("x_settled")
        call(P, st)
        assert ctx.counter("x_settled") - settled == lazy_x, what
        x = st[-1].x.to_host()
        assert ctx.counter("x_settled") - settled == lazy_x      # (settled: nothing more to form)
        return (x,)

    try:
        res = _with(ctx, OFF_ON, run)
        assert np.isfinite(res[0][0]).all()
        _all_equal(res, what)
    finally:
        _close(*keep)
        for P in grids:
            P.close()


# ---- 3. the reader memory ------------------------------------------------------------------------------------------------------------
def test_a_caller_that_reads_x_after_every_cycle(ctx, problems):
    P = problems(6)
    keep = []

    def run(lazy_x):
        P.forget()
        st = P.start()
        keep.append(st)
        out = []
        deferred = ctx.counter("x_deferred")
        P.cycles(st, 1)
        assert ctx.counter("x_deferred") - deferred == lazy_x
        out.append(st[-1].x.to_host())                             # the first read: pays for the split once
        for _ in range(3):
            P.cycles(st, 1)
            assert ctx.counter("lazy_x_form") == 0
            out.append(st[-1].x.to_host())
        assert ctx.counter("x_deferred") - deferred == lazy_x      # ... and every cycle since ran the eager tail
        P.cycles(st, 1)                                            # read by nobody
        assert ctx.counter("x_deferred") - deferred == lazy_x
        P.cycles(st, 1)                                            # ... so this one defers again
        assert ctx.counter("x_deferred") - deferred == 2 * lazy_x
        assert ctx.counter("lazy_x_form") == (3 if lazy_x else 0)
        out.append(st[-1].x.to_host())
        return tuple(out)

    try:
        _all_equal(_with(ctx, OFF_ON, run))
    finally:
        _close(*keep)


# ---- 4. where nothing is deferred ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["wrapped-x", "wrapped-p", "handed-out", "synthetic-cut", "jacobi", "chebyshev"])
def test_refusals(ctx, problems, why):
    import torch
    levels = 6
    keep, tensors = [], []
    own_ctx = None
    if why == "synthetic-cut":
        from homogenization_jl_amd import dist as hdist
        own_ctx = hmg.Context(0)                                   # (the exchange brings its own scalar bank)
        prob = hdist.partitioned_checkerboard(own_ctx, 2, levels, 1, 0, seed=3, backend="rccl", synthetic_cut=True)
        P = Problem.__new__(Problem)
        P.ctx, P.levels, P.g, P.op, P.bl, P.ops = own_ctx, levels, prob.implicit, prob.op, prob.base_level(), [prob.op] * levels
    else:
        P = problems(levels)
    c = P.ctx

    def run(lazy_x):
        st = P.start()
        keep.append(st)
        if why in ("wrapped-x", "wrapped-p"):
            name = why[-1]
            t = torch.zeros(P.g.ld(levels) * P.g.ncells(), dtype=torch.float64, device="cuda:0")
            tensors.append(t)
            old = getattr(st[-1], name)
            new = hmg.DeviceMatrix(P.g, levels, device_ptr=t.data_ptr())
            new.copyto(old)
            old.close()
            setattr(st[-1], name, new)
        if why == "handed-out":
            assert st[-1].x.device_ptr() != 0
        before = _counters(c)
        P.cycles(st, 2)
        assert c.counter("lazy_x_form") == 0
        assert _counters(c) == before
        return _observed(st)

    try:
        if why in ("jacobi", "chebyshev"):
            P.g.set_smoother(why)
        res = _with(c, OFF_ON, run)
        assert np.isfinite(res[0][-1]) and res[0][-1] > 0.0
        _all_equal(res, why)
    finally:
        if why in ("jacobi", "chebyshev"):
            P.g.set_smoother("cg")
        _close(*keep)
        if why == "synthetic-cut":
            P.g.close()
        if own_ctx is not None:
            own_ctx.close()


# ---- 5. flexible CG ------------------------------------------------------------------------------------------------------------------
def test_flexible_cg(ctx, problems):
    """hmg_fcg_step reads the V-cycle's x at once -- in the pass that forms z.q, which takes the pending updates once there is a
    direction (steps 2 and 3; nothing is settled by the x-only tail): the same iterates, residual norm and number of exchanges."""
    P = problems(6)
    keep = []

    def run(lazy_x):
        P.forget()
        st = P.start()
        keep.append(st)
        x, b = st[-1].x.copy(), st[-1].b.copy()
        keep.append([x, b])
        fcg = hmg.FlexibleCG(P.g, P.bl, P.ops, st, P.levels, steps=3)
        try:
            calls = ctx.counter("comm_calls")
            before = _counters(ctx)
            fcg.start(x, b)
            out = []
            for i in range(3):
                fcg.step()
                assert ctx.counter("lazy_x_form") == (3 if lazy_x and i > 0 else 0)
                out.append(x.to_host())
            assert _counters(ctx) == (before[0] + 2 * lazy_x, before[1], before[2])
            out.append(st[-1].x.to_host())                         # z of the last step, as the pass over z.q stored it
            out.append(fcg.residual_norm())
            out.append(ctx.counter("comm_calls") - calls)
            return tuple(out)
        finally:
            fcg.close()

    try:
        _all_equal(_with(ctx, OFF_ON, run))
    finally:
        _close(*keep)


def test_flexible_cg_after_deferred_vcycles(ctx, problems):
    """A flexible-CG step on states whose x a V-cycle left pending takes a zero guess: the updates are dropped, nothing is formed."""
    P = problems(6)
    keep = []

    def run(lazy_x):
        P.forget()
        st = P.start()
        keep.append(st)
        P.cycles(st, 2)
        assert ctx.counter("lazy_x_form") == (3 if lazy_x else 0)
        x, b = st[-1].b.copy(), st[-1].b.copy()
        keep.append([x, b])
        fcg = hmg.FlexibleCG(P.g, P.bl, P.ops, st, P.levels, steps=3)
        try:
            fcg.start(x, b)
            fcg.step()
            return x.to_host(), st[-1].x.to_host(), fcg.residual_norm()
        finally:
            fcg.close()

    try:
        _all_equal(_with(ctx, OFF_ON, run))
    finally:
        _close(*keep)


# ---- 6. with the neighbouring options off --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", ["lazy_r", "lazy_ap", "lazy_top", "lazy_top=1"])
def test_option_matrix(ctx, problems, off):
    """lazy_r, lazy_ap and lazy_top each switched off (lazy_top also down to the two-update form) with lazy_x on: the bits of the
    all-eager run."""
    P = problems(6)
    keep = []
    eager = {"lazy_x": 0, "lazy_r": 0, "lazy_ap": 0, "lazy_top": 0}
    mixed = {"lazy_x": 1, "lazy_top": 1} if off == "lazy_top=1" else {"lazy_x": 1, off: 0}
    forms = [0, {"lazy_r": 0, "lazy_ap": 3, "lazy_top": 0, "lazy_top=1": 2}[off], 3]      # (of the three settings below, in order)

    def run(lazy_x):
        st = P.start()
        keep.append(st)
        P.cycles(st, 3)
        assert ctx.counter("lazy_x_form") == forms.pop(0)
        return _observed(st)

    try:
        _all_equal(_with(ctx, (eager, mixed, {"lazy_x": 1}), run), off)
    finally:
        _close(*keep)
