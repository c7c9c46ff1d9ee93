"""
Option "lazy_pre": with three CG steps or more the finest level's pre-smoother leaves THREE x-updates to its local residual
(the step before the dead one writes its direction into the grid's spare vector and does no x-update; the residual forms
x = ((x + a0 p0) + a1 p1) + a2 (r2 + b2 p1) in its load phase, one fma per term: the roundings of the updates done one after the
other).  Taken on level 6 (the register-blocked kernel that restricts in its epilogue has the fourth stream); a level-5 top level,
a grid without the spare vector and a two-step smoother keep the two-update form and say so.  Everything is compared bit for bit,
by axpy + dot == 0 as the full-size tests do.
Option "fold_coarse_x": inside hmg_vcycle the post-smoother of the level below a level-6 top level leaves both its x-updates to the top
level's first residual, which combines the coarse x, p and r columns where it stages the coarse column (the roundings of the one
pass it replaces); hmg_vcycle_up takes a caller's coarse x as before.
"""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

pytestmark = pytest.mark.gpu

# every exact saving the pre-smoother's forms depend on: all off = the plain sequence of src/multigrid.jl:46-119
EXACT = ("lean_post", "lazy_post", "lazy_dead", "fold_x", "swap_rp", "fold_prolong", "prolong_in_image", "fold_faces", "fold_restrict",
         "zero_entry", "cell_order")
# (grid: cubes per edge, levels) -- 48 cells of 6545 nodes (level 6 on top), 384 cells of 969 nodes (level 5 on top)
GRIDS = {"l6": (2, 6), "l5": (4, 5)}


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=sorted(GRIDS))
def prob(request, ctx):
    n, levels = GRIDS[request.param]
    base, cond, g, op = driver.checkerboard_problem(ctx, hmg.Tet64, n, levels, seed=17, lam=0.8)
    yield request.param, g, op, levels
    g.close()


def _start(g, levels):
    st = [hmg.LevelState(g, i + 1) for i in range(levels)]
    st[-1].x.rand(3)
    st[-1].b.rand(4)
    hmg.broadcast_interfaces(st[-1].x, g, levels)
    hmg.apply_constraint(st[-1].x, levels, g)
    return st


def _same(a, b):
    """a == b to the last bit (b is used up)"""
    n2 = hmg.dot(a, a)
    assert np.isfinite(n2) and n2 > 0.0
    hmg.axpy(-1.0, a, b)
    return hmg.dot(b, b) == 0.0


def _close(states):
    for st in states:
        for s in st:
            if s is not None:
                s.close()


def _set(ctx, mode):
    """mode: "on" (defaults), "off" (lazy_pre alone off), "cx-off" (fold_coarse_x alone off), "plain" (every exact saving off);
    "wc0-on" / "wc0-off": defaults / both new options off with the class weights combined per cell (the instantiations without the
    class-weight cache; another kernel family on level 5, so that pair is compared with itself only)"""
    for o in EXACT:
        ctx.set_option(o, 0 if mode == "plain" else 1)
    ctx.set_option("lazy_top", 0 if mode == "plain" else 2)
    ctx.set_option("lazy_pre", 0 if mode in ("off", "wc0-off") else 1)
    ctx.set_option("fold_coarse_x", 0 if mode in ("cx-off", "wc0-off") else 1)
    ctx.set_option("weight_cache", 0 if mode.startswith("wc0") else 1)


MODES = ("on", "off", "cx-off", "plain", "wc0-on", "wc0-off")
PAIRS = ((0, 1), (0, 2), (0, 3), (4, 5))      # (indices into MODES) compared bit for bit


def _expected_form(which, mode, steps, spare=True):
    if mode == "plain":
        return 0
    if steps < 2:
        return 1
    return 3 if which == "l6" and mode not in ("off", "wc0-off") and steps >= 3 and spare else 2


@pytest.mark.parametrize("steps", [3, 4])
def test_vcycle_bits_do_not_depend_on_lazy_pre(ctx, prob, steps):
    """hmg_vcycle, steps + 2 steps, two cycles: x and r of the top level with the three-update pre-smoother, with lazy_pre alone
    off, with every exact saving off, and through the instantiation without the class-weight cache; the form taken is reported and
    no V-cycle allocates."""
    which, g, op, levels = prob
    bl = hmg.BaseLevel(g)
    res = []
    try:
        for mode in MODES:
            _set(ctx, mode)
            st = _start(g, levels)
            res.append(st)
            hmg.vcycle(g, bl, [op] * levels, st, levels, steps, 2)
            allocs, folds = ctx.counter("device_allocs"), ctx.counter("coarse_x_folds")
            hmg.vcycle(g, bl, [op] * levels, st, levels, steps, 2)
            assert ctx.counter("device_allocs") == allocs
            assert ctx.counter("lazy_pre_form") == _expected_form(which, mode, steps), mode
            # (one residual per V-cycle finishes the coarse x: level 6 on top, with the option and the savings it rests on)
            assert ctx.counter("coarse_x_folds") - folds == (1 if which == "l6" and mode in ("on", "off", "wc0-on") else 0), mode
    finally:
        _set(ctx, "on")
    try:
        for i, j in PAIRS:
            assert _same(res[i][-1].x, res[j][-1].x), (MODES[i], MODES[j])
            assert _same(res[i][-1].r, res[j][-1].r), (MODES[i], MODES[j])
    finally:
        _close(res)


def test_down_and_up_legs_bits_do_not_depend_on_lazy_pre(ctx, prob):
    """hmg_vcycle_down (three steps): x, the handed-back cell-local r and the coarse right-hand side; then hmg_vcycle_up on the same
    vectors with a coarse correction: x and r."""
    which, g, op, levels = prob
    res = []
    try:
        for mode in MODES:
            _set(ctx, mode)
            st = _start(g, levels)
            res.append(st)
            st[-2].x.rand(9)                                           # must come back as zeros
            hmg.vcycle_down(g, [op] * levels, st, levels, 3)
            assert ctx.counter("lazy_pre_form") == _expected_form(which, mode, 3), mode
            assert hmg.dot(st[-2].x, st[-2].x) == 0.0
            keep = (st[-1].x.copy(), st[-1].r.copy(), st[-2].b.copy())
            st[-2].x.rand(10)                                          # a coarse correction for the up leg
            hmg.broadcast_interfaces(st[-2].x, g, levels - 1)
            hmg.apply_constraint(st[-2].x, levels - 1, g)
            folds = ctx.counter("coarse_x_folds")
            hmg.vcycle_up(g, [op] * levels, st, levels, 3)
            assert ctx.counter("coarse_x_folds") == folds              # (the caller's coarse x is complete)
            st.extend(keep)
    finally:
        _set(ctx, "on")
    try:
        for i, j in PAIRS:
            for q in (-3, -2, -1):                                     # after the down leg: x, r, coarse b
                assert _same(res[i][q], res[j][q]), (MODES[i], MODES[j], q)
            assert _same(res[i][levels - 1].x, res[j][levels - 1].x), (MODES[i], MODES[j])   # after the up leg
            assert _same(res[i][levels - 1].r, res[j][levels - 1].r), (MODES[i], MODES[j])
    finally:
        for st in res:
            for v in st[levels:]:
                v.close()
            _close([st[:levels]])


def test_fallbacks_take_the_two_update_form_and_say_so(ctx, prob):
    """Without the spare vector (hmg_grid_reserve_spare(grid, 0)) and with two steps the pre-smoother defers two updates as before;
    the bits are those of the three-update form."""
    which, g, op, levels = prob
    bl = hmg.BaseLevel(g)
    res = []
    try:
        _set(ctx, "on")
        for spare, steps in ((True, 3), (False, 3), (True, 2), (True, 3)):
            g.reserve_spare(spare)
            st = _start(g, levels)
            res.append((steps, st))
            for _ in range(2):
                hmg.vcycle(g, bl, [op] * levels, st, levels, steps, 2)
            assert ctx.counter("lazy_pre_form") == _expected_form(which, "on", steps, spare), (spare, steps)
    finally:
        g.reserve_spare(True)
    try:
        for steps, other in res[1:]:
            if steps == 3:
                assert _same(res[0][1][-1].x, other[-1].x)
                assert _same(res[0][1][-1].r, other[-1].r)
    finally:
        _close([st for _, st in res])

