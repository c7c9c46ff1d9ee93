"""
The device side of the cut exchange with up to EIGHT members that each hold their own partial: k_cut_pack (pack and unpack),
k_seg_sum with its plan and member tables, the staging layout and the overlapped form of apply_then_sum (csrc/hmg_comm.cpp,
csrc/hmg_kernels.hip, csrc/hmg_smooth.cpp), run rank by rank in one process through the record / replay transport of
tests/_replay_exchange.py -- no process group, exact expectations.

Grids: the octants of a 4^3 brick (world 8: segments of 2, 4 and 8 members), the quadrants of a 6 x 6 square (world 4), and ragged
partitions (owner = a hash of the cell id, as tests/test_gpu_dist.py) of a Delaunay mesh and of a fan around one node at world 5
and 7: arbitrary member sets, peers that share a single node.  The copies of a DOF deliberately disagree in the input.

Tolerances: the interface sum 1e-13 of max|sum| (tests/test_dist_gloo.py holds the same sum to it with up to 24 copies added in
another order), the apply 1e-11 (tests/test_gpu_parity.py), a smoother's x, r, p 1e-10 (tests/test_gpu_pcg_smoother.py), the
first-copy norm 1e-12.
"""
import types

import numpy as np
import pytest

import homogenization_jl_amd as hmg
from homogenization_jl_amd import dist as hdist, driver

import _meshes
import _replay_exchange as RX
from _pcg_smoother_form import inverse_diagonal, smoothing_steps_jacobi

pytestmark = pytest.mark.gpu

LEVELS_3D, LEVELS_2D = (1, 2, 3, 5), (1, 2, 5, 8)


@pytest.fixture(scope="module")
def ctx():
    c = hmg.Context(0)
    yield c
    c.close()


def _hashed(ncells, world):
    return ((np.arange(ncells) * 2654435761 >> 7) % world).astype(np.int32)


_MESHES = {}


def mesh(O, name):
    """(global base mesh, owner, world, oracle mesh, oracle grid at the deepest level in use, constraint, sigma grid or None)"""
    if name in _MESHES:
        return _MESHES[name]
    m = types.SimpleNamespace(name=name, sgrid=None)
    if name == "octants":
        m.origin = (-2.0,) * 3
        m.base = driver.checkerboard_mesh(hmg.Tet64, (4, 4, 4), origin=m.origin, transposed_lookup=False)
        m.owner, m.world, m.top = hdist.block_owner(m.base, (2, 2, 2), 2, m.origin), 8, 6
        m.sgrid = np.where(np.random.default_rng(3).random((4, 4, 4, 3)) < 0.5, 1.0, 9.0)
    elif name == "quadrants":
        m.origin = (-3.0,) * 2
        m.base = driver.checkerboard_mesh(hmg.Tri64, (6, 6), origin=m.origin, transposed_lookup=False)
        m.owner, m.world, m.top = hdist.block_owner(m.base, (2, 2), 3, m.origin), 4, 8
        m.sgrid = np.where(np.random.default_rng(4).random((6, 6, 2)) < 0.5, 1.0, 9.0)
    else:
        kind, world = name.split("-w")
        om = {"delaunay3": lambda: _meshes.delaunay_mesh(O, 3, 70, 13), "fan3": lambda: _meshes.fan_mesh(O, 3, 12, 20, 5),
              "fan2": lambda: _meshes.fan_mesh(O, 2, 9, 11, 5)}[kind]()
        m.base = hmg.Mesh(om.nodes, om.elements + 1)
        m.world, m.top = int(world), 5 if om.dim == 3 else 8
        m.owner = _hashed(om.nelements(), m.world)
    m.dim = m.base.dim
    m.om = O.Mesh(m.base.nodes, m.base.elements - 1)
    m.oi = O.ImplicitFineGrid.create(m.om, m.top)
    m.cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(m.om))
    if m.sgrid is not None:
        m.cond = driver.conductivity_per_element(m.base, m.sgrid, tuple(1.0 - o for o in m.origin))
        assert set(np.unique(m.cond)) == {1.0, 9.0}
    _MESHES[name] = m
    return m


def make_rank(ctx, m, levels, smoother=None):
    def make(rank):
        g = hdist.PartitionedGrid(ctx, m.base, levels, m.owner, rank, m.world)
        if smoother:
            g.set_smoother(smoother)              # (before the level vectors)
        return g
    return make


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- (a), (b), (d), (f): the interface sum of a vector whose copies disagree -----------------------------------------------
_CASES = {}


def interface_body(m, level, y, with_norm=True):
    def body(rank, g, t):
        v = hmg.DeviceMatrix(g, level).from_host(y[:, g.local_cells])
        hmg.broadcast_interfaces(v, g, level)
        res = {"y": v.to_host(), "cells": g.local_cells.copy(), "layout": RX.cut_layout(g, level)}
        if with_norm:
            res["norm"] = hmg.norm_unique(v)
        v.close()
        return res
    return body


def order_matters_on_host(O, m, level, y, lays, cells):
    """The condition on the inputs, from the host data alone: the number of cut DOFs with three or more holders whose partials
    (rank by rank the oracle's sum of that rank's copies) add up to other bits in ascending than in descending rank order.
    Without one, check (ii) could not tell the orders apart."""
    parts = []
    for rank in range(m.world):
        v = np.asfortranarray(np.where((m.owner == rank)[None, :], y, 0.0))
        O.broadcast_interfaces(v, m.oi, level)
        parts.append(v)
    n = 0
    for lay, local in zip(lays, cells):
        seg = np.searchsorted(lay["soff"], lay["dst"], side="right") - 1      # (empty segments share their offset with the next)
        for q, mem in enumerate(lay["members"]):
            if len(mem) < 3 or lay["size"][q] == 0:
                continue
            rows, cols = lay["rows"][seg == q], local[lay["cols"][seg == q]]
            up = down = None
            for rank in mem:
                up = parts[rank][rows, cols] if up is None else up + parts[rank][rows, cols]
            for rank in reversed(mem):
                down = parts[rank][rows, cols] if down is None else down + parts[rank][rows, cols]
            n += int((up != down).sum())
    return n


def interface_case(ctx, O, monkeypatch, name, level):
    """The sharers form on one grid and level (run once per module): inputs, the oracle's sum, the replayed world.  The inputs are
    the first of a fixed list of seeds that meets order_matters_on_host (the quadrants have ONE DOF with more than two holders)."""
    monkeypatch.delenv("HMG_PARTITION_ANALYSIS", raising=False)          # the default: every rank analyses its halo only
    monkeypatch.delenv("HMG_EXCHANGE", raising=False)
    key = (name, level)
    if key not in _CASES:
        m = mesh(O, name)
        c = types.SimpleNamespace(m=m, level=level, levels=max(level, 2))
        lays, cells = [], []
        for rank in range(m.world):                                       # host-only grids: the tables, before anything runs
            g = hdist.PartitionedGrid(None, m.base, c.levels, m.owner, rank, m.world)
            RX.L.check(g._lib.hmg_grid_set_exchange_p2p(g.h, 1, RX.L.P2P_FN(0), RX.L.P2P_FN(0), None, 0))
            lays.append(RX.cut_layout(g, level))
            cells.append(g.local_cells.copy())
            g.close()
        for seed in range(100 * level + m.world, 100 * level + m.world + 20000, 1000):
            c.y = np.asfortranarray(np.random.default_rng(seed).standard_normal((m.oi.nf(level), m.om.nelements())))
            c.order_dependent = order_matters_on_host(O, m, level, c.y, lays, cells)
            if c.order_dependent > 0:
                break
        c.ysum = c.y.copy(order="F")
        O.broadcast_interfaces(c.ysum, m.oi, level)
        c.W = RX.run_world(ctx, m.world, make_rank(ctx, m, c.levels), interface_body(m, level, c.y))
        _CASES[key] = c
    return _CASES[key]


def check_oracle(c, W, what="y"):
    scale = np.abs(c.ysum).max()
    for rank, res in enumerate(W.results):
        err = np.abs(res[what] - c.ysum[:, res["cells"]]).max() / scale
        assert err <= 1e-13, (rank, err)


def check_exact(c, W):
    """(i) every holder of a cut DOF ends with the same bits, (ii) those bits are the ascending-rank sum of the partials the ranks
    sent, (iii) nothing off the cut is touched; the staging buffer is NaN wherever nothing was delivered."""
    lays = [res["layout"] for res in W.results]
    sent = [rec["buf"] for rec in W.records[0]]
    assert all(rec["kind"] == "p2p" for rec in W.records[0])
    want = RX.segment_sums(lays, sent)
    final = []
    for rank, (res, lay) in enumerate(zip(W.results, lays)):
        assert np.isfinite(want[rank]).all()
        got = res["y"][lay["rows"], lay["cols"]]
        np.testing.assert_array_equal(got, want[rank][lay["dst"]], err_msg=f"rank {rank}: (ii)")
        buf = np.full(want[rank].size, np.nan)
        buf[lay["dst"]] = got
        np.testing.assert_array_equal(buf[lay["dst"]], got, err_msg=f"rank {rank}: copies of one DOF differ")
        final.append(buf)
        off_cut = np.ones(res["y"].shape, dtype=bool)
        off_cut[lay["rows"], lay["cols"]] = False
        np.testing.assert_array_equal(res["y"][off_cut], W.first[rank]["y"][off_cut], err_msg=f"rank {rank}: (iii)")
        stage, delivered = W.stages[rank]
        assert np.isnan(stage[~delivered]).all(), f"rank {rank}: staging words nobody delivered were written"
        assert not np.isnan(stage[delivered]).any()
    for rank, lay in enumerate(lays):                                     # (i), from the results alone
        for q, mem in enumerate(lay["members"]):
            a = final[rank][lay["soff"][q]:lay["soff"][q + 1]]
            for other in mem:
                lo = lays[other]
                qo = lo["members"].index(mem)
                np.testing.assert_array_equal(final[other][lo["soff"][qo]:lo["soff"][qo + 1]], a, err_msg=f"(i): ranks {rank}, {other}")


def order_matters(c, W):
    """order_matters_on_host once more, from what the ranks really sent (their partials may differ from the oracle's in the last
    bit where a rank adds more than two local copies)."""
    lays = [res["layout"] for res in W.results]
    sent = [rec["buf"] for rec in W.records[0]]
    up, down = RX.segment_sums(lays, sent), RX.segment_sums(lays, sent, descending=True)
    n = 0
    for lay, a, b in zip(lays, up, down):
        for q, mem in enumerate(lay["members"]):
            if len(mem) >= 3:
                s = slice(int(lay["soff"][q]), int(lay["soff"][q + 1]))
                n += int((a[s] != b[s]).sum())
    return n


A_CASES = ([("octants", l) for l in LEVELS_3D + (6,)] + [("quadrants", l) for l in LEVELS_2D] +
           [(n, l) for n in ("delaunay3-w5", "delaunay3-w7", "fan3-w7") for l in LEVELS_3D] + [("fan2-w5", l) for l in LEVELS_2D])


@pytest.mark.parametrize("name,level", A_CASES)
def test_interface_sum_among_the_sharers(oracle, ctx, monkeypatch, name, level):
    """(a) hmg.broadcast_interfaces in the segment form: against the serial oracle on the global mesh (1e-13), and exactly -- the
    checks of check_exact -- with the condition on the inputs that makes the order of the members visible.  Level 1 has nodes only
    and level 2 no face DOFs: plan entries of empty segments share an offset there."""
    c = interface_case(ctx, oracle, monkeypatch, name, level)
    counts = RX.member_counts([res["layout"] for res in c.W.results])
    differ = order_matters(c, c.W)
    print(f"{name} level {level}: doubles by member count {dict(sorted(counts.items()))}, sums that depend on the order: "
          f"{c.order_dependent} of the inputs, {differ} of the partials sent; {c.W.passes} passes")
    assert c.W.kinds[0] == ["p2p", "scalar_sum"]
    if name == "octants":
        assert {2, 4, 8} <= {k for k, v in counts.items() if v > 0}
    if name.endswith("-w7"):
        assert any(k >= 3 and v > 0 for k, v in counts.items())
    assert c.order_dependent > 0 and differ > 0
    check_oracle(c, c.W)
    check_exact(c, c.W)


@pytest.mark.parametrize("name,level", [("octants", l) for l in LEVELS_3D] + [("quadrants", l) for l in LEVELS_2D])
def test_allreduce_form_gives_the_bits_of_the_sharers_form(oracle, ctx, monkeypatch, name, level):
    """(b) hmg_grid_set_exchange_p2p(g, 0, ...) on a globally analysed partition: one all-reduce over the global cut buffer.  With
    the transport adding the ranks' buffers in ascending order the results equal the sharers form's bit for bit -- for eight
    members what test_rccl_exchange_on_two_physical_gpus can only state for two.  The global cut ids also name a DOF on every
    rank without the segment tables: all its holders end with the same bits."""
    a = interface_case(ctx, oracle, monkeypatch, name, level)
    monkeypatch.setenv("HMG_PARTITION_ANALYSIS", "global")
    m = a.m
    W = RX.run_world(ctx, m.world, make_rank(ctx, m, a.levels), interface_body(m, level, a.y), sharers=False)
    assert W.kinds[0] == ["exchange", "scalar_sum"]
    check_oracle(a, W)
    ids, vals = [], []
    for rank, (res, ref) in enumerate(zip(W.results, a.W.results)):
        np.testing.assert_array_equal(res["cells"], ref["cells"])
        np.testing.assert_array_equal(res["y"], ref["y"], err_msg=f"rank {rank}")
        assert res["norm"] == ref["norm"]
        lay = res["layout"]
        np.testing.assert_array_equal(lay["rows"], ref["layout"]["rows"])
        np.testing.assert_array_equal(lay["cols"], ref["layout"]["cols"])
        assert lay["gid"].size == lay["rows"].size > 0
        ids.append(lay["gid"])
        vals.append(ref["y"][lay["rows"], lay["cols"]])
    ids, vals = np.concatenate(ids), np.concatenate(vals)
    uniq, first, inverse = np.unique(ids, return_index=True, return_inverse=True)
    assert uniq.size < ids.size
    np.testing.assert_array_equal(vals, vals[first][inverse])


@pytest.mark.parametrize("name,level", [("octants", 3), ("octants", 5), ("quadrants", 5), ("delaunay3-w7", 3)])
def test_first_copy_norm_over_the_ranks(oracle, ctx, monkeypatch, name, level):
    """(d) hmg.norm_unique of the interface-summed vector of (a): the first-copy masks on the device count every DOF once over
    the ranks, and the total is the same double on all of them."""
    c = interface_case(ctx, oracle, monkeypatch, name, level)
    ref = c.ysum.copy(order="F")
    oracle.zero_out_all_but_one(ref, c.m.oi, level)
    want = np.linalg.norm(ref)
    norms = [res["norm"] for res in c.W.results]
    assert all(n == norms[0] for n in norms), norms
    assert abs(norms[0] - want) <= 1e-12 * want, (norms[0], want)
    assert c.W.records[1][0]["kind"] == "scalar_sum" and c.W.records[1][0]["count"] == 1
    parts = [rec["data"][0] for rec in c.W.records[1]]
    assert min(parts) > 0.0 and abs(np.sqrt(sum(parts)) - norms[0]) <= 1e-15 * want


def test_a_wrong_delivery_is_noticed(oracle, ctx, monkeypatch):
    """(f) The checks can fail: on the octants, rank 0 is given two peers' partials of one 4-member segment the wrong way round
    (only the order of the additions changes: the oracle comparison still holds, check (ii) does not), and, in a second run, one
    message one double behind its staging offset (a NaN takes part in the sum).  Wrong numbers in a sum, nothing else."""
    level = 3
    c = interface_case(ctx, oracle, monkeypatch, "octants", level)
    lays = [res["layout"] for res in c.W.results]
    sent = [rec["buf"] for rec in c.W.records[0]]
    lay0 = lays[0]

    def sum_in_order(q, order):
        acc = None
        for rank in order:
            o = int(lays[rank]["soff"][lays[rank]["members"].index(lay0["members"][q])])
            v = sent[rank][o:o + int(lay0["size"][q])]
            acc = v.copy() if acc is None else acc + v
        return acc

    # (most sums of four survive one transposition bit for bit: take the first segment and pair of peers where one does not)
    q, pa, pb = next((q, mem[i], mem[j]) for q, mem in enumerate(lay0["members"]) if len(mem) == 4 and lay0["size"][q] > 0
                     for i, j in ((1, 2), (2, 3), (1, 3))
                     if not np.array_equal(sum_in_order(q, mem), sum_in_order(q, [mem[j] if k == i else mem[i] if k == j else mem[k]
                                                                                   for k in range(4)])))
    hit = []

    def swapped(rank, msgs, deliveries):
        if rank == 0:
            i, = np.flatnonzero((msgs[:, 1] == lay0["soff"][q]) & (msgs[:, 0] == pa))
            j, = np.flatnonzero((msgs[:, 1] == lay0["soff"][q]) & (msgs[:, 0] == pb))
            assert msgs[i, 2] == msgs[j, 2] == lay0["size"][q]
            deliveries[i][1], deliveries[j][1] = deliveries[j][1], deliveries[i][1]
            hit.append("swapped")
        return deliveries

    def shifted(rank, msgs, deliveries):
        if rank == 0:
            deliveries[0][0] += 1
            hit.append("shifted")
        return deliveries

    body = interface_body(c.m, level, c.y, with_norm=False)
    W = RX.run_world(ctx, c.m.world, make_rank(ctx, c.m, c.levels), body, fault=swapped)
    assert hit == ["swapped"]
    check_oracle(c, W)
    with pytest.raises(AssertionError, match=r"\(ii\)"):
        check_exact(c, W)
    W = RX.run_world(ctx, c.m.world, make_rank(ctx, c.m, c.levels), body, fault=shifted)
    assert hit == ["swapped", "shifted"]
    with pytest.raises(AssertionError):
        check_oracle(c, W)
    with pytest.raises(AssertionError):
        check_exact(c, W)
    good = RX.run_world(ctx, c.m.world, make_rank(ctx, c.m, c.levels), body, fault=lambda rank, msgs, deliveries: deliveries)
    check_exact(c, good)                                                   # (the hook itself changes nothing)


# ---- (c): the operator apply with the sum over the ranks --------------------------------------------------------------------
def residual_reference(O, m, level, lam, cond):
    """x, b and the oracle's r = S C (b - A x) and y = S (b - A x) on the global mesh (C: the constraint, S: the interface sum)."""
    lvl = m.oi.reference.levels[level - 1]
    A = O.L2PlusDivAGrad(O.build_local_diffusion_operators(lvl), O.mass_matrix(lvl), m.cons, lam, cond)
    rng = np.random.default_rng(level)
    x = np.asfortranarray(rng.standard_normal((m.oi.nf(level), m.om.nelements())))
    b = np.asfortranarray(rng.standard_normal(x.shape))
    y_want = b.copy(order="F")
    O.mul(-1.0, m.om, A, x, y_want)
    r_want = y_want.copy(order="F")
    O.apply_constraint(r_want, level, m.cons, m.oi)
    O.broadcast_interfaces(r_want, m.oi, level)
    O.broadcast_interfaces(y_want, m.oi, level)
    return x, b, r_want, y_want


def residual_body(level, lam, cond, x, b, overlap):
    def body(rank, g, t):
        t.set_overlap(overlap)
        op = hmg.L2PlusDivAGrad(g, lam, cond)
        st = hmg.LevelState(g, level)
        st.x.from_host(x[:, g.local_cells])
        st.b.from_host(b[:, g.local_cells])
        hmg.smoothing_steps(0, g, op, st, level)                        # first residual: apply_then_sum, alpha = -1, source b
        res = {"r": st.r.to_host(), "cells": g.local_cells.copy()}
        st.Ap.from_host(b[:, g.local_cells])
        hmg.mul(-1.0, g, op, st.x, st.Ap)                               # apply, alpha = -1, with a source
        hmg.broadcast_interfaces(st.Ap, g, level)
        res["y"] = st.Ap.to_host()
        st.close()
        return res
    return body


def check_residuals(W, r_want, y_want):
    for rank, res in enumerate(W.results):
        er = np.abs(res["r"] - r_want[:, res["cells"]]).max() / np.abs(r_want).max()
        ey = np.abs(res["y"] - y_want[:, res["cells"]]).max() / np.abs(y_want).max()
        assert er <= 1e-11 and ey <= 1e-11, (rank, er, ey)
        assert (res["r"] == 0.0).any()                                   # (the constraint took part)


@pytest.mark.parametrize("name,level", [("octants", 3), ("octants", 5), ("quadrants", 5)])
def test_apply_then_sum_with_the_overlap_on_and_off(oracle, ctx, monkeypatch, name, level):
    """(c) r = b - A x, constrained and summed over interfaces and ranks, sigma in {1, 9} from conductivity_per_element.  hmg.mul is
    cell-local (no sum over ranks, no overlap decision); the library's apply-then-sum (apply_then_sum) is reached through
    hmg_smooth's first residual, and hmg.smoothing_steps(0, ...) is just that: the apply with alpha = -1 and a source, the
    constraint, the sum.  The literal pair -- hmg.mul(-1, ...) with a source, then hmg.broadcast_interfaces -- runs in the same
    body.  Both against the oracle's mul on the global mesh (1e-11), with the overlap on (threshold 1 double) and off, under halo
    and global analysis, and in the all-reduce form: the same bits on every rank in all of them.  Every rank reaches the same
    overlap decision (run_world asserts identical callback sequences; under halo analysis the agreed cut size is the first
    scalar sum, to which the highest rank, leading no segment, contributes 0)."""
    O = oracle
    m = mesh(O, name)
    lam = 0.8
    x, b, r_want, y_want = residual_reference(O, m, level, lam, m.cond)

    runs = {}
    ctx.set_option("overlap_min_doubles", 1)                             # (small meshes: overlap wherever it is switched on)
    try:
        for analysis, sharers, overlap in (("halo", True, True), ("halo", True, False), ("global", True, True),
                                           ("global", True, False), ("global", False, True), ("global", False, False)):
            monkeypatch.setenv("HMG_PARTITION_ANALYSIS", analysis)
            W = RX.run_world(ctx, m.world, make_rank(ctx, m, level), residual_body(level, lam, m.cond, x, b, overlap),
                             sharers=sharers)
            runs[(analysis, sharers, overlap)] = W
            kinds = W.kinds[0]
            print(f"{name} level {level}, {analysis} analysis, {'sharers' if sharers else 'all-reduce'}, overlap {overlap}: "
                  f"{W.passes} passes, callbacks {kinds}")
            started = [k for k in kinds if k in ("begin", "p2p_begin")]
            if overlap:
                assert started == ["p2p_begin" if sharers else "begin"] and kinds.count("end") == 1
            else:
                assert not started and "end" not in kinds
            assert (kinds[0] == "scalar_sum") == (analysis == "halo")
            if analysis == "halo":                                       # the agreed cut: three counts, the last rank leads nothing
                first = [rec["data"] for rec in W.records[0]]
                assert all(f.size == 3 for f in first) and not first[-1].any() and sum(first).sum() > 0
    finally:
        ctx.set_option("overlap_min_doubles", 524288)
    ref = runs[("halo", True, True)]
    check_residuals(ref, r_want, y_want)
    for key, W in runs.items():
        for rank, (res, want) in enumerate(zip(W.results, ref.results)):
            np.testing.assert_array_equal(res["r"], want["r"], err_msg=f"{key}, rank {rank}")
            np.testing.assert_array_equal(res["y"], want["y"], err_msg=f"{key}, rank {rank}")


def test_overlap_decision_with_the_threshold_between_the_ranks(oracle, ctx, monkeypatch):
    """A ragged seven-rank partition with "overlap_min_doubles" between the smallest and the largest of the ranks' OWN cut sizes
    (tests/test_gpu_dist.py::test_overlap_decision_is_the_same_on_every_rank, three gloo ranks there): a decision taken from
    rank-local numbers would send some ranks down the overlapped form and the others down the plain one.  run_world asserts that all
    ranks issue the same callbacks; the agreed cut is larger than every local one, so all of them overlap."""
    O = oracle
    monkeypatch.delenv("HMG_PARTITION_ANALYSIS", raising=False)
    m = mesh(O, "delaunay3-w7")
    level, lam = 3, 0.8
    cond = np.random.default_rng(3).choice([1.0, 9.0], size=(m.om.nelements(), 3))
    x, b, r_want, y_want = residual_reference(O, m, level, lam, cond)
    sizes = []
    for rank in range(m.world):
        g = hdist.PartitionedGrid(None, m.base, level, m.owner, rank, m.world)
        RX.L.check(g._lib.hmg_grid_set_exchange_p2p(g.h, 1, RX.L.P2P_FN(0), RX.L.P2P_FN(0), None, 0))
        sizes.append(int(g._lib.hmg_grid_cut_buffer_doubles(g.h, level)))
        g.close()
    assert min(sizes) < max(sizes), sizes                                # (the partition must be asymmetric for this to mean anything)
    ctx.set_option("overlap_min_doubles", (min(sizes) + max(sizes)) // 2)
    try:
        W = RX.run_world(ctx, m.world, make_rank(ctx, m, level), residual_body(level, lam, cond, x, b, True))
    finally:
        ctx.set_option("overlap_min_doubles", 524288)
    print(f"local cut sizes {sizes}, callbacks {W.kinds[0]}, {W.passes} passes")
    assert W.kinds[0] == ["scalar_sum", "p2p_begin", "end", "scalar_sum", "p2p"]
    check_residuals(W, r_want, y_want)


# ---- (e): one smoothing step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fused", [("cg", 1), ("cg", 0), ("jacobi", 1), ("jacobi", 0)])
def test_one_smoothing_step_on_the_octants(oracle, ctx, monkeypatch, kind, fused):
    """(e) hmg.smoothing_steps(1, ...) on the octants at level 3, the fused pass on and off, "cg" and "jacobi" (whose inverse
    diagonal is summed over the cut first): x, r and p against the oracle's smoother on the global mesh (1e-10).  Prints the
    number of passes: one per sum over the ranks, plus one ("cg" 6 fused and 7 unfused, "jacobi" 12: five of them are the limbs of
    the diagonal's fixed-point sum)."""
    O = oracle
    monkeypatch.delenv("HMG_PARTITION_ANALYSIS", raising=False)
    m = mesh(O, "octants")
    level, lam = 3, 0.7
    lvl = m.oi.reference.levels[level - 1]
    A = O.L2PlusDivAGrad(O.build_local_diffusion_operators(lvl), O.mass_matrix(lvl), m.cons, lam, m.cond)
    rng = np.random.default_rng(17)
    st = O.LevelState.create(m.om.nelements(), m.oi.nf(level))
    st.x[...] = rng.standard_normal(st.x.shape)
    O.broadcast_interfaces(st.x, m.oi, level)
    O.apply_constraint(st.x, level, m.cons, m.oi)
    st.b[...] = rng.standard_normal(st.x.shape)
    x0, b0 = st.x.copy(order="F"), st.b.copy(order="F")
    if kind == "cg":
        O.smoothing_steps(1, m.oi, A, st, level)
    else:
        smoothing_steps_jacobi(O, 1, m.oi, A, st, level, inverse_diagonal(O, m.oi, A, level))

    def body(rank, g, t):
        op = hmg.L2PlusDivAGrad(g, lam, m.cond)
        d = hmg.LevelState(g, level)
        d.x.from_host(x0[:, g.local_cells])
        d.b.from_host(b0[:, g.local_cells])
        hmg.smoothing_steps(1, g, op, d, level)
        res = {"x": d.x.to_host(), "r": d.r.to_host(), "p": d.p.to_host(), "cells": g.local_cells.copy()}
        d.close()
        return res

    ctx.set_option("fuse_cg", fused)                                     # (read when a grid is created)
    try:
        W = RX.run_world(ctx, m.world, make_rank(ctx, m, level, smoother=kind), body)
    finally:
        ctx.set_option("fuse_cg", 1)
    print(f"{kind}, fuse_cg {fused}: {W.passes} passes, callbacks {W.kinds[0]}")
    for rank, res in enumerate(W.results):
        c = res["cells"]
        ex, er, ep = relerr(res["x"], st.x[:, c]), relerr(res["r"], st.r[:, c]), relerr(res["p"], st.p[:, c])
        assert ex <= 1e-10 and er <= 1e-10 and ep <= 1e-10, (rank, ex, er, ep)
