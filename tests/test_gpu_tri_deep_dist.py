"""
2D grids of 9 to 11 levels on PARTITIONED grids: the row-band apply of hmg_apply_rows.hip finds its cells through a cell list
(the cut-first / inner lists of the apply that is split around the exchange) instead of blockIdx.x, and the cut machinery
(k_cut_pack, the interface sums of cut groups, the cut buffers) sees edge runs of 255 .. 1023 nodes.

  * gloo ranks sharing the one GPU (the pattern of test_gpu_dist.py) against the serial oracle on the global mesh: perturbed
    Tri64 lattice of 4 x 4 squares, sigma in {1, 9}^2, lambda = 0.7; halves, quadrants and a hashed ragged partition;
  * one rank with a synthetic cut (cut_owner = quadrant, 1-rank RCCL communicator) against the unpartitioned grid, bit for bit;
  * the partitioned driver at refinements = 8 (9 levels) against the single-rank driver, device against device.
"""
import os
import sys

import numpy as np
import pytest

from test_gpu_dist import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

LAM = 0.7


def lattice(O, n=4, seed=9, perturb=0.2):
    """The mesh of test_gpu_tri_deep.Case: n x n unit squares about the origin, ordered by magnitude, nodes perturbed."""
    m = O.order_nodes_and_elements_by_magnitude(O.hypercube(2, n, origin=(-n / 2.0,) * 2))
    rng = np.random.default_rng(seed)
    m.nodes = m.nodes + perturb * (rng.random(m.nodes.shape) - 0.5)
    sig = rng.choice([1.0, 9.0], size=(m.nelements(), 2))
    return m, sig


def owners(O, m, spec, world):
    """halves in x / quadrants about the origin (a triangle's centre lies at least 1/3 - 0.1 from the lines x = 0, y = 0 whatever
    the perturbation), or the hashed cell id of test_gpu_dist.py (ragged)."""
    c = O.element_centers(m)
    if spec == "halves":
        assert world == 2
        return (c[:, 0] > 0).astype(np.int32)
    if spec == "quadrants":
        assert world == 4
        return (2 * (c[:, 0] > 0) + (c[:, 1] > 0)).astype(np.int32)
    assert spec == "hash"
    return ((np.arange(m.nelements()) * 2654435761 >> 7) % world).astype(np.int32)


def _worker(rank, world, port, levels, spec, overlap, q, n=4, radius=None):
    """radius: the grid is created on the n x n lattice and shrunk to the cells / nodes within `radius` of the origin (a prefix
    of both, radii taken before the nodes are perturbed) AFTER its level vectors were created and filled; the oracle runs on
    the sub-mesh."""
    try:
        sys.path.insert(0, ROOT)
        import torch
        import torch.distributed as dist
        import homogenization_jl_amd as hmg
        from homogenization_jl_amd import dist as hdist
        from oracle import oracle as O
        O.NTHREADS[0] = max(1, 16 // world)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        ctx = hmg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        L = levels
        gm, sig = lattice(O, n)
        owner = owners(O, gm, spec, world)
        gbase = hmg.Mesh(gm.nodes, gm.elements + 1)
        g = hdist.PartitionedGrid(ctx, gbase, levels, owner, rank, world)
        ex = hdist.Exchange(ctx, g)
        op = hmg.L2PlusDivAGrad(g, LAM, sig)
        ex.set_overlap(g, overlap)
        ctx.set_option("overlap_min_doubles", 1)
        rng = np.random.default_rng(5)
        x0 = np.asfortranarray(rng.random((g.nf(L), gm.nelements())))
        b0 = np.asfortranarray(rng.standard_normal(x0.shape))
        dsts = [hmg.LevelState(g, i + 1) for i in range(L)]
        dsts[-1].x.from_host(np.asfortranarray(x0[:, g.local_cells]))
        dsts[-1].b.from_host(np.asfortranarray(b0[:, g.local_cells]))
        if radius is not None:
            flat = O.order_nodes_and_elements_by_magnitude(O.hypercube(2, n, origin=(-n / 2.0,) * 2))
            ne, nn = O.find_elements_in_radius(flat, radius), O.find_nodes_in_radius(flat, radius)
            assert 0 < ne < gm.nelements() and gm.elements[:ne].max() < nn
            before = g.ncells()
            g.shrink(ne, nn)
            assert 0 < g.ncells() < before and g.local_cells.max() < ne
            gm = O.Mesh(gm.nodes[:nn], np.ascontiguousarray(gm.elements[:ne]))
            sig = np.ascontiguousarray(sig[:ne])
            x0, b0 = np.asfortranarray(x0[:, :ne]), np.asfortranarray(b0[:, :ne])
        hmg.broadcast_interfaces(dsts[-1].x, g, L)
        hmg.apply_constraint(dsts[-1].x, L, g)
        counts = g.table_i32("cut_counts")
        ncut, ninner = int(counts[9]), int(counts[10])
        assert ncut + ninner == g.ncells(), (counts, g.ncells())
        if spec == "hash":
            # ragged: every cell of every rank touches the cut, the inner list is empty ("an empty list must not read as all
            # cells"); the overlap threshold lies between the ranks' own cut sizes (test_gpu_dist.py, "between")
            assert ninner == 0 and ncut == g.ncells(), counts
            mine = torch.tensor([float(g._lib.hmg_grid_cut_buffer_doubles(g.h, levels))], dtype=torch.float64)
            every = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(every, mine)
            sizes = sorted(int(t.item()) for t in every)
            assert sizes[0] < sizes[-1], sizes
            ctx.set_option("overlap_min_doubles", (sizes[0] + sizes[-1]) // 2)
        else:
            assert ncut > 0 and ninner > 0, counts            # both cell lists are what the row kernel is sent
        gi = O.ImplicitFineGrid.create(gm, L)
        cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(gm))
        ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), cons, LAM, sig)
               for l in gi.reference.levels]
        sts = [O.LevelState.create(gm.nelements(), gi.nf(i + 1)) for i in range(L)]
        sts[-1].x[...] = x0; sts[-1].b[...] = b0
        O.broadcast_interfaces(sts[-1].x, gi, L)
        O.apply_constraint(sts[-1].x, L, cons, gi)
        base = O.make_base_level(gm, sig, LAM)
        dbase = hmg.BaseLevel(g)
        n0 = ctx.counter("rows_launches")
        errs = []
        for cyc in range(2):
            O.vcycle(gi, base, ops, sts, L, 3)
            hmg.vcycle(g, dbase, [op] * L, dsts, L, 3)
            got = dsts[-1].x.to_host()
            want = sts[-1].x[:, g.local_cells]
            errs.append(np.abs(got - want).max() / np.abs(sts[-1].x).max())
        r = sts[-1].r.copy(order="F")
        O.zero_out_all_but_one(r, gi, L)
        nr = np.linalg.norm(r)
        errs.append(abs(hmg.norm_unique(dsts[-1].r) - nr) / nr)
        print(f"tri_deep_dist rank {rank}/{world} L={L} {spec} overlap={overlap} cells {g.ncells()}/{gm.nelements()}: "
              f"x {errs[0]:.3e} {errs[1]:.3e} |r| {errs[2]:.3e} cut/inner {ncut}/{ninner}", flush=True)
        assert errs[0] <= 1e-9 and errs[1] <= 1e-9, errs
        assert errs[2] <= 1e-8, errs
        assert ctx.counter("rows_launches") > n0
        assert ex.stats()[0] > 0
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def _worker_shrunk(rank, world, port, levels, spec, overlap, q):
    _worker(rank, world, port, levels, spec, overlap, q, n=6, radius=2)


def _driver_worker(rank, world, port, n, refinements, tol, q):
    """test_gpu_dist._driver_worker for Tri64, with the row-band kernel's launches counted on both sides."""
    try:
        sys.path.insert(0, ROOT)
        import torch
        import torch.distributed as dist
        import homogenization_jl_amd as hmg
        from homogenization_jl_amd import driver, dist as hdist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        ctx = hmg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
        sgrid = driver.generate_conductivity(2, width, 31)
        import time
        t0 = time.perf_counter()
        n0 = ctx.counter("rows_launches")
        want, hist_s = driver.checkerboard_homogenization(n, hmg.Tri64, refinements=refinements, tolerance=tol, ctx=ctx,
                                                          sigma_grid=sgrid, seed=4)
        n1 = ctx.counter("rows_launches")
        t1 = time.perf_counter()
        ctx.set_option("overlap_min_doubles", 1)              # (a small cut: overlap every level, so that the cell lists are used)
        got, hist_p = hdist.partitioned_checkerboard_homogenization(ctx, n, hmg.Tri64, world, rank, refinements=refinements,
                                                                    tolerance=tol, sigma_grid=sgrid, seed=4)
        t2 = time.perf_counter()
        print(f"tri_deep_dist driver rank {rank}/{world}: one rank {t1 - t0:.2f} s, partitioned {t2 - t1:.2f} s, {len(hist_s)} V-cycles, "
              f"sigma {want:.12f} / {got:.12f}", flush=True)
        assert ctx.counter("rows_launches") > n1 > n0
        assert [h[:2] for h in hist_p] == [h[:2] for h in hist_s], (hist_p[-1], hist_s[-1])
        assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (got, want)
        for a, b in zip(hist_s, hist_p):
            assert abs(a[2] - b[2]) <= 1e-7 * max(a[2], 1e-12) and abs(a[3] - b[3]) <= 1e-10
        outer = len({h[0] for h in hist_s})
        dist.destroy_process_group()
        q.put((rank, f"ok {outer} {len(hist_s)}"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def _run_ranks(target, world, args, timeout):
    """One child per rank under a queue timeout; a rank that fails ends the test (no retry), nothing is left running."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=timeout) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return sorted(res)


@pytest.mark.parametrize("world,levels,spec,overlap",
                         [(2, 9, "halves", True), (2, 9, "halves", False), (4, 10, "quadrants", True), (2, 11, "halves", True),
                          (3, 9, "hash", True)])
def test_multi_rank_vcycle_matches_serial_oracle(world, levels, spec, overlap):
    """Two V-cycles on 32 cells of 9 / 10 / 11 levels over 2 / 4 / 3 ranks against the serial oracle on the global mesh:
    x <= 1e-9 per cycle, norm_unique(r) <= 1e-8.  With the overlap on the finest levels' applies are split into a cut-first and
    an inner launch of the row-band kernel, each with its cell list (both non-empty on the halves and the quadrants; the hashed
    partition has no inner cell on any rank)."""
    for rank, msg in _run_ranks(_worker, world, (levels, spec, overlap), 900):
        assert msg == "ok", f"rank {rank}: {msg}"


def test_multi_rank_shrink_then_vcycle_level9():
    """A partitioned grid of 9 levels that is shrunk: 6 x 6 squares (72 cells) in halves over two ranks, level vectors created and
    filled, then hmg_grid_shrink to the 32 cells within radius 2 -- the cell lists, cut tables and cell counts are those of the
    shrunk grid, the vectors keep their storage.  Two V-cycles against the serial oracle on the sub-mesh, bounds as above."""
    for rank, msg in _run_ranks(_worker_shrunk, 2, (9, "halves", True), 900):
        assert msg == "ok", f"rank {rank}: {msg}"


@pytest.mark.parametrize("L", [9, 10])
def test_synthetic_cut_rehearsal_is_bit_identical_2d(oracle, L):
    """test_gpu_dist.test_synthetic_cut_rehearsal_is_bit_identical on a 2D grid of 9 / 10 levels: the 4 x 4 lattice on ONE rank,
    cut at x = 0 and y = 0 (cut_owner = quadrant), a 1-rank RCCL communicator.  x, r and norm_unique(r) after two V-cycles
    equal the unpartitioned grid's bit for bit, overlap on and off."""
    import homogenization_jl_amd as hmg
    from homogenization_jl_amd import dist as hdist
    O = oracle
    gm, sig = lattice(O)
    gbase = hmg.Mesh(gm.nodes, gm.elements + 1)
    ne = gm.nelements()
    for overlap in (True, False):
        ctx = hmg.Context(0)
        try:
            g = hdist.PartitionedGrid(ctx, gbase, L, np.zeros(ne, np.int32), 0, 1, cut_owner=owners(O, gm, "quadrants", 4))
            ex = hdist.Exchange(ctx, g, None, "rccl")
            op = hmg.L2PlusDivAGrad(g, LAM, sig)
            ex.set_overlap(g, overlap)
            ctx.set_option("overlap_min_doubles", 1)
            counts = g.table_i32("cut_counts")
            assert counts[7] > 0 and counts[8] > 0 and counts[9] > 0 and counts[10] > 0, counts
            assert counts[9] + counts[10] == ne
            g1 = hmg.ImplicitFineGrid(ctx, gbase, L)
            op1 = hmg.L2PlusDivAGrad(g1, LAM, sig)
            np.testing.assert_array_equal(g.local_cells, np.arange(ne))
            sts_p = [hmg.LevelState(g, i + 1) for i in range(L)]
            sts_s = [hmg.LevelState(g1, i + 1) for i in range(L)]
            for st, gg in ((sts_p, g), (sts_s, g1)):
                st[-1].x.rand(5); st[-1].b.rand(6)
                hmg.broadcast_interfaces(st[-1].x, gg, L)
                hmg.apply_constraint(st[-1].x, L, gg)
            np.testing.assert_array_equal(sts_p[-1].x.to_host(), sts_s[-1].x.to_host())
            bl_p, bl_s = hmg.BaseLevel(g), hmg.BaseLevel(g1)
            calls0, _ = ex.stats()
            n0 = ctx.counter("rows_launches")
            for _ in range(2):
                hmg.vcycle(g, bl_p, [op] * L, sts_p, L, 3)
            n1 = ctx.counter("rows_launches")
            for _ in range(2):
                hmg.vcycle(g1, bl_s, [op1] * L, sts_s, L, 3)
            n2 = ctx.counter("rows_launches")
            assert n2 > n1 > n0
            if overlap:
                assert n1 - n0 > n2 - n1                # (the split applies are two launches each)
            x = sts_s[-1].x.to_host()
            assert np.isfinite(x).all() and np.abs(x).max() > 0
            np.testing.assert_array_equal(sts_p[-1].x.to_host(), x)
            np.testing.assert_array_equal(sts_p[-1].r.to_host(), sts_s[-1].r.to_host())
            assert hmg.norm_unique(sts_p[-1].r) == hmg.norm_unique(sts_s[-1].r)
            assert ex.stats()[0] > calls0
        finally:
            ctx.close()


@pytest.mark.parametrize("world", [2, 4])
def test_partitioned_driver_matches_single_gpu_driver_refinements8(world):
    """checkerboard_homogenization(1, Tri64, refinements = 8, tolerance = 1e-3) -- 800 triangles of 9 levels -- on one rank
    against partitioned_checkerboard_homogenization on 2 / 4 gloo ranks (overlap on every level, so that the applies are split and
    the row-band kernel gets its cell lists), same sigma_grid and seed, device against device:
    same V-cycle counts per outer step, sigma equal to 1e-10, per-cycle history as in
    test_gpu_dist.test_partitioned_driver_matches_single_gpu_driver.
    (n = 1 ends after its first outer step: the next sub-domain, radius 1 + 11, would be larger than the domain of radius
    2 + 8, so no domain shrink happens here; the smallest n whose outer loop shrinks is 5 -- 25 088 triangles, 6.6 GB per
    level-9 vector.  The shrink of a 9-level grid is held by test_gpu_tri_deep_forms.test_shrink_then_vcycle_level9.)"""
    for rank, msg in _run_ranks(_driver_worker, world, (1, 8, 1e-3), 900):
        assert msg.startswith("ok"), f"rank {rank}: {msg}"
        assert int(msg.split()[1]) >= 1 and int(msg.split()[2]) >= 2
