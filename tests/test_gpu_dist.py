"""
Two ranks sharing the one GPU of the test box (gloo all-reduces device tensors through the host): the
full device path of the partitioned solver -- pack / exchange / unpack after every interface sum, summed
CG scalars, fused CG pass with global multiplicities, replicated coarse solve -- against the serial
oracle V-cycle on the global mesh.
"""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, width, levels, overlap, q, own_stream=False, threshold="all"):
    try:
        sys.path.insert(0, ROOT)
        import torch
        import torch.distributed as dist
        import homogenization_jl_amd as hmg
        from homogenization_jl_amd import dist as hdist
        from oracle import oracle as O
        O.NTHREADS[0] = 2
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        # own_stream: a library-owned non-blocking stream that is NOT torch's current stream -- the callbacks must
        # still order their collectives behind the pack kernels and before the unpack kernels
        ctx = hmg.Context(0) if own_stream else hmg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        if isinstance(width, str):   # "delaunay3" / "delaunay2": unstructured base mesh, ragged partition (hash of the cell id)
            dim = int(width[-1])
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from _meshes import delaunay_mesh
            dm = delaunay_mesh(O, dim, 70, 13)
            gbase = hmg.Mesh(dm.nodes, dm.elements + 1)
            owner = ((np.arange(dm.nelements()) * 2654435761 >> 7) % world).astype(np.int32)
            prob = hdist.PartitionedProblem()
            prob.implicit = hdist.PartitionedGrid(ctx, gbase, levels, owner, rank, world)
            prob.exchange = hdist.Exchange(ctx, prob.implicit)
            prob.cond = np.random.default_rng(3).choice([1.0, 9.0], size=(dm.nelements(), dim))
            prob.op = hmg.L2PlusDivAGrad(prob.implicit, 1.0, prob.cond)
            prob.global_base = gbase
            prob.base_level = lambda: hmg.BaseLevel(prob.implicit)
        else:
            prob = hdist.partitioned_checkerboard(ctx, width, levels, world, rank, seed=3)
        g = prob.implicit
        prob.exchange.set_overlap(g, overlap)
        ctx.set_option("overlap_min_doubles", 1)              # (small meshes: overlap every level so that the path is exercised)
        if threshold == "between":
            # a threshold BETWEEN the ranks' own finest-level cut sizes.  A decision taken from rank-local
            # numbers would send some ranks down the overlapped form (exchange before the scalar sums) and the others down the
            # plain one (after them): mismatched collectives.  The library must decide from a number all ranks agree on.
            mine = torch.tensor([float(g._lib.hmg_grid_cut_buffer_doubles(g.h, levels))], dtype=torch.float64)
            every = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(every, mine)
            sizes = sorted(int(t.item()) for t in every)
            assert sizes[0] < sizes[-1], sizes                 # (the partition must be asymmetric for this test to mean anything)
            ctx.set_option("overlap_min_doubles", (sizes[0] + sizes[-1]) // 2)
        L = levels
        # serial oracle on the global mesh with the same inputs
        gm = O.Mesh(prob.global_base.nodes, prob.global_base.elements - 1)
        gi = O.ImplicitFineGrid.create(gm, L)
        cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(gm))
        ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), cons, 1.0, prob.cond)
               for l in gi.reference.levels]
        sts = [O.LevelState.create(gm.nelements(), gi.nf(i + 1)) for i in range(L)]
        rng = np.random.default_rng(5)
        sts[-1].x[...] = rng.random(sts[-1].x.shape)
        sts[-1].b[...] = rng.standard_normal(sts[-1].x.shape)
        O.broadcast_interfaces(sts[-1].x, gi, L)
        O.apply_constraint(sts[-1].x, L, cons, gi)
        x0, b0 = sts[-1].x.copy(order="F"), sts[-1].b.copy(order="F")
        base = O.make_base_level(gm, prob.cond, 1.0)
        dsts = [hmg.LevelState(g, i + 1) for i in range(L)]
        dsts[-1].x.from_host(x0[:, g.local_cells])
        dsts[-1].b.from_host(b0[:, g.local_cells])
        dbase = prob.base_level()
        for cyc in range(2):
            O.vcycle(gi, base, ops, sts, L, 3)
            hmg.vcycle(g, dbase, [prob.op] * L, dsts, L, 3)
            got = dsts[-1].x.to_host()
            want = sts[-1].x[:, g.local_cells]
            err = np.abs(got - want).max() / np.abs(sts[-1].x).max()
            assert err <= 1e-9, (cyc, err)
        r = sts[-1].r.copy(order="F")
        O.zero_out_all_but_one(r, gi, L)
        assert abs(hmg.norm_unique(dsts[-1].r) - np.linalg.norm(r)) <= 1e-8 * np.linalg.norm(r)
        assert prob.exchange.stats()[0] > 0
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


@pytest.mark.parametrize("world,width,levels,overlap,own_stream",
                         [(2, 4, 4, True, False), (2, 4, 4, False, False), (2, 2, 7, True, False), (4, 2, 4, True, False),
                          (3, "delaunay3", 3, True, False), (2, "delaunay2", 5, True, False), (2, "delaunay2", 5, False, False),
                          (2, 4, 4, True, True), (2, 4, 4, False, True),
                          (8, 2, 3, True, False)])               # octants of a 4^3 brick: eight processes on the one GPU
def test_multi_rank_vcycle_matches_serial_oracle(world, width, levels, overlap, own_stream):
    """overlap=True: cut-adjacent cells first, asynchronous sum over ranks in flight during the rest."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, width, levels, overlap, q, own_stream)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in sorted(res):
        assert msg == "ok", f"rank {rank}: {msg}"


@pytest.mark.parametrize("world,width,levels", [(3, "delaunay3", 3), (3, 3, 4)])
def test_overlap_decision_is_the_same_on_every_rank(world, width, levels):
    """Asymmetric partitions (hashed owners; three slabs: the middle rank has twice the cut of the end ranks) with the overlap
    threshold between the ranks' local cut sizes: two V-cycles against the serial oracle, no deadlock."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, width, levels, True, q, False, "between")) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=300) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank, msg in sorted(res):
        assert msg == "ok", f"rank {rank}: {msg}"


def _driver_worker(rank, world, port, n, dim, refinements, tol, q):
    try:
        sys.path.insert(0, ROOT)
        import torch
        import torch.distributed as dist
        import homogenization_jl_amd as hmg
        from homogenization_jl_amd import driver, dist as hdist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        ctx = hmg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        tag = hmg.Tri64 if dim == 2 else hmg.Tet64
        width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
        sgrid = driver.generate_conductivity(dim, width, 31)
        want, hist_s = driver.checkerboard_homogenization(n, tag, refinements=refinements, tolerance=tol, ctx=ctx,
                                                          sigma_grid=sgrid, seed=4)
        got, hist_p = hdist.partitioned_checkerboard_homogenization(ctx, n, tag, world, rank, refinements=refinements,
                                                                    tolerance=tol, sigma_grid=sgrid, seed=4)
        assert [h[:2] for h in hist_p] == [h[:2] for h in hist_s], (hist_p[-1], hist_s[-1])
        assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (got, want)
        for a, b in zip(hist_s, hist_p):
            assert abs(a[2] - b[2]) <= 1e-7 * max(a[2], 1e-12) and abs(a[3] - b[3]) <= 1e-10
        shrinks = len({h[0] for h in hist_s})
        dist.destroy_process_group()
        q.put((rank, f"ok {shrinks}"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


@pytest.mark.parametrize("world,n,dim,refinements,tol,min_outer", [(2, 5, 2, 2, 1e-3, 2), (4, 5, 2, 2, 1e-3, 2),
                                                                   (2, 0, 3, 2, 1e-3, 1)])
def test_partitioned_driver_matches_single_gpu_driver(world, n, dim, refinements, tol, min_outer):
    """checkerboard_homogenization over several ranks (halves / quadrants about the origin), including the domain
    shrink of a partitioned grid (n = 5: 56 -> 55 -> ...): same V-cycle counts, sigma equal to 1e-10."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_driver_worker, args=(r, world, port, n, dim, refinements, tol, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in sorted(res):
        assert msg.startswith("ok"), f"rank {rank}: {msg}"
        assert int(msg.split()[1]) >= min_outer


def test_in_library_rccl_communicator_single_rank(oracle):
    """hmg_comm_init / hmg_grid_use_comm with a one-rank RCCL communicator (all a single-GPU box allows: RCCL refuses two
    ranks on one device): the partitioned code path -- ncclAllReduce of the CG scalars and of the level-1 gather on the
    context's stream, batched r.r + p.Ap -- gives the single-GPU result; then the partitioned driver through the same
    communicator (hmg_comm_sum_host for the integrals)."""
    import homogenization_jl_amd as hmg
    from homogenization_jl_amd import driver, dist as hdist
    O = oracle
    ctx = hmg.Context(0)
    try:
        L, w = 4, 4
        prob = hdist.partitioned_checkerboard(ctx, w, L, 1, 0, seed=3, backend="rccl")
        g = prob.implicit
        g1 = hmg.ImplicitFineGrid(ctx, prob.global_base, L)            # the same mesh and field, not partitioned
        op1 = hmg.L2PlusDivAGrad(g1, 1.0, prob.cond)
        np.testing.assert_array_equal(g.local_cells, np.arange(g1.ncells()))
        sts_p = [hmg.LevelState(g, i + 1) for i in range(L)]
        sts_s = [hmg.LevelState(g1, i + 1) for i in range(L)]
        for st, gg in ((sts_p, g), (sts_s, g1)):
            st[-1].x.rand(5); st[-1].b.rand(6)
            hmg.broadcast_interfaces(st[-1].x, gg, L)
            hmg.apply_constraint(st[-1].x, L, gg)
        bl_p, bl_s = prob.base_level(), hmg.BaseLevel(g1)
        for _ in range(2):
            hmg.vcycle(g, bl_p, [prob.op] * L, sts_p, L, 3)
            hmg.vcycle(g1, bl_s, [op1] * L, sts_s, L, 3)
        a, b = sts_p[-1].x.to_host(), sts_s[-1].x.to_host()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
        calls, doubles = prob.exchange.stats()
        assert calls > 0 and doubles > 0
        assert abs(hmg.norm_unique(sts_p[-1].r) - hmg.norm_unique(sts_s[-1].r)) <= 1e-12 * hmg.norm_unique(sts_s[-1].r)
        assert prob.exchange.rank_sum(1.5, -2.0) == [1.5, -2.0]
        sg = driver.generate_conductivity(3, 10, 31)
        want, hist_s = driver.checkerboard_homogenization(0, hmg.Tet64, refinements=2, tolerance=1e-3, ctx=ctx, sigma_grid=sg, seed=4)
        got, hist_p = hdist.partitioned_checkerboard_homogenization(ctx, 0, hmg.Tet64, 1, 0, refinements=2, tolerance=1e-3,
                                                                    sigma_grid=sg, seed=4, backend="rccl")
        assert len(hist_s) == len(hist_p) and abs(got - want) <= 1e-10 * max(1.0, abs(want))
    finally:
        ctx.close()


@pytest.mark.parametrize("w,L", [(4, 4), (2, 6)])
def test_synthetic_cut_rehearsal_is_bit_identical(w, L):
    """The partitioned code path at work on ONE rank (src/implicit_fine_grid.jl:209-328 called at
    src/multigrid.jl:51,61,75): the block is cut at its three mid-planes (cut_owner = octant), a 1-rank RCCL communicator
    does the sums over ranks (the identity).  Cut-first cell lists, cut groups / cut face pairs summed before the pack,
    k_cut_pack / unpack, ev_packed / ev_summed and ncclAllReduce on the second stream all run; x and r after two V-cycles
    equal the unpartitioned grid's bit for bit, with the overlap on and off."""
    import homogenization_jl_amd as hmg
    from homogenization_jl_amd import dist as hdist
    for overlap in (True, False):
        ctx = hmg.Context(0)
        try:
            prob = hdist.partitioned_checkerboard(ctx, w, L, 1, 0, seed=3, backend="rccl", synthetic_cut=True)
            g = prob.implicit
            prob.exchange.set_overlap(g, overlap)
            ctx.set_option("overlap_min_doubles", 1)          # (these meshes are small: overlap every level)
            counts = g.table_i32("cut_counts")
            assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0 and counts[6] == counts[0] and counts[9] > 0
            g1 = hmg.ImplicitFineGrid(ctx, prob.global_base, L)
            op1 = hmg.L2PlusDivAGrad(g1, 1.0, prob.cond)
            sts_p = [hmg.LevelState(g, i + 1) for i in range(L)]
            sts_s = [hmg.LevelState(g1, i + 1) for i in range(L)]
            for st, gg in ((sts_p, g), (sts_s, g1)):
                st[-1].x.rand(5); st[-1].b.rand(6)
                hmg.broadcast_interfaces(st[-1].x, gg, L)
                hmg.apply_constraint(st[-1].x, L, gg)
            np.testing.assert_array_equal(sts_p[-1].x.to_host(), sts_s[-1].x.to_host())
            bl_p, bl_s = prob.base_level(), hmg.BaseLevel(g1)
            calls0, _ = prob.exchange.stats()
            for _ in range(2):
                hmg.vcycle(g, bl_p, [prob.op] * L, sts_p, L, 3)
                hmg.vcycle(g1, bl_s, [op1] * L, sts_s, L, 3)
            np.testing.assert_array_equal(sts_p[-1].x.to_host(), sts_s[-1].x.to_host())
            np.testing.assert_array_equal(sts_p[-1].r.to_host(), sts_s[-1].r.to_host())
            assert hmg.norm_unique(sts_p[-1].r) == hmg.norm_unique(sts_s[-1].r)
            calls, doubles = prob.exchange.stats()
            assert calls > calls0                  # (one rank: the scalar sums; the cut segments have no other member)
        finally:
            ctx.close()


def test_unsupported_world_size_raises_everywhere():
    """3, 6, 16 ranks (or 8 in 2D) would leave ranks without cells: refused before any collective."""
    import homogenization_jl_amd as hmg
    from homogenization_jl_amd import dist as hdist
    for world, tag in ((3, hmg.Tet64), (6, hmg.Tet64), (16, hmg.Tet64), (8, hmg.Tri64)):
        with pytest.raises(ValueError):
            hdist.partitioned_checkerboard_homogenization(None, 1, tag, world, 0)


def _rccl_worker(rank, world, port, q):
    """One rank per PHYSICAL GPU, the in-library RCCL communicator: both exchange forms against the serial oracle and against
    each other."""
    try:
        sys.path.insert(0, ROOT)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch
        import torch.distributed as dist
        import homogenization_jl_amd as hmg
        from homogenization_jl_amd import dist as hdist
        from oracle import oracle as O
        O.NTHREADS[0] = 2
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                device_id=torch.device("cuda", rank))
        ctx = hmg.Context(rank, stream=torch.cuda.current_stream().cuda_stream)
        levels, width = 5, 4
        res = {}
        for form in ("p2p", "allreduce"):
            if form == "allreduce":
                os.environ["HMG_EXCHANGE"] = "allreduce"
            else:
                os.environ.pop("HMG_EXCHANGE", None)
            for overlap in (True, False):
                prob = hdist.partitioned_checkerboard(ctx, width, levels, world, rank, seed=3)
                g = prob.implicit
                assert prob.exchange.backend == "rccl" and ctx.counter("comm_nranks") == world
                prob.exchange.set_overlap(g, overlap)
                ctx.set_option("overlap_min_doubles", 1)
                ne = prob.global_base.elements.shape[0]
                x0 = hmg.host_random((g.nf(levels), ne), 5)
                b0 = hmg.host_random((g.nf(levels), ne), 6) - 0.5
                st = [hmg.LevelState(g, i + 1) for i in range(levels)]
                st[-1].x.from_host(x0[:, g.local_cells]); st[-1].b.from_host(b0[:, g.local_cells])
                hmg.broadcast_interfaces(st[-1].x, g, levels)
                hmg.apply_constraint(st[-1].x, levels, g)
                bl = prob.base_level()
                for _ in range(2):
                    hmg.vcycle(g, bl, [prob.op] * levels, st, levels, 3)
                res[(form, overlap)] = (st[-1].x.to_host(), st[-1].r.to_host())
                for s in st:
                    s.close()
        os.environ.pop("HMG_EXCHANGE", None)
        # serial oracle on the global mesh
        gm = O.Mesh(prob.global_base.nodes, prob.global_base.elements - 1)
        gi = O.ImplicitFineGrid.create(gm, levels)
        cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(gm))
        ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), cons, 1.0, prob.cond)
               for l in gi.reference.levels]
        sts = [O.LevelState.create(gm.nelements(), gi.nf(i + 1)) for i in range(levels)]
        sts[-1].x[...] = x0; sts[-1].b[...] = b0
        O.broadcast_interfaces(sts[-1].x, gi, levels)
        O.apply_constraint(sts[-1].x, levels, cons, gi)
        base = O.make_base_level(gm, prob.cond, 1.0)
        for _ in range(2):
            O.vcycle(gi, base, ops, sts, levels, 3)
        want = sts[-1].x[:, g.local_cells]
        ref = res[("p2p", True)]
        assert np.abs(ref[0] - want).max() <= 1e-9 * np.abs(sts[-1].x).max()
        for key, (x, r) in res.items():      # every form and both overlap settings: the same bits (partials added in rank order)
            np.testing.assert_array_equal(x, ref[0], err_msg=str(key))
            np.testing.assert_array_equal(r, ref[1], err_msg=str(key))
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def test_rccl_exchange_on_two_physical_gpus():
    """The N > 1 RCCL path itself (grouped ncclSend / ncclRecv among the sharers, ncclAllReduce, second stream): needs two
    physical GPUs -- RCCL refuses two ranks on one device --, so it is SKIPPED on the one-GPU boxes this suite normally runs on
    (the path is then unvalidated on hardware: README).  Where it runs: two V-cycles on 2 x 4^3 cubes, level 5, both exchange
    forms, overlap on and off, against the serial oracle (1e-9) and against each other (bit for bit)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two physical GPUs (RCCL refuses two ranks on one device)")
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rccl_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=600) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank, msg in sorted(res):
        assert msg == "ok", f"rank {rank}: {msg}"
