"""
The V-cycle-preconditioned flexible CG on partitioned grids: gloo ranks sharing the one GPU of the test box (the harness of
tests/test_gpu_dist.py).  The outer iteration adds no cut exchange, only two small sums over the ranks per step (z.q; p.q and
p.R together) through the grid's scalar_sum hook.  Against the serial cell-local statement of tests/_fcg_form.py on the global
mesh (1e-9 max|x|, that file's tolerance for V-cycles), against the unpartitioned grid (synthetic cut on one rank: the same
bits) and through the partitioned driver.  A world-2 CPU case is not possible: the CPU harness of tests/test_dist_gloo.py
carries partition tables only, the library has no compute path without a device.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(target, world, args, timeout=900):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=timeout) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank, msg in sorted(res):
        assert msg.startswith("ok"), f"rank {rank}: {msg}"
    return sorted(res)


def _worker(rank, world, port, width, levels, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import torch
        import torch.distributed as dist
        import homogenization_jl_amd as hmg
        from homogenization_jl_amd import dist as hdist
        from oracle import oracle as O
        from _fcg_form import fcg_local
        O.NTHREADS[0] = 2
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        ctx = hmg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        prob = hdist.partitioned_checkerboard(ctx, width, levels, world, rank, seed=3)
        g, L = prob.implicit, levels
        gm = O.Mesh(prob.global_base.nodes, prob.global_base.elements - 1)
        gi = O.ImplicitFineGrid.create(gm, L)
        cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(gm))
        ops = [O.L2PlusDivAGrad(O.build_local_diffusion_operators(l), O.mass_matrix(l), cons, 1.0, prob.cond)
               for l in gi.reference.levels]
        sts = [O.LevelState.create(gm.nelements(), gi.nf(i + 1)) for i in range(L)]
        rng = np.random.default_rng(5)
        x0 = np.asfortranarray(rng.random(sts[-1].x.shape))
        b0 = np.asfortranarray(rng.standard_normal(sts[-1].x.shape))
        O.broadcast_interfaces(x0, gi, L)
        O.apply_constraint(x0, L, cons, gi)
        dsts = [hmg.LevelState(g, i + 1) for i in range(L)]
        x = hmg.DeviceMatrix(g, L).from_host(x0[:, g.local_cells])
        b = hmg.DeviceMatrix(g, L).from_host(b0[:, g.local_cells])
        f = hmg.FlexibleCG(g, prob.base_level(), [prob.op] * L, dsts, L, 3)
        f.start(x, b)
        loc = fcg_local(O, gi, O.make_base_level(gm, prob.cond, 1.0), ops, sts, L, 3, x0, b0)
        for it in range(3):
            wx, wR, wp, wa, wb = next(loc)
            calls0 = prob.exchange.stats()[0]
            f.step()
            alpha, beta, pq, pr = f.scalars()
            calls = prob.exchange.stats()[0] - calls0
            err = np.abs(x.to_host() - wx[:, g.local_cells]).max() / np.abs(wx).max()
            assert err <= 1e-9, (it, err)
            assert abs(alpha - wa) <= 1e-8 * abs(wa) and abs(beta - wb) <= 1e-8 * abs(wb), (it, alpha, wa, beta, wb)
            mine = torch.tensor([alpha, beta, pq, pr], dtype=torch.float64)
            every = [torch.zeros(4, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(every, mine)
            for t in every:
                assert torch.equal(t, every[0]), (it, every)        # the same bits on every rank
        want_r = float(np.linalg.norm(_unique(O, gi, L, wR)))
        assert abs(f.residual_norm() - want_r) <= 1e-8 * want_r
        dist.destroy_process_group()
        q.put((rank, f"ok {calls}"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def _unique(O, gi, L, R):
    r = np.asfortranarray(R.copy())
    O.broadcast_interfaces(r, gi, L)
    O.zero_out_all_but_one(r, gi, L)
    return r


@pytest.mark.parametrize("world,width,levels", [(2, 4, 4), (4, 2, 4)])
def test_partitioned_steps_match_the_serial_statement(world, width, levels):
    """Halves and quadrants: x after each of 3 steps, alpha and beta identical on all ranks, the true residual norm."""
    _run(_worker, world, (width, levels))


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
                                                          sigma_grid=sgrid, seed=4, accelerate=True)
        got, hist_p = hdist.partitioned_checkerboard_homogenization(ctx, n, tag, world, rank, refinements=refinements,
                                                                    tolerance=tol, sigma_grid=sgrid, seed=4, accelerate=True)
        assert [h[:2] for h in hist_p] == [h[:2] for h in hist_s], (hist_p[-1], hist_s[-1])
        assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (got, want)
        shrinks = len({h[0] for h in hist_s})
        dist.destroy_process_group()
        q.put((rank, f"ok {shrinks}"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


@pytest.mark.parametrize("world,n,dim,refinements,tol,min_outer", [(2, 5, 2, 2, 1e-3, 2), (4, 5, 2, 2, 1e-3, 2),
                                                                   (2, 0, 3, 2, 1e-3, 1)])
def test_partitioned_accelerated_driver_matches_the_single_gpu_one(world, n, dim, refinements, tol, min_outer):
    """accelerate=True over halves / quadrants, domain shrink of a partitioned grid included: the single-GPU accelerated
    driver's cycle counts, sigma to 1e-10 max(1, |sigma|) (the tolerance of the plain drivers' comparison)."""
    res = _run(_driver_worker, world, (n, dim, refinements, tol))
    for rank, msg in res:
        assert int(msg.split()[1]) >= min_outer


@pytest.mark.parametrize("w,L", [(4, 4), (2, 6)])
def test_synthetic_cut_is_bit_identical_and_adds_two_collectives(w, L):
    """One rank, the block cut at its mid-planes, a 1-rank RCCL communicator: x, R, p after three steps equal the
    unpartitioned grid's bit for bit; a step issues the V-cycle's collectives plus two (one in the first step)."""
    import homogenization_jl_amd as hmg
    from homogenization_jl_amd import dist as hdist
    ctx = hmg.Context(0)
    try:
        prob = hdist.partitioned_checkerboard(ctx, w, L, 1, 0, seed=3, backend="rccl", synthetic_cut=True)
        g = prob.implicit
        g1 = hmg.ImplicitFineGrid(ctx, prob.global_base, L)
        op1 = hmg.L2PlusDivAGrad(g1, 1.0, prob.cond)
        out = []
        for gg, op, bl in ((g, prob.op, prob.base_level), (g1, op1, lambda: hmg.BaseLevel(g1))):
            sts = [hmg.LevelState(gg, i + 1) for i in range(L)]
            x, b = hmg.DeviceMatrix(gg, L), hmg.DeviceMatrix(gg, L)
            x.rand(5)
            b.rand(6)
            hmg.broadcast_interfaces(x, gg, L)
            hmg.apply_constraint(x, L, gg)
            base_level = bl()
            calls = []
            if gg is g:                                               # collectives of one V-cycle on this grid
                sts[-1].b.copyto(b)
                hmg.vcycle(gg, base_level, [op] * L, sts, L, 3)       # (the first one also agrees on the cut and sets up level 1)
                c0 = prob.exchange.stats()[0]
                hmg.vcycle(gg, base_level, [op] * L, sts, L, 3)
                calls.append(prob.exchange.stats()[0] - c0)
            f = hmg.FlexibleCG(gg, base_level, [op] * L, sts, L, 3)
            f.start(x, b)
            for _ in range(3):
                c0 = prob.exchange.stats()[0]
                f.step()
                calls.append(prob.exchange.stats()[0] - c0)
            out.append((x.to_host(), f.vec("R"), f.vec("p"), f.scalars(), calls))
            f.close()
        for a, b_ in zip(out[0][:3], out[1][:3]):
            np.testing.assert_array_equal(a, b_)
        assert out[0][3] == out[1][3]
        vc, s1, s2, s3 = out[0][4]
        print(f"comm_calls: V-cycle {vc}, first step {s1}, later steps {s2}, {s3}")
        assert s1 == vc + 1 and s2 == s3 == vc + 2
    finally:
        ctx.close()
