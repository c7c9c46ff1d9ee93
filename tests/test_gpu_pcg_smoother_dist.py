"""
The Jacobi-preconditioned CG smoother on partitioned grids: gloo ranks sharing the one GPU of the test box (the harness of
tests/test_gpu_fcg_dist.py) and the synthetic cut on one rank, against the unpartitioned grid in the same process.  The inverse
diagonal is summed across the cut once per operator (one exchange per level, every rank in the same call): bit for bit the
unpartitioned grid's; x after two V-cycles to 1e-9 max|x|, that file's tolerance.  The partitioned driver takes the keyword.
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


def _compare(hmg, prob, L, local_cells, cycles=2):
    """dinv of every level and x after `cycles` V-cycles: the partitioned grid of `prob` against the unpartitioned one."""
    ctx, g = prob.implicit.ctx, prob.implicit
    g1 = hmg.ImplicitFineGrid(ctx, prob.global_base, L)
    g1.set_smoother("jacobi")
    op1 = hmg.L2PlusDivAGrad(g1, 1.0, prob.cond)
    g.set_smoother("jacobi")
    for lev in range(2, L + 1):
        mine, whole = hmg.smoother_diag(g, lev).to_host(), hmg.smoother_diag(g1, lev).to_host()[:, local_cells]
        assert np.isfinite(mine).all() and (mine == 0.0).any() and (mine > 0.0).any()
        np.testing.assert_array_equal(mine, whole, err_msg=f"dinv of level {lev}")
    rng = np.random.default_rng(5)
    nf, ne = g1.nf(L), g1.ncells()
    x0 = np.asfortranarray(rng.random((nf, ne)))
    b0 = np.asfortranarray(rng.standard_normal((nf, ne)))
    out = []
    for gg, op, bl, cols in ((g, prob.op, prob.base_level(), local_cells), (g1, op1, hmg.BaseLevel(g1), slice(None))):
        sts = [hmg.LevelState(gg, i + 1) for i in range(L)]
        sts[-1].x.from_host(np.asfortranarray(x0[:, cols]))
        sts[-1].b.from_host(np.asfortranarray(b0[:, cols]))
        hmg.broadcast_interfaces(sts[-1].x, gg, L)
        hmg.apply_constraint(sts[-1].x, L, gg)
        for _ in range(cycles):
            hmg.vcycle(gg, bl, [op] * L, sts, L, 3)
        out.append(sts[-1].x.to_host())
    err = np.abs(out[0] - out[1][:, local_cells]).max() / np.abs(out[1]).max()
    assert np.isfinite(out[0]).all() and err <= 1e-9, err
    return err, out


def _worker(rank, world, port, width, levels, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import torch
        import torch.distributed as dist
        import homogenization_jl_amd as hmg
        from homogenization_jl_amd import dist as hdist
        from test_gpu_pcg_smoother_dist import _compare
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        ctx = hmg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        prob = hdist.partitioned_checkerboard(ctx, width, levels, world, rank, seed=3, values=(1.0, 100.0))
        err, _ = _compare(hmg, prob, levels, prob.implicit.local_cells)
        dist.destroy_process_group()
        q.put((rank, f"ok {err:.2e}"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


@pytest.mark.parametrize("world,width,levels", [(2, 4, 4), (4, 2, 4)])
def test_partitioned_grid_matches_the_unpartitioned_one(world, width, levels):
    """Halves and quadrants at contrast 100: dinv of levels 2-4 bit for bit (the diagonal is summed in fixed point, so the order
    in which copies and ranks are added does not matter), x after two V-cycles to 1e-9."""
    for rank, msg in _run(_worker, world, (width, levels)):
        print(f"rank {rank}: x {msg.split()[1]}")


@pytest.mark.parametrize("w,L", [(4, 4), (2, 6)])
def test_synthetic_cut_is_bit_identical(w, L):
    """One rank, the block cut at its mid-planes, a 1-rank RCCL communicator: dinv and x after two V-cycles equal the
    unpartitioned grid's bit for bit."""
    import homogenization_jl_amd as hmg
    from homogenization_jl_amd import dist as hdist
    ctx = hmg.Context(0)
    try:
        prob = hdist.partitioned_checkerboard(ctx, w, L, 1, 0, seed=3, values=(1.0, 100.0), backend="rccl", synthetic_cut=True)
        err, out = _compare(hmg, prob, L, prob.implicit.local_cells)
        np.testing.assert_array_equal(out[0], out[1][:, prob.implicit.local_cells])
    finally:
        ctx.close()


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
        sgrid = driver.generate_conductivity(dim, width, 31, values=(1.0, 100.0))
        kw = dict(refinements=refinements, tolerance=tol, sigma_grid=sgrid, seed=4)
        st = {}
        cg, hist_cg = hdist.partitioned_checkerboard_homogenization(ctx, n, tag, world, rank, smoother="cg", **kw)
        got, hist = hdist.partitioned_checkerboard_homogenization(ctx, n, tag, world, rank, smoother="jacobi", stats=st, **kw)
        assert st["smoother"] == "jacobi"
        assert abs(got - cg) <= 1e-3 * abs(cg), (got, cg)
        dist.destroy_process_group()
        q.put((rank, f"ok {len(hist)} {len(hist_cg)} {len({h[0] for h in hist})}"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def test_partitioned_driver_takes_the_keyword():
    """2D halves, n = 5, two refinements, contrast 100, a domain shrink of the partitioned grid included: smoother="jacobi" agrees
    with the partitioned "cg" run to 1e-3 (the two stop about a tolerance apart)."""
    res = _run(_driver_worker, 2, (5, 2, 2, 1e-4))
    for rank, msg in res:
        cycles, cycles_cg, outer = (int(v) for v in msg.split()[1:])
        print(f"rank {rank}: jacobi {cycles} cycles, cg {cycles_cg}, {outer} outer steps")
        assert outer >= 2
