"""
dist.partitioned_checkerboard_homogenization_tensor on 2 and 4 gloo ranks sharing the one GPU of the test box (the harness of
tests/test_gpu_fcg_dist.py): the 2D n = 5 case, which includes a shrink of the partitioned domain, against the unpartitioned
device tensor.  The shares of the pair integrals (hmg_integrate modes 3 and 4 return this rank's share) are summed over the
ranks like the existing integrals.  Every entry within 1e-8, the |delta sigma| bound of BASELINE.md.
"""
import os
import sys

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


def _worker(rank, world, port, n, refinements, tol, q):
    try:
        sys.path.insert(0, ROOT)
        import numpy as np
        import torch
        import torch.distributed as dist
        import homogenization_jl_amd as hmg
        from homogenization_jl_amd import driver, dist as hdist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        ctx = hmg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        width = 2 * (driver.compute_box_radius(0, n) + driver.compute_boundary_layer(1.0, n))
        sgrid = driver.generate_conductivity(2, width, 3)
        want, hist_s = driver.checkerboard_homogenization_tensor(n, hmg.Tri64, refinements=refinements, tolerance=tol, ctx=ctx,
                                                                 sigma_grid=sgrid, seed=3)
        stats = {}
        got, hist_p = hdist.partitioned_checkerboard_homogenization_tensor(ctx, n, hmg.Tri64, world, rank, refinements=refinements,
                                                                           tolerance=tol, sigma_grid=sgrid, seed=3, stats=stats)
        err = float(np.abs(got - want).max())
        assert got.shape == (2, 2) and np.array_equal(got, got.T)
        assert err <= 1e-8, (got, want)
        assert {(h[0], h[1]) for h in hist_p} == {(h[0], h[1]) for h in hist_s}
        assert stats["inexact_vcycles"] == 0
        mine = torch.tensor(got.ravel())
        every = [torch.zeros(4, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(every, mine)
        for t in every:
            assert torch.equal(t, every[0]), every                    # identical on every rank
        shrinks = len({h[0] for h in hist_p})
        dist.destroy_process_group()
        q.put((rank, f"ok {shrinks} {err:.3e}"))
    except Exception:                                                    # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 4])
def test_partitioned_tensor_matches_the_single_gpu_one(world):
    """Halves and quadrants, 2D n = 5, one refinement, tolerance 1e-12: two outer steps, so the shrink of a partitioned grid, the
    exchange of the v_k / v_{k-1} handles and the k >= 1 form of the pair integrals are all on the path."""
    res = _run(_worker, world, (5, 1, 1e-12))
    for rank, msg in res:
        print(rank, msg)
        assert int(msg.split()[1]) == 2
