"""What the device tests of grids on a torus share (tests/test_gpu_periodic.py, tests/test_gpu_periodic_general.py): the device
grid next to the oracle on the cells as disjoint simplices, and the check of every primitive against statements that never see
the torus connectivity (tests/_periodic_form.py).  Tolerance: the project's 1e-11 for primitives."""
import numpy as np

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

import _tensor_sigma_form as TS
from _periodic_form import broadcast, disjoint, fine_ids

TOL = 1e-11


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def per_cube(mesh, sgrid):
    """a field per unit cube, C order of the cube's multi-index, on the cells of driver.periodic_mesh (and of what
    _periodic_form.general_torus makes of it: the cells keep their order)"""
    ncubes = mesh.nodes.shape[0]
    return np.repeat(np.asarray(sgrid).reshape((ncubes,) + np.shape(sgrid)[mesh.dim:]), mesh.elements.shape[0] // ncubes, axis=0)


class Torus:
    """A torus, its sigma, the device grid, and the oracle on the disjoint simplices (no interface: cell-local operators only).
    Defaults: 3 x 3 (x 3) unit cubes (`mesh` None), sigma in {1, 9} per cube and direction (`sig` None).  `tensor`: a full SPD
    tensor per cell (`sig` None: _tensor_sigma_form.random_spd, eigenvalues 1 ... 100); the statement of the operator is then
    _tensor_sigma_form.TensorOp / mul.  `den`: the denominator of the coarse positions (_periodic_form.keys)."""

    def __init__(self, O, ctx, dim, levels, seed, classes=0, mesh=None, sig=None, tensor=False, den=1):
        self.O, self.dim, self.levels, self.tensor, self.den = O, dim, levels, tensor, den
        self.mesh = driver.periodic_mesh(hmg.Tet64 if dim == 3 else hmg.Tri64, 3) if mesh is None else mesh
        assert self.mesh.dim == dim
        self.rng = np.random.default_rng(seed)
        ncubes = self.mesh.nodes.shape[0]
        if sig is not None:
            self.sig = np.ascontiguousarray(sig, dtype=np.float64)
        elif tensor:
            self.sig = TS.random_spd(self.rng, self.mesh.elements.shape[0], dim)
        else:
            self.sig = np.repeat(self.rng.choice([1.0, 9.0], size=(ncubes, dim)), self.mesh.elements.shape[0] // ncubes, axis=0)
        assert self.sig.ndim == (3 if tensor else 2)
        nodes, elements = disjoint(self.mesh)
        self.dmesh = O.Mesh(nodes, elements)
        self.impl = O.ImplicitFineGrid.create(self.dmesh, levels)
        self.cons = O.ZeroDirichletConstraint(*O.list_boundary_nodes_edges_faces(self.dmesh))      # (never applied)
        ctx.set_option("weight_cache_classes", classes)                  # (read where the operator is set)
        try:
            self.g = hmg.ImplicitFineGrid(ctx, self.mesh, levels)
            self.A = hmg.L2PlusDivAGrad(self.g, 0.7, self.sig)
        finally:
            ctx.set_option("weight_cache_classes", 0)
        self._parts, self._ids = {}, {}

    def op(self, lev, lam):
        O = self.O
        if lev not in self._parts:
            l = self.impl.reference.levels[lev - 1]
            self._parts[lev] = (O.build_local_diffusion_operators(l), O.mass_matrix(l))
        if self.tensor:
            return TS.TensorOp(*self._parts[lev], self.cons, lam, self.sig)
        return O.L2PlusDivAGrad(*self._parts[lev], self.cons, lam, self.sig)

    def mul(self, alpha, A, x, y):
        """y <- alpha A x + y on the disjoint simplices, cell-local"""
        if self.tensor:
            return TS.mul(self.O, alpha, self.dmesh, A, x, y)
        return self.O.mul(alpha, self.dmesh, A, x, y)

    def ids(self, lev):
        if lev not in self._ids:
            self._ids[lev] = fine_ids(self.g, lev, self.den)
        return self._ids[lev]

    def rand(self, lev):
        return np.asfortranarray(self.rng.standard_normal((self.impl.nf(lev), self.mesh.elements.shape[0])))

    def dev(self, lev, a):
        return hmg.DeviceMatrix(self.g, lev).from_host(a)

    def close(self):
        self.g.close()


def check_primitives(c, levels_checked, lams=(0.7, 0.0)):
    """hmg_apply_ex and hmg_residual against the statement's cell-local mul! on the disjoint simplices; hmg_interface_sum against
    the sum over the copies of every torus node, found by position; the copies agree bitwise; hmg_vec_norm_unique counts a node
    once.  Returns the largest of the errors."""
    worst = 0.0
    for lev in levels_checked:
        ids, n = c.ids(lev)
        for lam in lams:
            c.A.lam = lam
            x, src = c.rand(lev), c.rand(lev)
            want = src.copy(order="F")
            c.mul(-1.3, c.op(lev, lam), x, want)
            out = hmg.DeviceMatrix(c.g, lev)
            dx, dsrc = c.dev(lev, x), c.dev(lev, src)
            c.A._bind()
            hmg.apply_ex(-1.3, c.g, dx, dsrc, out, constrain=True)
            e_apply = relerr(out.to_host(), want)
            wres = src.copy(order="F")
            c.mul(-1.0, c.op(lev, lam), x, wres)
            dst = hmg.LevelState(c.g, lev)
            dst.x.from_host(x)
            dst.b.from_host(src)
            hmg.local_residual(c.g, c.A, dst, lev)
            e_res = relerr(dst.r.to_host(), wres)
            hmg.broadcast_interfaces(out, c.g, lev)
            got = out.to_host()
            e_sum = relerr(got, broadcast(want, ids, n))
            u = np.zeros(n)
            u[ids.ravel()] = got.ravel()
            np.testing.assert_array_equal(u[ids], got)                   # every copy of a torus node holds the same bits
            nu = hmg.norm_unique(out)
            e_norm = abs(nu - np.linalg.norm(u)) / np.linalg.norm(u)
            print(f"level {lev}, lambda {lam}: apply_ex {e_apply:.2e}  residual {e_res:.2e}  interface sum {e_sum:.2e}  norm_unique {e_norm:.2e}")
            assert e_apply <= TOL and e_res <= TOL and e_sum <= TOL and e_norm <= TOL, (lev, lam, e_apply, e_res, e_sum, e_norm)
            worst = max(worst, e_apply, e_res, e_sum, e_norm)
            for v in (out, dx, dsrc):
                v.close()
            dst.close()
    return worst
