"""The ordinary grids whose tables tests/golden/ordinary_tables_parent.npz records, as the commit before periodic grids built
them: a perturbed 3 x 3 square mesh on 3 levels and a perturbed 2 x 2 x 2 cube mesh on 3 levels, a two-valued conductivity,
lambda = 0.7.  `ordinary_tables` forms them again on a host-only grid."""
import numpy as np

import homogenization_jl_amd as hmg
from homogenization_jl_amd import driver

I32 = ("upload_hash", "face_pairs", "edge_ent", "node_ent", "dmask", "dupmask", "mult", "coarse_colidx")
F64 = ("coef", "coarse_val")


def ordinary_mesh(name):
    tag, n, seed = {"tri": (hmg.Tri64, 3, 5), "tet": (hmg.Tet64, 2, 6)}[name]
    base = driver.hypercube(tag, n)
    rng = np.random.default_rng(seed)
    nodes = base.nodes + 0.2 * (rng.random(base.nodes.shape) - 0.5)
    cond = rng.choice([1.0, 9.0], size=(base.elements.shape[0], base.dim))
    return hmg.Mesh(nodes, base.elements), cond


def ordinary_tables(name):
    mesh, cond = ordinary_mesh(name)
    g = hmg.ImplicitFineGrid(None, mesh, 3)
    g.set_operator(cond, 0.7)
    g.coarse_setup()
    out = {k: g.table_i32(k) for k in I32}
    out.update({k: g.table_f64(k) for k in F64})
    g.close()
    return out
