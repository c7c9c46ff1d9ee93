"""hmg_grid_set_dirichlet_faces on a host-only grid (NULL context: tables, no device): "dmask" and "interior_nodes" against the
closure rule written in numpy (tests/_dirichlet_faces_form.py), the getter, the way back to the default set, and every refusal
-- each with its message and with the tables left as they were."""
import numpy as np
import pytest

import homogenization_jl_amd as hmg
from _dirichlet_faces_form import (all_faces, block_boundary_faces, closure, default_faces, interior_faces, one_based,
                                   plane_faces)


def host_grid(m, levels=2):
    return hmg.ImplicitFineGrid(None, hmg.Mesh(m.nodes, m.elements + 1), levels)


def tables(g):
    return g.table_i32("dmask").copy(), g.table_i32("interior_nodes").copy()


def expect(m, faces):
    dmask, con = closure(m.elements, faces, m.nnodes())
    return dmask, np.flatnonzero(~con)


def sets_of(m, n):
    lo, hi = m.nodes.min(axis=0), m.nodes.max(axis=0)
    mid = plane_faces(m.nodes, m.elements, 0, lo[0] + n // 2)
    sides = np.concatenate([plane_faces(m.nodes, m.elements, m.dim - 1, lo[-1]), plane_faces(m.nodes, m.elements, m.dim - 1, hi[-1])])
    return {"mid-plane": mid, "two sides": sides, "blocks": block_boundary_faces(m.nodes, m.elements, n // 2),
            "empty": np.zeros((0, m.dim), dtype=np.int64)}


@pytest.mark.parametrize("dim,n", [(3, 2), (2, 4), (3, 4)])
def test_default_named_face_by_face_is_the_default(oracle, dim, n):
    m = oracle.hypercube(dim, n)
    never, g = host_grid(m), host_grid(m)
    want = expect(m, default_faces(m.elements))
    for got, ref in zip(tables(never), want):
        np.testing.assert_array_equal(got, ref)                          # the numpy closure states today's tables
    np.testing.assert_array_equal(never.dirichlet_faces(), one_based(default_faces(m.elements)))
    np.testing.assert_array_equal(hmg.api.boundary_faces(never.base), one_based(default_faces(m.elements)))
    g.set_dirichlet_faces(one_based(default_faces(m.elements))[::-1, ::-1])      # any order of faces and within a face
    for got, ref in zip(tables(g), tables(never)):
        np.testing.assert_array_equal(got, ref)
    for which in ("dupmask", "mult", "face_pairs", "edge_ent", "node_ent", "node_first"):
        np.testing.assert_array_equal(g.table_i32(which), never.table_i32(which))
    g.shrink(m.nelements(), m.nnodes())                                  # ... and holds no set of the caller's


@pytest.mark.parametrize("dim,n", [(3, 2), (2, 4), (3, 4), (2, 6)])
@pytest.mark.parametrize("which", ["mid-plane", "two sides", "blocks", "empty"])
def test_tables_follow_the_closure(oracle, dim, n, which):
    m = oracle.hypercube(dim, n)
    faces = sets_of(m, n)[which]
    assert which == "empty" or faces.shape[0] > 0
    g = host_grid(m)
    before = tables(g)
    g.set_dirichlet_faces(one_based(faces))
    for got, ref in zip(tables(g), expect(m, faces)):
        np.testing.assert_array_equal(got, ref)
    if which != "blocks":
        assert not np.array_equal(tables(g)[0], before[0])
    np.testing.assert_array_equal(g.dirichlet_faces(), one_based(np.unique(faces.reshape(-1, dim), axis=0)))
    twice = np.concatenate([faces, faces[:1]]) if faces.shape[0] else faces
    g.set_dirichlet_faces(one_based(twice))                              # a duplicate is accepted once
    assert g.dirichlet_faces().shape[0] == np.unique(faces.reshape(-1, dim), axis=0).shape[0]
    g.set_dirichlet_faces(None)                                          # -1: the default bits
    for got, ref in zip(tables(g), before):
        np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(g.dirichlet_faces(), one_based(default_faces(m.elements)))


def test_faces_between_the_tetrahedra_of_one_cube(oracle):
    """A chosen face sets its bit in BOTH cells; a face whose nodes are all constrained but which was not chosen stays free: with
    the interior faces of one cube every node is constrained (they all contain the diagonal's ends or touch every corner), and no
    outer face carries a face bit."""
    m = oracle.hypercube(3, 1)
    faces = interior_faces(m.elements)
    assert faces.shape[0] == 6
    g = host_grid(m)
    g.set_dirichlet_faces(one_based(faces))
    dmask, interior = tables(g)
    want, _ = expect(m, faces)
    np.testing.assert_array_equal(dmask, want)
    assert interior.size == 0
    assert all(bin(int(d) & 0xF).count("1") == 2 for d in dmask)         # two inner faces per tetrahedron, the outer two free
    assert all((int(d) >> 10) == 0xF for d in dmask)                     # every node bit
    assert sum(bin(int(d) & 0xF).count("1") for d in dmask) == 2 * 6     # each face in two cells


@pytest.mark.parametrize("dim", [3, 2])
def test_refusals_leave_the_tables_alone(oracle, dim):
    from homogenization_jl_amd import dist
    n = 2
    m = oracle.hypercube(dim, n)
    g = host_grid(m)
    mid = one_based(sets_of(m, n)["mid-plane"])
    g.set_dirichlet_faces(mid)
    before = tables(g), g.dirichlet_faces()

    def refused(faces, message):
        with pytest.raises(hmg._lib.HmgError, match=message):
            g.set_dirichlet_faces(faces)
        for got, ref in zip(tables(g), before[0]):
            np.testing.assert_array_equal(got, ref)
        np.testing.assert_array_equal(g.dirichlet_faces(), before[1])

    bad = mid.copy()
    bad[1, 0] = m.nnodes() + 1
    refused(bad, "1 has a node id out of range")
    bad[1, 0] = 0
    refused(bad, "1 has a node id out of range")
    bad = mid.copy()
    bad[1, 0] = bad[1, 1]
    refused(bad, "1 names a node twice")
    known = {tuple(f) for f in all_faces(m.elements)[0]}
    stranger = next(t for t in ((0, m.nnodes() - 1), (0, 1, m.nnodes() - 1)) if len(t) == dim and t not in known)
    bad = np.concatenate([mid, one_based(np.array([stranger]))])
    refused(bad, f"{mid.shape[0]} is not a (face|edge) of any cell")
    with pytest.raises(hmg._lib.HmgError, match="restore the default set first"):
        g.shrink(m.nelements() // 2, m.nnodes())                         # a caller's set is held
    for got, ref in zip(tables(g), before[0]):
        np.testing.assert_array_equal(got, ref)
    # the empty set and lambda = 0: no level-1 system
    sig = np.ones((m.nelements(), dim))
    g.set_operator(sig, 0.0)
    g.set_dirichlet_faces(np.zeros((0, dim), dtype=np.int64))
    with pytest.raises(hmg._lib.HmgError, match="no node is constrained.*lambda = 0"):
        g.coarse_setup()
    g.set_lambda(0.5)
    g.coarse_setup()                                                     # (with a mass term it is regular)
    assert g.table_i32("coarse_rowptr").size == m.nnodes() + 1
    g.set_dirichlet_faces(None)
    # a shrunk grid
    mo = oracle.order_nodes_and_elements_by_magnitude(oracle.hypercube(dim, 4, origin=(-2.0,) * dim))
    s = host_grid(mo)
    s.shrink(oracle.find_elements_in_radius(mo, 1), oracle.find_nodes_in_radius(mo, 1))
    shrunk = tables(s)
    with pytest.raises(hmg._lib.HmgError, match="has been shrunk"):
        s.set_dirichlet_faces(None)
    for got, ref in zip(tables(s), shrunk):
        np.testing.assert_array_equal(got, ref)
    # a partitioned grid
    owner = (np.arange(m.nelements()) % 2).astype(np.int32)
    p = dist.PartitionedGrid(None, hmg.Mesh(m.nodes, m.elements + 1), 2, owner, 0, 2)
    part = p.table_i32("dmask").copy()
    with pytest.raises(hmg._lib.HmgError, match="partitioned grid"):
        p.set_dirichlet_faces(mid)
    np.testing.assert_array_equal(p.table_i32("dmask"), part)
    np.testing.assert_array_equal(p.dirichlet_faces(), one_based(default_faces(m.elements)))   # (the whole mesh's default set)


def test_level1_matrix_follows_the_set(oracle):
    """hmg_coarse_setup after the call assembles (lambda M + K)[free, free] for the set's free nodes."""
    O = oracle
    dim, n = 2, 4
    m = O.hypercube(dim, n)
    rng = np.random.default_rng(3)
    sig = rng.choice([1.0, 9.0], size=(m.nelements(), dim))
    faces = sets_of(m, n)["two sides"]
    g = host_grid(m)
    g.set_operator(sig, 0.0)
    g.set_dirichlet_faces(one_based(faces))
    g.coarse_setup()
    free = g.table_i32("interior_nodes")
    import scipy.sparse as sp
    A = sp.csr_matrix((g.table_f64("coarse_val"), g.table_i32("coarse_colidx"), g.table_i32("coarse_rowptr")), shape=(free.size,) * 2)
    want = O.assemble_checkerboard(m, sig, 0.0).tocsr()[free][:, free]
    assert abs(A - want).max() <= 1e-13 * abs(want).max()
