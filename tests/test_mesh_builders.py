"""CPU checks of the irregular mesh builders (frontistr_amd/mesh.py: PieMesh, renumber) that the GPU assembly tests
(test_gpu_assembly_meshes.py) run on: the oracle assembles them into symmetric matrices with a positive diagonal for all three
C3D8 formulations, the library's profile equals the oracle's, and the host colouring lands on the paths it is meant to reach
(48 colours, exactly 64, a failed colouring, one element per colour)."""
import ctypes as C

import numpy as np
import pytest

from frontistr_amd.mesh import CubeMesh, PieMesh, color_elements, renumber

# name -> (builder, colours of the host's greedy colouring; None: it fails and the assembly scatters with atomics)
BUILDERS = {
    "pie24x2x2": (lambda: PieMesh(24, 2, 2), 48),
    "pie32x1x2": (lambda: PieMesh(32, 1, 2), 64),
    "pie33x1x2": (lambda: PieMesh(33, 1, 2), None),
    "pie8x1x1": (lambda: PieMesh(8, 1, 1), 8),
    "pie7x3x1": (lambda: PieMesh(7, 3, 1), 7),
    "wedge1": (lambda: PieMesh(8, 1, 1, sectors=1), 1),
    "pie72x2x3": (lambda: PieMesh(72, 2, 3), None),
    "cube9_renum": (lambda: renumber(CubeMesh(9, skew=0.1), 11), None),
    "pie24x2x2_renum": (lambda: renumber(PieMesh(24, 2, 2), 12), None),
}


def collapsed(conn):
    return np.array([np.unique(e).size < 8 for e in conn])


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_builder_assembles_and_profiles_like_the_oracle(oracle, name):
    from frontistr_amd import hecmw
    build, ncolor = BUILDERS[name]
    m = build()
    assert m.coord.shape == (m.n_node, 3) and m.conn.shape == (m.n_elem, 8) and m.conn.dtype == np.int32
    assert m.conn.min() == 1 and m.conn.max() == m.n_node and np.unique(m.conn).size == m.n_node
    for eo in (1, 2, 3):
        A = oracle.assemble(eo, m.coord, m.conn, 210000.0, 0.3)
        M = dense(A)
        scale = np.abs(M).max()
        assert np.abs(M - M.T).max() <= 1e-12 * scale, eo
        assert np.all(np.diag(M) > 0.0), eo
    hm = hecmw.hecmwST_local_mesh(n_node=m.n_node)
    hm.elem_node_item = m.conn.ravel()
    mat = hecmw.hecmw_mat_con(hm, hecmw.hecmwST_matrix())
    iL, jL, iU, jU = oracle.mat_con(m.n_node, m.conn)
    assert np.array_equal(mat.indexL, iL) and np.array_equal(mat.itemL, jL)
    assert np.array_equal(mat.indexU, iU) and np.array_equal(mat.itemU, jU)
    col = color_elements(m.conn, m.n_node)
    nc = library_colours(m)
    assert nc == (0 if col is None else int(col.max()) + 1)
    if ncolor is not None:
        assert nc == ncolor, nc


def test_pie_facts():
    """What each pie is in the GPU tests for."""
    p = PieMesh(24, 2, 2)
    assert collapsed(p.conn).sum() == p.n_elem // 2                        # the innermost ring of every layer
    for e in p.conn[collapsed(p.conn)]:
        assert e[0] == e[3] and e[4] == e[7] and e[0] in p.axis_nodes and e[4] in p.axis_nodes
    assert np.bincount(color_elements(p.conn, p.n_node)).max() == 12
    e = PieMesh(8, 1, 1)
    assert np.all(np.bincount(color_elements(e.conn, e.n_node)) == 1)
    q = PieMesh(32, 1, 2)
    assert (q.conn == q.axis_nodes[1]).any(axis=1).sum() == 64           # 64 elements around the middle axis node
    w = PieMesh(8, 1, 1, sectors=1)
    assert w.n_elem == 1 and collapsed(w.conn).all()
    big = PieMesh(72, 2, 3)
    iL, jL, iU, jU = _profile(big)
    axis = big.axis_nodes[1] - 1
    assert (iL[axis + 1] - iL[axis]) + (iU[axis + 1] - iU[axis]) + 1 > 160   # wider than FX_BELL_MAXROW: a hub row
    assert PieMesh(7, 3, 1).n_elem % 16 and PieMesh(72, 2, 3).n_elem % 32   # partly filled last workgroups


def test_renumber_is_a_relabelling():
    base = PieMesh(24, 2, 2)
    r = renumber(base, 5)
    assert not np.array_equal(r.conn, base.conn)
    assert np.array_equal(renumber(base, 5).conn, r.conn)                 # deterministic per seed
    old_of_new = np.argsort(r.new_of_old)
    assert np.array_equal(r.coord, base.coord[old_of_new])
    assert np.array_equal(old_of_new[r.conn - 1] + 1, base.conn[r.elem_order])
    node, dof, val = r.dirichlet()
    bn, bd, bv = base.dirichlet()
    assert np.array_equal(old_of_new[node - 1] + 1, bn) and np.array_equal(dof, bd) and np.array_equal(val, bv)
    ld = r.load().reshape(-1, 3)
    assert np.array_equal(ld[r.new_of_old - 1], base.load().reshape(-1, 3))
    assert np.array_equal(old_of_new[r.axis_nodes - 1] + 1, base.axis_nodes)


def _profile(m):
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle.mat_con(m.n_node, m.conn)


def library_colours(m):
    from frontistr_amd import hecmw
    conn = np.ascontiguousarray(m.conn, dtype=np.int32)
    order = np.zeros(conn.shape[0], dtype=np.int32)
    off = np.zeros(65, dtype=np.int32)
    nc = C.c_int32(0)
    assert hecmw.lib().fx_color_elements(m.n_node, conn.shape[0], 8, hecmw._ptr(conn), hecmw._ptr(order), hecmw._ptr(off),
                                         C.byref(nc)) == 0
    return nc.value


def dense(A):
    NP = A.D.size // 9
    M = np.zeros((3 * NP, 3 * NP))
    D, AL, AU = A.D.reshape(-1, 3, 3), A.AL.reshape(-1, 3, 3), A.AU.reshape(-1, 3, 3)
    for i in range(NP):
        M[3 * i:3 * i + 3, 3 * i:3 * i + 3] = D[i]
        for j in range(A.indexL[i], A.indexL[i + 1]):
            k = A.itemL[j] - 1
            M[3 * i:3 * i + 3, 3 * k:3 * k + 3] = AL[j]
        for j in range(A.indexU[i], A.indexU[i + 1]):
            k = A.itemU[j] - 1
            M[3 * i:3 * i + 3, 3 * k:3 * k + 3] = AU[j]
    return M
