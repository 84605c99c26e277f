"""CPU tests of the mixed-mesh work: the MixedMesh builder, and the restatement tests/mixed_ref.py of an assembly over several
element types against the unmodified reference's own matrices (tests/golden/mixed_decks.npz, made by
tests/golden/make_mixed_golden.py with oracle/_ref/fistr1_ref).

Bound: 1e-11 of the largest entry of the matrix, what test_c3_ref.py and test_tet_ref.py hold the single-type restatements to
(the dump prints 12 digits).  The right-hand side is compared for the cube decks (!CLOAD); the two reference decks load a
surface group (!DLOAD, S), whose surface integration the restatement does not have: there the matrix after the boundary
conditions and the prescribed rows of the right-hand side are compared."""
import os
from collections import Counter

import numpy as np
import pytest

import mixed_ref as M
from frontistr_amd.mesh import C3_NODES, MixedMesh, renumber_groups

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mixed_decks.npz")
VERTS = {361: 8, 362: 8, 351: 6, 352: 6, 341: 4, 342: 4}


@pytest.mark.parametrize("deck", M.CUBE_DECKS, ids=[d[0] for d in M.CUBE_DECKS])
def test_restatement_matches_the_reference_on_the_cube_decks(deck):
    g = np.load(GOLDEN)
    name, order, n, two = deck
    m, groups, E, nu = M.cube_deck(order, n, two)
    K, f = M.assemble(m.coord, groups, E, nu, bc=m.dirichlet(), load=m.load())
    Kd, Bd = M.dense_of_dump(g, name), g[name + "/B"]
    scale = np.abs(Kd).max()
    print("%s: |K - K_ref| / max = %.3e, |B - B_ref| = %.3e" % (name, np.abs(K - Kd).max() / scale, np.abs(f - Bd).max()))
    assert K.shape == Kd.shape
    assert np.abs(K - Kd).max() <= 1e-11 * scale
    assert np.abs(f - Bd).max() <= 1e-11 * max(np.abs(Bd).max(), 1.0)


@pytest.mark.parametrize("name", M.REF_DECKS)
def test_restatement_matches_the_reference_on_its_own_decks(name):
    g = np.load(GOLDEN)
    coord, groups, E, nu, bc = M.read_ref_deck(name)
    assert len(groups) == (3 if name == "hexpritet" else 2)
    K, f = M.assemble(coord, groups, E, nu, bc=bc)
    Kd, Bd = M.dense_of_dump(g, name), g[name + "/B"]
    scale = np.abs(Kd).max()
    print("%s: |K - K_ref| / max = %.3e" % (name, np.abs(K - Kd).max() / scale))
    assert np.abs(K - Kd).max() <= 1e-11 * scale
    fixed = 3 * (bc[0] - 1) + bc[1] - 1
    assert np.abs(Bd[fixed] - bc[2]).max() == 0.0


CASES = [(1, 2, 0.0, 0.0), (1, 5, 0.1, 0.0), (2, 2, 0.0, 0.0), (2, 3, 0.1, 0.04), (1, 3, 0.1, 0.0), (2, 4, 0.08, 0.03)]


@pytest.mark.parametrize("order,n,skew,curve", CASES)
def test_mixed_mesh_is_conforming_with_positive_jacobians(order, n, skew, curve):
    m = MixedMesh(n, order=order, skew=skew, curve=curve)
    assert m.etypes == ((361, 351, 341) if order == 1 else (362, 352, 342))
    h = n // 2
    cells = [h * n * h, (n - h) * n * h + h * n * (n - h), (n - h) * n * (n - h)]
    assert [c.shape[0] for c in m.conns] == [cells[0], 2 * cells[1], 6 * cells[2]]
    assert list(m.elem_offsets) == [0, cells[0], cells[0] + 2 * cells[1], cells[0] + 2 * cells[1] + 6 * cells[2]]
    assert m.n_elem == m.elem_offsets[-1] and m.coord.shape == (m.n_node, 3)
    faces = Counter()
    used = np.zeros(m.n_node, dtype=bool)
    for et, conn, elemopt, em in m.groups:
        assert conn.shape[1] == C3_NODES[et] and conn.dtype == np.int32 and elemopt == 1 and em is None
        assert conn.min() >= 1 and conn.max() <= m.n_node
        used[conn.ravel() - 1] = True
        for e in conn:
            assert len(set(e.tolist())) == e.size
            assert (M.element_dets(et, m.coord[e - 1]) > 0).all(), (et, e)
            faces.update(M.faces_of(et, e[:VERTS[et]]))
    assert used.all()
    assert set(faces.values()) <= {1, 2}
    lo, hi = 0.0, float(n)
    for face, count in faces.items():                       # a face held once lies on the cube's surface; every other face twice
        c = m.coord[np.array(face) - 1]
        on_surface = any((np.abs(c[:, d] - lo) < 1e-12).all() or (np.abs(c[:, d] - hi) < 1e-12).all() for d in range(3))
        assert (count == 1) == on_surface, face
    if order == 2:                                          # a mid-edge node is shared by every element that holds its edge
        edge_node = {}
        from frontistr_amd.mesh import C3_EDGES
        for et, conn, _, _ in m.groups:
            nv = VERTS[et]
            for e in conn:
                for k, (a, b) in enumerate(C3_EDGES[et]):
                    key = (min(e[a], e[b]), max(e[a], e[b]))
                    assert edge_node.setdefault(key, e[nv + k]) == e[nv + k]
        assert len(edge_node) == m.n_node - (n + 1) ** 3
    assert m.bottom_nodes.size > 0 and m.top_nodes.size > 0
    assert m.load().shape == (3 * m.n_node,) and m.dirichlet()[0].size == 3 * m.bottom_nodes.size


def test_groups_with_cuts_the_materials_at_the_group_offsets():
    m = MixedMesh(3, order=1)
    em = (1 + np.arange(m.n_elem) % 3).astype(np.int32)
    g = m.groups_with(elemopt=2, elem_mat=em)
    assert [x[2] for x in g] == [2, 2, 2]
    assert np.array_equal(np.concatenate([x[3] for x in g]), em)
    r = renumber_groups(m, 5)
    gr = r.groups_with(elem_mat=em)
    for k in range(3):
        assert np.array_equal(np.sort(r.conns[k], axis=None), np.sort(r.new_of_old[m.conns[k] - 1], axis=None))
        assert np.array_equal(gr[k][3], g[k][3][r.elem_orders[k]])


def test_renumbered_mixed_mesh_gives_the_permuted_matrix():
    m = MixedMesh(2, order=1, skew=0.1)
    r = renumber_groups(m, 3)
    K = M.global_matrix(m.coord, m.groups, 210000.0, 0.3)
    Kr = M.global_matrix(r.coord, r.groups, 210000.0, 0.3)
    p = (3 * (r.new_of_old[:, None] - 1) + np.arange(3)).ravel()      # old dof -> new dof
    assert np.abs(Kr[np.ix_(p, p)] - K).max() <= 1e-12 * np.abs(K).max()


def test_profile_of_groups_is_the_union_of_the_elements():
    from frontistr_amd import hecmw as hip
    m = MixedMesh(3, order=2)
    mat = M.profile(hip, m.n_node, m.groups)
    want = set()
    for _, conn, _, _ in m.groups:
        want |= M.T.profile_blocks(conn, m.n_node)
    got = {(i, i) for i in range(m.n_node)}
    for i in range(m.n_node):
        got |= {(i, int(j) - 1) for j in mat.itemL[mat.indexL[i]:mat.indexL[i + 1]]}
        got |= {(i, int(j) - 1) for j in mat.itemU[mat.indexU[i]:mat.indexU[i + 1]]}
    assert got == want
    assert all(np.all(np.diff(mat.itemL[mat.indexL[i]:mat.indexL[i + 1]]) > 0) for i in range(m.n_node))
