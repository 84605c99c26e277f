"""CPU checks of the wedge / 20-node hexahedron restatement (tests/c3_ref.py) and of the WedgeMesh / Hex20Mesh builders the
device tests use.

c3_ref restates STF_C3 / UPDATE_C3 at TYPE=351 / 352 / 362.  It is pinned to the unmodified reference: fistr1's own assembled K
and right-hand side of small cube decks (tests/golden/c3_decks.npz, make_c3_golden.py), at the 1e-11 of the largest entry
that test_tet_ref.py uses for the same comparison (the dump prints 12 digits).  Beside that, what holds for any correct
linear-elastic element: the shape-function derivatives are the derivatives of the shape functions, which are 1 at their own
node and 0 at the others; a symmetric matrix with the six rigid-body modes in its null space (at 352 / 362 nothing else;
351's two-point rule leaves the reference's element more); exact reproduction of a
linear displacement field; the volume from the quadrature weights.  The builders must give positively oriented conforming
elements in FrontISTR's node order: det J > 0 at every quadrature point, the node counts of the structured cube, every
mid-edge node at the middle of the edge its position in the element names and shared by every element holding that edge."""
import os

import numpy as np
import pytest

import c3_ref as R
from frontistr_amd.mesh import C3_EDGES, C3_NODES, C3_POINTS, Hex20Mesh, WedgeMesh, renumber, solid_mesh

E, NU = 210000.0, 0.3
TYPES = [351, 352, 362]


def distorted(etype, seed):
    """One element: the natural element sheared and stretched, every node moved a little (curved edges at 352 / 362)."""
    rng = np.random.default_rng(seed)
    A = np.eye(3) + 0.15 * rng.standard_normal((3, 3))
    x = R.natural_nodes(etype) @ A.T
    return x + 0.03 * rng.standard_normal(x.shape)


def rigid_modes(ec):
    n = ec.shape[0]
    M = np.zeros((3 * n, 6))
    for d in range(3):
        M[d::3, d] = 1.0
    for k, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
        M[i::3, 3 + k] = -ec[:, j]
        M[j::3, 3 + k] = ec[:, i]
    return M


@pytest.mark.parametrize("etype", TYPES)
def test_tables_and_shape_functions(etype):
    pts, w = R.QUAD[etype]
    assert pts.shape == (C3_POINTS[etype], 3) and R.NN[etype] == C3_NODES[etype]
    vol = 1.0 if etype in (351, 352) else 8.0                  # the natural element's volume (15 printed digits)
    assert abs(w.sum() - vol) <= 1e-14 * vol * 10
    nodes = R.natural_nodes(etype)
    N = np.array([R.shape_func(etype, x) for x in nodes])
    assert np.abs(N - np.eye(R.NN[etype])).max() <= 1e-15
    rng = np.random.default_rng(etype)
    h = 1e-6
    for lc in list(pts) + list(0.3 * rng.random((3, 3))):
        d = R.shape_deriv(etype, lc)
        assert np.abs(d.sum(axis=0)).max() <= 1e-14              # partition of unity
        for j in range(3):
            e = np.zeros(3); e[j] = h
            fd = (R.shape_func(etype, lc + e) - R.shape_func(etype, lc - e)) / (2 * h)
            assert np.abs(fd - d[:, j]).max() <= 1e-9


@pytest.mark.parametrize("etype", TYPES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_element_stiffness_is_symmetric_with_rigid_null_space(etype, seed):
    ec = distorted(etype, seed)
    assert (R.element_dets(etype, ec) > 0).all()
    K = R.element_stiffness(etype, ec, E, NU)
    scale = np.abs(K).max()
    assert np.abs(K - K.T).max() <= 1e-14 * scale
    assert np.abs(K @ rigid_modes(ec)).max() <= 1e-11 * scale
    ev = np.linalg.eigvalsh(K) / scale
    assert (np.abs(ev[:6]) < 1e-12).all()
    # 352 / 362: exactly six zero modes.  351's two-point rule (gauss3d7: the triangle's centroid at two heights) gives the
    # matrix rank 12 at most and leaves the reference's element further zero-energy modes; only the count 6 + is checked there
    assert ev[6] > 1e-7 if etype != 351 else (ev > -1e-12).all()


@pytest.mark.parametrize("etype", TYPES)
def test_patch_linear_field(etype):
    """u = A x + c: constant strain sym(A) and stress at every quadrature point of a distorted mesh."""
    m = solid_mesh(2, etype, skew=0.1, **({"curve": 0.04} if etype != 351 else {}))
    rng = np.random.default_rng(3)
    A = 1e-3 * rng.standard_normal((3, 3))
    u = (m.coord @ A.T + 1e-3).ravel()
    strain, stress, _ = R.update(etype, m.coord, m.conn, E, NU, u)
    eps = np.array([A[0, 0], A[1, 1], A[2, 2], A[0, 1] + A[1, 0], A[1, 2] + A[2, 1], A[2, 0] + A[0, 2]])
    assert strain.shape == (m.n_elem, C3_POINTS[etype], 6)
    assert np.abs(strain - eps).max() <= 1e-12 * np.abs(eps).max()
    assert np.abs(stress - R.elastic_matrix(E, NU) @ eps).max() <= 1e-9 * np.abs(stress).max()


@pytest.mark.parametrize("etype", TYPES)
def test_volume_from_quadrature(etype):
    m = solid_mesh(2, etype)
    w = R.QUAD[etype][1]
    vol = sum((R.element_dets(etype, m.coord[c - 1]) * w).sum() for c in m.conn)
    assert abs(vol - 8.0) <= 1e-12 * 8.0 * 1e2


@pytest.mark.parametrize("etype,n", [(351, 1), (351, 3), (352, 1), (352, 3), (362, 1), (362, 3)])
def test_builders_conforming_positive(etype, n):
    kw = {"skew": 0.1 if n > 1 else 0.0}
    if etype != 351:
        kw["curve"] = 0.04 if n > 1 else 0.0
    m = solid_mesh(n, etype, **kw)
    nn = C3_NODES[etype]
    per_cell = 1 if etype == 362 else 2
    assert m.conn.shape == (per_cell * n ** 3, nn) and m.conn.min() >= 1 and m.conn.max() == m.n_node
    v, edges_axis, edges_diag = (n + 1) ** 3, 3 * n * (n + 1) ** 2, n * n * (n + 1)
    expect = {351: v, 352: v + edges_axis + edges_diag, 362: v + edges_axis}[etype]
    assert m.n_node == expect
    dets = np.array([R.element_dets(etype, m.coord[c - 1]) for c in m.conn])
    assert (dets > 0).all()
    assert all(len(set(c)) == nn for c in m.conn.tolist())
    if etype in C3_EDGES:   # FrontISTR's edge order: one mid-edge node per edge, whoever holds it, at the edge's middle when straight
        straight = solid_mesh(n, etype, skew=kw["skew"])
        nv = nn - len(C3_EDGES[etype])
        mid = {}
        for c in straight.conn.tolist():
            for k, (a, b) in enumerate(C3_EDGES[etype]):
                key = tuple(sorted((c[a], c[b])))
                assert mid.setdefault(key, c[nv + k]) == c[nv + k]
                x = straight.coord[[c[a] - 1, c[b] - 1]].mean(axis=0)
                assert np.abs(straight.coord[c[nv + k] - 1] - x).max() <= 1e-14 * n
        assert len(set(mid.values())) == len(mid) == m.n_node - v
        assert np.array_equal(straight.conn, m.conn)


def test_builders_share_the_cube_and_its_boundary_sets():
    w, h = WedgeMesh(2, etype=352), Hex20Mesh(2)
    assert h.bottom_nodes.size == 9 + 12 and h.top_nodes.size == 21        # 3 x 3 vertices + 12 face edges
    assert w.bottom_nodes.size == 9 + 12 + 4                                   # + one diagonal per cell
    node, dof, val = h.dirichlet()
    assert node.size == 63 and set(dof.tolist()) == {1, 2, 3} and not val.any()
    assert h.load().sum() == 21.0
    r = renumber(h, 4)
    assert (np.array([R.element_dets(362, r.coord[c - 1]) for c in r.conn]) > 0).all()
    with pytest.raises(ValueError):
        WedgeMesh(1, etype=342)
    with pytest.raises(ValueError):
        solid_mesh(1, 361)


def test_tet_types_pass_through():
    """c3_ref serves 341 / 342 with tet_ref's element data."""
    import tet_ref as T
    from frontistr_amd.mesh import TetMesh
    m = TetMesh(1, etype=342)
    assert np.array_equal(R.global_matrix(342, m.coord, m.conn, E, NU), T.global_matrix(342, m.coord, m.conn, E, NU))


@pytest.mark.parametrize("deck", R.GOLDEN_DECKS, ids=[d[0] for d in R.GOLDEN_DECKS])
def test_restatement_reproduces_the_reference_dump(deck):
    """The unmodified fistr1's assembled K after the boundary conditions and its right-hand side (DUMPTYPE=BSR, printed with 12
    digits: e20.12e3) for 351 / 352 / 362 cube decks with one and two sections: the restatement within 1e-11 of the largest
    entry (test_tet_ref.py's bound for the same comparison)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3_decks.npz"))
    m, sec, Kd, Bd = R.golden_deck(g, *deck)
    assert Kd.shape[0] == m.ndof
    K, f = R.assemble(deck[1], m.coord, m.conn, E, NU, bc=m.dirichlet(), load=m.load(), sections=sec)
    assert np.abs(K - Kd).max() <= 1e-11 * np.abs(Kd).max()
    assert np.abs(f - Bd).max() <= 1e-11 * max(np.abs(Bd).max(), 1.0)
