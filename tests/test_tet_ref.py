"""CPU checks of the tetrahedral restatement (tests/tet_ref.py) and of the TetMesh builder the device tests use.

tet_ref restates STF_C3 / UPDATE_C3 at TYPE=341 / 342; what is checked here holds for any correct linear-elastic element:
a symmetric matrix whose null space is exactly the six rigid-body modes, the closed form V B^T D B of the constant-strain
tetrahedron, exact reproduction of a linear displacement field (the patch test: constant strain at every quadrature point,
internal forces in equilibrium), and the element volume from the quadrature weights.  TetMesh must give conforming, positively
oriented elements: every det J > 0, every interior face shared by exactly two elements with opposite orientation, every
mid-edge node shared by all elements holding its edge."""
import itertools

import numpy as np
import pytest

import tet_ref as T
from frontistr_amd.mesh import TetMesh, renumber

E, NU = 210000.0, 0.3


def distorted(etype, seed):
    """One element: a skewed unit tetrahedron, mid-edge nodes (342) moved off their edges."""
    rng = np.random.default_rng(seed)
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) + 0.15 * rng.standard_normal((4, 3))
    if etype == 341:
        return v
    mid = np.array([0.5 * (v[a] + v[b]) for a, b in T.TET10_EDGES]) + 0.03 * rng.standard_normal((6, 3))
    return np.concatenate([v, mid])


def rigid_modes(ec):
    n = ec.shape[0]
    R = np.zeros((3 * n, 6))
    for d in range(3):
        R[d::3, d] = 1.0
    for k, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):  # small rotations: u_i = -x_j, u_j = x_i
        R[i::3, 3 + k] = -ec[:, j]
        R[j::3, 3 + k] = ec[:, i]
    return R


@pytest.mark.parametrize("etype", [341, 342])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_element_stiffness_is_symmetric_with_rigid_null_space(etype, seed):
    ec = distorted(etype, seed)
    assert (T.element_dets(etype, ec) > 0).all()
    K = T.element_stiffness(etype, ec, E, NU)
    scale = np.abs(K).max()
    assert np.abs(K - K.T).max() <= 1e-14 * scale
    assert np.abs(K @ rigid_modes(ec)).max() <= 1e-11 * scale
    ev = np.linalg.eigvalsh(K) / scale
    assert (np.abs(ev[:6]) < 1e-12).all() and ev[6] > 1e-6      # exactly six zero modes


def test_constant_strain_tetrahedron_closed_form():
    ec = distorted(341, 5)
    x = ec - ec[0]
    V = np.linalg.det(x[1:]) / 6.0
    G = np.linalg.inv(np.column_stack([np.ones(4), ec]))[1:].T   # gradients of the barycentric coordinates, (4, 3)
    B = T.b_matrix(G)
    K = V * B.T @ T.elastic_matrix(E, NU) @ B
    # the reference's weight 0.166666666666667 is 1/6 to 15 digits
    assert np.abs(T.element_stiffness(341, ec, E, NU) - K).max() <= 1e-13 * np.abs(K).max()


@pytest.mark.parametrize("etype", [341, 342])
def test_patch_linear_field(etype):
    """u = A x + c: constant strain sym(A) and stress at every quadrature point; the element's internal forces sum to zero."""
    m = TetMesh(2, etype=etype, skew=0.1, curve=0.04)
    rng = np.random.default_rng(3)
    A = 1e-3 * rng.standard_normal((3, 3))
    u = (m.coord @ A.T + 1e-3).ravel()
    strain, stress, qf = T.update(etype, m.coord, m.conn, E, NU, u)
    eps = np.array([A[0, 0], A[1, 1], A[2, 2], A[0, 1] + A[1, 0], A[1, 2] + A[2, 1], A[2, 0] + A[0, 2]])
    assert np.abs(strain - eps).max() <= 1e-12 * np.abs(eps).max()
    assert np.abs(stress - T.elastic_matrix(E, NU) @ eps).max() <= 1e-9 * np.abs(stress).max()
    # interior nodes carry no net force under a constant stress (straight-sided elements: the rule integrates grad N exactly)
    m = TetMesh(2, etype=etype, skew=0.1)
    _, _, qf = T.update(etype, m.coord, m.conn, E, NU, (m.coord @ A.T).ravel())
    interior = np.all((m.coord > 1e-9) & (m.coord < 2 - 1e-9), axis=1)
    assert interior.any()
    assert np.abs(qf.reshape(-1, 3)[interior]).max() <= 1e-12 * np.abs(qf).max()


@pytest.mark.parametrize("etype", [341, 342])
def test_volume_from_quadrature(etype):
    m = TetMesh(3, etype=etype, skew=0.12)
    w = T.QUAD[etype][1]
    vol = sum((T.element_dets(etype, m.coord[c - 1]) * w).sum() for c in m.conn)
    assert abs(vol - 27.0) <= 1e-12 * 27.0 * 1e2


@pytest.mark.parametrize("etype,n", [(341, 1), (341, 3), (342, 1), (342, 3)])
def test_tetmesh_conforming_positive(etype, n):
    m = TetMesh(n, etype=etype, skew=0.1 if n > 1 else 0.0, curve=0.04 if n > 1 else 0.0)
    nn = T.NN[etype]
    assert m.conn.shape == (6 * n ** 3, nn) and m.conn.min() >= 1 and m.conn.max() == m.n_node
    assert m.n_node == ((n + 1) ** 3 if etype == 341 else (2 * n + 1) ** 3)
    dets = np.array([T.element_dets(etype, m.coord[c - 1]) for c in m.conn])
    assert (dets > 0).all()
    assert all(len(set(c)) == nn for c in m.conn.tolist())
    # faces: oriented so that the fourth vertex lies on the positive side; interior faces twice, once each way round
    faces = {}
    for c in m.conn[:, :4].tolist():
        for f in ((0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)):    # outward normals of a positive tetrahedron
            key = tuple(sorted(c[i] for i in f))
            faces.setdefault(key, []).append(tuple(c[i] for i in f))
    for key, fs in faces.items():
        assert len(fs) in (1, 2)
        if len(fs) == 2:   # opposite orientations: the two cyclic orders differ
            a, b = fs
            rot = [a[k:] + a[:k] for k in range(3)]
            assert b not in rot
        else:
            x = m.coord[np.array(key) - 1]
            on_boundary = np.any(np.all(np.isclose(x, 0.0), axis=0) | np.all(np.isclose(x, float(n)), axis=0))
            assert on_boundary
    if etype == 342:  # one mid-edge node per edge, whoever holds the edge
        mid = {}
        for c in m.conn.tolist():
            for k, (a, b) in enumerate(T.TET10_EDGES):
                key = tuple(sorted((c[a], c[b])))
                assert mid.setdefault(key, c[4 + k]) == c[4 + k]
        assert len(set(mid.values())) == len(mid) == m.n_node - (n + 1) ** 3


def test_tetmesh_boundary_sets_and_renumber():
    m = TetMesh(2, etype=342)
    assert m.bottom_nodes.size == 25 and m.top_nodes.size == 25
    node, dof, val = m.dirichlet()
    assert node.size == 75 and set(dof.tolist()) == {1, 2, 3} and not val.any()
    assert m.load().sum() == 25.0
    r = renumber(m, 4)
    dets = np.array([T.element_dets(342, r.coord[c - 1]) for c in r.conn])
    assert (dets > 0).all()


def test_assembly_profile_and_bc():
    """The dense global matrix is symmetric and its blocks lie in the element-pair profile; after the boundary conditions the
    clamped rows are unit rows and the system is positive definite."""
    m = TetMesh(1, etype=342, skew=0.0)
    K = T.global_matrix(342, m.coord, m.conn, E, NU)
    assert np.abs(K - K.T).max() <= 1e-13 * np.abs(K).max()
    prof = T.profile_blocks(m.conn, m.n_node)
    for i, j in itertools.product(range(m.n_node), repeat=2):
        if (i, j) not in prof:
            assert not K[3 * i:3 * i + 3, 3 * j:3 * j + 3].any()
    Kb, f = T.assemble(342, m.coord, m.conn, E, NU, bc=m.dirichlet(), load=m.load())
    fixed = 3 * (m.dirichlet()[0] - 1) + m.dirichlet()[1] - 1
    assert (Kb[fixed][:, fixed] == np.eye(fixed.size)).all()
    assert np.linalg.eigvalsh(Kb).min() > 0
    assert (f[fixed] == 0).all()


@pytest.mark.parametrize("deck", T.GOLDEN_DECKS, ids=[d[0] for d in T.GOLDEN_DECKS])
def test_restatement_reproduces_the_reference_dump(deck):
    """The unmodified fistr1's assembled K after the boundary conditions and its right-hand side (DUMPTYPE=BSR, printed with 12
    digits: e20.12e3) for 341 / 342 cube decks with one and two sections: the restatement within 1e-11 of the largest entry."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tet_decks.npz"))
    m, sec, Kd, Bd = T.golden_deck(g, *deck)
    K, f = T.assemble(deck[1], m.coord, m.conn, E, NU, bc=m.dirichlet(), load=m.load(), sections=sec)
    assert np.abs(K - Kd).max() <= 1e-11 * np.abs(Kd).max()
    assert np.abs(f - Bd).max() <= 1e-11 * max(np.abs(Bd).max(), 1.0)
