"""Numpy restatement of the reference's linear tetrahedra (TYPE=341, 342) for the device-assembly tests.

STF_C3 (fistr1/src/lib/static_LIB_3d.f90:47-205) and UPDATE_C3 (:516-837) with etype 341 / 342, small strain, isotropic
ELASTIC (calElasticMatrix, ElasticLinear.f90:43-55):
- shape-function derivatives ShapeDeriv_tet4n (tet4n.f90) and ShapeDeriv_tet10n (tet10n.f90); node order: the vertices
  (origin, xi, eta, zeta), then the mid-edge nodes of (1,2), (2,3), (3,1), (1,4), (2,4), (3,4);
- quadrature gauss3d4 / weight3d4 (341, one point) and gauss3d5 / weight3d5 (342, four points) of quadrature.f90, with the
  weights as the reference prints them (0.166666666666667, 0.041666666666667);
- getJacobian / getGlobalDeriv (element.f90:693-818): J = X^T dN, the explicit cofactor inverse, gderiv = dN J^-1.

`assemble` adds the element matrices of a mesh in element order (hecmw_mat_ass_elem) and eliminates Dirichlet dofs as
hecmw_mat_ass_bc does (right-hand side of the free rows first, then zero rows / columns and a unit diagonal); the result is
laid out in the block profile of a matrix built by hecmw_mat_con.
"""
import numpy as np

A5, B5 = 0.138196601125011, 0.585410196624968
QUAD = {
    341: (np.array([[0.25, 0.25, 0.25]]), np.array([0.166666666666667])),
    342: (np.array([[A5, A5, A5], [B5, A5, A5], [A5, B5, A5], [A5, A5, B5]]), np.full(4, 0.041666666666667)),
}
NN = {341: 4, 342: 10}
# mid-edge node k (0-based 4..9) sits between these two vertices (0-based)
TET10_EDGES = ((0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3))


def nq(etype):
    return QUAD[etype][0].shape[0]


def shape_deriv(etype, lc):
    """(nn, 3) derivatives of the shape functions with respect to the volume coordinates."""
    if etype == 341:
        return np.array([[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    xi, et, ze = lc
    a = 1.0 - xi - et - ze
    d = np.zeros((10, 3))
    d[0] = 1.0 - 4.0 * a
    d[1, 0] = 4.0 * xi - 1.0
    d[2, 1] = 4.0 * et - 1.0
    d[3, 2] = 4.0 * ze - 1.0
    d[4] = [4.0 * (1.0 - 2.0 * xi - et - ze), -4.0 * xi, -4.0 * xi]
    d[5] = [4.0 * et, 4.0 * xi, 0.0]
    d[6] = [-4.0 * et, 4.0 * (1.0 - xi - 2.0 * et - ze), -4.0 * et]
    d[7] = [-4.0 * ze, -4.0 * ze, 4.0 * (1.0 - xi - et - 2.0 * ze)]
    d[8] = [4.0 * ze, 0.0, 4.0 * xi]
    d[9] = [0.0, 4.0 * ze, 4.0 * et]
    return d


def jacobian(ec, dN):
    """det and inverse of J = ec^T dN with the reference's expressions (element.f90:798-817)."""
    J = ec.T @ dN
    det = (J[0, 0] * J[1, 1] * J[2, 2] + J[1, 0] * J[2, 1] * J[0, 2] + J[2, 0] * J[0, 1] * J[1, 2]
           - J[2, 0] * J[1, 1] * J[0, 2] - J[1, 0] * J[0, 1] * J[2, 2] - J[0, 0] * J[2, 1] * J[1, 2])
    dum = 1.0 / det
    inv = np.array([
        [J[1, 1] * J[2, 2] - J[2, 1] * J[1, 2], -J[0, 1] * J[2, 2] + J[2, 1] * J[0, 2], J[0, 1] * J[1, 2] - J[1, 1] * J[0, 2]],
        [-J[1, 0] * J[2, 2] + J[2, 0] * J[1, 2], J[0, 0] * J[2, 2] - J[2, 0] * J[0, 2], -J[0, 0] * J[1, 2] + J[1, 0] * J[0, 2]],
        [J[1, 0] * J[2, 1] - J[2, 0] * J[1, 1], -J[0, 0] * J[2, 1] + J[2, 0] * J[0, 1], J[0, 0] * J[1, 1] - J[1, 0] * J[0, 1]]]) * dum
    return det, inv


def elastic_matrix(E, nu):
    D11 = E * (1.0 - nu) / (1.0 - 2.0 * nu) / (1.0 + nu)
    D12 = E * nu / (1.0 - 2.0 * nu) / (1.0 + nu)
    D44 = E / (1.0 + nu) * 0.5
    D = np.zeros((6, 6))
    D[:3, :3] = D12
    D[[0, 1, 2], [0, 1, 2]] = D11
    D[[3, 4, 5], [3, 4, 5]] = D44
    return D


def b_matrix(gd):
    """(6, 3 nn) strain-displacement matrix, rows xx yy zz xy yz zx (static_LIB_3d.f90:126-136)."""
    nn = gd.shape[0]
    B = np.zeros((6, 3 * nn))
    B[0, 0::3] = gd[:, 0]
    B[1, 1::3] = gd[:, 1]
    B[2, 2::3] = gd[:, 2]
    B[3, 0::3] = gd[:, 1]; B[3, 1::3] = gd[:, 0]
    B[4, 1::3] = gd[:, 2]; B[4, 2::3] = gd[:, 1]
    B[5, 0::3] = gd[:, 2]; B[5, 2::3] = gd[:, 0]
    return B


def gauss_points(etype, ec):
    """[(B, wg, det)] per quadrature point; wg = getWeight * det."""
    pts, w = QUAD[etype]
    out = []
    for q in range(pts.shape[0]):
        dN = shape_deriv(etype, pts[q])
        det, inv = jacobian(ec, dN)
        out.append((b_matrix(dN @ inv), w[q] * det, det))
    return out


def element_stiffness(etype, ec, E, nu):
    """STF_C3: (3 nn, 3 nn) element matrix of the element with node coordinates ec (nn, 3)."""
    D = elastic_matrix(E, nu)
    nn = NN[etype]
    K = np.zeros((3 * nn, 3 * nn))
    for B, wg, _ in gauss_points(etype, np.asarray(ec, dtype=np.float64)):
        K += (B.T @ (D @ B)) * wg
    return K


def element_dets(etype, ec):
    return np.array([det for _, _, det in gauss_points(etype, np.asarray(ec, dtype=np.float64))])


def update(etype, coord, conn, E, nu, disp, elem_mat=None):
    """UPDATE_C3, linear: strain = B u, stress = D strain at every quadrature point ((n_elem, nq, 6) each) and the internal
    force qf = sum_g wg B^T stress (3 n_node).  E, nu scalars, or per-material arrays with elem_mat (1-based)."""
    Es, nus = np.atleast_1d(E), np.atleast_1d(nu)
    n_elem = conn.shape[0]
    strain = np.zeros((n_elem, nq(etype), 6))
    stress = np.zeros_like(strain)
    qf = np.zeros(3 * coord.shape[0])
    u = disp.reshape(-1, 3)
    for e in range(n_elem):
        m = 0 if elem_mat is None else elem_mat[e] - 1
        D = elastic_matrix(Es[m], nus[m])
        nodes = conn[e] - 1
        ue = u[nodes].ravel()
        fe = np.zeros(ue.size)
        for g, (B, wg, _) in enumerate(gauss_points(etype, coord[nodes])):
            strain[e, g] = B @ ue
            stress[e, g] = D @ strain[e, g]
            fe += (B.T @ stress[e, g]) * wg
        np.add.at(qf, (3 * nodes[:, None] + np.arange(3)).ravel(), fe)
    return strain, stress, qf


def global_matrix(etype, coord, conn, E, nu, sections=None):
    """Dense global stiffness (3 n_node square), element matrices added in element order."""
    n = coord.shape[0]
    K = np.zeros((3 * n, 3 * n))
    for e in range(conn.shape[0]):
        if sections is None:
            Ee, ne = E, nu
        else:
            m = sections[2][e] - 1
            Ee, ne = sections[0][m], sections[1][m]
        dofs = (3 * (conn[e][:, None] - 1) + np.arange(3)).ravel()
        K[np.ix_(dofs, dofs)] += element_stiffness(etype, coord[conn[e] - 1], Ee, ne)
    return K


def apply_bc(K, f, bc):
    """hecmw_mat_ass_bc: the free rows' right-hand side first, with the original columns; then the prescribed rows and columns
    become zero with a unit diagonal and the prescribed value on the right."""
    K, f = K.copy(), f.copy()
    if bc is None:
        return K, f
    node, dof, val = bc
    idx = 3 * (np.asarray(node) - 1) + np.asarray(dof) - 1
    v = np.zeros(f.size)
    fixed = np.zeros(f.size, dtype=bool)
    v[idx] = val
    fixed[idx] = True
    f[~fixed] -= K[np.ix_(~fixed, fixed)] @ v[fixed]
    K[fixed, :] = 0.0
    K[:, fixed] = 0.0
    K[fixed, fixed] = 1.0
    f[fixed] = v[fixed]
    return K, f


def to_blocks(K, mat):
    """(D, AL, AU) of dense K in the block profile of `mat` (indexL / itemL / indexU / itemU, 1-based items)."""
    NP = mat.NP
    D = np.zeros(9 * NP)
    AL = np.zeros(9 * max(mat.NPL, 1))
    AU = np.zeros(9 * max(mat.NPU, 1))
    for i in range(NP):
        D[9 * i:9 * i + 9] = K[3 * i:3 * i + 3, 3 * i:3 * i + 3].ravel()
        for k in range(mat.indexL[i], mat.indexL[i + 1]):
            j = mat.itemL[k] - 1
            AL[9 * k:9 * k + 9] = K[3 * i:3 * i + 3, 3 * j:3 * j + 3].ravel()
        for k in range(mat.indexU[i], mat.indexU[i + 1]):
            j = mat.itemU[k] - 1
            AU[9 * k:9 * k + 9] = K[3 * i:3 * i + 3, 3 * j:3 * j + 3].ravel()
    return D, AL[:9 * mat.NPL], AU[:9 * mat.NPU]


def profile_blocks(conn, n_node):
    """Set of (row, col) 0-based node pairs with a nonzero block: the profile hecmw_mat_con builds."""
    out = set()
    for nodes in conn - 1:
        for a in nodes:
            for b in nodes:
                out.add((int(a), int(b)))
    return out


def assemble(etype, coord, conn, E, nu, bc=None, load=None, sections=None):
    """Dense K and right-hand side after the boundary conditions."""
    K = global_matrix(etype, coord, conn, E, nu, sections)
    f = np.zeros(3 * coord.shape[0]) if load is None else np.asarray(load, dtype=np.float64).copy()
    return apply_bc(K, f, bc)


# ---- the reference's own assembly: tests/golden/tet_decks.npz (make_tet_golden.py) --------------------------------------
# (name, etype, cube size n, two sections) of each recorded deck: scripts/fistr1_cube_deck.py DIR n --linear --etype ETYPE
GOLDEN_DECKS = (("t341_n2", 341, 2, False), ("t341_n2_two", 341, 2, True), ("t342_n1", 342, 1, False), ("t342_n1_two", 342, 1, True))
DECK_E, DECK_NU = np.array([210000.0, 70000.0]), np.array([0.3, 0.33])     # the decks' MAT1 / MAT2 (!ELASTIC of cube.cnt)


def golden_deck(g, name, etype, n, two):
    """(TetMesh, sections or None, dense K of the dump, its right-hand side) of one recorded deck.  The mesh is TetMesh(n, etype)
    in the library's node order (the deck writer lists 342's mid-edge nodes in the mesh file's order, fistr1 reads them back
    into this one); with two sections the first half of the elements is MAT1, the second MAT2."""
    from frontistr_amd.mesh import TetMesh
    m = TetMesh(n, etype=etype)
    sec = (DECK_E, DECK_NU, np.where(np.arange(m.n_elem) < m.n_elem // 2, 1, 2).astype(np.int32)) if two else None
    iL, jL, iU, jU = (g[name + "/" + k] for k in ("indexL", "itemL", "indexU", "itemU"))
    D, AL, AU = g[name + "/D"], g[name + "/AL"], g[name + "/AU"]
    nr = iL.size - 1
    K = np.zeros((3 * nr, 3 * nr))
    for i in range(nr):
        K[3 * i:3 * i + 3, 3 * i:3 * i + 3] = D[9 * i:9 * i + 9].reshape(3, 3)
        for k in range(iL[i], iL[i + 1]):
            j = jL[k] - 1
            K[3 * i:3 * i + 3, 3 * j:3 * j + 3] = AL[9 * k:9 * k + 9].reshape(3, 3)
        for k in range(iU[i], iU[i + 1]):
            j = jU[k] - 1
            K[3 * i:3 * i + 3, 3 * j:3 * j + 3] = AU[9 * k:9 * k + 9].reshape(3, 3)
    return m, sec, K, g[name + "/B"]


def dense_of(mat):
    """Dense matrix of a hecmwST_matrix's D / AL / AU."""
    n = mat.NP
    K = np.zeros((3 * n, 3 * n))
    for i in range(n):
        K[3 * i:3 * i + 3, 3 * i:3 * i + 3] = mat.D[9 * i:9 * i + 9].reshape(3, 3)
        for k in range(mat.indexL[i], mat.indexL[i + 1]):
            j = mat.itemL[k] - 1
            K[3 * i:3 * i + 3, 3 * j:3 * j + 3] = mat.AL[9 * k:9 * k + 9].reshape(3, 3)
        for k in range(mat.indexU[i], mat.indexU[i + 1]):
            j = mat.itemU[k] - 1
            K[3 * i:3 * i + 3, 3 * j:3 * j + 3] = mat.AU[9 * k:9 * k + 9].reshape(3, 3)
    return K
