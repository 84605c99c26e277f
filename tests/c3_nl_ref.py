"""Numpy restatement of the reference's nonlinear wedges and 20-node hexahedron (TYPE=351, 352, 362): STF_C3
(fistr1/src/lib/static_LIB_3d.f90:47-205) with `u` present and UPDATE_C3 (:516-837) without temperatures, in the INFINITE /
TOTALLAG / UPDATELAG branches, on the shape functions and quadrature of c3_ref.py.  The entry points are tet_nl_ref.py's (stf_c3,
update_c3 with `order=`, Model, random_case, golden_deck, summary); what does not depend on the element type is used from there:
GEOMAT_C3, MatlMatrix with its latch, BL1, `real()` of the UPDATELAG stress increment (see that module's docstring for the latch
and the rounding), and, through oracle.pyoracle, the material point.  The routines also serve 341 / 342 (c3_ref carries their
element data), which is how test_c3_nl_ref.py checks this module against tet_nl_ref.
"""
import numpy as np

import c3_ref as R
import tet_nl_ref as T
from tet_nl_ref import (COMPONENTS, DECK_CONVERG, DECK_STRAIN, DECK_SUBSTEPS, DECK_TABLE, INFINITE, TOTALLAG, UPDATELAG,  # noqa: F401
                        geomat, matl_matrix, mises, real_default)


def _points(etype, ec, order=None):
    """[(gderiv (nn, 3), det)] per quadrature point.  order: the nodes are summed in this order (the summation-order check)."""
    pts, _ = R.QUAD[etype]
    out = []
    for q in range(pts.shape[0]):
        dN = R.shape_deriv(etype, pts[q])
        if order is None:
            det, inv = R.jacobian(ec, dN)
        else:
            J = np.zeros((3, 3))
            for a in order:
                J += np.outer(ec[a], dN[a])
            det, inv = R.jacobian(np.eye(3), J)        # jacobian() forms ec^T dN: with ec = identity that is J itself
        out.append((dN @ inv, det))
    return out


def stf_c3(etype, ec, u, mat, latch, stress, istat, fstat):
    """STF_C3: (3 nn, 3 nn) tangent of one element.  u (nn, 3) = unode + dunode; stress (nq, 6), istat / fstat (nq,)."""
    flag = mat.nlgeom
    w = R.QUAD[etype][1]
    nn = R.NN[etype]
    elem = ec + u if flag == UPDATELAG else ec
    K = np.zeros((3 * nn, 3 * nn))
    for q, (gd, det) in enumerate(_points(etype, elem)):
        D = matl_matrix(mat, latch, stress[q], istat[q], fstat[q])
        if flag == UPDATELAG:
            D = D - geomat(stress[q])
        wg = w[q] * det
        B = R.b_matrix(gd)
        if flag == TOTALLAG:
            B = B + T._bl1(gd, T._gdisp(u, gd))
        K += (B.T @ (D @ B)) * wg
        if flag != INFINITE:
            s = stress[q]
            S = np.array([[s[0], s[3], s[5]], [s[3], s[1], s[4]], [s[5], s[4], s[2]]])
            K += np.kron(gd @ S @ gd.T, np.eye(3)) * wg
    return K


def update_c3(etype, ec, u, ddu, mat, stress_bak, strain_bak, plstrain, istat, fstat, order=None):
    """UPDATE_C3 of one element -> (qf (3 nn), stress, strain, istat, fstat, dstress); dstress (nq, 6) is the (rounded) stress
    increment of the UPDATELAG branch, zeros otherwise."""
    flag = mat.nlgeom
    w = R.QUAD[etype][1]
    nn, nq = R.NN[etype], R.nq(etype)
    elem, total = ec, u + ddu
    if flag == UPDATELAG:
        elem = (0.5 * ddu + u) + ec
        elem1 = (ddu + u) + ec
        total = ddu
    D = R.elastic_matrix(mat.E, mat.nu)
    qf = np.zeros(3 * nn)
    stress, strain = np.zeros((nq, 6)), np.zeros((nq, 6))
    istat, fstat = np.array(istat, dtype=np.int32).copy(), np.array(fstat, dtype=np.float64).copy()
    dsr = np.zeros((nq, 6))
    pts1 = _points(etype, elem1, order) if flag == UPDATELAG else None
    for q, (gd, det) in enumerate(_points(etype, elem, order)):
        g = T._gdisp(total, gd, order)
        de = np.array([g[0, 0], g[1, 1], g[2, 2], g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])
        if flag == INFINITE:
            strain[q] = de
            stress[q] = D @ de
        elif flag == TOTALLAG:
            de[0] += 0.5 * g[:, 0] @ g[:, 0]
            de[1] += 0.5 * g[:, 1] @ g[:, 1]
            de[2] += 0.5 * g[:, 2] @ g[:, 2]
            de[3] += g[:, 0] @ g[:, 1]
            de[4] += g[:, 1] @ g[:, 2]
            de[5] += g[:, 0] @ g[:, 2]
            strain[q] = de
            stress[q] = D @ de
        else:
            rot = 0.5 * (g - g.T)
            strain[q] = strain_bak[q] + de
            dsr[q] = real_default(D @ de)
            sb = stress_bak[q]
            S = np.array([[sb[0], sb[3], sb[5]], [sb[3], sb[1], sb[4]], [sb[5], sb[4], sb[2]]])
            dum = rot @ S - S @ rot
            stress[q] = sb + dsr[q] + np.array([dum[0, 0], dum[1, 1], dum[2, 2], dum[0, 1], dum[1, 2], dum[2, 0]])
        if mat.plastic:
            from oracle import pyoracle as po
            stress[q], istat[q], fstat[q] = po.backward_euler(mat, stress[q], plstrain[q], istat[q], fstat[q])
        B = R.b_matrix(gd)
        if flag == TOTALLAG:
            B = B + T._bl1(gd, g)
        elif flag == UPDATELAG:
            gd1, det = pts1[q]
            B = R.b_matrix(gd1)
        qf += (stress[q] @ B) * (w[q] * det)
    return qf, stress, strain, istat, fstat, dsr


class Model(T.Model):
    """fstr_solid of one mesh of an STF_C3 type (tet_nl_ref.Model with this module's element routines and state shapes)."""

    def __init__(self, etype, coord, conn, mats, elem_mat=None):
        self.etype, self.coord, self.conn = etype, np.asarray(coord, dtype=np.float64), np.asarray(conn)
        self.mats = list(mats) if isinstance(mats, (list, tuple)) else [mats]
        self.elem_mat = np.ones(self.conn.shape[0], dtype=np.int32) if elem_mat is None else np.asarray(elem_mat)
        ne, q, n = self.conn.shape[0], R.nq(etype), self.coord.shape[0]
        self.st = {k: np.zeros((ne, q, 6)) for k in ("stress", "strain", "stress_bak", "strain_bak")}
        self.st.update(plstrain=np.zeros((ne, q)), fstat=np.zeros((ne, q)), istat=np.zeros((ne, q), dtype=np.int32))
        self.unode, self.dunode, self.qforce = np.zeros(3 * n), np.zeros(3 * n), np.zeros(3 * n)
        self.latch = 0

    def element_tangents(self):
        u = (self.unode + self.dunode).reshape(-1, 3)
        s = self.st
        return np.array([stf_c3(self.etype, self.coord[nd], u[nd], self.mat(e), self.latch, s["stress"][e], s["istat"][e], s["fstat"][e])
                         for e, nd in enumerate(self.conn - 1)])

    def element_update(self, order=None):
        u, du = self.unode.reshape(-1, 3), self.dunode.reshape(-1, 3)
        s = self.st
        qf = np.zeros((self.conn.shape[0], 3 * R.NN[self.etype]))
        self.dstress = np.zeros_like(s["stress"])
        for e, nd in enumerate(self.conn - 1):
            qf[e], s["stress"][e], s["strain"][e], s["istat"][e], s["fstat"][e], self.dstress[e] = update_c3(
                self.etype, self.coord[nd], u[nd], du[nd], self.mat(e), s["stress_bak"][e], s["strain_bak"][e], s["plstrain"][e],
                s["istat"][e], s["fstat"][e], order)
        if any(m.plastic for m in self.mats):
            self.latch = 1
        return qf


def random_case(etype, mat, mesh, seed, amp=2.0e-3, history=True):
    """tet_nl_ref.random_case with this module's points per element."""
    rng = np.random.default_rng(seed)
    x = mesh.coord
    L = max(np.ptp(x, axis=0).max(), 1.0)
    G1, G2 = rng.uniform(-1, 1, (3, 3)) * amp, rng.uniform(-1, 1, (3, 3)) * amp
    unode = (x @ G1.T + 0.3 * amp * np.sin(2.0 * x / L) * L).ravel()
    dunode = (x @ G2.T + 0.3 * amp * np.cos(1.5 * x[:, ::-1] / L) * L).ravel()
    ne, q = mesh.n_elem, R.nq(etype)
    st = {k: np.zeros((ne, q, 6)) for k in ("stress", "strain", "stress_bak", "strain_bak")}
    st.update(plstrain=np.zeros((ne, q)), fstat=np.zeros((ne, q)), istat=np.zeros((ne, q), dtype=np.int32))
    if history:
        D = R.elastic_matrix(mat.E, mat.nu)
        st["strain_bak"] = rng.uniform(-1, 1, (ne, q, 6)) * amp
        st["stress_bak"] = st["strain_bak"] @ D.T
        st["stress"] = st["stress_bak"] * (1.0 + 0.05 * rng.uniform(-1, 1, (ne, q, 1)))
        st["strain"] = st["strain_bak"].copy()
        if mat.plastic:
            st["plstrain"] = rng.uniform(0.0, 2.0e-3, (ne, q))
            st["fstat"] = st["plstrain"].copy()
            st["istat"] = (rng.uniform(size=(ne, q)) < 0.5).astype(np.int32)
    return unode, dunode, st


# ---- the reference's own runs: tests/golden/nl_c3_decks.npz (make_nl_c3_golden.py) -------------------------------------------------
# name -> (etype, cube size n, MAT1 of scripts/fistr1_cube_deck.py --nl-material, two sections); 3 sub-steps, CONVERG = 1e-3
# (two sections need two elements: the single 362 cell becomes the 2^3 cube there)
GOLDEN_DECKS = {"c%d_%s%s" % (et, mat, "_two" if two else ""): (et, 2 if two and et == 362 else n, mat, two)
                for et, n in ((351, 2), (352, 1), (362, 1))
                for mat, two in (("elastic_tl", False), ("elastic_ul", False), ("bilinear", False), ("multilinear", True))}


def golden_deck(name):
    """(mesh, materials, elem_mat or None, bc) of one recorded deck, as fistr1_cube_deck.py writes it (tet_nl_ref.golden_deck on
    solid_mesh(n, etype))."""
    from frontistr_amd.mesh import solid_mesh
    from oracle.refrun import Material
    et, n, mat, two = GOLDEN_DECKS[name]
    m = solid_mesh(n, et)
    mat1 = {"elastic_tl": Material(206900.0, 0.29, nlgeom=TOTALLAG), "elastic_ul": Material(206900.0, 0.29, nlgeom=UPDATELAG),
            "bilinear": Material(206900.0, 0.29, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=UPDATELAG),
            "multilinear": Material(206900.0, 0.29, plastic=True, harden=1, table=DECK_TABLE, nlgeom=UPDATELAG)}[mat]
    mats, em = mat1, None
    if two:
        mats = [mat1, Material(70000.0, 0.33, nlgeom=TOTALLAG)]
        em = np.where(np.arange(m.n_elem) < m.n_elem // 2, 1, 2).astype(np.int32)
    node, dof, val = m.dirichlet()
    t = m.top_nodes
    bc = (np.concatenate([node, t, t]).astype(np.int32),
          np.concatenate([dof, np.full(t.size, 3), np.full(t.size, 1)]).astype(np.int32),
          np.concatenate([val, np.full(t.size, DECK_STRAIN * n), np.full(t.size, 0.2 * DECK_STRAIN * n)]))
    return m, mats, em, bc


# quadrature points (0-based) whose values NodalStress_INV3 extrapolates to the vertices, with the shape functions of the
# linear element of the same shape (fstr_NodalStress.f90:81-104): the two end triangles of 352, the eight corners of 362
_CORNER_POINTS = {352: (0, 1, 2, 6, 7, 8), 362: (0, 2, 6, 8, 18, 20, 24, 26)}
_EDGES = {352: R.PRISM15_EDGES, 362: R.HEX20_EDGES}


def _linear_shape(etype, lc):
    """ShapeFunc_prism6n / ShapeFunc_hex8n at lc"""
    if etype == 352:
        return R.shape_func(351, lc)
    return np.array([0.125 * (1 + sx * lc[0]) * (1 + sy * lc[1]) * (1 + sz * lc[2]) for sx, sy, sz in R.HEX_VERTS])


def nodal_and_element_values(etype, conn, n_node, strain, stress):
    """fstr_NodalStress3D (fstr_NodalStress.f90:15-272) from the quadrature-point strain / stress ((n_elem, nq, 6) each) ->
    (nodal strain, nodal stress, element strain, element stress).  Element values: the mean over the points (ElementStress_C3).
    Nodal values, 351: every node gets that mean (NodalStress_C3); 352 / 362: the vertices get the values of the corner points
    extrapolated with the inverse of the linear shape functions there, the mid-edge nodes the mean of their edge's vertices
    (NodalStress_INV3); then the mean over the elements that hold the node."""
    if etype in (341, 342):
        return T.nodal_and_element_values(etype, conn, n_node, strain, stress)
    est, ess = strain.mean(axis=1), stress.mean(axis=1)
    nn = R.NN[etype]
    if etype == 351:
        nde, nds = np.repeat(est[:, None, :], nn, axis=1), np.repeat(ess[:, None, :], nn, axis=1)
    else:
        sel = list(_CORNER_POINTS[etype])
        func = np.array([_linear_shape(etype, R.QUAD[etype][0][q]) for q in sel])      # func(i, j): shape function j at point i
        inv = np.linalg.inv(func)

        def spread(v):
            vert = np.einsum("ij,ejk->eik", inv, v[:, sel])
            mid = np.stack([0.5 * (vert[:, a] + vert[:, b]) for a, b in _EDGES[etype]], axis=1)
            return np.concatenate([vert, mid], axis=1)
        nde, nds = spread(strain), spread(stress)
    cnt = np.zeros(n_node)
    ns, nt = np.zeros((n_node, 6)), np.zeros((n_node, 6))
    idx = (np.asarray(conn) - 1).ravel()
    np.add.at(cnt, idx, 1.0)
    np.add.at(ns, idx, nde.reshape(-1, 6))
    np.add.at(nt, idx, nds.reshape(-1, 6))
    held = cnt > 0
    ns[held] /= cnt[held, None]
    nt[held] /= cnt[held, None]
    return ns, nt, est, ess


def summary(etype, conn, unode, strain, stress):
    """tet_nl_ref.summary for the five types: the Global summaries of 0.log with the five digits the program prints."""
    U = np.asarray(unode).reshape(-1, 3)
    ns, nt, est, ess = nodal_and_element_values(etype, conn, U.shape[0], np.asarray(strain), np.asarray(stress))
    ext = lambda v: (float("%.4E" % v.max()), float("%.4E" % v.min()))      # as 0.log prints them (1PE11.4)
    node = {"U%d" % (c + 1): ext(U[:, c]) for c in range(3)}
    elem = {}
    for k, c in enumerate(COMPONENTS):
        node["E" + c], node["S" + c] = ext(ns[:, k]), ext(nt[:, k])
        elem["E" + c], elem["S" + c] = ext(est[:, k]), ext(ess[:, k])
    node["SMS"], elem["SMS"] = ext(mises(nt)), ext(mises(ess))
    return {"Node": node, "Element": elem}
