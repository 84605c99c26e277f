"""Numpy restatement of the reference's hyperelastic materials in the total-Lagrange static loop.

Material point, fistr1/src/lib/physics/Hyperelastic.f90 with the arrays the reference has (dibdc (3,3,3), d2ibdc2 (3,3,3,3,3):
clarity over speed): cderiv (:14-132), calElasticMooneyRivlin (:221-247), calUpdateElasticMooneyRivlin (:252-286),
calElasticArrudaBoyce (:138-172), calUpdateElasticArrudaBoyce (:176-216); mat_c2d (calMatMatrix.f90:154-197).  The routines work
in the dtype of the strain they are given (float64, or np.longdouble for the sensitivity check).

Elements: MatlMatrix takes the tangent of a hyperelastic point from the point's STORED strain gauss%strain (calMatMatrix.f90:81-86)
-- the Green-Lagrange strain the last stress update left there, zero before the first one -- and the TOTALLAG branches of the
update routines (static_LIB_3d.f90:681-684, static_LIB_C3D8.f90:387-390) store the strain and call StressUpdate, which gives the 2nd
Piola-Kirchhoff stress from that TOTAL strain.  stf_c3 / update_c3 are STF_C3 / UPDATE_C3 for TYPE=341, 342, 351, 352, 362 on the
element data of c3_ref.py and the pieces of tet_nl_ref.py / c3_nl_ref.py; stf_c3d8bbar / update_c3d8bbar are the INFINITE and
TOTALLAG branches of STF_C3D8Bbar (static_LIB_C3D8.f90:23-198) and Update_C3D8Bbar (:203-547) for TYPE=361.  A material that is not
hyperelastic goes through the same routines with the elastic matrix, so that a hyperelastic section can sit beside ELASTIC ones.
"""
from decimal import Decimal

import numpy as np

import c3_nl_ref as CN
import c3_ref as R
import tet_nl_ref as T
from tet_nl_ref import INFINITE, TOTALLAG, UPDATELAG  # noqa: F401

ELASTIC, MISES, MOONEY, ARRUDA = 0, 1, 2, 3       # fx_material_view::plastic, the material kind


class Material:
    """tMaterial of a !HYPERELASTIC card (fstr_ctrl_material.f90:166-255): kind MOONEY (NEOHOOKE is C01 = 0) with plconst = (C10, C01,
    D1), or ARRUDA with (mu, lambda_m, D); nlgeom_flag TOTALLAG.  Carries the attributes the elastic restatements read."""

    def __init__(self, kind, plconst, nlgeom=TOTALLAG):
        self.kind, self.plconst, self.nlgeom = int(kind), tuple(float(v) for v in plconst), int(nlgeom)
        self.E = self.nu = 0.0
        self.plastic, self.harden, self.table = False, 0, np.zeros((0, 2))


def neohooke(C10, D1):
    return Material(MOONEY, (C10, 0.0, D1))


def mooney_rivlin(C10, C01, D1):
    return Material(MOONEY, (C10, C01, D1))


def arruda_boyce(mu, lam, D):
    return Material(ARRUDA, (mu, lam, D))


def kind_of(mat):
    return getattr(mat, "kind", MISES if mat.plastic else ELASTIC)


# ---- Hyperelastic.f90 ---------------------------------------------------------------------------------------------------------------
def cderiv(strain):
    """-> ctn, inv1b, inv2b, inv3b, dibdc (3,3,3), d2ibdc2 (3,3,3,3,3); the last index is the invariant."""
    strain = np.asarray(strain)
    dt = strain.dtype
    one, two, three = dt.type(1), dt.type(2), dt.type(3)
    delta = np.eye(3, dtype=dt)
    ctn = np.zeros((3, 3), dtype=dt)
    ctn[0, 0] = strain[0] * two + one
    ctn[1, 1] = strain[1] * two + one
    ctn[2, 2] = strain[2] * two + one
    ctn[0, 1] = ctn[1, 0] = strain[3]
    ctn[1, 2] = ctn[2, 1] = strain[4]
    ctn[2, 0] = ctn[0, 2] = strain[5]
    inv1 = ctn[0, 0] + ctn[1, 1] + ctn[2, 2]
    inv2 = (ctn[1, 1] * ctn[2, 2] + ctn[0, 0] * ctn[2, 2] + ctn[0, 0] * ctn[1, 1]
            - ctn[1, 2] * ctn[1, 2] - ctn[0, 2] * ctn[0, 2] - ctn[0, 1] * ctn[0, 1])
    inv3 = (ctn[0, 0] * ctn[1, 1] * ctn[2, 2] + ctn[1, 0] * ctn[2, 1] * ctn[0, 2] + ctn[2, 0] * ctn[0, 1] * ctn[1, 2]
            - ctn[2, 0] * ctn[1, 1] * ctn[0, 2] - ctn[1, 0] * ctn[0, 1] * ctn[2, 2] - ctn[0, 0] * ctn[2, 1] * ctn[1, 2])
    inv33 = inv3 ** (-one / three)
    ci = np.zeros((3, 3), dtype=dt)
    ci[0, 0] = (ctn[1, 1] * ctn[2, 2] - ctn[1, 2] * ctn[1, 2]) / inv3
    ci[1, 1] = (ctn[0, 0] * ctn[2, 2] - ctn[0, 2] * ctn[0, 2]) / inv3
    ci[2, 2] = (ctn[0, 0] * ctn[1, 1] - ctn[0, 1] * ctn[0, 1]) / inv3
    ci[0, 1] = ci[1, 0] = (ctn[0, 2] * ctn[1, 2] - ctn[0, 1] * ctn[2, 2]) / inv3
    ci[0, 2] = ci[2, 0] = (ctn[0, 1] * ctn[1, 2] - ctn[1, 1] * ctn[0, 2]) / inv3
    ci[1, 2] = ci[2, 1] = (ctn[0, 1] * ctn[0, 2] - ctn[0, 0] * ctn[1, 2]) / inv3
    didc = np.zeros((3, 3, 3), dtype=dt)
    didc[:, :, 0] = delta
    didc[:, :, 1] = inv1 * delta - ctn
    didc[:, :, 2] = inv3 * ci
    d2idc2 = np.zeros((3, 3, 3, 3, 3), dtype=dt)
    for k in range(3):
        for l in range(3):
            for m in range(3):
                for n in range(3):
                    d2idc2[k, l, m, n, 1] = delta[k, l] * delta[m, n] - (delta[k, m] * delta[l, n] + delta[k, n] * delta[l, m]) / two
                    d2idc2[k, l, m, n, 2] = inv3 * (ci[m, n] * ci[k, l] - (ci[k, m] * ci[n, l] + ci[k, n] * ci[m, l]) / two)
    inv1b = inv1 * inv33
    inv2b = inv2 * inv33 * inv33
    inv3b = np.sqrt(inv3)
    dibdc = np.zeros((3, 3, 3), dtype=dt)
    dibdc[:, :, 0] = -inv33 ** 4 * inv1 * didc[:, :, 2] / three + inv33 * didc[:, :, 0]
    dibdc[:, :, 1] = -two * inv33 ** 5 * inv2 * didc[:, :, 2] / three + inv33 ** 2 * didc[:, :, 1]
    dibdc[:, :, 2] = didc[:, :, 2] / (two * np.sqrt(inv3))
    d2ibdc2 = np.zeros((3, 3, 3, 3, 3), dtype=dt)
    f4, f9, f10, f15 = dt.type(4), dt.type(9), dt.type(10), dt.type(1.5)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                for l in range(3):
                    d2ibdc2[i, j, k, l, 0] = (f4 / f9 * inv33 ** 7 * inv1 * didc[i, j, 2] * didc[k, l, 2]
                                              - inv33 ** 4 / three * (didc[k, l, 0] * didc[i, j, 2] + didc[i, j, 0] * didc[k, l, 2])
                                              - inv33 ** 4 / three * inv1 * d2idc2[i, j, k, l, 2]
                                              + inv33 * d2idc2[i, j, k, l, 0])
                    d2ibdc2[i, j, k, l, 1] = (f10 / f9 * inv33 ** 8 * inv2 * didc[i, j, 2] * didc[k, l, 2]
                                              - two / three * inv33 ** 5 * (didc[k, l, 1] * didc[i, j, 2] + didc[i, j, 1] * didc[k, l, 2])
                                              - two / three * inv33 ** 5 * inv2 * d2idc2[i, j, k, l, 2]
                                              + inv33 ** 2 * d2idc2[i, j, k, l, 1])
                    d2ibdc2[i, j, k, l, 2] = (-didc[i, j, 2] * didc[k, l, 2] / (f4 * inv3 ** f15)
                                              + d2idc2[i, j, k, l, 2] / (two * np.sqrt(inv3)))
    return ctn, inv1b, inv2b, inv3b, dibdc, d2ibdc2


def _consts(plconst, dt):
    return [dt.type(v) for v in plconst]


def cal_elastic_mooney_rivlin(plconst, strain):
    strain = np.asarray(strain)
    dt = strain.dtype
    c = _consts(plconst, dt)
    _, _, _, inv3b, dibdc, d2ibdc2 = cderiv(strain)
    dj2 = np.einsum("kl,mn->klmn", dibdc[:, :, 2], dibdc[:, :, 2])
    cijkl = d2ibdc2[..., 0] * c[0] + d2ibdc2[..., 1] * c[1] + dt.type(2) * (dj2 + (inv3b - dt.type(1)) * d2ibdc2[..., 2]) / c[2]
    return dt.type(4) * cijkl


def cal_update_elastic_mooney_rivlin(plconst, strain):
    strain = np.asarray(strain)
    dt = strain.dtype
    c = _consts(plconst, dt)
    _, _, _, inv3b, dibdc, _ = cderiv(strain)
    two = dt.type(2)
    dudc = dibdc[:, :, 0] * c[0] + dibdc[:, :, 1] * c[1] + two * (inv3b - dt.type(1)) * dibdc[:, :, 2] / c[2]
    return np.array([two * dudc[0, 0], two * dudc[1, 1], two * dudc[2, 2], two * dudc[0, 1], two * dudc[1, 2], two * dudc[0, 2]], dtype=dt)


def _arruda_series(c, inv1b, dt):
    n = dt.type
    coef = c[1]
    first = c[0] * (n(0.5) + inv1b / (n(10) * coef ** 2) + n(33) * inv1b * inv1b / (n(1050) * coef ** 4)
                    + n(76) * inv1b ** 3 / (n(7000) * coef ** 6) + n(2595) * inv1b ** 4 / (n(673750) * coef ** 8))
    second = c[0] * (n(1) / (n(10) * coef ** 2) + n(66) * inv1b / (n(1050) * coef ** 4) + n(228) * inv1b ** 2 / (n(7000) * coef ** 6)
                     + n(10380) * inv1b ** 3 / (n(673750) * coef ** 8))
    return first, second


def cal_elastic_arruda_boyce(plconst, strain):
    strain = np.asarray(strain)
    dt = strain.dtype
    c = _consts(plconst, dt)
    _, inv1b, _, inv3b, dibdc, d2ibdc2 = cderiv(strain)
    first, second = _arruda_series(c, inv1b, dt)
    one = dt.type(1)
    d11 = np.einsum("ij,kl->ijkl", dibdc[:, :, 0], dibdc[:, :, 0])
    d33 = np.einsum("ij,kl->ijkl", dibdc[:, :, 2], dibdc[:, :, 2])
    cijkl = (second * d11 + first * d2ibdc2[..., 0] + (one + one / inv3b ** 2) * d33 / c[2]
             + (inv3b - one / inv3b) * d2ibdc2[..., 2] / c[2])
    return dt.type(4) * cijkl


def cal_update_elastic_arruda_boyce(plconst, strain):
    strain = np.asarray(strain)
    dt = strain.dtype
    c = _consts(plconst, dt)
    _, inv1b, _, inv3b, dibdc, _ = cderiv(strain)
    first, _ = _arruda_series(c, inv1b, dt)
    pk = first * dibdc[:, :, 0] + (inv3b - dt.type(1) / inv3b) * dibdc[:, :, 2] / c[2]
    two = dt.type(2)
    return np.array([two * pk[0, 0], two * pk[1, 1], two * pk[2, 2], pk[0, 1] + pk[1, 0], pk[1, 2] + pk[2, 1], pk[0, 2] + pk[2, 0]], dtype=dt)


_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0))


def mat_c2d(cijkl):
    """rank 4 -> 6 x 6, case D3: dij(I, J) = cijkl(pair I, pair J) with the pairs 11, 22, 33, 12, 23, 31."""
    return np.array([[cijkl[i, j, k, l] for k, l in _PAIRS] for i, j in _PAIRS], dtype=cijkl.dtype)


def tangent(mat, strain):
    """MatlMatrix of a hyperelastic point: 6 x 6 from the stored strain."""
    f = cal_elastic_arruda_boyce if mat.kind == ARRUDA else cal_elastic_mooney_rivlin
    return mat_c2d(f(mat.plconst, strain))


def stress_update(mat, strain):
    """StressUpdate of a hyperelastic point: 2nd Piola-Kirchhoff stress from the total Green-Lagrange strain."""
    f = cal_update_elastic_arruda_boyce if mat.kind == ARRUDA else cal_update_elastic_mooney_rivlin
    return f(mat.plconst, strain)


def energy(mat, strain):
    """Strain-energy functions the two materials derive from (independent of the routines above): Mooney-Rivlin
    C10 (I1b - 3) + C01 (I2b - 3) + (J - 1)^2 / D1; Arruda-Boyce mu sum_i c_i / lm^(2 i - 2) (I1b^i - 3^i) + ((J^2 - 1) / 2 - ln J) / D
    with c = 1/2, 1/20, 11/1050, 19/7000, 519/673750."""
    e = np.asarray(strain)
    Cm = np.array([[2 * e[0] + 1, e[3], e[5]], [e[3], 2 * e[1] + 1, e[4]], [e[5], e[4], 2 * e[2] + 1]])
    i1, i3 = np.trace(Cm), np.linalg.det(Cm)
    i2 = 0.5 * (i1 * i1 - np.trace(Cm @ Cm))
    J = np.sqrt(i3)
    i1b, i2b = i1 * J ** (-2.0 / 3.0), i2 * J ** (-4.0 / 3.0)
    c = mat.plconst
    if mat.kind == ARRUDA:
        co = (0.5, 1.0 / 20.0, 11.0 / 1050.0, 19.0 / 7000.0, 519.0 / 673750.0)
        return (c[0] * sum(a / c[1] ** (2 * k) * (i1b ** (k + 1) - 3.0 ** (k + 1)) for k, a in enumerate(co))
                + ((J * J - 1.0) / 2.0 - np.log(J)) / c[2])
    return c[0] * (i1b - 3.0) + c[1] * (i2b - 3.0) + (J - 1.0) ** 2 / c[2]


# ---- the element routines ------------------------------------------------------------------------------------------------------------
def _material_matrix(mat, strain):
    return tangent(mat, strain) if kind_of(mat) >= MOONEY else R.elastic_matrix(mat.E, mat.nu)


def _green_lagrange(de, g):
    de[0] += 0.5 * g[:, 0] @ g[:, 0]
    de[1] += 0.5 * g[:, 1] @ g[:, 1]
    de[2] += 0.5 * g[:, 2] @ g[:, 2]
    de[3] += g[:, 0] @ g[:, 1]
    de[4] += g[:, 1] @ g[:, 2]
    de[5] += g[:, 0] @ g[:, 2]


def _initial_stress(gd, s):
    S = np.array([[s[0], s[3], s[5]], [s[3], s[1], s[4]], [s[5], s[4], s[2]]])
    return np.kron(gd @ S @ gd.T, np.eye(3))


def stf_c3(etype, ec, u, mat, strain, stress):
    """STF_C3 with flag INFINITE / TOTALLAG: (3 nn, 3 nn).  strain, stress (nq, 6): the points' stored values."""
    w = R.QUAD[etype][1]
    nn = R.NN[etype]
    K = np.zeros((3 * nn, 3 * nn))
    for q, (gd, det) in enumerate(CN._points(etype, ec)):
        D = _material_matrix(mat, strain[q])
        B = R.b_matrix(gd)
        if mat.nlgeom == TOTALLAG:
            B = B + T._bl1(gd, T._gdisp(u, gd))
        K += (B.T @ (D @ B)) * (w[q] * det)
        if mat.nlgeom == TOTALLAG:
            K += _initial_stress(gd, stress[q]) * (w[q] * det)
    return K


def update_c3(etype, ec, total, mat):
    """UPDATE_C3 with flag INFINITE / TOTALLAG -> qf (3 nn), stress (nq, 6), strain (nq, 6).  total = u + ddu."""
    w = R.QUAD[etype][1]
    nn, nq = R.NN[etype], R.nq(etype)
    qf, stress, strain = np.zeros(3 * nn), np.zeros((nq, 6)), np.zeros((nq, 6))
    for q, (gd, det) in enumerate(CN._points(etype, ec)):
        g = T._gdisp(total, gd)
        de = np.array([g[0, 0], g[1, 1], g[2, 2], g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])
        B = R.b_matrix(gd)
        if mat.nlgeom == TOTALLAG:
            _green_lagrange(de, g)
            B = B + T._bl1(gd, g)
        strain[q] = de
        stress[q] = stress_update(mat, de) if kind_of(mat) >= MOONEY else R.elastic_matrix(mat.E, mat.nu) @ de
        qf += (stress[q] @ B) * (w[q] * det)
    return qf, stress, strain


_G2 = 0.577350269189626
HEX8_POINTS = np.array([[sx * _G2, sy * _G2, sz * _G2] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)])   # gauss3d2, weights 1


def hex8_shape_deriv(lc):
    """ShapeDeriv_hex8n (hex8n.f90): (8, 3)"""
    xi, et, ze = lc
    return np.array([[0.125 * sx * (1 + sy * et) * (1 + sz * ze), 0.125 * sy * (1 + sx * xi) * (1 + sz * ze),
                      0.125 * sz * (1 + sx * xi) * (1 + sy * et)] for sx, sy, sz in R.HEX_VERTS])


def _hex8_gderiv(ec, lc):
    dN = hex8_shape_deriv(lc)
    det, inv = R.jacobian(ec, dN)
    return dN @ inv, det


def _bbar_matrix(gd, bbar):
    """BL0 with the dilatational part taken at the centroid (static_LIB_C3D8.f90:103-125)"""
    B = R.b_matrix(gd)
    h = (bbar - gd) / 3.0
    for r in range(3):
        for c in range(3):
            B[r, c::3] += h[:, c]
    return B


def stf_c3d8bbar(ec, u, mat, strain, stress):
    """STF_C3D8Bbar with flag INFINITE / TOTALLAG: (24, 24)"""
    bbar, _ = _hex8_gderiv(ec, np.zeros(3))
    K = np.zeros((24, 24))
    for q in range(8):
        gd, det = _hex8_gderiv(ec, HEX8_POINTS[q])
        D = _material_matrix(mat, strain[q])
        B = _bbar_matrix(gd, bbar)
        if mat.nlgeom == TOTALLAG:
            B = B + T._bl1(gd, u.T @ gd)
        K += (B.T @ (D @ B)) * det
        if mat.nlgeom == TOTALLAG:
            K += _initial_stress(gd, stress[q]) * det
    return K


def update_c3d8bbar(ec, total, mat):
    """Update_C3D8Bbar with flag INFINITE / TOTALLAG -> qf (24), stress (8, 6), strain (8, 6)"""
    bbar, _ = _hex8_gderiv(ec, np.zeros(3))
    dd = total.T @ bbar
    vol0 = (dd[0, 0] + dd[1, 1] + dd[2, 2]) / 3.0
    qf, stress, strain = np.zeros(24), np.zeros((8, 6)), np.zeros((8, 6))
    for q in range(8):
        gd, det = _hex8_gderiv(ec, HEX8_POINTS[q])
        g = total.T @ gd
        dvol = vol0 - (g[0, 0] + g[1, 1] + g[2, 2]) / 3.0
        de = np.array([g[0, 0] + dvol, g[1, 1] + dvol, g[2, 2] + dvol, g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])
        B = _bbar_matrix(gd, bbar)
        if mat.nlgeom == TOTALLAG:
            _green_lagrange(de, g)
            B = B + T._bl1(gd, g)
        strain[q] = de
        stress[q] = stress_update(mat, de) if kind_of(mat) >= MOONEY else R.elastic_matrix(mat.E, mat.nu) @ de
        qf += (stress[q] @ B) * det
    return qf, stress, strain


NODES = {361: 8, **R.NN}
POINTS = {361: 8, 341: 1, 342: 4, 351: 2, 352: 9, 362: 27}


class Model(T.Model):
    """fstr_solid of one mesh of one of the six solid types with hyperelastic and / or ELASTIC (INFINITE, TOTALLAG) materials:
    tet_nl_ref.Model's steps of fstr_Newton (dense solve) on this module's element routines."""

    def __init__(self, etype, coord, conn, mats, elem_mat=None):
        self.etype, self.coord, self.conn = etype, np.asarray(coord, dtype=np.float64), np.asarray(conn)
        self.mats = list(mats) if isinstance(mats, (list, tuple)) else [mats]
        self.elem_mat = np.ones(self.conn.shape[0], dtype=np.int32) if elem_mat is None else np.asarray(elem_mat)
        ne, q, n = self.conn.shape[0], POINTS[etype], self.coord.shape[0]
        self.st = {k: np.zeros((ne, q, 6)) for k in ("stress", "strain", "stress_bak", "strain_bak")}
        self.st.update(plstrain=np.zeros((ne, q)), fstat=np.zeros((ne, q)), istat=np.zeros((ne, q), dtype=np.int32))
        self.unode, self.dunode, self.qforce = np.zeros(3 * n), np.zeros(3 * n), np.zeros(3 * n)
        self.latch = 0

    def element_tangents(self):
        u = (self.unode + self.dunode).reshape(-1, 3)
        s = self.st
        if self.etype == 361:
            return np.array([stf_c3d8bbar(self.coord[nd], u[nd], self.mat(e), s["strain"][e], s["stress"][e])
                             for e, nd in enumerate(self.conn - 1)])
        return np.array([stf_c3(self.etype, self.coord[nd], u[nd], self.mat(e), s["strain"][e], s["stress"][e])
                         for e, nd in enumerate(self.conn - 1)])

    def stiffness(self):
        """fstr_StiffMatrix: dense global tangent.  hecmw_mat_ass_elem adds every (row node, column node) block of the element matrix, so
        the blocks of a node that a collapsed hexahedron names twice add up (a fancy-indexed += would keep only one of them)."""
        n = self.coord.shape[0]
        K = np.zeros((3 * n, 3 * n))
        for e, ke in enumerate(self.element_tangents()):
            dofs = (3 * (self.conn[e][:, None] - 1) + np.arange(3)).ravel()
            np.add.at(K, (dofs[:, None], dofs[None, :]), ke)
        return K

    def element_update(self, order=None):
        total = (self.unode + self.dunode).reshape(-1, 3)
        s = self.st
        qf = np.zeros((self.conn.shape[0], 3 * NODES[self.etype]))
        for e, nd in enumerate(self.conn - 1):
            if self.etype == 361:
                qf[e], s["stress"][e], s["strain"][e] = update_c3d8bbar(self.coord[nd], total[nd], self.mat(e))
            else:
                qf[e], s["stress"][e], s["strain"][e] = update_c3(self.etype, self.coord[nd], total[nd], self.mat(e))
        return qf


# ---- inputs of the comparisons ---------------------------------------------------------------------------------------------------------
# The constants of the reference's own tutorials (tutorial/03_hyperelastic_cylinder, 04_hyperelastic_spring); Neo-Hooke with the first
# and third of the Mooney-Rivlin set
TEST_MATERIALS = {"mooney": lambda: mooney_rivlin(0.1486, 0.4849, 0.0789), "neohooke": lambda: neohooke(0.1486, 0.0789),
                  "arruda": lambda: arruda_boyce(0.71, 1.7029, 0.1408)}


def random_strains(n, amp, seed):
    """n admissible Green-Lagrange strains E = (F^T F - I) / 2 of F = I + amp * uniform(-1, 1): det C > 0 by construction;
    engineering shear components, the reference's order."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 6))
    for k in range(n):
        F = np.eye(3) + amp * rng.uniform(-1, 1, (3, 3))
        E = 0.5 * (F.T @ F - np.eye(3))
        out[k] = [E[0, 0], E[1, 1], E[2, 2], 2 * E[0, 1], 2 * E[1, 2], 2 * E[0, 2]]
    return out


def random_displacement(coord, seed, amp):
    """Smooth displacement fields unode / dunode of relative size amp (tet_nl_ref.random_case's)."""
    rng = np.random.default_rng(seed)
    x = np.asarray(coord)
    L = max(np.ptp(x, axis=0).max(), 1.0)
    G1, G2 = rng.uniform(-1, 1, (3, 3)) * amp, rng.uniform(-1, 1, (3, 3)) * amp
    unode = (x @ G1.T + 0.3 * amp * np.sin(2.0 * x / L) * L).ravel()
    dunode = (x @ G2.T + 0.3 * amp * np.cos(1.5 * x[:, ::-1] / L) * L).ravel()
    return unode, dunode


GPU_AMP = 0.05          # relative size of the displacement fields of the GPU comparisons: strains of a few per cent to 20 %


def gpu_mesh(etype):
    """The distorted small meshes of the GPU comparisons (those of test_gpu_tet_nonlinear.py / test_gpu_c3_nonlinear.py): 2^3 skewed
    cells, curved edges at the quadratic types, the skewed 3^3 cube at 352 / 362 (no multiple of the elements per workgroup); at 361
    the skewed 2^3 cube plus one collapsed hexahedron (a prism that names two nodes twice) on the nodes of the last cell."""
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    if etype == 361:
        m = CubeMesh(2, skew=0.1)
        c = m.conn[-1]
        m.conn = np.ascontiguousarray(np.vstack([m.conn, [[c[0], c[1], c[2], c[2], c[4], c[5], c[6], c[6]]]]).astype(np.int32))
        m.n_elem += 1
        m.etype = 361
        return m
    kw = {"curve": 0.03} if etype in (342, 352, 362) else {}
    m = solid_mesh(3 if etype in (352, 362) else 2, etype, skew=0.1, **kw)
    m.etype = etype
    return m


def gpu_strains(etype, name, seed=17):
    """The strains the GPU comparisons store: (n_elem, nq, 6) after an update at random_displacement(seed, GPU_AMP)."""
    m = gpu_mesh(etype)
    ref = Model(etype, m.coord, m.conn, TEST_MATERIALS[name]())
    ref.unode[:], ref.dunode[:] = random_displacement(m.coord, seed, GPU_AMP)
    ref.element_update()
    return ref.st["strain"]


# ---- the reference program's own runs: tests/golden/hyper_decks.npz (tests/golden/make_hyper_golden.py) ----------------------------------
DECK_STRETCH, DECK_SUBSTEPS, DECK_CONVERG = 0.1, 3, 1.0e-3
_SIZES = {361: 2, 341: 2, 342: 1, 351: 2, 352: 1, 362: 1}
# name -> (etype, cube size n, MAT1 of scripts/fistr1_cube_deck.py --nl-material, two sections)
GOLDEN_DECKS = {"h%d_%s" % (et, mat): (et, n, mat, False) for et, n in _SIZES.items() for mat in ("neohooke", "mooney", "arruda")}
GOLDEN_DECKS.update({"h361_mooney_two": (361, 2, "mooney", True), "h342_arruda_two": (342, 1, "arruda", True),
                     "h352_neohooke_two": (352, 1, "neohooke", True), "h362_mooney_two": (362, 2, "mooney", True)})


def golden_deck(name):
    """(mesh, materials, elem_mat or None, bc) of one recorded cube deck, as fistr1_cube_deck.py writes it: z = 0 clamped, the top face
    moved by 10 % in z and a fifth of that in x; with two sections the second half of the elements is ELASTIC 2.5 / 0.3, total Lagrange."""
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    from oracle.refrun import Material as Elastic
    et, n, mat, two = GOLDEN_DECKS[name]
    m = CubeMesh(n) if et == 361 else solid_mesh(n, et)
    m.etype = et
    mats, em = TEST_MATERIALS[mat](), None
    if two:
        mats = [mats, Elastic(2.5, 0.3, nlgeom=TOTALLAG)]
        em = np.where(np.arange(m.n_elem) < m.n_elem // 2, 1, 2).astype(np.int32)
    node, dof, val = m.dirichlet()
    t = m.top_nodes
    bc = (np.concatenate([node, t, t]).astype(np.int32),
          np.concatenate([dof, np.full(t.size, 3), np.full(t.size, 1)]).astype(np.int32),
          np.concatenate([val, np.full(t.size, DECK_STRETCH * n), np.full(t.size, 0.2 * DECK_STRETCH * n)]))
    return m, mats, em, bc


def summary(etype, conn, unode, strain, stress):
    """The Global summaries of 0.log (c3_nl_ref.summary); at 361 fstr_NodalStress3D takes NodalStress_INV3 with the eight quadrature
    points: the vertices get the point values extrapolated with the inverse of the shape functions at the points."""
    if etype != 361:
        return CN.summary(etype, conn, unode, strain, stress)
    strain, stress = np.asarray(strain), np.asarray(stress)
    U = np.asarray(unode).reshape(-1, 3)
    func = np.array([[0.125 * (1 + sx * p[0]) * (1 + sy * p[1]) * (1 + sz * p[2]) for sx, sy, sz in R.HEX_VERTS] for p in HEX8_POINTS])
    inv = np.linalg.inv(func)
    nde, nds = np.einsum("ij,ejk->eik", inv, strain), np.einsum("ij,ejk->eik", inv, stress)
    est, ess = strain.mean(axis=1), stress.mean(axis=1)
    n_node = U.shape[0]
    cnt, ns, nt = np.zeros(n_node), np.zeros((n_node, 6)), np.zeros((n_node, 6))
    idx = (np.asarray(conn) - 1).ravel()
    np.add.at(cnt, idx, 1.0)
    np.add.at(ns, idx, nde.reshape(-1, 6))
    np.add.at(nt, idx, nds.reshape(-1, 6))
    ns, nt = ns / cnt[:, None], nt / cnt[:, None]
    ext = lambda v: (float("%.4E" % v.max()), float("%.4E" % v.min()))      # as 0.log prints them (1PE11.4)
    node = {"U%d" % (c + 1): ext(U[:, c]) for c in range(3)}
    elem = {}
    for k, c in enumerate(CN.COMPONENTS):
        node["E" + c], node["S" + c] = ext(ns[:, k]), ext(nt[:, k])
        elem["E" + c], elem["S" + c] = ext(est[:, k]), ext(ess[:, k])
    node["SMS"], elem["SMS"] = ext(CN.mises(nt)), ext(CN.mises(ess))
    return {"Node": node, "Element": elem}


def within_1e4(actual, correct):
    """oracle.fistr1_run.compare_step (|delta| <= 1e-4 on every maximum and minimum two logs hold, examples/test_FrontISTR.rb:10) with
    the difference of the printed decimals taken exactly -> list of mismatches.  The float subtraction of two printed numbers that are
    1e-4 apart lands on either side of the bound (6.7575 - 6.7574 = 1.0000000000065512e-4); repr of a float parsed from the five
    digits a log prints is that decimal again.  Why it matters: tests/test_hyper_1elem_ref.py."""
    bad = []
    for part in ("Node", "Element"):
        for k, v in actual[part].items():
            c = correct[part].get(k)
            if c is None:
                continue
            for j, what in ((0, "max"), (1, "min")):
                if not abs(Decimal(repr(float(c[j]))) - Decimal(repr(float(v[j])))) <= Decimal("1e-4"):
                    bad.append((part, k, what, v[j], c[j]))
    return bad
