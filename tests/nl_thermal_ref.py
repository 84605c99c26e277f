"""Numpy restatement of the thermal branches of the reference's nonlinear update routines and of what goes with them:

    fetch_TableData / GetTableData     fistr1/src/lib/utilities/ttable.f90:282-354       table_lookup (one dependency)
    Update_C3D8Bbar                    fistr1/src/lib/static_LIB_C3D8.f90:203-547        update_c3d8bbar
    UPDATE_C3                          fistr1/src/lib/static_LIB_3d.f90:516-837          update_c3
    Update_C3D8Fbar                    fistr1/src/lib/static_LIB_Fbar.f90:341-769        update_c3d8fbar (INFINITE, TOTALLAG)
    the choice of tt0 per element      fistr1/src/analysis/static/fstr_Update.f90:92-102   elem_tt0
    last_temp = temperature            fstr_Update.f90:308-312, fstr_Cutback.f90:127,:173  Model.commit / snapshot
    TLOAD of every element             fstr_ass_load.f90:287-428                           Model.thermal_load
    STF_* with MatlMatrix(..., tt)     fstr_StiffMatrix.f90:72-73                          stf_* (E, nu of the point's temperature)

The update routines are restated here in full: the existing *_ref modules have no place to subtract EPSTH between the small
strain and the Green-Lagrange terms.  Shape functions, Jacobians, B matrices, the material points (Mises through the C oracle,
Mohr-Coulomb / Drucker-Prager yield_ref, hyperelastic hyper_ref) and the F-bar averages are theirs.

Materials are the objects of those modules with three more attributes, all optional: ``expansion`` (M_EXAPNSION), ``expansion_table``
(MC_THEMOEXP, rows alpha, T) and ``elastic_table`` (MC_ISOELASTIC, rows E, nu, T).
"""
import copy

import numpy as np

import c3_nl_ref as CN
import c3_ref as R
import fbar_ref as FB
import hyper_ref as H
import tet_nl_ref as T
import thermal_ref as TR
import yield_ref as Y
from tet_nl_ref import INFINITE, TOTALLAG, UPDATELAG  # noqa: F401


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def table_lookup(tab, a):
    """fetch_TableData on a table with one dependency: rows (values..., T), T ascending -> the values at a"""
    tab = np.asarray(tab)
    nv = tab.shape[1] - 1
    if tab.shape[0] == 1 or a < tab[0, nv]:
        return tab[0, :nv].copy()
    if a >= tab[-1, nv]:
        return tab[-1, :nv].copy()
    for i in range(tab.shape[0] - 1):
        if tab[i, nv] <= a < tab[i + 1, nv]:
            lam = (a - tab[i, nv]) / (tab[i + 1, nv] - tab[i, nv])
            return (tab.dtype.type(1) - lam) * tab[i, :nv] + lam * tab[i + 1, :nv]
    raise ValueError("table_lookup: the temperatures are not ascending")


# Every routine below works in the dtype of its inputs (float64, or np.longdouble for the conditioning check of
# tests/test_nl_thermal_ref.py): temperatures, tables and constants are taken in the dtype of the temperature handed in.
def _dt(x):
    return np.asarray(x).dtype if np.asarray(x).dtype.kind == "f" else np.dtype(np.float64)


def expansion_at(mat, t):
    """MC_THEMOEXP at t, or M_EXAPNSION where the fetch fails (no table)"""
    dt = _dt(t)
    tab = getattr(mat, "expansion_table", None)
    return dt.type(getattr(mat, "expansion", 0.0)) if tab is None else table_lookup(np.asarray(tab, dtype=dt).reshape(-1, 2), dt.type(t))[0]


def material_at(mat, t):
    """The material MatlMatrix(..., temp) and BackwardEuler(..., temp) see: E, nu of MC_ISOELASTIC at t where there is a table"""
    dt = _dt(t)
    tab = getattr(mat, "elastic_table", None)
    if tab is None:
        return mat
    m = copy.copy(mat)
    m.E, m.nu = table_lookup(np.asarray(tab, dtype=dt).reshape(-1, 3), dt.type(t))
    if dt == np.float64:
        m.E, m.nu = float(m.E), float(m.nu)
    return m


def epsth(mat, ttc, tt0, ref):
    """EPSTH(1:3) = alp (ttc - ref_temp) - alp0 (tt0 - ref_temp)"""
    dt = _dt(ttc)
    e = np.zeros(6, dtype=dt)
    e[:3] = expansion_at(mat, ttc) * (ttc - dt.type(ref)) - expansion_at(mat, dt.type(tt0)) * (dt.type(tt0) - dt.type(ref))
    return e


def _emat(m, dt):
    return R.elastic_matrix(m.E, m.nu) if dt == np.float64 else FB._elastic_matrix(m, dt)


def _bmat(gd):
    """BL0 (c3_ref.b_matrix) in the dtype of gd"""
    if gd.dtype == np.float64:
        return R.b_matrix(gd)
    B = np.zeros((6, 3 * gd.shape[0]), dtype=gd.dtype)
    B[0, 0::3] = gd[:, 0]
    B[1, 1::3] = gd[:, 1]
    B[2, 2::3] = gd[:, 2]
    B[3, 0::3] = gd[:, 1]; B[3, 1::3] = gd[:, 0]
    B[4, 1::3] = gd[:, 2]; B[4, 2::3] = gd[:, 1]
    B[5, 0::3] = gd[:, 2]; B[5, 2::3] = gd[:, 0]
    return B


def _bl1(gd, F):
    """BL1 (tet_nl_ref._bl1) in the dtype of gd"""
    if gd.dtype == np.float64:
        return T._bl1(gd, F)
    B1 = np.zeros((6, 3 * gd.shape[0]), dtype=gd.dtype)
    for c in range(3):
        B1[0, c::3] = F[c, 0] * gd[:, 0]
        B1[1, c::3] = F[c, 1] * gd[:, 1]
        B1[2, c::3] = F[c, 2] * gd[:, 2]
        B1[3, c::3] = F[c, 1] * gd[:, 0] + F[c, 0] * gd[:, 1]
        B1[4, c::3] = F[c, 1] * gd[:, 2] + F[c, 2] * gd[:, 1]
        B1[5, c::3] = F[c, 2] * gd[:, 0] + F[c, 0] * gd[:, 2]
    return B1


def _points(etype, ec):
    """c3_nl_ref._points in the dtype of ec"""
    if ec.dtype == np.float64:
        return CN._points(etype, ec)
    out = []
    for p in R.QUAD[etype][0]:
        dN = np.array(R.shape_deriv(etype, [ec.dtype.type(v) for v in p]), dtype=ec.dtype)
        det, inv = R.jacobian(ec, dN)
        out.append((dN @ inv, det))
    return out


def _hexg(ec, lc):
    return H._hex8_gderiv(ec, lc) if ec.dtype == np.float64 else FB._gderiv(ec, lc)


def _shape(etype, lc, dt):
    return np.array(TR.shape_func(etype, [dt.type(v) for v in lc]), dtype=dt)


def _bbar(gd, bbar):
    """hyper_ref._bbar_matrix in the dtype of gd"""
    B = _bmat(gd)
    h = (bbar - gd) / gd.dtype.type(3)
    for r in range(3):
        for c in range(3):
            B[r, c::3] += h[:, c]
    return B


def mises_backward_euler(mat, stress, plstrain, istat, fstat1):
    """BackwardEuler, Mises (Elastoplastic.f90:351-459, :557) in the dtype of the stress: what the C oracle computes in float64, for
    the conditioning check in np.longdouble.  The routine is point_ref's (all four hardening laws)."""
    import point_ref
    return point_ref.backward_euler(mat, stress, plstrain, istat, fstat1)


class Thermal:
    """ref_temp, the initial condition, last_temp and the temperature of the coming call (n_node each)"""

    def __init__(self, ref_temp, n_node, temp_init=None):
        self.ref_temp = float(ref_temp)
        self.temp_init = np.zeros(n_node) if temp_init is None else np.array(temp_init, dtype=np.float64)
        self.last_temp = self.temp_init.copy()          # fstr_solve_NLGEOM.f90:53-57
        self.temperature = self.temp_init.copy()


def is_elastoplastic(mat):
    return bool(getattr(mat, "plastic", False)) or Y.is_yield(mat)


def elem_tt0(mat, nd, th):
    """tt0 of one element: last_temp for an elastoplastic material, else the initial condition"""
    return th.last_temp[nd] if is_elastoplastic(mat) else th.temp_init[nd]


def _is_hyper(mat):
    return FB._is_hyper(mat)


def _elastic_stress(mat, de):
    return H.stress_update(mat, de) if _is_hyper(mat) else _emat(mat, de.dtype) @ de


def _return_map(mat, stress, plstrain, istat, fstat):
    if not is_elastoplastic(mat):
        return stress, istat, fstat
    if np.asarray(stress).dtype == np.float64:
        return Y.point_update(mat, stress, plstrain, istat, fstat)
    if Y.is_yield(mat):
        return Y.backward_euler(mat, np.asarray(stress), plstrain, istat, fstat)
    return mises_backward_euler(mat, stress, plstrain, istat, fstat)


def _rotate(sb, g):
    rot = g.dtype.type(0.5) * (g - g.T)
    S = np.array([[sb[0], sb[3], sb[5]], [sb[3], sb[1], sb[4]], [sb[5], sb[4], sb[2]]], dtype=g.dtype)
    dum = rot @ S - S @ rot
    return np.array([dum[0, 0], dum[1, 1], dum[2, 2], dum[0, 1], dum[1, 2], dum[2, 0]])


def _small(g):
    return np.array([g[0, 0], g[1, 1], g[2, 2], g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])


# ---- the three update routines -------------------------------------------------------------------------------------------------------
def update_c3(etype, ec, u, ddu, mat, st, tt, t0, ref):
    """UPDATE_C3 with TT, T0 -> qf, stress, strain, istat, fstat.  st: the element's dict of per-point arrays."""
    flag = mat.nlgeom
    dt = np.result_type(ec, u, ddu, tt)
    ec, u, ddu, tt, t0 = (np.asarray(x, dtype=dt) for x in (ec, u, ddu, tt, t0))
    pts, w = R.QUAD[etype]
    w = np.asarray(w, dtype=dt)
    nn, nq = R.NN[etype], R.nq(etype)
    elem, total = ec, u + ddu
    if flag == UPDATELAG:
        elem, elem1, total = (dt.type(0.5) * ddu + u) + ec, (ddu + u) + ec, ddu
    qf, stress, strain = np.zeros(3 * nn, dtype=dt), np.zeros((nq, 6), dtype=dt), np.zeros((nq, 6), dtype=dt)
    istat, fstat = np.array(st["istat"], dtype=np.int32).copy(), np.array(st["fstat"], dtype=dt).copy()
    pts1 = _points(etype, elem1) if flag == UPDATELAG else None
    for q, (gd, det) in enumerate(_points(etype, elem)):
        h = _shape(etype, pts[q], dt)
        ttc, tt0 = h @ tt, h @ t0
        m = material_at(mat, ttc)
        eth = epsth(mat, ttc, tt0, ref)
        g = total.T @ gd
        de = _small(g) - eth                                    # :653
        if flag == TOTALLAG:
            H._green_lagrange(de, g)
        if flag == UPDATELAG:
            strain[q] = st["strain_bak"][q] + de + eth
            stress[q] = st["stress_bak"][q] + T.real_default(_emat(m, dt) @ de) + _rotate(st["stress_bak"][q], g)
        else:
            strain[q] = de + eth
            stress[q] = _elastic_stress(m, de)
        stress[q], istat[q], fstat[q] = _return_map(m, stress[q], st["plstrain"][q], istat[q], fstat[q])
        B = _bmat(gd)
        if flag == TOTALLAG:
            B = B + _bl1(gd, g)
        elif flag == UPDATELAG:
            gd1, det = pts1[q]
            B = _bmat(gd1)
        qf += (stress[q] @ B) * (w[q] * det)
    return qf, stress, strain, istat, fstat


def update_c3d8bbar(ec, u, ddu, mat, st, tt, t0, ref):
    """Update_C3D8Bbar with TT, T0"""
    flag = mat.nlgeom
    dt = np.result_type(ec, u, ddu, tt)
    ec, u, ddu, tt, t0 = (np.asarray(x, dtype=dt) for x in (ec, u, ddu, tt, t0))
    elem, total = ec, u + ddu
    if flag == UPDATELAG:
        elem, elem1, total = (0.5 * ddu + u) + ec, (ddu + u) + ec, ddu
    bbar, _ = _hexg(elem, np.zeros(3))
    dd = total.T @ bbar
    vol0 = (dd[0, 0] + dd[1, 1] + dd[2, 2]) / 3.0
    if flag == UPDATELAG:
        bbar2, _ = _hexg(elem1, np.zeros(3))
    qf, stress, strain = np.zeros(24, dtype=dt), np.zeros((8, 6), dtype=dt), np.zeros((8, 6), dtype=dt)
    istat, fstat = np.array(st["istat"], dtype=np.int32).copy(), np.array(st["fstat"], dtype=dt).copy()
    for q in range(8):
        gd, det = _hexg(elem, H.HEX8_POINTS[q])
        h = _shape(361, H.HEX8_POINTS[q], dt)
        ttc, tt0 = h @ tt, h @ t0
        m = material_at(mat, ttc)
        eth = epsth(mat, ttc, tt0, ref)
        g = total.T @ gd
        dvol = vol0 - (g[0, 0] + g[1, 1] + g[2, 2]) / 3.0
        de = _small(g)
        de[:3] += dvol
        de = de - eth                                           # :359
        if flag == TOTALLAG:
            H._green_lagrange(de, g)
        if flag == UPDATELAG:
            sb = st["stress_bak"][q]
            strain[q] = st["strain_bak"][q] + de + eth
            stress[q] = sb + _emat(m, dt) @ de + _rotate(sb, g) - sb * 3.0 * vol0
        else:
            strain[q] = de + eth
            stress[q] = _elastic_stress(m, de)
        stress[q], istat[q], fstat[q] = _return_map(m, stress[q], st["plstrain"][q], istat[q], fstat[q])
        if flag == UPDATELAG:
            gd1, det = _hexg(elem1, H.HEX8_POINTS[q])
            B = _bbar(gd1, bbar2) if dt != np.float64 else H._bbar_matrix(gd1, bbar2)
        else:
            B = _bbar(gd, bbar) if dt != np.float64 else H._bbar_matrix(gd, bbar)
            if flag == TOTALLAG:
                B = B + _bl1(gd, g)
        qf += (stress[q] @ B) * det
    return qf, stress, strain, istat, fstat


def update_c3d8fbar(ec, u, ddu, mat, st, tt, t0, ref):
    """Update_C3D8Fbar with TT, T0, INFINITE / TOTALLAG: EPSTH leaves the strain before it enters B2 (:565, :720-725)"""
    flag = mat.nlgeom
    if flag == UPDATELAG:
        raise ValueError("Update_C3D8Fbar's UPDATELAG branch is not restated (fbar_ref)")
    dt = np.result_type(ec, u, ddu, tt)
    ec, u, ddu, tt, t0 = (np.asarray(x, dtype=dt) for x in (ec, u, ddu, tt, t0))
    total = u + ddu
    I3 = np.eye(3, dtype=dt)
    _, _, jr, g1ave, _ = FB.averages(ec, total, flag)
    qf, stress, strain = np.zeros(24, dtype=dt), np.zeros((8, 6), dtype=dt), np.zeros((8, 6), dtype=dt)
    istat, fstat = np.array(st["istat"], dtype=np.int32).copy(), np.array(st["fstat"], dtype=dt).copy()
    for q in range(8):
        gd, det = FB._gderiv(ec, H.HEX8_POINTS[q])
        h = _shape(361, H.HEX8_POINTS[q], dt)
        ttc, tt0 = h @ tt, h @ t0
        m = material_at(mat, ttc)
        eth = epsth(mat, ttc, tt0, ref)
        g = total.T @ gd
        if flag == INFINITE:
            dvol = total[:, 0] @ g1ave[:, 0] + total[:, 1] @ g1ave[:, 1] + total[:, 2] @ g1ave[:, 2]
            dvol = (dvol - (g[0, 0] + g[1, 1] + g[2, 2])) / 3.0
            de = _small(g)
            de[:3] += dvol
            de = de - eth
            B = FB._bl_infinite(gd, g1ave)
        else:
            de = FB._fbar_strain(jr[q] * (I3 + g)) - eth
            g1, _ = FB._gderiv(ec + total, H.HEX8_POINTS[q])
            B = jr[q] * jr[q] * (FB._b0(gd) + FB._bl1(gd, g)) + FB._bl2(de, (g1ave - g1) / 3.0)
        strain[q] = de + eth
        stress[q] = _elastic_stress(m, de)
        stress[q], istat[q], fstat[q] = _return_map(m, stress[q], st["plstrain"][q], istat[q], fstat[q])
        qf += (stress[q] @ B) * det
    return qf, stress, strain, istat, fstat


# ---- tangents with MatlMatrix(..., tt) -----------------------------------------------------------------------------------------------
def _point_matrix(mat, latch, strain, stress, istat, fstat):
    D = FB._material_matrix(mat, latch, strain, stress, istat, fstat, np.dtype(np.float64))
    return D - T.geomat(stress) if mat.nlgeom == UPDATELAG else D


def stf_c3(etype, ec, u, mat, latch, st, tt):
    flag = mat.nlgeom
    pts, w = R.QUAD[etype]
    nn = R.NN[etype]
    elem = ec + u if flag == UPDATELAG else ec
    K = np.zeros((3 * nn, 3 * nn))
    for q, (gd, det) in enumerate(CN._points(etype, elem)):
        m = material_at(mat, TR.shape_func(etype, pts[q]) @ tt)
        D = _point_matrix(m, latch, st["strain"][q], st["stress"][q], st["istat"][q], st["fstat"][q])
        B = R.b_matrix(gd)
        if flag == TOTALLAG:
            B = B + T._bl1(gd, u.T @ gd)
        K += (B.T @ (D @ B)) * (w[q] * det)
        if flag != INFINITE:
            K += H._initial_stress(gd, st["stress"][q]) * (w[q] * det)
    return K


def stf_c3d8bbar(ec, u, mat, latch, st, tt):
    flag = mat.nlgeom
    elem = ec + u if flag == UPDATELAG else ec
    bbar, _ = H._hex8_gderiv(elem, np.zeros(3))
    K = np.zeros((24, 24))
    for q in range(8):
        gd, det = H._hex8_gderiv(elem, H.HEX8_POINTS[q])
        m = material_at(mat, TR.shape_func(361, H.HEX8_POINTS[q]) @ tt)
        D = _point_matrix(m, latch, st["strain"][q], st["stress"][q], st["istat"][q], st["fstat"][q])
        B = H._bbar_matrix(gd, bbar)
        if flag == TOTALLAG:
            B = B + T._bl1(gd, u.T @ gd)
        K += (B.T @ (D @ B)) * det
        if flag != INFINITE:
            K += H._initial_stress(gd, st["stress"][q]) * det
    return K


def stf_c3d8fbar(ec, u, mat, latch, st, tt):
    """fbar_ref.stf_c3d8fbar asks for the material matrix once per point, in point order: the material of each point's temperature is
    handed to it in that order"""
    mats = [material_at(mat, TR.shape_func(361, H.HEX8_POINTS[q]) @ tt) for q in range(8)]
    calls = iter(mats)
    orig = FB._material_matrix
    FB._material_matrix = lambda _m, *a: orig(next(calls), *a)
    try:
        return FB.stf_c3d8fbar(ec, u, mat, latch, st["strain"], st["stress"], st["istat"], st["fstat"])
    finally:
        FB._material_matrix = orig


# ---- the thermal load vector -----------------------------------------------------------------------------------------------------------
def tload(etype, ec, mat, tt, t0, ref, strain=None):
    """TLOAD_C3D8Bbar (every 361 element, fstr_ass_load.f90:391-398) / TLOAD_C3: the coefficients and D at the point's
    temperatures; B-bar takes the strain from the centroid's (static_LIB_C3D8.f90:607-608, :688).  strain (nq, 6): the points'
    stored strain, from which MatlMatrix takes the tangent of a hyperelastic material (calMatMatrix.f90:81-86)."""
    pts, w = TR.quad(etype)
    nn = TR.NN[etype]
    vect = np.zeros(3 * nn)
    if etype == 361:
        bbar, _ = TR._gderiv(361, ec, (0.0, 0.0, 0.0))
        h0 = TR.shape_func(361, (0.0, 0.0, 0.0))
        c0, c00 = h0 @ tt, h0 @ t0
    for q in range(pts.shape[0]):
        gd, det = TR._gderiv(etype, ec, pts[q])
        h = TR.shape_func(etype, pts[q])
        tc, tc0 = h @ tt, h @ t0
        m = material_at(mat, tc)
        alp, alp0 = expansion_at(mat, tc), expansion_at(mat, tc0)
        e = np.zeros(6)
        if etype == 361:
            B = TR._bbar_matrix(gd, bbar)
            e[:3] = alp * (c0 - ref) - alp0 * (c00 - ref)
        else:
            B = R.b_matrix(gd)
            e[:3] = alp * (tc - ref) - alp0 * (tc0 - ref)
        D = H.tangent(mat, strain[q]) if _is_hyper(mat) else R.elastic_matrix(m.E, m.nu)
        vect += ((D @ e) @ B) * (w[q] * det)
    return vect


# ---- the model -------------------------------------------------------------------------------------------------------------------------
class Model:
    """fstr_solid of a mesh of element groups [(etype, conn, elemopt)] (elemopt 4: F-bar) with thermal strain: state per group,
    the steps of fstr_Newton on dense matrices.  elem_mats: per group the 1-based material ids (None: material 1)."""

    def __init__(self, coord, groups, mats, thermal, elem_mats=None):
        self.coord = np.asarray(coord, dtype=np.float64)
        self.mats = list(mats) if isinstance(mats, (list, tuple)) else [mats]
        self.th = thermal
        self.parts = []
        for i, g in enumerate(groups):
            etype, conn = int(g[0]), np.asarray(g[1])
            ne, q = conn.shape[0], H.POINTS[etype]
            st = {k: np.zeros((ne, q, 6)) for k in ("stress", "strain", "stress_bak", "strain_bak")}
            st.update(plstrain=np.zeros((ne, q)), fstat=np.zeros((ne, q)), istat=np.zeros((ne, q), dtype=np.int32))
            em = np.ones(ne, dtype=np.int32) if elem_mats is None or elem_mats[i] is None else np.asarray(elem_mats[i])
            self.parts.append(dict(etype=etype, conn=conn, fbar=etype == 361 and len(g) > 2 and g[2] == 4, st=st, emat=em))
        n = self.coord.shape[0]
        self.unode, self.dunode, self.qforce = np.zeros(3 * n), np.zeros(3 * n), np.zeros(3 * n)
        self.latch = 0
        self.saved = None

    def _elem_state(self, p, e):
        return {k: v[e] for k, v in p["st"].items()}

    def widen(self, dt=np.longdouble):
        """The same model with every floating-point input and state array in dt (the conditioning check): nothing is recomputed"""
        self.coord, self.unode, self.dunode, self.qforce = (np.asarray(x, dtype=dt) for x in (self.coord, self.unode, self.dunode, self.qforce))
        for k in ("temp_init", "last_temp", "temperature"):
            setattr(self.th, k, np.asarray(getattr(self.th, k), dtype=dt))
        for p in self.parts:
            p["st"] = {k: (v if k == "istat" else np.asarray(v, dtype=dt)) for k, v in p["st"].items()}
        return self

    def element_update(self):
        """fstr_UpdateNewton's element loop -> per group qf (n_elem, 3 nn)"""
        u, du, th = self.unode.reshape(-1, 3), self.dunode.reshape(-1, 3), self.th
        out = []
        for p in self.parts:
            qf = np.zeros((p["conn"].shape[0], 3 * H.NODES[p["etype"]]), dtype=self.coord.dtype)
            s = p["st"]
            for e, nd in enumerate(p["conn"] - 1):
                mat = self.mats[p["emat"][e] - 1]
                a = (self.coord[nd], u[nd], du[nd], mat, self._elem_state(p, e), th.temperature[nd], elem_tt0(mat, nd, th), th.ref_temp)
                if p["etype"] != 361:
                    r = update_c3(p["etype"], *a)
                else:
                    r = update_c3d8fbar(*a) if p["fbar"] else update_c3d8bbar(*a)
                qf[e], s["stress"][e], s["strain"][e], s["istat"][e], s["fstat"][e] = r
            out.append(qf)
        if any(is_elastoplastic(m) for m in self.mats):
            self.latch = 1
        return out

    def element_tangents(self):
        u = (self.unode + self.dunode).reshape(-1, 3)
        out = []
        for p in self.parts:
            ks = []
            for e, nd in enumerate(p["conn"] - 1):
                a = (self.coord[nd], u[nd], self.mats[p["emat"][e] - 1], self.latch, self._elem_state(p, e), self.th.temperature[nd])
                if p["etype"] != 361:
                    ks.append(stf_c3(p["etype"], *a))
                else:
                    ks.append(stf_c3d8fbar(*a) if p["fbar"] else stf_c3d8bbar(*a))
            out.append(np.array(ks))
        return out

    def _scatter(self, per_group):
        v = np.zeros_like(self.unode)
        for p, qf in zip(self.parts, per_group):
            for e, nd in enumerate(p["conn"] - 1):
                np.add.at(v, (3 * nd[:, None] + np.arange(3)).ravel(), qf[e])
        return v

    def update(self):
        self.qforce = self._scatter(self.element_update())
        return self.qforce

    def stiffness(self):
        n = self.coord.shape[0]
        K = np.zeros((3 * n, 3 * n))
        for p, ke in zip(self.parts, self.element_tangents()):
            for e, nd in enumerate(p["conn"] - 1):
                dofs = (3 * nd[:, None] + np.arange(3)).ravel()
                np.add.at(K, (dofs[:, None], dofs[None, :]), ke[e])
        return K

    hyper_load = True       # False: what libfistr_hip adds -- no load from a hyperelastic element

    def thermal_load(self):
        """fstr_ass_load.f90:287-428 on node + unode, TEMP0 = last_temp for every element"""
        x = self.coord + self.unode.reshape(-1, 3)
        th = self.th
        per = []
        for p in self.parts:
            per.append(np.array([np.zeros(3 * H.NODES[p["etype"]]) if _is_hyper(self.mats[p["emat"][e] - 1]) and not self.hyper_load else
                                 tload(p["etype"], x[nd], self.mats[p["emat"][e] - 1], th.temperature[nd], th.last_temp[nd], th.ref_temp,
                                       p["st"]["strain"][e])
                                 for e, nd in enumerate(p["conn"] - 1)]))
        return self._scatter(per)

    def commit(self):
        """fstr_UpdateState, with last_temp = temperature"""
        self.unode += self.dunode
        self.dunode[:] = 0.0
        for p in self.parts:
            s = p["st"]
            s["stress_bak"][:] = s["stress"]
            s["strain_bak"][:] = s["strain"]
            for e in range(p["conn"].shape[0]):
                if is_elastoplastic(self.mats[p["emat"][e] - 1]):
                    s["plstrain"][e] = s["fstat"][e]
        self.th.last_temp = self.th.temperature.copy()

    def snapshot(self, load):
        """fstr_cutback_save / _load: the point history and last_temp"""
        if not load:
            self.saved = ([{k: v.copy() for k, v in p["st"].items()} for p in self.parts], self.th.last_temp.copy())
            return
        for p, s in zip(self.parts, self.saved[0]):
            for k, v in s.items():
                p["st"][k][:] = v
        self.th.last_temp = self.saved[1].copy()

    def newton_substep(self, f0, f1, bc, cload, max_iter, converg, temperature):
        """One sub-step of fstr_Newton with a dense direct solve; the first right-hand side carries the thermal load.
        -> (converged, Newton iterations)"""
        self.th.temperature = np.array(temperature, dtype=np.float64)
        n3 = self.unode.size
        node, dof, val = bc
        idx = 3 * (np.asarray(node) - 1) + np.asarray(dof) - 1
        fixed = np.zeros(n3, dtype=bool)
        fixed[idx] = True
        GL = np.zeros(n3) if cload is None else np.asarray(cload) * f1
        self.dunode[:] = 0.0
        rhs = GL - self.qforce + self.thermal_load()
        for it in range(1, max_iter + 1):
            inc = np.asarray(val, dtype=np.float64) * (f1 - f0) if it == 1 else np.zeros(len(idx))
            K, b = R.apply_bc(self.stiffness(), rhs, (node, dof, inc))
            x = np.linalg.solve(K, b)
            self.dunode += x
            self.update()
            rhs = GL - self.qforce
            rhs[fixed] = 0.0
            res, xn = np.sqrt(rhs @ rhs), np.sqrt(x @ x)
            qn = np.sqrt(self.qforce @ self.qforce)
            if qn < 1.0e-8:
                qn = 1.0
            dun = xn if it == 1 else np.sqrt(self.dunode @ self.dunode)
            if res / qn < converg or xn / dun < converg:
                self.commit()
                return True, it
        return False, max_iter

    def solve_nlgeom(self, bc, cload, substeps, max_iter, converg, temperature):
        """fstr_solve_NLGEOM's sub-step loop; the temperature is ramped from temp_bak, the temperature at the start of the step
        (fstr_solve_NLGEOM.f90:92, fstr_ass_load.f90:291-300)"""
        bak = self.th.temperature.copy()
        self.th.last_temp = self.th.temperature.copy()      # fstr_UpdateState at the start of the step (fstr_solve_NLGEOM.f90:96)
        its = []
        for sub in range(1, substeps + 1):
            f0, f1 = (sub - 1) / substeps, sub / substeps
            ok, it = self.newton_substep(f0, f1, bc, cload, max_iter, converg, bak + (np.asarray(temperature) - bak) * f1)
            its.append(it)
        return its


# ---- the inputs of the GPU comparisons (tests/test_gpu_nl_thermal.py; tests/test_nl_thermal_ref.py checks their margins on the CPU) ----
FAMILIES = ("361", "361f", "341", "342", "351", "352", "362")      # type and formulation: 361 B-bar, 361 F-bar, the STF_C3 types
E0, NU0, ALPHA0 = 206900.0, 0.29, 1.2e-5
REF_TEMP = 20.0
ELASTIC_TAB = np.array([[210000.0, 0.28, 0.0], [200000.0, 0.30, 100.0], [150000.0, 0.33, 300.0]])     # !ELASTIC, DEPENDENCIES=1
ALPHA_TAB = np.array([[1.0e-5, 0.0], [1.3e-5, 100.0], [1.8e-5, 300.0]])                               # !EXPANSION_COEFF, DEPENDENCIES=1
AMP = 2.0e-3            # relative size of the displacement fields (the amplitude of the Mises comparisons of the other families)


def family_type(fam):
    return int(fam[:3])


def mises_flag(fam):
    """The NLGEOM flag of the Mises material of a family's cases: UPDATELAG where the family restates it in double precision (361
    B-bar); TOTALLAG at F-bar, which serves no UPDATELAG, and at the STF_C3 types, whose UPDATELAG branch rounds the stress
    increment to single precision (static_LIB_3d.f90:718) and is compared at that precision by their own tests, not at 1e-11."""
    return UPDATELAG if fam == "361" else TOTALLAG


DRUCKER_C, DRUCKER_PHI, DRUCKER_H = 150.0, 20.0, 2000.0      # cohesion, friction angle [degrees], hardening of the Drucker-Prager material
MOHR_C, MOHR_PHI, MOHR_H = 250.0, 5.0, 20000.0               # the Mohr-Coulomb material (angle and hardening of the cube decks; the cohesion: the first of 100 .. 300 at which the margins of test_nl_thermal_ref.py hold in every family, with points on both sides of the yield surface)
HYPER_E, HYPER_NU = 2.5, 0.3                                 # the ELASTIC partner of the hyperelastic material (the hyperelastic decks' second section)


# The cohesion of the Drucker-Prager material in the thermal cases of tests/nl_shapes.py where DRUCKER_C leaves a point within 10 tol
# of the yield edge (case id -> c): the first of 160, 140, 170, 130, ... at which test_nl_thermal_ref.check_plastic_points holds on
# the case's mesh, deal and temperatures (search_shape_cohesion).  Every other case keeps DRUCKER_C: 32 .. 71 % of its points yield.
SHAPE_COHESION = {"362_th_solo_dp_ul": 160.0, "362_th_mix_dp": 160.0}


def search_shape_cohesion(case, check, cs=(160, 140, 170, 130, 180, 120, 190, 110, 200)):
    """case: nl_shapes.ThermalCase; check: test_nl_thermal_ref.check_plastic_points"""
    for c in cs:
        case.cohesion = float(c)
        try:
            check(case.build())
            return float(c)
        except AssertionError:
            pass
        finally:
            case.cohesion = None
    raise RuntimeError("no cohesion found")


def material(kind, fam, tables=False, flag=None, c=None):
    """flag: the NLGEOM flag where the kind leaves a choice (default: TOTALLAG for ELASTIC, mises_flag for the elastoplastic ones);
    c: another cohesion (drucker, mohr) or yield stress (mises) than the module's"""
    from oracle.refrun import Material
    if kind == "elastic":
        m = Material(E0, NU0, nlgeom=TOTALLAG if flag is None else flag)
    elif kind == "soft":
        m = Material(HYPER_E, HYPER_NU, nlgeom=TOTALLAG)
    elif kind == "mises":
        m = Material(E0, NU0, plastic=True, harden=0, plconst=(450.0 if c is None else c, 2000.0, 0.0), nlgeom=mises_flag(fam) if flag is None else flag)
    elif kind == "drucker":
        m = Y.drucker_prager(E0, NU0, DRUCKER_C if c is None else c, DRUCKER_PHI, DRUCKER_H, nlgeom=mises_flag(fam) if flag is None else flag)
    elif kind == "mohr":
        m = Y.mohr_coulomb(E0, NU0, MOHR_C if c is None else c, MOHR_PHI, MOHR_H, nlgeom=mises_flag(fam) if flag is None else flag)
    elif kind == "hyper":
        m = H.mooney_rivlin(0.1486, 0.4849, 0.0789)
    else:
        raise ValueError(kind)
    m.expansion = ALPHA0 if kind in ("elastic", "soft") else 1.1e-5
    if tables:
        m.expansion_table = ALPHA_TAB
        if kind != "hyper":
            m.elastic_table = ELASTIC_TAB if kind != "soft" else ELASTIC_TAB * np.array([HYPER_E / E0, 1.0, 1.0])
    return m


def update_elems_per_workgroup(fam):
    """Elements per workgroup of the family's nonlinear update kernel, read from the kernels' own constants: FXN_BLOCK / 8 lanes
    at 361 (B-bar and F-bar: k_nl_update, k_nl_update_fbar), C3El<ET>::BS / ULPE at the STF_C3 types (k_nl_update_tet, k_nl_update_c3)"""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "frontistr_amd", "csrc")
    et = family_type(fam)
    if et == 361:
        return int(re.search(r"#define FXN_BLOCK (\d+)", open(os.path.join(src, "fx_nonlinear.h")).read()).group(1)) // 8
    text = open(os.path.join(src, "fx_c3_element.h")).read()
    bs = int(re.search(r"static constexpr int BS = (\d+);", text).group(1))
    ulpe = {int(a): int(e) for a, e in re.findall(r"\{(\d+), \d+, \d+, \d+, (\d+)\}", text)}
    return bs // ulpe[et]


def family_mesh(fam, size):
    """size "one": one distorted element; "cube": the smallest skewed cube whose elements fill more than one workgroup of the
    family's update kernel without being a multiple of its elements per workgroup (update_elems_per_workgroup); "small": the
    2^3 skewed cube."""
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    et = family_type(fam)
    n = {"one": 1, "small": 2}.get(size)
    if n is None:
        per_cell, epb = {361: 1, 341: 6, 342: 6, 351: 2, 352: 2, 362: 1}[et], update_elems_per_workgroup(fam)
        n = next(k for k in range(2, 20) if per_cell * k ** 3 > epb and (per_cell * k ** 3) % epb != 0)
    kw = {"curve": 0.03} if et in (342, 352, 362) else {}
    m = CubeMesh(n, skew=0.15) if et == 361 else solid_mesh(n, et, skew=0.15, **kw)
    if size == "one":
        m.conn = np.ascontiguousarray(m.conn[:1])
        m.n_elem = 1
    return m


def node_temperatures(coord, lo, hi, seed):
    """A different temperature at every node between lo and hi: a gradient plus noise"""
    rng = np.random.default_rng(seed)
    x = np.asarray(coord)
    s = (x - x.min(0)) @ np.array([0.5, 0.3, 0.2]) / max(np.ptp(x, axis=0).max(), 1.0)
    return lo + (hi - lo) * np.clip(s + 0.15 * rng.uniform(-1, 1, x.shape[0]), 0.0, 1.0)


def gpu_case(fam, variant, mesh=None, mats=None, elem_mat=None):
    """mesh, mats, elem_mat: another mesh of the family with these materials dealt over it (the temperatures of the `tables` variant).
    -> dict(mesh, groups, mats, elem_mats, ref_temp, temp_init, last_temp, temperature, unode, dunode).  Variants:
    one / cube: ELASTIC total Lagrange, constants; two: ELASTIC and Mises in one group with last_temp, temp_init and ref_temp all
    different; tables: both materials with both tables, node temperatures from below the first row to above the last; yield: the
    same with a Drucker-Prager material (E(T), nu(T) inside its return mapping); mohr: the same with Mohr-Coulomb; hyper: a Mooney-Rivlin material (tt0 is the initial
    condition, the stored strain is dstrain + EPSTH) beside a soft ELASTIC one, tables; infinite: both materials INFINITE;
    updatelag: ELASTIC and Mises both UPDATELAG (at the STF_C3 types the branch that rounds to single precision)."""
    et = family_type(fam)
    m = family_mesh(fam, {"one": "one", "cube": "cube"}.get(variant, "small")) if mesh is None else mesh
    two = variant not in ("one", "cube")
    tab = variant in ("tables", "yield", "mohr", "hyper")
    if mats is not None:
        lo, hi = -60.0, 380.0
        unode, dunode = H.random_displacement(m.coord, 17, AMP)
        return dict(mesh=m, groups=[(et, m.conn, 4 if fam == "361f" else 2, elem_mat)], mats=list(mats), elem_mats=[elem_mat], ref_temp=REF_TEMP,
                    temp_init=node_temperatures(m.coord, 15.0, 35.0, 3), last_temp=node_temperatures(m.coord, lo, 0.5 * (lo + hi), 5),
                    temperature=node_temperatures(m.coord, lo, hi, 7), unode=unode, dunode=dunode)
    mats = {"two": ("elastic", "mises"), "tables": ("elastic", "mises"), "yield": ("elastic", "drucker"), "mohr": ("elastic", "mohr"),
            "hyper": ("soft", "hyper"),
            "infinite": ("elastic", "mises"), "updatelag": ("elastic", "mises")}.get(variant, ("elastic",))
    flag = {"infinite": INFINITE, "updatelag": UPDATELAG}.get(variant)
    mats = [material(k, fam, tab, flag) for k in mats]
    em = (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32) if two else None
    lo, hi = (-60.0, 380.0) if tab else (10.0, 90.0)
    unode, dunode = H.random_displacement(m.coord, 17, AMP)
    return dict(mesh=m, groups=[(et, m.conn, 4 if fam == "361f" else 2, em)], mats=mats, elem_mats=[em], ref_temp=REF_TEMP,
                temp_init=node_temperatures(m.coord, 15.0, 35.0, 3), last_temp=node_temperatures(m.coord, lo, 0.5 * (lo + hi), 5),
                temperature=node_temperatures(m.coord, lo, hi, 7), unode=unode, dunode=dunode)


def mixed_case():
    """An F-bar group, a wedge group and a tetrahedral group (MixedMesh, linear) with the two materials over all elements"""
    from frontistr_amd.mesh import MixedMesh
    m = MixedMesh(2, 1, skew=0.1)
    em = (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32)
    groups = [(g[0], g[1], 4 if g[0] == 361 else 2, g[3]) for g in m.groups_with(2, em)]
    mats = [material("elastic", "361f"), material("mises", "361f")]
    unode, dunode = H.random_displacement(m.coord, 17, AMP)
    return dict(mesh=m, groups=groups, mats=mats, elem_mats=[g[3] for g in groups], ref_temp=REF_TEMP,
                temp_init=node_temperatures(m.coord, 15.0, 35.0, 3), last_temp=node_temperatures(m.coord, 10.0, 50.0, 5),
                temperature=node_temperatures(m.coord, 10.0, 90.0, 7), unode=unode, dunode=dunode)


def model_of(case):
    th = Thermal(case["ref_temp"], case["mesh"].n_node, case["temp_init"])
    th.last_temp = case["last_temp"].copy()
    th.temperature = case["temperature"].copy()
    ref = Model(case["mesh"].coord, case["groups"], case["mats"], th, case["elem_mats"])
    ref.unode[:], ref.dunode[:] = case["unode"], case["dunode"]
    return ref



# ---- the reference program's own runs: tests/golden/nl_thermal_decks.npz (tests/golden/make_nl_thermal_golden.py) -----------------------
DECK_ALPHA, DECK_SUBSTEPS, DECK_CONVERG = 1.2e-5, 3, 1.0e-3


def _deck(etype, n, material, strain=0.005, fbar=False, tables=False, temp_init=None, temp_top=120.0, ref_temp=20.0):
    return dict(etype=etype, n=n, material=material, strain=strain, fbar=fbar, tables=tables, temp_init=temp_init, temp_top=temp_top,
                ref_temp=ref_temp)


# Cube decks of scripts/fistr1_cube_deck.py with `!TEMPERATURE` on the top face (every other node keeps the initial condition, or 0):
# every solid type ELASTIC total Lagrange with a constant coefficient; Mises MULTILINEAR updated Lagrange (B-bar) with an initial
# condition different from ref_temp, so that tt0 differs between the elastic and the plastic rule; Mooney-Rivlin on F-bar hexahedra;
# tables at 361 and at 342 with temperatures from below the first row to above the last
THERMAL_DECKS = {
    "t341_elastic": _deck(341, 2, "elastic_tl"), "t342_elastic": _deck(342, 1, "elastic_tl"), "t351_elastic": _deck(351, 2, "elastic_tl"),
    "t352_elastic": _deck(352, 1, "elastic_tl"), "t362_elastic": _deck(362, 1, "elastic_tl"),
    "t361_mises_ic": _deck(361, 2, "multilinear", temp_init=25.0),
    "t361f_mooney": _deck(361, 2, "mooney", strain=0.1, fbar=True, temp_init=25.0),
    "t361_elastic_tab": _deck(361, 2, "elastic_tl", tables=True, temp_top=250.0),
    "t342_elastic_tab": _deck(342, 1, "elastic_tl", tables=True, temp_init=-20.0, temp_top=350.0),
}


def golden_deck(name):
    """-> (Model, bc, target temperature) of one recorded deck as make_nl_thermal_golden.py writes it: z = 0 clamped, the top face
    moved by `strain` in z and a fifth of that in x, the top face's temperature `temp_top` at load factor 1"""
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    from oracle.refrun import Material
    d = THERMAL_DECKS[name]
    et, n = d["etype"], d["n"]
    m = CubeMesh(n) if et == 361 else solid_mesh(n, et)
    mat = {"elastic_tl": lambda: Material(206900.0, 0.29, nlgeom=TOTALLAG),
           "multilinear": lambda: Material(206900.0, 0.29, plastic=True, harden=1, table=T.DECK_TABLE, nlgeom=UPDATELAG),
           "mooney": lambda: H.mooney_rivlin(0.1486, 0.4849, 0.0789)}[d["material"]]()
    mat.expansion = DECK_ALPHA
    if d["tables"]:
        mat.expansion_table, mat.elastic_table = ALPHA_TAB, ELASTIC_TAB
    node, dof, val = m.dirichlet()
    t = m.top_nodes
    bc = (np.concatenate([node, t, t]).astype(np.int32), np.concatenate([dof, np.full(t.size, 3), np.full(t.size, 1)]).astype(np.int32),
          np.concatenate([val, np.full(t.size, d["strain"] * n), np.full(t.size, 0.2 * d["strain"] * n)]))
    # without an initial condition the program's temperature starts at REF_TEMP (fstr_setup.f90:780) while last_temp and the tt0 of a
    # material that is not elastoplastic are 0 (:788, fstr_Update.f90:97); with one, all three are the initial condition
    # (fstr_solve_NLGEOM.f90:51-59).  temp_bak is the temperature at the start of the step (:92).
    init = np.full(m.n_node, 0.0 if d["temp_init"] is None else d["temp_init"])
    th = Thermal(d["ref_temp"], m.n_node, init)
    th.temperature = np.full(m.n_node, d["ref_temp"] if d["temp_init"] is None else d["temp_init"])
    target = th.temperature.copy()
    target[np.asarray(t) - 1] = d["temp_top"]
    model = Model(m.coord, [(et, m.conn, 4 if d["fbar"] else 2, None)], [mat], th)
    return model, bc, target


def deck_summary(model):
    p = model.parts[0]
    return H.summary(p["etype"], p["conn"], model.unode, p["st"]["strain"], p["st"]["stress"])


# ---- the reference's own deck examples/static/thermal_stress/sample1 (tests/golden/decks/thermal_stress1) ----------------------------------
SAMPLE1 = "thermal_stress1"
SAMPLE1_CONVERG = 1.0e-8


def _sample1_dir():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decks", SAMPLE1)


def _cards(path):
    """{card header line: [data lines]} of a mesh or control file, comments dropped, in file order [(header, lines)]"""
    out = []
    for line in open(path):
        s = line.strip()
        if not s or s.startswith("#") or s.startswith("!!"):
            continue
        if s.startswith("!"):
            out.append((s.upper().replace(" ", ""), []))
        elif out:
            out[-1][1].append(s)
    return out


def sample1_deck():
    """-> (Model, bc, temperature) of thermal_stress/sample1 as the program reads it: TYPE=361 (B-bar under NLSTATIC), !ELASTIC and
    !EXPANSION_COEFF with DEPENDENCIES=1, FIX clamped, no !REFTEMP (0) and no initial condition, one sub-step, and
    `!TEMPERATURE, READRESULT=8, SSTEP=1, INTERVAL=1`: with the load factor 1 of the only sub-step read_temperature_result takes the
    eighth result file whole (readtemp.f90:26-55: kt = 7, w = 1).  HEC-MW keeps the nodes in file order; the mesh's 525 nodes and the
    result files' 99 are matched by node id, and the nodes no element names carry no stiffness (kept out of the model here)."""
    import os
    from oracle.refrun import Material
    d = _sample1_dir()
    msh, cnt = _cards(os.path.join(d, "A361.msh")), _cards(os.path.join(d, "A300.cnt"))
    nodes = {}
    for h, lines in msh:
        if h == "!NODE":
            for ln in lines:
                v = ln.split(",")
                nodes[int(v[0])] = [float(x) for x in v[1:4]]
    elems = [[int(x) for x in ln.split(",")][1:] for h, lines in msh if h.startswith("!ELEMENT,TYPE=361") for ln in lines]
    used = sorted({n for e in elems for n in e})
    local = {g: i + 1 for i, g in enumerate(used)}
    coord = np.array([nodes[g] for g in used])
    conn = np.array([[local[n] for n in e] for e in elems], dtype=np.int32)
    fix = []
    for h, lines in msh:
        if h.startswith("!NGROUP,NGRP=FIX"):
            for ln in lines:
                a, b, s = (int(x) for x in ln.split(","))
                fix += [g for g in range(a, b + 1, s) if g in local]
    tab = {h.split(",")[0]: np.array([[float(x.rstrip(".")) if x.strip().endswith(".") else float(x) for x in ln.split(",")] for ln in lines])
           for h, lines in cnt if h.startswith("!ELASTIC") or h.startswith("!EXPANSION_COEFF")}
    mat = Material(float(tab["!ELASTIC"][0, 0]), float(tab["!ELASTIC"][0, 1]), nlgeom=TOTALLAG)
    mat.expansion, mat.expansion_table, mat.elastic_table = 0.0, tab["!EXPANSION_COEFF"], tab["!ELASTIC"]
    tok = open(os.path.join(d, "V361.res.0.8")).read().split()
    k = tok.index("TEMPERATURE") + 1
    temp = np.zeros(len(used))
    seen = 0
    while k + 1 < len(tok) and seen < len(used):
        temp[local[int(tok[k])] - 1] = float(tok[k + 1])
        k, seen = k + 2, seen + 1
    assert seen == len(used)
    fixl = np.array([local[g] for g in fix], dtype=np.int32)
    bc = (np.repeat(fixl, 3), np.tile(np.array([1, 2, 3], dtype=np.int32), fixl.size), np.zeros(3 * fixl.size))
    model = Model(coord, [(361, conn, 2, None)], [mat], Thermal(0.0, len(used), None))
    return model, bc, temp
