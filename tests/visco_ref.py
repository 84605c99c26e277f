"""Numpy restatement of the reference's viscoelastic material (mtype VISCOELASTIC, card !VISCOELASTIC) in the static loop.

Material point, fistr1/src/lib/physics/Viscoelastic.f90 as written: hvisc (:16-31, with its series branch below 1e-4),
calViscoelasticMatrix (:91-178), UpdateViscoelastic (:182-277), updateViscoElasticState (:280-300).  The routines work in the dtype
they are given (float64, or np.longdouble for the sensitivity check).

What one would not write first, and where it is:
  * MatlMatrix tests isViscoelastic BEFORE its saved flag (calMatMatrix.f90:51): the latch never changes this tangent, and the
    update routines set isEp only for elastoplastic and NORTON materials (static_LIB_3d.f90:595), so this material never sets it.
  * With dt == 0 the tangent is the elastic matrix (:108-115) and the update routines do not call StressUpdate at all
    (`isViscoelastic(mtype) .AND. tincr /= 0.0D0`, static_LIB_3d.f90:659, :685): stress = matmul(D, dstrain), history untouched.
  * With dt /= 0 the routines first form matmul(D, dstrain) with the VISCOELASTIC D and then overwrite it by StressUpdate.
  * Kg = K - 0.6666666666666666d0 * Gg (:165): sixteen sixes, not 2/3.
  * The shear components of the deviator are HALF the engineering strains (:235-237), also in the stored one (:297-299).
  * UpdateViscoelastic reads the old q of a term in vsig(12 (n-1) + 1..6) and writes the new one to +7..12 (:258): repeated Newton
    iterations from one committed state are idempotent; updateViscoElasticState shifts new -> old and stores the deviator of
    gauss%strain behind the terms, and fstr_UpdateState runs it only under tincr > 0 (fstr_Update.f90:333-337).
  * The INFINITE branches end in `stress = real(stress)` (static_LIB_3d.f90:665, static_LIB_C3D8.f90:371, static_LIB_Fbar.f90:552):
    a rounding to default real, which the TOTALLAG branches do not have.

Elements: the INFINITE / TOTALLAG branches of UPDATE_C3 (static_LIB_3d.f90:655-696), Update_C3D8Bbar (static_LIB_C3D8.f90:361-403) and
Update_C3D8Fbar (static_LIB_Fbar.f90:530-583) and the three tangents, on the element pieces of c3_ref.py, c3_nl_ref.py, tet_nl_ref.py,
hyper_ref.py and fbar_ref.py.  A section that is not viscoelastic goes through hyper_ref's routines (ELASTIC INFINITE / TOTALLAG or
hyperelastic), so a viscoelastic section can sit beside those.

The factors that depend on the material and dt alone (exp_n, dq_n, mu_0, gfac) are formed once per dt by `factors`, in the order of the
routines' loops; the device library forms them the same way on the host (nl_visco_factors) and hands them to the kernels.
"""
import numpy as np

import c3_nl_ref as CN
import c3_ref as R
import fbar_ref as FB
import hyper_ref as H
import tet_nl_ref as T
from tet_nl_ref import INFINITE, TOTALLAG, UPDATELAG  # noqa: F401

VISCOELASTIC = 7        # fx_material_view::plastic


class Material:
    """tMaterial of !ELASTIC E, nu with !VISCOELASTIC rows (g_n, tau_n); nlgeom TOTALLAG, or INFINITE with the card's INFINITE
    parameter (fstr_ctrl_material.f90:277-279)."""

    def __init__(self, E, nu, prony, nlgeom=TOTALLAG):
        self.E, self.nu, self.nlgeom = float(E), float(nu), int(nlgeom)
        self.prony = np.ascontiguousarray(prony, dtype=np.float64).reshape(-1, 2)
        self.kind = VISCOELASTIC
        self.plastic, self.harden, self.plconst, self.table = False, 0, (0.0, 0.0, 0.0), self.prony

    @property
    def width(self):
        return 12 * self.prony.shape[0] + 6


def is_visco(mat):
    return getattr(mat, "kind", 0) == VISCOELASTIC


def hvisc(x, expx):
    """hvisc (:16-31): H(x) = (1 - exp(-x)) / x"""
    t = type(x)
    if x < 1.0e-4:
        return t(1) - t(0.5) * x * (t(1) - x / t(3) * (t(1) - t(0.25) * x * (t(1) - t(0.2) * x)))
    return (t(1) - expx) / x


def factors(mat, dt, dtype=np.float64):
    """-> rows (nrow, 2) of (exp_n, dq_n), mu_0, gfac as calViscoelasticMatrix (:143-161) and UpdateViscoelastic (:249-265) form them"""
    t = np.dtype(dtype).type
    rows = np.zeros((mat.prony.shape[0], 2), dtype=dtype)
    mu_0, gfac = t(0), t(0)
    for n, (mu_n, tau) in enumerate(mat.prony):
        dtau = t(dt) / t(tau)
        exp_n = np.exp(-dtau)
        dq_n = t(mu_n) * hvisc(dtau, exp_n)
        gfac = gfac + dq_n
        mu_0 = mu_0 + t(mu_n)
        rows[n] = exp_n, dq_n
    mu_0 = t(1) - mu_0
    gfac = gfac + mu_0
    return rows, mu_0, gfac


def hvisc_arguments(mat, dt):
    """dt / tau_n of every term: the argument of hvisc's 1e-4 switch"""
    return dt / mat.prony[:, 1]


def cal_viscoelastic_matrix(mat, dt, dtype=np.float64):
    """calViscoelasticMatrix: (6, 6)"""
    t = np.dtype(dtype).type
    if dt == 0.0:
        return R.elastic_matrix(mat.E, mat.nu).astype(dtype) if dtype == np.float64 else FB._elastic_matrix(mat, np.dtype(dtype))
    E, nu = t(mat.E), t(mat.nu)
    G = E / (t(2) * (t(1) + nu))
    K = E / (t(3) * (t(1) - t(2) * nu))
    _, _, gfac = factors(mat, dt, dtype)
    Gg = G * gfac
    Kg = K - t(0.6666666666666666) * Gg
    D = np.zeros((6, 6), dtype=dtype)
    D[:3, :3] = Kg
    for j in range(3):
        D[j, j] = D[j, j] + t(2) * Gg
    for i in range(3, 6):
        D[i, i] = Gg
    return D


def update_viscoelastic(mat, eps, vsig, dt):
    """UpdateViscoelastic: stress (6) from the strain eps; vsig (12 nrow + 6) gets the new q of every term (in place)."""
    dtype = np.result_type(eps, vsig)
    t = dtype.type
    E, nu = t(mat.E), t(mat.nu)
    G = E / (t(2) * (t(1) + nu))
    K = E / (t(3) * (t(1) - t(2) * nu))
    theta = (eps[0] + eps[1] + eps[2]) / t(3)
    dev = np.array([eps[0] - theta, eps[1] - theta, eps[2] - theta, eps[3] * t(0.5), eps[4] * t(0.5), eps[5] * t(0.5)], dtype=dtype)
    nrow = mat.prony.shape[0]
    rows, mu_0, _ = factors(mat, dt, dtype)
    en = vsig[12 * nrow:12 * nrow + 6].copy()
    sig = np.zeros(6, dtype=dtype)
    for n in range(nrow):
        exp_n, dq_n = rows[n]
        for i in range(6):
            vsig[12 * n + 6 + i] = exp_n * vsig[12 * n + i] + dq_n * (dev[i] - en[i])
            sig[i] = sig[i] + vsig[12 * n + 6 + i]
    for i in range(6):
        sig[i] = t(2) * G * (mu_0 * dev[i] + sig[i])
    Kth = K * theta * t(3)
    sig[:3] = sig[:3] + Kth
    return sig


def update_viscoelastic_state(mat, vsig, strain):
    """updateViscoElasticState (in place)"""
    nrow = mat.prony.shape[0]
    for n in range(nrow):
        vsig[12 * n:12 * n + 6] = vsig[12 * n + 6:12 * n + 12]
    thetan = (strain[0] + strain[1] + strain[2]) / 3.0
    vsig[12 * nrow:12 * nrow + 3] = strain[:3] - thetan
    vsig[12 * nrow + 3:12 * nrow + 6] = strain[3:6] * 0.5


def real_default(x):
    """`real(x)` without KIND: default real"""
    return np.asarray(x).astype(np.float32).astype(np.asarray(x).dtype)


def point_stress(mat, de, vsig, dt):
    """The stress a point's update routine leaves: matmul(D, dstrain) at tincr == 0, else StressUpdate, rounded under INFINITE."""
    if dt == 0.0:
        return cal_viscoelastic_matrix(mat, 0.0, np.result_type(de)) @ de
    sig = update_viscoelastic(mat, de, vsig, dt)
    return real_default(sig) if mat.nlgeom == INFINITE else sig


# ---- NORTON creep: fistr1/src/lib/physics/creep.f90 --------------------------------------------------------------------------------------
# What one would not write first, and where it is:
#   * The update routines set isEp = 1 for a NORTON element (static_LIB_3d.f90:595), so its first stress update sets MatlMatrix's saved
#     flag whatever tincr is, and from then on every tangent of every material but the viscoelastic one is elastic.  iso_creep's
#     tangent is reachable only while the latch is clear (a restored state).
#   * update_iso_creep writes gauss%plstrain = dg itself, in every Newton iteration (:204); the commit only adds it to fstatus(2)
#     (updateViscoState :210-215, under tincr > 0).
#   * The update is called with the UPDATELAG trial stress (stress_bak + real(D dstrain) + rotation terms) under
#     `tincr /= 0 .AND. any(stress /= 0)` (static_LIB_3d.f90:738); at tincr == 0 the point is an ELASTIC one, except for the latch.
#   * The local iteration has no bound and a signed exit test, `(ddg<dg*1.d-6).or.(ddg<1.d-12)` (:193): a negative ddg exits.
#   * aa = A ((t + dt)**(m+1) - t**(m+1)) / (m+1) with t the time at the START of the increment (:66, :165).
#   * iso_creep clamps eqvs at 1e-10 (:87) but divides the deviator by the unclamped dstri (:84).
NORTON = 8
CREEP_CAP = 100          # the device's bound on the iteration; the reference has none


class NortonMaterial:
    """tMaterial of !ELASTIC E, nu with !CREEP A, n, m; nlgeom UPDATELAG (the card's default, fstr_ctrl_material.f90:502-504)"""

    def __init__(self, E, nu, A, n, m, nlgeom=UPDATELAG):
        self.E, self.nu, self.nlgeom = float(E), float(nu), int(nlgeom)
        self.plconst = (float(A), float(n), float(m))
        self.kind = NORTON
        self.plastic, self.harden, self.table = False, 0, np.zeros((0, 2))
        self.width = 2


def is_creep(mat):
    return getattr(mat, "kind", 0) == NORTON


def creep_aa(mat, ttime, dtime, dtype=np.float64):
    t = np.dtype(dtype).type
    A, _, m = (t(v) for v in mat.plconst)
    return A * ((t(ttime) + t(dtime)) ** (m + t(1)) - t(ttime) ** (m + t(1))) / (m + t(1))


def _creep_deviator(stress):
    t = stress.dtype.type
    stri = stress.copy()
    p = -(stri[0] + stri[1] + stri[2]) / t(3)
    stri[:3] = stri[:3] + p
    dstri = np.sqrt(t(1.5) * (stri[0] * stri[0] + stri[1] * stri[1] + stri[2] * stri[2]
                              + t(2) * (stri[3] * stri[3] + stri[4] * stri[4] + stri[5] * stri[5])))
    return stri, p, dstri


def iso_creep(mat, stress, plstrain, dtime, ttime):
    """iso_creep (:17-113): (6, 6)"""
    stress = np.asarray(stress)
    t = stress.dtype.type
    D = FB._elastic_matrix(mat, stress.dtype)
    if dtime == 0.0 or not stress.any():
        return D
    xxn, aa = t(mat.plconst[1]), creep_aa(mat, ttime, dtime, stress.dtype)
    G = t(0.5) * t(mat.E) / (t(1) + t(mat.nu))
    stri, p, dstri = _creep_deviator(stress)
    stri = stri / dstri
    eqvs = dstri
    if eqvs < 1.0e-10:
        eqvs = t(1.0e-10)
    f = aa * eqvs ** xxn
    df = xxn * f / eqvs
    c3 = t(6) * G * G
    c4 = c3 * t(plstrain) / (dstri + t(3) * G * t(plstrain))
    c3 = c4 - c3 * df / (t(3) * G * df + t(1))
    c5 = c4 / t(3)
    D = D + c3 * np.outer(stri, stri)
    for i in range(3):
        D[i, i] = D[i, i] - c4
        D[i, :3] = D[i, :3] + c5
    for i in range(3, 6):
        D[i, i] = D[i, i] - c4 / t(2)
    return D


class CreepSpins(ArithmeticError):
    """the reference's unbounded loop would not end (a dg that is not finite) -- the device stops with FX_ERROR_RUNTIME there"""


def update_iso_creep(mat, stress, dtime, ttime, cap=None):
    """update_iso_creep (:117-207) -> stress, plstrain (dg), fstatus(1) (eqvs), iterations.  cap None: the loop as written (it ends on
    its own test only; a dg that is not finite raises CreepSpins instead of spinning)."""
    stress = np.asarray(stress)
    t = stress.dtype.type
    xxn, aa = t(mat.plconst[1]), creep_aa(mat, ttime, dtime, stress.dtype)
    G = t(0.5) * t(mat.E) / (t(1) + t(mat.nu))
    stri, p, dstri = _creep_deviator(stress)
    dg, it = t(0), 0
    with np.errstate(all="ignore"):
        while True:
            it += 1
            eqvs = dstri - t(3) * G * dg
            f = aa * eqvs ** xxn
            df = xxn * f / eqvs
            ddg = (f - dg) / (t(3) * G * df + t(1))
            dg = dg + ddg
            if not np.isfinite(dg) or (cap is not None and it >= cap and not (ddg < dg * t(1.0e-6) or ddg < t(1.0e-12))):
                raise CreepSpins("dg = %r after %d iterations" % (dg, it))
            if ddg < dg * t(1.0e-6) or ddg < t(1.0e-12):
                break
    stri = stri - t(3) * G * dg * stri / dstri
    out = stri.copy()
    out[:3] = stri[:3] - p
    return out, dg, eqvs, it


CREEP_ITERATIONS = []        # iteration counts of every update_iso_creep the element routines made (the cap condition of the tests)


def creep_point(mat, trial, plstrain, fstat, dtime, ttime):
    """the NORTON branch behind the UPDATELAG stress (static_LIB_3d.f90:736-746) -> stress, plstrain, fstatus(1)"""
    if dtime == 0.0 or not np.asarray(trial).any():
        return trial, plstrain, fstat
    s, dg, eqvs, it = update_iso_creep(mat, trial, dtime, ttime)
    CREEP_ITERATIONS.append(it)
    return s, dg, eqvs


def creep_tangents(etype, ec, u, mat, latch, stress, plstrain, dtime, ttime):
    """STF_C3 / STF_C3D8Bbar, UPDATELAG, with MatlMatrix's NORTON branch: yield_ref's routines with the module's matl_matrix swapped
    for the call (the files are not edited); the points' plstrain travels in the place of fstatus(1)"""
    import yield_ref as Y
    keep = Y.matl_matrix
    Y.matl_matrix = lambda m, l, s, istat, pl: FB._elastic_matrix(m, np.dtype(np.float64)) if l else iso_creep(m, np.asarray(s, dtype=np.float64), pl, dtime, ttime)
    try:
        z = np.zeros(len(stress), dtype=np.int32)
        if etype == 361:
            return Y.stf_c3d8bbar(ec, u, mat, latch, stress, z, plstrain)
        return Y.stf_c3(etype, ec, u, mat, latch, stress, z, plstrain)
    finally:
        Y.matl_matrix = keep


def creep_update(etype, ec, u, ddu, mat, stress_bak, strain_bak, plstrain, fstat, dtime, ttime):
    """UPDATE_C3 (:698-747) / Update_C3D8Bbar (:405-442), UPDATELAG, NORTON -> qf, stress, strain, plstrain, fstat"""
    import yield_ref as Y
    elem, elem1, total = (0.5 * ddu + u) + ec, (ddu + u) + ec, ddu
    D = R.elastic_matrix(mat.E, mat.nu)
    nq = H.POINTS[etype]
    qf, stress, strain = np.zeros(3 * H.NODES[etype]), np.zeros((nq, 6)), np.zeros((nq, 6))
    plstrain, fstat = np.array(plstrain, dtype=np.float64).copy(), np.array(fstat, dtype=np.float64).copy()
    if etype == 361:
        bbar, _ = H._hex8_gderiv(elem, np.zeros(3))
        bbar1, _ = H._hex8_gderiv(elem1, np.zeros(3))
        dd = total.T @ bbar
        vol0 = (dd[0, 0] + dd[1, 1] + dd[2, 2]) / 3.0
        pts = [H._hex8_gderiv(elem, H.HEX8_POINTS[q]) for q in range(8)]
        pts1 = [H._hex8_gderiv(elem1, H.HEX8_POINTS[q]) for q in range(8)]
        w = np.ones(8)
    else:
        pts, pts1, w = CN._points(etype, elem), CN._points(etype, elem1), R.QUAD[etype][1]
    for q, (gd, det) in enumerate(pts):
        g = total.T @ gd if etype == 361 else T._gdisp(total, gd)
        de = np.array([g[0, 0], g[1, 1], g[2, 2], g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])
        if etype == 361:
            de[:3] += vol0 - (g[0, 0] + g[1, 1] + g[2, 2]) / 3.0
        rot = 0.5 * (g - g.T)
        strain[q] = strain_bak[q] + de
        sb = stress_bak[q]
        S = np.array([[sb[0], sb[3], sb[5]], [sb[3], sb[1], sb[4]], [sb[5], sb[4], sb[2]]])
        if etype == 361:
            trial = sb + D @ de + Y._voigt(rot @ S - S @ rot) - sb * 3.0 * vol0
        else:
            trial = sb + T.real_default(D @ de) + Y._voigt(rot @ S - S @ rot)
        stress[q], plstrain[q], fstat[q] = creep_point(mat, trial, plstrain[q], fstat[q], dtime, ttime)
        gd1, det1 = pts1[q]
        B = H._bbar_matrix(gd1, bbar1) if etype == 361 else R.b_matrix(gd1)
        qf += (stress[q] @ B) * (w[q] * det1)
    return qf, stress, strain, plstrain, fstat


# ---- elements ------------------------------------------------------------------------------------------------------------------------
def stf_c3(etype, ec, u, mat, stress, dt):
    """STF_C3 (static_LIB_3d.f90:108-199) with flag INFINITE / TOTALLAG for a viscoelastic material"""
    w, nn = R.QUAD[etype][1], R.NN[etype]
    K = np.zeros((3 * nn, 3 * nn))
    D = cal_viscoelastic_matrix(mat, dt)
    for q, (gd, det) in enumerate(CN._points(etype, ec)):
        B = R.b_matrix(gd)
        if mat.nlgeom == TOTALLAG:
            B = B + T._bl1(gd, T._gdisp(u, gd))
        K += (B.T @ (D @ B)) * (w[q] * det)
        if mat.nlgeom == TOTALLAG:
            K += H._initial_stress(gd, stress[q]) * (w[q] * det)
    return K


def update_c3(etype, ec, total, mat, hist, dt):
    """UPDATE_C3 (:655-696) -> qf, stress (nq, 6), strain (nq, 6); hist (nq, W) gets the new q (in place)"""
    w, nn, nq = R.QUAD[etype][1], R.NN[etype], R.nq(etype)
    qf, stress, strain = np.zeros(3 * nn), np.zeros((nq, 6)), np.zeros((nq, 6))
    for q, (gd, det) in enumerate(CN._points(etype, ec)):
        g = T._gdisp(total, gd)
        de = np.array([g[0, 0], g[1, 1], g[2, 2], g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])
        B = R.b_matrix(gd)
        if mat.nlgeom == TOTALLAG:
            H._green_lagrange(de, g)
            B = B + T._bl1(gd, g)
        strain[q] = de
        stress[q] = point_stress(mat, de, hist[q], dt)
        qf += (stress[q] @ B) * (w[q] * det)
    return qf, stress, strain


def stf_c3d8bbar(ec, u, mat, stress, dt):
    """STF_C3D8Bbar (static_LIB_C3D8.f90:90-198)"""
    bbar, _ = H._hex8_gderiv(ec, np.zeros(3))
    K = np.zeros((24, 24))
    D = cal_viscoelastic_matrix(mat, dt)
    for q in range(8):
        gd, det = H._hex8_gderiv(ec, H.HEX8_POINTS[q])
        B = H._bbar_matrix(gd, bbar)
        if mat.nlgeom == TOTALLAG:
            B = B + T._bl1(gd, u.T @ gd)
        K += (B.T @ (D @ B)) * det
        if mat.nlgeom == TOTALLAG:
            K += H._initial_stress(gd, stress[q]) * det
    return K


def update_c3d8bbar(ec, total, mat, hist, dt):
    """Update_C3D8Bbar (:352-403)"""
    bbar, _ = H._hex8_gderiv(ec, np.zeros(3))
    dd = total.T @ bbar
    vol0 = (dd[0, 0] + dd[1, 1] + dd[2, 2]) / 3.0
    qf, stress, strain = np.zeros(24), np.zeros((8, 6)), np.zeros((8, 6))
    for q in range(8):
        gd, det = H._hex8_gderiv(ec, H.HEX8_POINTS[q])
        g = total.T @ gd
        dvol = vol0 - (g[0, 0] + g[1, 1] + g[2, 2]) / 3.0
        de = np.array([g[0, 0] + dvol, g[1, 1] + dvol, g[2, 2] + dvol, g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])
        B = H._bbar_matrix(gd, bbar)
        if mat.nlgeom == TOTALLAG:
            H._green_lagrange(de, g)
            B = B + T._bl1(gd, g)
        strain[q] = de
        stress[q] = point_stress(mat, de, hist[q], dt)
        qf += (stress[q] @ B) * det
    return qf, stress, strain


class _ElasticProxy:
    """The material fbar_ref's tangent takes its matrix from: STF_C3D8Fbar uses the point's D only as a matrix (static_LIB_Fbar.f90),
    so the routine runs unchanged with calViscoelasticMatrix's D in the place of calElasticMatrix's."""
    plastic, kind = False, 0

    def __init__(self, mat):
        self.nlgeom = mat.nlgeom


def stf_c3d8fbar(ec, u, mat, stress, dt):
    """STF_C3D8Fbar: fbar_ref.stf_c3d8fbar with the viscoelastic D.  The module's _material_matrix is swapped for the call and put
    back: the file is not edited."""
    D = cal_viscoelastic_matrix(mat, dt)
    keep = FB._material_matrix
    FB._material_matrix = lambda *a: D
    try:
        z8 = np.zeros(8)
        return FB.stf_c3d8fbar(ec, u, _ElasticProxy(mat), 0, np.zeros((8, 6)), stress, z8.astype(np.int32), z8)
    finally:
        FB._material_matrix = keep


def update_c3d8fbar(ec, total, mat, hist, dt):
    """Update_C3D8Fbar (:530-583, :661-765)"""
    flag = mat.nlgeom
    I3 = np.eye(3)
    _, _, jr, g1ave, _ = FB.averages(ec, total, flag)
    qf, stress, strain = np.zeros(24), np.zeros((8, 6)), np.zeros((8, 6))
    for q in range(8):
        gd, det = FB._gderiv(ec, H.HEX8_POINTS[q])
        g = total.T @ gd
        if flag == INFINITE:
            dvol = total[:, 0] @ g1ave[:, 0] + total[:, 1] @ g1ave[:, 1] + total[:, 2] @ g1ave[:, 2]
            dvol = (dvol - (g[0, 0] + g[1, 1] + g[2, 2])) / 3.0
            de = np.array([g[0, 0] + dvol, g[1, 1] + dvol, g[2, 2] + dvol, g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])
            B = FB._bl_infinite(gd, g1ave)
        else:
            Fbar = jr[q] * (I3 + g)
            de = FB._fbar_strain(Fbar)
            g1, _ = FB._gderiv(ec + total, H.HEX8_POINTS[q])
            B = jr[q] * jr[q] * (FB._b0(gd) + FB._bl1(gd, g)) + FB._bl2(de, (g1ave - g1) / 3.0)
        strain[q] = de
        stress[q] = point_stress(mat, de, hist[q], dt)
        qf += (stress[q] @ B) * det
    return qf, stress, strain


class Model(H.Model):
    """fstr_solid of one mesh of one of the six solid types (361: B-bar, or F-bar with fbar=True) whose sections are viscoelastic,
    ELASTIC (INFINITE / TOTALLAG) or hyperelastic: hyper_ref.Model's state and steps with the time increment `tincr` of the coming
    sub-step and the history `hist` (n_elem, nq, W), W the widest 12 nrow + 6 of the materials (zero padding behind a narrower one)."""

    def __init__(self, etype, coord, conn, mats, elem_mat=None, fbar=False):
        super().__init__(etype, coord, conn, mats, elem_mat)
        self.fbar = bool(fbar)
        self.tincr = self.time = 0.0
        self.width = max([m.width for m in self.mats if is_visco(m) or is_creep(m)] + [0])
        self.hist = np.zeros((self.conn.shape[0], H.POINTS[etype], self.width))

    def _others(self):
        """the model of the sections of another kind: hyper_ref's where one is hyperelastic (ELASTIC INFINITE / TOTALLAG beside it),
        else yield_ref's (ELASTIC of any flag, Mises, Mohr-Coulomb, Drucker-Prager)"""
        import yield_ref as Y
        if self.fbar:
            return FB.Model(self.coord, self.conn, self.mats, self.elem_mat)
        if any(H.kind_of(m) in (H.MOONEY, H.ARRUDA) for m in self.mats):
            return H.Model(self.etype, self.coord, self.conn, self.mats, self.elem_mat)
        return Y.Model(self.etype, self.coord, self.conn, self.mats, self.elem_mat)

    def _own(self, e):
        return is_visco(self.mat(e)) or is_creep(self.mat(e))

    def element_tangents(self):
        u = (self.unode + self.dunode).reshape(-1, 3)
        s = self.st
        out = np.zeros((self.conn.shape[0], 3 * H.NODES[self.etype], 3 * H.NODES[self.etype]))
        rest = [e for e in range(self.conn.shape[0]) if not self._own(e)]
        if rest:       # the sections of another kind: their own model on this state
            o = self._others()
            o.unode, o.dunode, o.latch = self.unode, self.dunode, self.latch
            o.conn, o.elem_mat = self.conn[rest], self.elem_mat[rest]
            o.st = {k: v[rest] for k, v in s.items()}
            out[rest] = o.element_tangents()
        for e, nd in enumerate(self.conn - 1):
            mat = self.mat(e)
            if not self._own(e):
                continue
            if is_creep(mat):
                out[e] = creep_tangents(self.etype, self.coord[nd], u[nd], mat, self.latch, s["stress"][e], s["plstrain"][e], self.tincr,
                                        self.time)
            elif self.fbar:
                out[e] = stf_c3d8fbar(self.coord[nd], u[nd], mat, s["stress"][e], self.tincr)
            elif self.etype == 361:
                out[e] = stf_c3d8bbar(self.coord[nd], u[nd], mat, s["stress"][e], self.tincr)
            else:
                out[e] = stf_c3(self.etype, self.coord[nd], u[nd], mat, s["stress"][e], self.tincr)
        return out

    def element_update(self, order=None):
        total = (self.unode + self.dunode).reshape(-1, 3)
        s = self.st
        qf = np.zeros((self.conn.shape[0], 3 * H.NODES[self.etype]))
        ne = self.conn.shape[0]
        rest = [e for e in range(ne) if not self._own(e)]
        u, du = self.unode.reshape(-1, 3), self.dunode.reshape(-1, 3)
        if rest:
            o = self._others()
            o.unode, o.dunode, o.latch = self.unode, self.dunode, self.latch
            o.conn, o.elem_mat = self.conn[rest], self.elem_mat[rest]
            o.st = {k: v[rest].copy() for k, v in s.items()}
            qf[rest] = o.element_update(order)
            for k in s:
                s[k][rest] = o.st[k]
            self.latch = o.latch
        for e, nd in enumerate(self.conn - 1):
            mat = self.mat(e)
            if not self._own(e):
                continue
            if is_creep(mat):
                qf[e], s["stress"][e], s["strain"][e], s["plstrain"][e], s["fstat"][e] = creep_update(
                    self.etype, self.coord[nd], u[nd], du[nd], mat, s["stress_bak"][e], s["strain_bak"][e], s["plstrain"][e], s["fstat"][e],
                    self.tincr, self.time)
                self.hist[e, :, 0] = s["fstat"][e]
                self.latch = 1          # isEp = 1 (static_LIB_3d.f90:595), whatever tincr is
                continue
            h = self.hist[e][:, :mat.width]
            if self.fbar:
                qf[e], s["stress"][e], s["strain"][e] = update_c3d8fbar(self.coord[nd], total[nd], mat, h, self.tincr)
            elif self.etype == 361:
                qf[e], s["stress"][e], s["strain"][e] = update_c3d8bbar(self.coord[nd], total[nd], mat, h, self.tincr)
            else:
                qf[e], s["stress"][e], s["strain"][e] = update_c3(self.etype, self.coord[nd], total[nd], mat, h, self.tincr)
        return qf

    def commit(self):
        """fstr_UpdateState: T.Model's, and under tincr > 0 updateViscoElasticState of every viscoelastic point"""
        if self.tincr > 0.0:
            for e in range(self.conn.shape[0]):
                mat = self.mat(e)
                if is_visco(mat):
                    for q in range(self.hist.shape[1]):
                        update_viscoelastic_state(mat, self.hist[e, q, :mat.width], self.st["strain"][e, q])
                elif is_creep(mat):         # updateViscoState
                    self.hist[e, :, 1] = self.hist[e, :, 1] + self.st["plstrain"][e]
        super().commit()


# ---- inputs of the comparisons ---------------------------------------------------------------------------------------------------------
# E, nu and the Prony row of the reference's tutorial 07 (viscoelastic cylinder) come first; the two- and three-row sets add terms of
# other time scales.  TINCR: dt / tau lies between 2e-3 and 25 for these rows, a factor of 20 and more above hvisc's 1e-4 switch;
# TINCR_SERIES puts the first row of "one" on the series side (dt / tau = 1e-6, a factor of 100 below it).
PRONY = {"one": [[0.5, 1.0]], "two": [[0.3, 0.2], [0.25, 5.0]], "three": [[0.2, 0.02], [0.3, 1.0], [0.15, 250.0]]}
TINCR, TINCR_SERIES = 0.5, 1.0e-6
GPU_AMP = H.GPU_AMP


def gpu_material(rows="one", nlgeom=TOTALLAG):
    return Material(1000.0, 0.3, PRONY[rows], nlgeom=nlgeom)


def gpu_history(model, seed):
    """A committed history as earlier sub-steps would have left it: old q of every term and the stored deviator at a few per cent of
    strain, new slots equal to the old ones."""
    rng = np.random.default_rng(seed)
    h = np.zeros_like(model.hist)
    for e in range(h.shape[0]):
        mat = model.mat(e)
        if not is_visco(mat):
            continue
        nrow = mat.prony.shape[0]
        for q in range(h.shape[1]):
            for n in range(nrow):
                h[e, q, 12 * n:12 * n + 6] = rng.uniform(-1, 1, 6) * 0.01
                h[e, q, 12 * n + 6:12 * n + 12] = h[e, q, 12 * n:12 * n + 6]
            d = rng.uniform(-1, 1, 6) * 0.02
            d[:3] -= d[:3].mean()
            h[e, q, 12 * nrow:12 * nrow + 6] = d
    return h


def gpu_case(etype, rows="one", nlgeom=TOTALLAG, fbar=False, seed=17, mats=None, elem_mat=None, mesh=None):
    """(mesh, Model) of a GPU comparison: hyper_ref.gpu_mesh, hyper_ref.random_displacement at GPU_AMP, a committed history, tincr =
    TINCR.  mats / elem_mat: several sections instead of the one viscoelastic material.  mesh: another mesh of the type."""
    m = H.gpu_mesh(etype) if mesh is None else mesh
    model = Model(etype, m.coord, m.conn, gpu_material(rows, nlgeom) if mats is None else mats, elem_mat, fbar=fbar)
    model.unode[:], model.dunode[:] = H.random_displacement(m.coord, seed, GPU_AMP)
    model.hist = gpu_history(model, seed)
    model.tincr = TINCR
    return m, model


def gpu_point_inputs(etype, rows, nlgeom, fbar=False):
    """(material, strain handed to StressUpdate (6), history (W)) of every viscoelastic point of gpu_case: what the conditioning
    checks of tests/test_visco_ref.py evaluate in two precisions.  No point is left out."""
    m, model = gpu_case(etype, rows, nlgeom, fbar)
    h0 = model.hist.copy()
    model.element_update()
    out = []
    for e in range(model.conn.shape[0]):
        for q in range(h0.shape[1]):
            out.append((model.mat(e), model.st["strain"][e, q].copy(), h0[e, q].copy()))
    return out


# ---- NORTON inputs ---------------------------------------------------------------------------------------------------------------------
# E, nu, A, n, m of the reference's tutorial 08 (creep cylinder).  CREEP_AMP: strains of 2e-3, stresses of several hundred; at
# CREEP_TINCR the creep strain increment dg of every such point is between 3 % and 130 % of its elastic strain increment
# (tests/test_visco_ref.py prints the range and asserts that at least half the points are above 1e-6 of it): a kernel that skips the
# relaxation fails the comparisons.  The local iteration takes at most 9 passes on these inputs.
CREEP_AMP, CREEP_TINCR, CREEP_TIME = 2.0e-3, 2.0e-6, 1.0e-5


def creep_material():
    return NortonMaterial(206900.0, 0.29, 1.0e-10, 5.0, 0.0)


def creep_case(etype, seed=17, mats=None, elem_mat=None, mesh=None):
    """(mesh, Model) of a NORTON GPU comparison: a committed state as a previous sub-step would have left it (stress_bak = D strain_bak,
    a creep strain increment in plstrain, an accumulated one in fstatus(2)), displacement fields of size CREEP_AMP, the time pair
    (CREEP_TIME, CREEP_TINCR), latch clear.  mesh: another mesh of the type than hyper_ref.gpu_mesh."""
    m = H.gpu_mesh(etype) if mesh is None else mesh
    model = Model(etype, m.coord, m.conn, creep_material() if mats is None else mats, elem_mat)
    model.unode[:], model.dunode[:] = H.random_displacement(m.coord, seed, CREEP_AMP)
    rng = np.random.default_rng(seed)
    s = model.st
    ne, q = s["plstrain"].shape
    s["strain_bak"][:] = rng.uniform(-1, 1, (ne, q, 6)) * CREEP_AMP
    for e in range(ne):
        s["stress_bak"][e] = s["strain_bak"][e] @ R.elastic_matrix(model.mat(e).E, model.mat(e).nu).T
        if is_creep(model.mat(e)):
            s["plstrain"][e] = rng.uniform(0.0, 2.0e-5, q)
            model.hist[e, :, 1] = rng.uniform(0.0, 1.0e-4, q)
    s["stress"][:], s["strain"][:] = s["stress_bak"], s["strain_bak"]
    model.tincr, model.time = CREEP_TINCR, CREEP_TIME
    return m, model


# ---- the reference program's own runs: tests/golden/visco_decks.npz (tests/golden/make_visco_golden.py) ---------------------------------
summary = H.summary
within_1e4 = H.within_1e4
DECK_SUBSTEPS, DECK_CONVERG = 3, 1.0e-3
DECK_LOADS = {"visco": (0.005, 0.5), "visco_inf": (0.005, 0.5), "norton": (0.0003, 2.0e-4)}      # material -> (stretch, time increment)
# name -> (etype, cube size n, MAT1 of scripts/fistr1_cube_deck.py --nl-material, two sections, F-bar)
GOLDEN_DECKS = {"v%d_%s" % (et, mat): (et, n, mat, False, False) for et, n in H._SIZES.items() for mat in ("visco", "norton")}
GOLDEN_DECKS.update({"v361_visco_inf": (361, 2, "visco_inf", False, False), "v342_visco_inf": (342, 1, "visco_inf", False, False),
                     "v361_visco_fbar": (361, 2, "visco", False, True), "v361_visco_two": (361, 2, "visco", True, False),
                     "v342_norton_two": (342, 1, "norton", True, False)})
REFERENCE_DECKS = ("1elem_creep", "1elem_relax", "1elem_viscoe", "1elem_viscof")        # recorded from the reference's own decks


def golden_deck(name):
    """(mesh, materials, elem_mat or None, bc, time increment, F-bar) of one recorded cube deck, as fistr1_cube_deck.py writes it:
    z = 0 clamped, the top face moved in z and by a fifth of that in x in the first of the DECK_SUBSTEPS increments of a VISCO step
    and held (deck_schedule; NORTON: once in a STATIC step of one increment before it, time 0 to 1, and a second time in the VISCO step); with two sections the second half
    of the elements is Mises BILINEAR."""
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    from oracle.refrun import Material as RefMaterial
    et, n, mat, two, fbar = GOLDEN_DECKS[name]
    m = CubeMesh(n) if et == 361 else solid_mesh(n, et)
    m.etype = et
    strain, dt = DECK_LOADS[mat]
    mats = {"visco": lambda: Material(206900.0, 0.29, [[0.5, 1.0]], TOTALLAG), "visco_inf": lambda: Material(206900.0, 0.29, [[0.5, 1.0]], INFINITE),
            "norton": creep_material}[mat]()
    em = None
    if two:
        mats = [mats, RefMaterial(206900.0, 0.29, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=UPDATELAG)]
        em = np.where(np.arange(m.n_elem) < m.n_elem // 2, 1, 2).astype(np.int32)
    node, dof, val = m.dirichlet()
    t = m.top_nodes
    bc = (np.concatenate([node, t, t]).astype(np.int32),
          np.concatenate([dof, np.full(t.size, 3), np.full(t.size, 1)]).astype(np.int32),
          np.concatenate([val, np.full(t.size, strain * n), np.full(t.size, 0.2 * strain * n)]))
    return m, mats, em, bc, dt, fbar


def deck_schedule(name):
    """[(share of the boundary values applied, time, tincr)] of the sub-steps of a recorded cube deck in the order of FSTR.sta.  ctime
    is the time at the start of the increment (fstr_solve_NLGEOM.f90:129-130); a STATIC step passes tincr = 0
    (fstr_solve_NonLinear.f90:60-61) and lasts from 0 to 1.  In a VISCO step fstr_AddBC does not ramp the prescribed displacements:
    the first sub-step (FACTOR(1) < 1e-10) gets the whole value, every later one nothing (fstr_AddBC.f90:44-47) -- step and hold."""
    mat = GOLDEN_DECKS[name][2]
    dt = DECK_LOADS[mat][1]
    n = DECK_SUBSTEPS
    t0 = 1.0 if mat == "norton" else 0.0
    return ([(1.0, 0.0, 0.0)] if mat == "norton" else []) + [(1.0 if k == 1 else 0.0, t0 + (k - 1) * dt, dt) for k in range(1, n + 1)]


# ---- the reference's own one-element decks: examples/static/1elem/{creep,relax,viscoe,viscof} (tests/golden/decks/visco1/) ---------------
# One unit TYPE=361 cube (B-bar under NLSTATIC).  The mesh file numbers its nodes 1, 2, 9, 10, 21, 22, 29, 30; here they are 1..8 in
# that order.  BOT (y = 0) is held in y, CENT (x = 0) in x, FRONT (z = 1) in z; the face y = 1 (file nodes 9, 10, 29, 30) is moved or
# loaded in y.
ONE_ELEM_COORD = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]], dtype=np.float64)
ONE_ELEM_CONN = np.array([[1, 2, 4, 3, 5, 6, 8, 7]], dtype=np.int32)
_SUPPORTS = [(1, 2), (2, 2), (5, 2), (6, 2), (1, 1), (3, 1), (5, 1), (7, 1), (5, 3), (6, 3), (7, 3), (8, 3)]
_TOP = [(3, 2), (4, 2), (7, 2), (8, 2)]
# name -> (material, [step]); step = (VISCO?, dtime, etime, max_iter, value on the top face in y, nodal load on its nodes in y or None)
ONE_ELEM_DECKS = {
    # !VISCOELASTIC 0.5, 1.0 on 1e5 / 0.25; one VISCO increment of 1.0 that moves the face by 0.1
    "1elem_viscoe": (lambda: Material(1.0e5, 0.25, [[0.5, 1.0]], TOTALLAG), [(True, 1.0, 1.0, 50, 0.1, None)]),
    # `!VISCOELASTIC, CAUCHY`: the card knows no CAUCHY parameter (fstr_ctrl_material.f90:277-279), the flag stays TOTALLAG; its step
    # names `CLOAD, 1` where the step card's word is LOAD (creep.cnt), so no load group is active: nothing moves, one iteration
    "1elem_viscof": (lambda: Material(1.0e5, 0.25, [[0.5, 1.0]], TOTALLAG), [(True, 1.0, 1.0, 50, None, None)]),
    # !CREEP 2.5e-27, 5, -0.2 on 2e7 / 0.3: the only recorded deck whose time exponent is not zero.  STATIC: the face moved by 0.01;
    # VISCO: ten increments of 0.1 from time 1.0 with the face held (BOUNDARY group 2: zeros)
    "1elem_relax": (lambda: NortonMaterial(20.0e6, 0.3, 2.5e-27, 5.0, -0.2), [(False, 1.0, 1.0, 50, 0.01, None), (True, 0.1, 1.0, 20, 0.0, None)]),
    # !CREEP 1e-10, 5, 0 on 1e5 / 0.25 under a nodal load of -10 per node: STATIC, then VISCO increments of 0.1 in which the load
    # stays whole: a load group that was active in the step before keeps factor 1 (fstr_ass_load.f90:69-70).  The creep strain of an
    # increment is 2.5 times the elastic strain and the tangent is the elastic one (the latch): the unmodified program stops in
    # the first increment at ITMAX = 20.
    "1elem_creep": (lambda: NortonMaterial(1.0e5, 0.25, 1.0e-10, 5.0, 0.0), [(False, 1.0, 1.0, 50, None, -10.0), (True, 0.1, 1.0, 20, None, -10.0)]),
}


def run_one_elem_deck(name):
    """the restatement's loop over one of these decks -> (Newton counts in the order of FSTR.sta, summaries of the converged
    sub-steps, converged to the end?).  Steps follow each other in time (setup_stepInfo_starttime, m_step.f90:83-92); a STATIC step
    passes tincr = 0; a VISCO step gives its first sub-step the whole prescribed value and the others nothing (fstr_AddBC.f90:44-47)
    while the nodal load follows the load factor -- or stays whole where its group was active in the step before
    (fstr_ass_load.f90:69-70); an increment that runs out of iterations ends the run."""
    mat, steps = ONE_ELEM_DECKS[name]
    model = Model(361, ONE_ELEM_COORD, ONE_ELEM_CONN, mat())
    counts, sums, start, loaded = [], [], 0.0, False
    for visco, dtime, etime, max_iter, top, load in steps:
        dofs = _SUPPORTS + (_TOP if top is not None else [])
        vals = [0.0] * len(_SUPPORTS) + ([top] * 4 if top is not None else [])
        bc = (np.array([d[0] for d in dofs], dtype=np.int32), np.array([d[1] for d in dofs], dtype=np.int32), np.array(vals))
        cload = None
        if load is not None:
            cload = np.zeros(24)
            for nd, dof in _TOP:
                cload[3 * (nd - 1) + dof - 1] = load
        n = int((etime + 0.999999999 * dtime) / dtime)        # fstr_ctrl_common.f90:257
        for k in range(1, n + 1):
            model.time, model.tincr = start + (k - 1) * dtime, dtime if visco else 0.0
            f0, f1 = (k - 1) / n, k / n
            gl = None if cload is None else cload * (1.0 if loaded else f1)
            if visco:       # step and hold for the prescribed values
                held = (bc[0], bc[1], bc[2] if k == 1 else np.zeros_like(bc[2]))
                ok, it = model.newton_substep(0.0, 1.0, held, gl, max_iter, 1.0e-3)
            else:
                ok, it = model.newton_substep(f0, f1, bc, None if gl is None else gl / f1, max_iter, 1.0e-3)
            counts.append(it)
            if not ok:
                return counts, sums, False
            sums.append(summary(361, ONE_ELEM_CONN, model.unode, model.st["strain"], model.st["stress"]))
        start += etime
        loaded = load is not None
    return counts, sums, True


# ---- the cases of tests/test_gpu_visco.py, one registry for the GPU comparisons and for the conditioning checks of test_visco_ref.py ----
def mises_material():
    """a Mises BILINEAR section of the mixed cases: yields at strains of 2 % on E = 1000 (viscoelastic cases)"""
    from oracle.refrun import Material as Ref
    return Ref(1000.0, 0.3, plastic=True, harden=0, plconst=(20.0, 50.0, 0.0), nlgeom=UPDATELAG)


def sections_case(etype, which):
    """a viscoelastic section beside others, elements dealt out irregularly"""
    from oracle.refrun import Material as Ref
    m = H.gpu_mesh(etype)
    if which == "neohooke":        # group 8 beside group 3
        mats = [gpu_material("two", TOTALLAG), H.TEST_MATERIALS["neohooke"]()]
    elif which == "mises":         # groups 7 and 8 beside group 2: the latch of the Mises section does not reach the viscoelastic tangent
        mats = [gpu_material("two", TOTALLAG), mises_material(), gpu_material("one", INFINITE)]
    else:                          # groups 7 and 8 with histories of 30 and 42 components beside groups 0 and 1
        mats = [gpu_material("two", INFINITE), Ref(900.0, 0.25, nlgeom=TOTALLAG), gpu_material("three", TOTALLAG), Ref(1100.0, 0.33, nlgeom=INFINITE)]
    em = (1 + (np.arange(m.n_elem) * 7 // 3) % len(mats)).astype(np.int32)
    return gpu_case(etype, mats=mats, elem_mat=em)


def creep_sections_case(etype, which):
    from oracle.refrun import Material as Ref
    m = H.gpu_mesh(etype)
    if which == "mises":
        mats = [creep_material(), Ref(206900.0, 0.29, plastic=True, harden=0, plconst=(300.0, 2000.0, 0.0), nlgeom=UPDATELAG),
                Ref(70000.0, 0.33, nlgeom=TOTALLAG)]
    else:       # groups 9, 8 and 2 in one context: history of 2 and of 30 components
        mats = [creep_material(), Material(206900.0, 0.29, PRONY["two"], TOTALLAG), Ref(70000.0, 0.33, nlgeom=UPDATELAG)]
    em = (1 + (np.arange(m.n_elem) * 7 // 3) % len(mats)).astype(np.int32)
    return creep_case(etype, mats=mats, elem_mat=em)


_FLAG = {INFINITE: "infinite", TOTALLAG: "totallag"}
# id -> (factory of (mesh, Model), tincr of the case)
VISCO_CASES = {"%d_%s" % (et, _FLAG[fl]): ((lambda et=et, fl=fl: gpu_case(et, "one", fl)), TINCR)
               for et in (361, 341, 342, 351, 352, 362) for fl in (INFINITE, TOTALLAG)}
VISCO_CASES.update({"fbar_%s" % _FLAG[fl]: ((lambda fl=fl: gpu_case(361, "one", fl, fbar=True)), TINCR) for fl in (INFINITE, TOTALLAG)})
VISCO_CASES.update({"rows_%d_%s_%s" % (et, rows, _FLAG[fl]): ((lambda et=et, rows=rows, fl=fl: gpu_case(et, rows, fl)), TINCR)
                    for et, rows, fl in ((361, "two", TOTALLAG), (342, "three", INFINITE), (352, "three", TOTALLAG))})
VISCO_CASES.update({"series_%d_%s" % (et, _FLAG[fl]): ((lambda et=et, fl=fl: gpu_case(et, "one", fl)), TINCR_SERIES)
                    for et, fl in ((361, INFINITE), (341, TOTALLAG))})
VISCO_CASES.update({"beside_%s_%d" % (w, et): ((lambda et=et, w=w: sections_case(et, w)), TINCR)
                    for et, w in ((361, "neohooke"), (342, "neohooke"), (361, "elastic"), (351, "elastic"), (362, "elastic"),
                                  (361, "mises"), (342, "mises"))})
CREEP_CASES = {"%d" % et: (lambda et=et: creep_case(et)) for et in (361, 341, 342, 351, 352, 362)}
CREEP_CASES.update({"beside_%s_%d" % (w, et): (lambda et=et, w=w: creep_sections_case(et, w))
                    for et, w in ((361, "mises"), (342, "mises"), (361, "visco"), (352, "visco"))})
SECOND_SEED, SECOND_SHARE = 29, 0.3          # the displacement increment of the second sub-step: random_displacement(seed, share * amp)


def second_increment(coord, amp):
    return H.random_displacement(coord, SECOND_SEED, SECOND_SHARE * amp)[1]


def case_point_inputs(model, amp):
    """What the material routines are handed at every viscoelastic and NORTON point in the two stress updates a parity test runs on
    `model` (the first from the case's state, the second after the commit with second_increment; a NORTON case moves its time on by
    tincr).  -> [("visco", material, strain (6), history before the update (W), tincr) |
                 ("creep", material, trial stress (6), strain increment (6), time, tincr)], no point left out.
    The trial stress of a NORTON point is what the same update leaves with the relaxation switched off (tincr = 0)."""
    import copy
    out = []
    for step in (1, 2):
        trial = None
        if any(is_creep(x) for x in model.mats):
            dry = copy.deepcopy(model)
            dry.tincr = 0.0
            dry.element_update()
            trial, de = dry.st["stress"], dry.st["strain"] - dry.st["strain_bak"]
        h0 = model.hist.copy()
        model.element_update()
        for e in range(model.conn.shape[0]):
            mat = model.mat(e)
            for q in range(h0.shape[1]):
                if is_visco(mat):
                    out.append(("visco", mat, model.st["strain"][e, q].copy(), h0[e, q, :mat.width].copy(), model.tincr))
                elif is_creep(mat):
                    out.append(("creep", mat, trial[e, q].copy(), de[e, q].copy(), model.time, model.tincr))
        if step == 1:
            model.commit()
            model.dunode[:] = second_increment(model.coord, amp)
            if trial is not None:
                model.time = model.time + model.tincr
    return out


class GroupModel:
    """fstr_solid of a mesh of several element groups (fx_nl_init_groups) with viscoelastic, NORTON and other sections: one Model per
    group on the shared nodes.  The flat layouts are the library's: the groups one after the other, [elem][point][.] inside."""

    def __init__(self, coord, groups, mats):
        self.coord = np.asarray(coord, dtype=np.float64)
        self.parts = [Model(g[0], self.coord, g[1], mats, g[3], fbar=(g[0] == 361 and g[2] == 4)) for g in groups]
        n = self.coord.shape[0]
        self.unode, self.dunode = np.zeros(3 * n), np.zeros(3 * n)
        for p in self.parts:
            p.unode, p.dunode = self.unode, self.dunode
        self.width = self.parts[0].width
        self.latch = 0

    def set_time(self, time, tincr):
        for p in self.parts:
            p.time, p.tincr = time, tincr

    def flat(self, name):
        if name == "hist":
            return np.concatenate([p.hist.reshape(-1, self.width) for p in self.parts])
        return np.concatenate([p.st[name].reshape((-1, 6) if p.st[name].ndim == 3 else -1) for p in self.parts])

    def _latch(self, value=None):
        if value is None:
            value = max([self.latch] + [p.latch for p in self.parts])
        self.latch = value
        for p in self.parts:
            p.latch = value

    def element_tangents(self):
        self._latch(self.latch)
        return np.concatenate([p.element_tangents().ravel() for p in self.parts])

    def element_update(self):
        out = np.concatenate([p.element_update().ravel() for p in self.parts])
        self._latch()
        return out

    def commit(self):
        du = self.dunode.copy()
        for p in self.parts:        # every Model.commit adds dunode to the shared unode and clears it: once is what fstr_UpdateState does
            self.dunode[:] = 0.0
            p.commit()
        self.unode += du


def group_case(order, seed=17):
    """(mesh, groups, GroupModel) of the fx_nl_init_groups comparison: MixedMesh(2, order) -- 361 + 351 + 341, or 362 + 352 + 342 --
    with a viscoelastic TOTALLAG (two rows), a NORTON and an ELASTIC UPDATELAG section dealt out over all elements, so that every
    group holds all three; a committed state and history as creep_case makes them; the time pair (CREEP_TIME, CREEP_TINCR)."""
    from frontistr_amd.mesh import MixedMesh
    from oracle.refrun import Material as Ref
    mesh = MixedMesh(2, order)
    mats = [Material(206900.0, 0.29, PRONY["two"], TOTALLAG), creep_material(), Ref(70000.0, 0.33, nlgeom=UPDATELAG)]
    em = (1 + (np.arange(mesh.n_elem) * 7 // 3) % 3).astype(np.int32)
    groups = mesh.groups_with(2, em)
    model = GroupModel(mesh.coord, groups, mats)
    model.unode[:], model.dunode[:] = H.random_displacement(mesh.coord, seed, CREEP_AMP)
    rng = np.random.default_rng(seed)
    for p in model.parts:
        s = p.st
        ne, q = s["plstrain"].shape
        s["strain_bak"][:] = rng.uniform(-1, 1, (ne, q, 6)) * CREEP_AMP
        for e in range(ne):
            mat = p.mat(e)
            s["stress_bak"][e] = s["strain_bak"][e] @ R.elastic_matrix(mat.E, mat.nu).T
            if is_creep(mat):
                s["plstrain"][e] = rng.uniform(0.0, 2.0e-5, q)
                p.hist[e, :, 1] = rng.uniform(0.0, 1.0e-4, q)
        s["stress"][:], s["strain"][:] = s["stress_bak"], s["strain_bak"]
        p.hist += gpu_history(p, seed) * (CREEP_AMP / 0.02)
    model.set_time(CREEP_TIME, CREEP_TINCR)
    return mesh, groups, model
