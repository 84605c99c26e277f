"""Numpy restatement of the reference's Mohr-Coulomb and Drucker-Prager materials (!PLASTIC, YIELD=MOHR-COULOMB | DRUCKER-PRAGER) in
the nonlinear static loop of the six solid types.

Material point, fistr1/src/lib/physics/Elastoplastic.f90 as it is written: calYieldFunc (:297-348), the yield-type branches of
BackwardEuler (:461-558) and of calElastoPlasticMatrix (:69-117), with eigen3 (lib/utilities/utilities.f90:107-201).  The routines
work in the dtype of the stress they are given (float64, or np.longdouble for the sensitivity check).  What the reference does that
one would not write down first -- the trace in calYieldFunc against the mean stress in the Drucker-Prager return, calYieldFunc's
Mohr-Coulomb f being half of the one the return iterates on, the clamp of small stress components before the eigen-solve, absolute
tolerances, five iterations, `dlambda < 0` resetting istat, the hardening coefficient taken at the sub-step's first plastic strain,
first-of-ties maxloc / minloc -- is kept, each place cited where it stands.  The reference's `stop` statements raise MathError.

Elements: STF_C3 / UPDATE_C3 for TYPE=341, 342, 351, 352, 362 and STF_C3D8Bbar / Update_C3D8Bbar for TYPE=361 in all three NLGEOM
branches, on the element data and pieces of c3_ref.py, tet_nl_ref.py, c3_nl_ref.py and hyper_ref.py (none of them edited): what is
new here is the material point and the UPDATELAG branch of the B-bar element.  A Mises or ELASTIC material goes through the same
element routines with the existing material point (oracle.pyoracle), so that sections of different kinds sit in one Model.

This module is itself pinned to the unmodified program: tests/golden/yield_decks.npz (tests/golden/make_yield_golden.py) holds the
Newton counts and printed summaries of fistr1 on its own 1elem decks, the Drucker-Prager tutorial and small cube decks, and
tests/test_yield_ref.py reproduces them with Model.
"""
import numpy as np

import c3_nl_ref as CN
import c3_ref as R
import hyper_ref as H
import tet_nl_ref as T
from tet_nl_ref import INFINITE, TOTALLAG, UPDATELAG  # noqa: F401

MOHR, DRUCKER = 4, 5                   # fx_material_view::plastic, the material kind
PLASTICITY_PI = 3.14159265358979       # fstr_ctrl_get_PLASTICITY's own PI (fstr_ctrl_material.f90:355)
TOL, MAXITER = 1.0e-3, 5               # BackwardEuler :360-361


class MathError(ArithmeticError):
    """One of the reference's `stop` statements"""


class Material:
    """tMaterial after a !PLASTIC card with YIELD=MOHR-COULOMB / DRUCKER-PRAGER (fstr_ctrl_material.f90:451-469): plconst =
    M_PLCONST1..3 = (c, H, phi [rad] or eta), plconst4 = M_PLCONST4 = xi; hardening digit 0."""

    def __init__(self, kind, E, nu, plconst, plconst4=0.0, nlgeom=UPDATELAG):
        self.kind, self.E, self.nu, self.nlgeom = int(kind), float(E), float(nu), int(nlgeom)
        self.plconst, self.plconst4 = tuple(float(v) for v in plconst), float(plconst4)
        self.plastic, self.harden, self.table = True, 0, np.zeros((0, 2))


def mohr_coulomb(E, nu, c, phi_deg, H=0.0, nlgeom=UPDATELAG):
    return Material(MOHR, E, nu, (c, H, phi_deg * PLASTICITY_PI / 180.0), nlgeom=nlgeom)


def drucker_prager(E, nu, c, phi_deg, H=0.0, nlgeom=UPDATELAG):
    dum = phi_deg * PLASTICITY_PI / 180.0
    eta = 2.0 * np.sin(dum) / (np.sqrt(3.0) * (3.0 + np.sin(dum)))
    xi = 6.0 * np.cos(dum) / (np.sqrt(3.0) * (3.0 + np.sin(dum)))
    return Material(DRUCKER, E, nu, (c, H, float(eta)), float(xi), nlgeom=nlgeom)


def kind_of(mat):
    return getattr(mat, "kind", 1 if mat.plastic else 0)


def is_yield(mat):
    return kind_of(mat) in (MOHR, DRUCKER)


# ---- lib/utilities/utilities.f90 ------------------------------------------------------------------------------------------------------
def eigen3(tensor, info=None):
    """eigen3 :107-201 -> eigval (3), princ (3, 3) with the principal vectors as columns.  Only the upper triangle of btens is read.
    info (a dict, optional) receives the number of rotations made and of those skipped because the off-diagonal term is negligible."""
    t = np.asarray(tensor)
    dt = t.dtype
    n = dt.type
    b = np.zeros((3, 3), dtype=dt)
    b[0, 0], b[1, 1], b[2, 2] = t[0], t[1], t[2]
    b[0, 1] = b[1, 0] = t[3]
    b[1, 2] = b[2, 1] = t[4]
    b[2, 0] = b[0, 2] = t[5]
    princ = np.eye(3, dtype=dt)
    ev = np.array([b[0, 0], b[1, 1], b[2, 2]], dtype=dt)
    if info is not None:
        info.update(rotated=0, skipped=0)
    for _ in range(50):
        fsum = abs(b[0, 1]) + abs(b[0, 2]) + abs(b[1, 2])
        if fsum < n(1.0e-10):
            return ev, princ
        for ip in range(2):
            for iq in range(ip + 1, 3):
                od = n(100) * abs(b[ip, iq])
                rotate = od + abs(ev[ip]) != abs(ev[ip]) and od + abs(ev[iq]) != abs(ev[iq])
                if info is not None:
                    info["rotated" if rotate else "skipped"] += 1
                if rotate:
                    hd = ev[iq] - ev[ip]
                    if abs(hd) + od == abs(hd):
                        tt = b[ip, iq] / hd
                    else:
                        theta = n(0.5) * hd / b[ip, iq]
                        tt = n(1) / (abs(theta) + np.sqrt(n(1) + theta * theta))
                        if theta < 0:
                            tt = -tt
                    c = n(1) / np.sqrt(n(1) + tt * tt)
                    s = tt * c
                    tau = s / (n(1) + c)
                    h = tt * b[ip, iq]
                    ev[ip] = ev[ip] - h
                    ev[iq] = ev[iq] + h
                    ir = 3 - ip - iq
                    rp, rq = (min(ir, ip), max(ir, ip)), (min(ir, iq), max(ir, iq))
                    g, h = b[rp], b[rq]
                    b[rp] = g - s * (h + g * tau)
                    b[rq] = h + s * (g - h * tau)
                    for k in range(3):
                        g, h = princ[k, ip], princ[k, iq]
                        princ[k, ip] = g - s * (h + g * tau)
                        princ[k, iq] = h + s * (g - h * tau)
                b[ip, iq] = n(0)
    raise MathError("Jacobi iteration unable to converge")


# ---- lib/physics/Elastoplastic.f90 ----------------------------------------------------------------------------------------------------
def _consts(mat, dt):
    n = dt.type
    return n(mat.E), n(mat.nu), n(mat.plconst[0]), n(mat.plconst[1]), n(mat.plconst[2]), n(mat.plconst4)


def _j3(d):
    """J3 as BackwardEuler :467-471, cal_equivalent_stress :147-151 and calElastoPlasticMatrix :74-78 order its products"""
    two = d.dtype.type(2)
    return d[0] * d[1] * d[2] + two * d[3] * d[4] * d[5] - d[5] * d[1] * d[5] - d[3] * d[3] * d[2] - d[0] * d[4] * d[4]


def sin3theta(J2, J3):
    n = J2.dtype.type
    return -n(3) * np.sqrt(n(3)) * J3 / (n(2) * J2 ** n(1.5))


def _lode(J2, J3):
    """sin 3 theta -> theta, calYieldFunc :336-339 / BackwardEuler :472-475"""
    n = J2.dtype.type
    sita = sin3theta(J2, J3)
    if abs(abs(sita) - n(1)) < n(1.0e-8):
        sita = np.copysign(n(1), sita)
    if abs(sita) > n(1):
        raise MathError("Math Error in Mohr-Coulomb calculation")
    return np.arcsin(sita) / n(3)


def cal_yield_func(mat, stress, pstrain):
    """calYieldFunc :297-348 for yield types 1 and 2: J1 is the TRACE here (:313)"""
    s = np.asarray(stress)
    dt = s.dtype
    n = dt.type
    _, _, c, Hd, p3, p4 = _consts(mat, dt)
    J1 = s[0] + s[1] + s[2]
    d = np.array([s[0] - J1 / n(3), s[1] - J1 / n(3), s[2] - J1 / n(3), s[3], s[4], s[5]], dtype=dt)
    J2 = n(0.5) * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + (d[3] * d[3] + d[4] * d[4] + d[5] * d[5])
    eqvs = c + Hd * n(pstrain)
    if mat.kind == MOHR:
        # :331-335 orders J3's products differently from the other places
        J3 = d[0] * d[1] * d[2] + n(2) * d[3] * d[4] * d[5] - d[1] * d[5] * d[5] - d[2] * d[3] * d[3] - d[0] * d[4] * d[4]
        sita = _lode(J2, J3)
        return (np.cos(sita) - np.sin(sita) * np.sin(p3) / np.sqrt(n(3))) * np.sqrt(J2) + J1 * np.sin(p3) / n(3) - eqvs * np.cos(p3)
    return np.sqrt(J2) + p3 * J1 - eqvs * p4


def backward_euler(mat, stress, plstrain, istat, fstat1, info=None, *, maxiter=MAXITER, first_of_ties=True, mm_rule=True,
                   reset_istat=0, exits_write_fstat=False, zeroing=True):
    """BackwardEuler :351-561, yield types 1 and 2 -> (stress, istat, fstat(1)).  info (a dict, optional) receives what the margin
    checks read: f of the trial stress, whether the return ended through the `dlambda < 0` reset, sin 3 theta and the principal
    stresses; the exit taken (`band`: |f| < tol, `elastic`: f < 0, `reset`, `converged`, `exhausted`: the loop ran out), the number of
    iterations begun, and maxp / minp / mm (0-based) of the Mohr-Coulomb return.
    The keyword parameters default to what the reference does; any other value is a deliberately wrong point function, for the
    check that the edge cases of tests/point_ref.py tell the two apart: maxiter (:361); first_of_ties (maxloc / minloc :481-482, False:
    the last of ties); mm_rule (:483-485, False: the index that is neither maxp nor minp); reset_istat (:497 / :542 set 0);
    exits_write_fstat (:386-393 leave fstat alone, True: they store plstrain); zeroing (:476-478)."""
    s = np.array(stress)
    dt = s.dtype
    n = dt.type
    E, nu, c, Hd, p3, p4 = _consts(mat, dt)
    plstrain = n(plstrain)
    f = cal_yield_func(mat, s, plstrain)
    if info is not None:
        info.update(f=float(f), reset=False, iterations=0)
    if abs(f) < n(TOL) or f < 0:
        ist = 1 if abs(f) < n(TOL) else 0
        if info is not None:
            info["exit"] = "band" if ist else "elastic"
        return s, ist, (plstrain if exits_write_fstat else fstat1)
    istat = 1
    J1 = (s[0] + s[1] + s[2]) / n(3)                      # :402, the MEAN stress from here on
    d = np.array([s[0] - J1, s[1] - J1, s[2] - J1, s[3], s[4], s[5]], dtype=dt)
    J2 = n(0.5) * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + (d[3] * d[3] + d[4] * d[4] + d[5] * d[5])
    G = E / (n(2) * (n(1) + nu))
    K = E / (n(3) * (n(1) - n(2) * nu))
    dlambda, pstrain = n(0), plstrain
    how, it = "exhausted", 0
    if mat.kind == MOHR:
        J3 = _j3(d)
        if info is not None:
            info["sin3"] = float(sin3theta(J2, J3))
        sita = _lode(J2, J3)
        sf, cf, ss = np.sin(p3), np.cos(p3), np.sin(sita)
        if zeroing:
            s[np.abs(s) < n(1.0e-10)] = n(0)              # :476-478
        prn, prj = eigen3(s, info)
        if first_of_ties:
            maxp, minp = int(np.argmax(prn)), int(np.argmin(prn))  # the first of ties, as maxloc / minloc
        else:
            maxp, minp = 2 - int(np.argmax(prn[::-1])), 2 - int(np.argmin(prn[::-1]))
        mm = 0
        if maxp == 0 or minp == 0:
            mm = 1
        if maxp == 1 or minp == 1:
            mm = 2
        if not mm_rule and maxp != minp:
            mm = 3 - maxp - minp
        if info is not None:
            info.update(principal=[float(v) for v in prn], maxp=maxp, minp=minp, mm=mm)
        smax, smin = prn[maxp], prn[minp]
        stiff = n(4) * G * (n(1) + sf * ss / n(3)) + n(4) * K * sf * ss
        for it in range(1, maxiter + 1):
            dd = stiff + n(4) * Hd * cf * cf                # H at the sub-step's first plastic strain (:488-490; linear law: a constant)
            dlambda = dlambda + f / dd
            if n(2) * dlambda * cf < 0:
                if cf == 0:
                    raise MathError("Math error in return mapping")
                dlambda, istat, how = n(0), reset_istat, "reset"
                break
            yd = c + Hd * (pstrain + n(2) * dlambda * cf)
            f = smax - smin + (smax + smin) * sf - stiff * dlambda - n(2) * yd * cf
            if abs(f) < n(TOL):
                how = "converged"
                break
        pstrain = pstrain + n(2) * dlambda * cf
        prn[maxp] = prn[maxp] - (n(2) * G * (n(1) + sf / n(3)) + n(2) * K * sf) * dlambda
        prn[minp] = prn[minp] + (n(2) * G * (n(1) - sf / n(3)) - n(2) * K * sf) * dlambda
        prn[mm] = prn[mm] + (n(4) * G / n(3) - n(2) * K) * sf * dlambda
        m = (prj * prn[None, :]) @ prj.T
        s = np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[1, 2], m[2, 0]], dtype=dt)
    else:
        yd = np.sqrt(J2)                                   # cal_equivalent_stress :158-159
        for it in range(1, maxiter + 1):
            dd = G + K * p3 * p3 + Hd * p4 * p4
            dlambda = dlambda + f / dd
            if p4 * dlambda < 0:
                if p4 == 0:
                    raise MathError("Math error in return mapping")
                dlambda, istat, how = n(0), reset_istat, "reset"
                break
            f = c + Hd * (pstrain + p4 * dlambda)
            f = yd - G * dlambda + p3 * (J1 - K * p3 * dlambda) - p4 * f
            if abs(f) < n(TOL) * n(TOL):
                how = "converged"
                break
        pstrain = pstrain + p4 * dlambda
        d = (n(1) - G * dlambda / yd) * d
        J1 = J1 - K * p3 * dlambda
        s = np.array([d[0] + J1, d[1] + J1, d[2] + J1, d[3], d[4], d[5]], dtype=dt)
    if info is not None:
        info.update(reset=how == "reset", exit=how, iterations=it, residual=float(f))
    return s, istat, pstrain


def elastic_matrix(mat, dt):
    n = dt.type
    E, nu = n(mat.E), n(mat.nu)
    lam = E * nu / ((n(1) + nu) * (n(1) - n(2) * nu))
    mu = E / (n(2) * (n(1) + nu))
    D = np.zeros((6, 6), dtype=dt)
    D[:3, :3] = lam
    for i in range(3):
        D[i, i] = lam + n(2) * mu
        D[i + 3, i + 3] = mu
    return D


def flow_vector(mat, stress, info=None):
    """`a` of calElastoPlasticMatrix :49-108 for yield types 1 and 2.  info['branch']: 'edge' (| |sin 3 theta| - 1 | < 1e-8) or 'trig'."""
    s = np.asarray(stress)
    dt = s.dtype
    n = dt.type
    p3 = n(mat.plconst[2])
    J1 = s[0] + s[1] + s[2]
    d = np.array([s[0] - J1 / n(3), s[1] - J1 / n(3), s[2] - J1 / n(3), s[3], s[4], s[5]], dtype=dt)
    J2 = n(0.5) * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + (d[3] * d[3] + d[4] * d[4] + d[5] * d[5])
    dj2 = np.array([d[0], d[1], d[2], n(2) * d[3], n(2) * d[4], n(2) * d[5]], dtype=dt) / (n(2) * np.sqrt(J2))
    dj1 = np.array([1, 1, 1, 0, 0, 0], dtype=dt)
    if mat.kind == DRUCKER:
        return p3 * dj1 + dj2
    sita = sin3theta(J2, _j3(d))
    if info is not None:
        info["sin3"] = float(sita)
    if abs(abs(sita) - n(1)) < n(1.0e-8):
        C1, C2, C3 = n(0), np.sqrt(n(3)), n(0)
        if info is not None:
            info["branch"] = "edge"
    else:
        if abs(sita) > n(1):
            raise MathError("Math Error in Mohr-Coulomb calculation")
        if info is not None:
            info["branch"] = "trig"
        sita = np.arcsin(sita) / n(3)
        sf = np.sin(p3)
        C2 = np.cos(sita) * (n(1) * np.tan(sita) * np.tan(n(3) * sita) + sf * (np.tan(n(3) * sita) - np.tan(sita) / np.sqrt(n(3))))
        C1 = sf / n(3)
        C3 = np.sqrt(n(3)) * np.sin(sita) + np.cos(sita) * sf / (n(2) * J2 * np.cos(n(3) * sita))
    dj3 = np.array([d[1] * d[2] - d[4] * d[4] + J2 / n(3), d[0] * d[2] - d[5] * d[5] + J2 / n(3), d[0] * d[1] - d[3] * d[3] + J2 / n(3),
                    n(2) * (d[4] * d[5] - d[2] * d[3]), n(2) * (d[3] * d[5] - d[0] * d[4]), n(2) * (d[3] * d[4] - d[1] * d[5])], dtype=dt)
    return C1 * dj1 + C2 * dj2 + C3 * dj3


def elastoplastic_matrix(mat, stress, istat, fstat1, info=None):
    """calElastoPlasticMatrix :16-117, yield types 1 and 2 (linear hardening: calHardenCoeff = M_PLCONST2)"""
    s = np.asarray(stress)
    dt = s.dtype
    De = elastic_matrix(mat, dt)
    if istat == 0:
        return De
    a = flow_vector(mat, s, info)
    da = De @ a
    dum = dt.type(mat.plconst[1]) + da @ a
    return De - np.outer(da, da) / dum


def matl_matrix(mat, latch, stress, istat, fstat1):
    """MatlMatrix for the tangent (tet_nl_ref.matl_matrix with the two yield functions): the latch holds for every elastoplastic material"""
    if is_yield(mat):
        if not latch and istat != 0:
            return elastoplastic_matrix(mat, np.asarray(stress, dtype=np.float64), istat, fstat1)
        return R.elastic_matrix(mat.E, mat.nu)
    return T.matl_matrix(mat, latch, stress, istat, fstat1)


def point_update(mat, stress, plstrain, istat, fstat1):
    """BackwardEuler of a point of any elastoplastic material"""
    if is_yield(mat):
        return backward_euler(mat, np.asarray(stress, dtype=np.float64), plstrain, istat, fstat1)
    from oracle import pyoracle as po
    return po.backward_euler(mat, stress, plstrain, istat, fstat1)


# ---- the element routines ------------------------------------------------------------------------------------------------------------
def _initial_stress(gd, s):
    S = np.array([[s[0], s[3], s[5]], [s[3], s[1], s[4]], [s[5], s[4], s[2]]])
    return np.kron(gd @ S @ gd.T, np.eye(3))


def _voigt(m):
    return np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[1, 2], m[2, 0]])


def stf_c3(etype, ec, u, mat, latch, stress, istat, fstat):
    """STF_C3 (c3_nl_ref.stf_c3 with this module's MatlMatrix)"""
    flag = mat.nlgeom
    w = R.QUAD[etype][1]
    nn = R.NN[etype]
    elem = ec + u if flag == UPDATELAG else ec
    K = np.zeros((3 * nn, 3 * nn))
    for q, (gd, det) in enumerate(CN._points(etype, elem)):
        D = matl_matrix(mat, latch, stress[q], istat[q], fstat[q])
        if flag == UPDATELAG:
            D = D - T.geomat(stress[q])
        wg = w[q] * det
        B = R.b_matrix(gd)
        if flag == TOTALLAG:
            B = B + T._bl1(gd, T._gdisp(u, gd))
        K += (B.T @ (D @ B)) * wg
        if flag != INFINITE:
            K += _initial_stress(gd, stress[q]) * wg
    return K


def update_c3(etype, ec, u, ddu, mat, stress_bak, strain_bak, plstrain, istat, fstat):
    """UPDATE_C3 (c3_nl_ref.update_c3 with this module's BackwardEuler) -> qf, stress, strain, istat, fstat"""
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
    pts1 = CN._points(etype, elem1) if flag == UPDATELAG else None
    for q, (gd, det) in enumerate(CN._points(etype, elem)):
        g = T._gdisp(total, gd)
        de = np.array([g[0, 0], g[1, 1], g[2, 2], g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])
        if flag == TOTALLAG:
            H._green_lagrange(de, g)
        if flag != UPDATELAG:
            strain[q] = de
            stress[q] = D @ de
        else:
            rot = 0.5 * (g - g.T)
            strain[q] = strain_bak[q] + de
            sb = stress_bak[q]
            S = np.array([[sb[0], sb[3], sb[5]], [sb[3], sb[1], sb[4]], [sb[5], sb[4], sb[2]]])
            stress[q] = sb + T.real_default(D @ de) + _voigt(rot @ S - S @ rot)      # real(): static_LIB_3d.f90:718
        if mat.plastic:
            stress[q], istat[q], fstat[q] = point_update(mat, stress[q], plstrain[q], istat[q], fstat[q])
        B = R.b_matrix(gd)
        if flag == TOTALLAG:
            B = B + T._bl1(gd, g)
        elif flag == UPDATELAG:
            gd1, det = pts1[q]
            B = R.b_matrix(gd1)
        qf += (stress[q] @ B) * (w[q] * det)
    return qf, stress, strain, istat, fstat


def stf_c3d8bbar(ec, u, mat, latch, stress, istat, fstat):
    """STF_C3D8Bbar (static_LIB_C3D8.f90:23-198) in its three branches: (24, 24)"""
    flag = mat.nlgeom
    elem = ec + u if flag == UPDATELAG else ec
    bbar, _ = H._hex8_gderiv(elem, np.zeros(3))
    K = np.zeros((24, 24))
    for q in range(8):
        gd, det = H._hex8_gderiv(elem, H.HEX8_POINTS[q])
        D = matl_matrix(mat, latch, stress[q], istat[q], fstat[q])
        if flag == UPDATELAG:
            D = D - T.geomat(stress[q])
        B = H._bbar_matrix(gd, bbar)
        if flag == TOTALLAG:
            B = B + T._bl1(gd, u.T @ gd)
        K += (B.T @ (D @ B)) * det
        if flag != INFINITE:
            K += _initial_stress(gd, stress[q]) * det
    return K


def update_c3d8bbar(ec, u, ddu, mat, stress_bak, strain_bak, plstrain, istat, fstat):
    """Update_C3D8Bbar (static_LIB_C3D8.f90:203-547) in its three branches -> qf (24), stress, strain, istat, fstat.  UPDATELAG
    (:255-260, :405-429): mid-point configuration, strain_bak + dstrain, stress_bak + D dstrain + (rot S - S rot) - 3 vol0 stress_bak
    (no real() here), internal force on the end configuration (:460-470)."""
    flag = mat.nlgeom
    elem, total = ec, u + ddu
    if flag == UPDATELAG:
        elem = (0.5 * ddu + u) + ec
        elem1 = (ddu + u) + ec
        total = ddu
    D = R.elastic_matrix(mat.E, mat.nu)
    bbar, _ = H._hex8_gderiv(elem, np.zeros(3))
    dd = total.T @ bbar
    vol0 = (dd[0, 0] + dd[1, 1] + dd[2, 2]) / 3.0
    if flag == UPDATELAG:
        bbar1, _ = H._hex8_gderiv(elem1, np.zeros(3))
    qf, stress, strain = np.zeros(24), np.zeros((8, 6)), np.zeros((8, 6))
    istat, fstat = np.array(istat, dtype=np.int32).copy(), np.array(fstat, dtype=np.float64).copy()
    for q in range(8):
        gd, det = H._hex8_gderiv(elem, H.HEX8_POINTS[q])
        g = total.T @ gd
        dvol = vol0 - (g[0, 0] + g[1, 1] + g[2, 2]) / 3.0
        de = np.array([g[0, 0] + dvol, g[1, 1] + dvol, g[2, 2] + dvol, g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]])
        if flag == TOTALLAG:
            H._green_lagrange(de, g)
        if flag != UPDATELAG:
            strain[q] = de
            stress[q] = D @ de
        else:
            rot = 0.5 * (g - g.T)
            strain[q] = strain_bak[q] + de
            sb = stress_bak[q]
            S = np.array([[sb[0], sb[3], sb[5]], [sb[3], sb[1], sb[4]], [sb[5], sb[4], sb[2]]])
            stress[q] = sb + D @ de + _voigt(rot @ S - S @ rot) - sb * 3.0 * vol0
        if mat.plastic:
            stress[q], istat[q], fstat[q] = point_update(mat, stress[q], plstrain[q], istat[q], fstat[q])
        B = H._bbar_matrix(gd, bbar)
        if flag == TOTALLAG:
            B = B + T._bl1(gd, g)
        elif flag == UPDATELAG:
            gd1, det = H._hex8_gderiv(elem1, H.HEX8_POINTS[q])
            B = H._bbar_matrix(gd1, bbar1)
        qf += (stress[q] @ B) * det
    return qf, stress, strain, istat, fstat


class Model(H.Model):
    """fstr_solid of one mesh of one of the six solid types whose sections are Mohr-Coulomb, Drucker-Prager, Mises or ELASTIC:
    hyper_ref.Model's state and steps (dense solve, blocks of collapsed hexahedra added up) on this module's element routines."""

    def element_tangents(self):
        u = (self.unode + self.dunode).reshape(-1, 3)
        s = self.st
        out = []
        for e, nd in enumerate(self.conn - 1):
            a = (self.coord[nd], u[nd], self.mat(e), self.latch, s["stress"][e], s["istat"][e], s["fstat"][e])
            out.append(stf_c3d8bbar(*a) if self.etype == 361 else stf_c3(self.etype, *a))
        return np.array(out)

    def element_update(self, order=None):
        u, du = self.unode.reshape(-1, 3), self.dunode.reshape(-1, 3)
        s = self.st
        qf = np.zeros((self.conn.shape[0], 3 * H.NODES[self.etype]))
        for e, nd in enumerate(self.conn - 1):
            a = (self.coord[nd], u[nd], du[nd], self.mat(e), s["stress_bak"][e], s["strain_bak"][e], s["plstrain"][e], s["istat"][e],
                 s["fstat"][e])
            r = update_c3d8bbar(*a) if self.etype == 361 else update_c3(self.etype, *a)
            qf[e], s["stress"][e], s["strain"][e], s["istat"][e], s["fstat"][e] = r
        if any(m.plastic for m in self.mats):
            self.latch = 1
        return qf


summary = H.summary
within_1e4 = H.within_1e4


# ---- the reference program's own runs: tests/golden/yield_decks.npz (tests/golden/make_yield_golden.py) ---------------------------------
DECK_STRAIN, DECK_SUBSTEPS, DECK_CONVERG = 0.005, 3, 1.0e-3
DECK_FAMILIES = {"drucker": lambda: drucker_prager(206900.0, 0.29, 300.0, 20.0, 2000.0), "mohr": lambda: mohr_coulomb(206900.0, 0.29, 300.0, 5.0, 20000.0)}
# name -> (etype, cube size n, MAT1 of scripts/fistr1_cube_deck.py --nl-material, two sections): the sizes of hyper_ref's decks
GOLDEN_DECKS = {"y%d_%s" % (et, fam): (et, n, fam, False) for et, n in H._SIZES.items() for fam in ("drucker", "mohr")}
GOLDEN_DECKS.update({"y361_drucker_two": (361, 2, "drucker", True), "y342_mohr_two": (342, 1, "mohr", True),
                     "y352_drucker_two": (352, 1, "drucker", True), "y362_mohr_two": (362, 2, "mohr", True)})


def golden_deck(name):
    """(mesh, materials, elem_mat or None, bc) of one recorded cube deck, as fistr1_cube_deck.py writes it: z = 0 clamped, the top face
    moved by 0.5 % in z and a fifth of that in x; with two sections the second half of the elements is Mises BILINEAR."""
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    from oracle.refrun import Material as RefMaterial
    et, n, fam, two = GOLDEN_DECKS[name]
    m = CubeMesh(n) if et == 361 else solid_mesh(n, et)
    m.etype = et
    mats, em = DECK_FAMILIES[fam](), None
    if two:
        mats = [mats, RefMaterial(206900.0, 0.29, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=UPDATELAG)]
        em = np.where(np.arange(m.n_elem) < m.n_elem // 2, 1, 2).astype(np.int32)
    node, dof, val = m.dirichlet()
    t = m.top_nodes
    bc = (np.concatenate([node, t, t]).astype(np.int32),
          np.concatenate([dof, np.full(t.size, 3), np.full(t.size, 1)]).astype(np.int32),
          np.concatenate([val, np.full(t.size, DECK_STRAIN * n), np.full(t.size, 0.2 * DECK_STRAIN * n)]))
    return m, mats, em, bc


# The reference's own examples/static/1elem/{drucker,mohr,mohrshear}.cnt (committed copies: tests/golden/decks/yield1/): one unit
# TYPE=361 cube, E = 1e5, nu = 0, c = 500, H = 0; Drucker-Prager with phi = 20 degrees, Mohr-Coulomb with phi = 0; one sub-step.
# drucker / mohr pull the face x = 1 by 0.012 with the minimal supports of uniaxial tension: every point ends on the
# |sin 3 theta| = 1 branch with two tied principal stresses.  mohrshear (the tree holds no mesh of that name: it runs on mohr.msh,
# the mesh its node numbers fit) clamps the face y = 0 and moves the face y = 1 by 0.016 in x.
ONE_ELEM_COORD = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
ONE_ELEM_CONN = np.arange(1, 9, dtype=np.int32).reshape(1, 8)
_TENSION_BC = [(1, 1), (1, 2), (1, 3), (4, 1), (4, 3), (5, 1), (5, 2), (8, 1)]
ONE_ELEM_DECKS = {
    "1elem_drucker": ("drucker.msh", "drucker.cnt", lambda: drucker_prager(1.0e5, 0.0, 500.0, 20.0, 0.0),
                      _TENSION_BC + [(2, 1), (3, 1), (6, 1), (7, 1)], [0.0] * 8 + [0.012] * 4),
    "1elem_mohr": ("mohr.msh", "mohr.cnt", lambda: mohr_coulomb(1.0e5, 0.0, 500.0, 0.0, 0.0),
                   _TENSION_BC + [(2, 1), (3, 1), (6, 1), (7, 1)], [0.0] * 8 + [0.012] * 4),
    "1elem_mohrshear": ("mohr.msh", "mohrshear.cnt", lambda: mohr_coulomb(1.0e5, 0.0, 500.0, 0.0, 0.0),
                        [(nd, d) for nd in (1, 2, 5, 6) for d in (1, 2, 3)] + [(nd, 1) for nd in (3, 4, 7, 8)] + [(nd, 2) for nd in (3, 4, 7, 8)],
                        [0.0] * 12 + [0.016] * 4 + [0.0] * 4),
}
ONE_ELEM_CONVERG = 1.0e-3          # the default of !STEP (init_stepInfo, m_step.f90:77)


def one_elem_deck(name):
    """(material, bc) of one of the reference's 1elem decks"""
    _, _, mat, dofs, vals = ONE_ELEM_DECKS[name]
    bc = (np.array([d[0] for d in dofs], dtype=np.int32), np.array([d[1] for d in dofs], dtype=np.int32), np.array(vals, dtype=np.float64))
    return mat(), bc


# ---- inputs of the GPU comparisons ------------------------------------------------------------------------------------------------------
# hyper_ref.gpu_mesh's distorted meshes, zero history, smooth displacement fields unode / dunode (hyper_ref.random_displacement) of
# relative size GPU_AMP: strains of a few per cent on E = 20000, stresses of the order 1e3 -- large against the absolute 1e-3 of the
# return's tests and against the 1e-10 at which eigen3 stops sweeping.  The cohesion c is what puts the yield surface through the
# cloud of trial stresses: f is linear in c, so for every (element type, family) the seed and c below were chosen on the CPU such
# that, under all three NLGEOM flags, the margins of tests/test_yield_ref.py hold at every point (no point is left out anywhere).
GPU_E, GPU_NU, GPU_PHI, GPU_H, GPU_AMP = 20000.0, 0.3, 25.0, 400.0, 0.02
GPU_CASES = {(361, "drucker"): (8, 228.0), (361, "mohr"): (19, 337.0), (341, "drucker"): (8, 232.0), (341, "mohr"): (19, 350.0),
             (342, "drucker"): (8, 235.0), (342, "mohr"): (76, 245.0), (351, "drucker"): (8, 232.0), (351, "mohr"): (19, 350.0),
             (352, "drucker"): (8, 230.0), (352, "mohr"): (128, 239.0), (362, "drucker"): (8, 220.0),
             (362, "mohr"): (128, 228.0)}          # (etype, family) -> (seed, c), from search_gpu_case
# The elastoplastic cases of tests/nl_shapes.py, on its meshes: (mesh name of nl_shapes.mesh_of, which) -> (seed, c).  "all":
# Drucker-Prager on every element, from search_gpu_case(..., mesh=) over seeds 1..39; "colour1": the same with elems= the 48 elements
# of the mesh's second colour (no seed of 1..39 meets the margins at all 2744 points of the 7^3 cube); "mohr": Mohr-Coulomb, from
# search_gpu_case(etype, "mohr", mesh=) (gpu352 / gpu362 are hyper_ref.gpu_mesh: GPU_CASES' values); "mises": seed 8 and the yield
# stress of search_mises_stress on the trial stresses of the case's three sections.
SHAPE_CASES = {("cube4", "all"): (8, 234.0), ("cubedup4", "all"): (8, 226.0), ("cube7", "colour1"): (8, 219.0), ("3414", "all"): (8, 233.0),
               ("3423", "all"): (8, 229.0), ("3514", "all"): (8, 233.0), ("gpu352", "all"): (8, 230.0), ("gpu362", "all"): (8, 220.0),
               # F-bar, from fbar_ref.search_plastic_case(..., mesh=, elems=) on the F-bar trial stresses (INFINITE and TOTALLAG)
               ("cube4", "fbar"): (1, 412.0), ("cube5", "fbar colours 1, 2"): (1, 414.0), ("cube4", "fbar mohr"): (1, 426.0),
               ("cube4", "fbar mises"): (8, 508.0),
               ("cube4", "mohr"): (19, 356.0), ("3414", "mohr"): (71, 420.0), ("3423", "mohr"): (128, 250.0), ("3514", "mohr"): (71, 420.0),
               ("gpu352", "mohr"): (128, 239.0), ("gpu362", "mohr"): (128, 228.0),
               ("cube7", "mises"): (8, 524.0), ("3414", "mises"): (8, 521.0), ("3423", "mises"): (8, 524.0), ("3514", "mises"): (8, 523.0),
               ("gpu352", "mises"): (8, 523.0), ("gpu362", "mises"): (8, 521.0)}


def gpu_material(family, nlgeom, c):
    f = drucker_prager if family == "drucker" else mohr_coulomb
    return f(GPU_E, GPU_NU, c, GPU_PHI, GPU_H, nlgeom=nlgeom)


def gpu_case(etype, family, nlgeom, seed=None, c=None, mesh=None):
    """(mesh, material, unode, dunode) of one GPU comparison.  mesh: another mesh of the type than hyper_ref.gpu_mesh (seed and c
    are then the caller's, SHAPE_CASES)"""
    if seed is None:
        seed, c = GPU_CASES[(etype, family)]
    m = H.gpu_mesh(etype) if mesh is None else mesh
    unode, dunode = H.random_displacement(m.coord, seed, GPU_AMP)
    return m, gpu_material(family, nlgeom, c), unode, dunode


def trial_stresses(etype, family, nlgeom, seed=None, c=None, mesh=None):
    """The trial stresses of gpu_case's first update: the same update with a cohesion no point reaches"""
    m, _, unode, dunode = gpu_case(etype, family, nlgeom, seed, c, mesh)
    ref = Model(etype, m.coord, m.conn, gpu_material(family, nlgeom, 1.0e12))
    ref.unode[:], ref.dunode[:] = unode, dunode
    ref.element_update()
    assert not ref.st["istat"].any()
    return ref.st["stress"].reshape(-1, 6)


def point_report(mat, trial):
    """What the margin checks read, per trial stress: f, istat, the `dlambda < 0` reset, sin 3 theta of the trial and of the returned
    stress, the smallest gap between principal stresses over the largest magnitude; and the returned stress, fstat, tangent."""
    rep = dict(f=[], istat=[], reset=[], sin3=[], sin3_ret=[], gap=[], stress=[], fstat=[], tangent=[])
    for s in trial:
        info = {}
        out, ist, fs = backward_euler(mat, s, 0.0, 0, 0.0, info)
        tinfo = {}
        D = elastoplastic_matrix(mat, out, ist, fs, tinfo)
        p = np.sort(np.linalg.eigvalsh(np.array([[s[0], s[3], s[5]], [s[3], s[1], s[4]], [s[5], s[4], s[2]]])))
        rep["f"].append(info["f"]); rep["istat"].append(ist); rep["reset"].append(info["reset"])
        J1 = s[0] + s[1] + s[2]
        d = np.array([s[0] - J1 / 3, s[1] - J1 / 3, s[2] - J1 / 3, s[3], s[4], s[5]])
        J2 = 0.5 * (d[:3] @ d[:3]) + d[3:] @ d[3:]
        rep["sin3"].append(float(sin3theta(J2, _j3(d))))
        rep["sin3_ret"].append(tinfo.get("sin3", 0.0))
        rep["gap"].append(float(min(p[1] - p[0], p[2] - p[1]) / np.abs(p).max()))
        rep["stress"].append(out); rep["fstat"].append(fs); rep["tangent"].append(D)
    return {k: np.array(v) for k, v in rep.items()}


def margins_hold(mat, rep):
    """The conditions that keep every point off a branch edge (tests/test_yield_ref.py asserts them one by one)"""
    ok = np.all(np.abs(np.abs(rep["f"]) - TOL) >= 10 * TOL) and not rep["reset"].any()
    ok = ok and rep["istat"].mean() >= 0.25 and (1 - rep["istat"]).mean() >= 0.10
    if mat.kind == MOHR:
        ok = ok and np.abs(rep["sin3"]).max() <= 0.95 and np.abs(rep["sin3_ret"]).max() <= 0.95 and rep["gap"].min() >= 1.0e-6
    return bool(ok)


def search_gpu_case(etype, family, seeds=range(1, 200), mesh=None, elems=None):
    """How GPU_CASES (and, with a mesh, SHAPE_CASES) was filled: the first seed, and the cohesion (a round number near the 45th
    percentile of the points' critical cohesions, then lower ones), at which the margins hold under all three flags.  elems: at the
    points of those elements of the mesh only."""
    for seed in seeds:
        trial = {g: trial_stresses(etype, family, g, seed, 1.0, mesh) for g in (INFINITE, TOTALLAG, UPDATELAG)}
        if elems is not None:
            trial = {g: t.reshape(mesh.conn.shape[0], -1, 6)[elems].reshape(-1, 6) for g, t in trial.items()}
        probe = gpu_material(family, INFINITE, 0.0)
        k = np.cos(probe.plconst[2]) if family == "mohr" else probe.plconst4
        crit = np.array([cal_yield_func(probe, s, 0.0) for s in trial[INFINITE]]) / k
        for q in (45, 40, 50, 35, 55, 30, 60):
            c = float(np.round(np.percentile(crit, q), 0))
            if c <= 1.0:
                continue
            if all(margins_hold(gpu_material(family, g, c), point_report(gpu_material(family, g, c), trial[g])) for g in trial):
                return seed, c
    raise RuntimeError("no case found")


def branch_case(generic):
    """(material, dunode) of the two one-element inputs that reach the two branches of calElastoPlasticMatrix's Mohr-Coulomb case: the
    unit cube with nu = 0, INFINITE, displacement along x only.
    generic: u_x = 0.012 x + 0.009 y + 0.004 z, c = 500: every point yields and the returned stress has |sin 3 theta| < 0.95.
    not generic: u_x = 0.012 x, an exactly uniaxial stress, | |sin 3 theta| - 1 | < 1e-8.  A return leaves that edge (the first of the
    two tied minimum principal stresses is raised, the other is not), so the cohesion is out of reach here: the update leaves the
    uniaxial trial stress, and the comparison marks the points as yielded by hand (istat = 1) before it asks for the tangent."""
    mat = mohr_coulomb(1.0e5, 0.0, 500.0 if generic else 1.0e9, 20.0, 1000.0, nlgeom=INFINITE)
    u = np.zeros((8, 3))
    x = ONE_ELEM_COORD
    u[:, 0] = 0.012 * x[:, 0] + ((0.009 * x[:, 1] + 0.004 * x[:, 2]) if generic else 0.0)
    return mat, u.ravel()


# A stress at which calElastoPlasticMatrix stops with `Math Error in Mohr-Coulomb calculation`.  |sin 3 theta| <= 1 holds for every
# real stress, so only the arithmetic can break it: at this uniaxial magnitude J2**1.5 and J3 are subnormal (they round to 2 and 1 units of
# 2**-1074), their quotient is 0.5 where 2 / (3 sqrt 3) = 0.385 is the bound, and sita = -3 sqrt(3) / 4 = -1.299.
STOP_STRESS = np.array([3.7e-108, 0.0, 0.0, 0.0, 0.0, 0.0])


# ---- mixed sections: a Drucker-Prager section (updated Lagrange) beside a Mises or an ELASTIC one ---------------------------------------
# The elements are dealt out irregularly (mixed_deal); section 1 is Drucker-Prager, section 2 Mises BILINEAR (H = GPU_H, updated
# Lagrange) or ELASTIC total Lagrange, all on GPU_E / GPU_NU.  Seed, cohesion and Mises yield stress per element type were chosen on
# the CPU (search_mixed_case) so that the Drucker-Prager SUBSET meets the margins and the shares of the single-material cases (a
# quarter plastic, a tenth elastic), and so that every Mises point is at least 10 tol away from the |f| < tol edge of its own return,
# with at least a tenth of them on either side.  (A Mises return with linear hardening cannot end through `dlambda < 0`: f > tol
# there and the denominator 3 G + H is positive.)
MIXED_CASES = {361: (1, 153.0, 497.0), 342: (1, 161.0, 479.0), 352: (1, 163.0, 486.0)}      # etype -> (seed, c, Mises yield stress), from search_mixed_case


def mixed_deal(n_elem):
    return (1 + (np.arange(n_elem) * 7 // 3) % 2).astype(np.int32)


def mixed_case(etype, other):
    """(mesh, [Drucker-Prager, second material], elem_mat, unode, dunode); other: 'mises' or 'elastic'"""
    from oracle.refrun import Material as RefMaterial
    seed, c, sy = MIXED_CASES[etype]
    m, mat, unode, dunode = gpu_case(etype, "drucker", UPDATELAG, seed, c)
    second = (RefMaterial(GPU_E, GPU_NU, plastic=True, harden=0, plconst=(sy, GPU_H, 0.0), nlgeom=UPDATELAG) if other == "mises"
              else RefMaterial(GPU_E, GPU_NU, nlgeom=TOTALLAG))
    return m, [mat, second], mixed_deal(m.n_elem), unode, dunode


def mises_margins_hold(trials, sy):
    """every Mises point 10 tol away from the |f| < tol edge of its return, a tenth of each section's points on either side"""
    return all(bool(np.all(np.abs(np.abs(mises_f(t, sy)) - TOL) >= 10 * TOL)) and (mises_f(t, sy) > 0).mean() >= 0.10
               and (mises_f(t, sy) < 0).mean() >= 0.10 for t in trials)


def search_mises_stress(trials):
    """How the yield stresses of SHAPE_CASES were filled: the round number nearest the median Mises stress of the sections' trial
    stresses (then the next ones on either side) at which mises_margins_hold"""
    sy0 = float(np.round(np.median(T.mises(np.concatenate(trials))), 0))
    for d in range(0, 200):
        for sy in ((sy0 + d, sy0 - d) if d else (sy0,)):
            if sy > 1.0 and mises_margins_hold(trials, sy):
                return sy
    raise RuntimeError("no yield stress found")


def mises_f(trial, sy):
    """f of the Mises return (Elastoplastic.f90:328) at zero plastic strain, per trial stress"""
    return T.mises(trial) - sy


def mixed_report(etype, seed=None, c=None, sy=None):
    """(Drucker-Prager material, point_report of the Drucker-Prager subset, Mises f of the other subset).  Both sections are updated
    Lagrange on the same elastic constants, so the trial stresses are those of the single-material update."""
    if seed is None:
        seed, c, sy = MIXED_CASES[etype]
    m = H.gpu_mesh(etype)
    trial = trial_stresses(etype, "drucker", UPDATELAG, seed, 1.0).reshape(m.n_elem, -1, 6)
    first = mixed_deal(m.n_elem) == 1
    mat = gpu_material("drucker", UPDATELAG, c)
    return mat, point_report(mat, trial[first].reshape(-1, 6)), mises_f(trial[~first].reshape(-1, 6), sy)


def mixed_margins_hold(mat, rep, fm):
    return (margins_hold(mat, rep) and bool(np.all(np.abs(np.abs(fm) - TOL) >= 10 * TOL)) and (fm > 0).mean() >= 0.10
            and (fm < 0).mean() >= 0.10)


def search_mixed_case(etype, seeds=range(1, 200)):
    """How MIXED_CASES was filled (as search_gpu_case, on the Drucker-Prager subset of the deal)"""
    m = H.gpu_mesh(etype)
    first = mixed_deal(m.n_elem) == 1
    probe = gpu_material("drucker", UPDATELAG, 0.0)
    for seed in seeds:
        trial = trial_stresses(etype, "drucker", UPDATELAG, seed, 1.0).reshape(m.n_elem, -1, 6)
        crit = np.array([cal_yield_func(probe, s, 0.0) for s in trial[first].reshape(-1, 6)]) / probe.plconst4
        for q in (50, 45, 55, 40, 60, 35, 65):
            c = float(np.round(np.percentile(crit, q), 0))
            if c <= 1.0:
                continue
            sy = float(np.round(np.median(T.mises(trial[~first].reshape(-1, 6))), 0))
            mat, rep, fm = mixed_report(etype, seed, c, sy)
            if mixed_margins_hold(mat, rep, fm):
                return seed, c, sy
    raise RuntimeError("no case found")
