"""Numpy restatement of the reference's F-bar hexahedron (TYPE=361, !SECTION FORM361=FBAR) in the nonlinear static loop:
STF_C3D8Fbar (fistr1/src/lib/static_LIB_Fbar.f90:26-336) with `u` present and Update_C3D8Fbar (:341-769) without temperatures, in
their INFINITE and TOTALLAG branches, with the arrays the reference has (B, B1, B2 (6, 24), BN (9, 24), Smat (9, 9), gderiv2_ave
(24, 24): clarity over speed).  The material point is the one the other restatements use: tet_nl_ref / oracle.pyoracle (ELASTIC,
Mises and the latch), hyper_ref (Neo-Hooke, Mooney-Rivlin, Arruda-Boyce: tangent from the stored strain, stress from the total
strain), yield_ref (Mohr-Coulomb, Drucker-Prager).

The UPDATELAG branch is not restated, because the reference does not define it: Update_C3D8Fbar builds `rot` there (:600-602) from
the local array Fbar, declared at :389 and assigned only in the TOTALLAG branch (:556).

Model is hyper_ref.Model (state, dense Newton steps, blocks of collapsed hexahedra added up) on these routines; MixedModel is
mixed_nl_ref.Model whose 361 groups with elemopt 4 go through them, beside B-bar 361 groups and the other five types.

The element routines work in the dtype of the coordinates and displacements they are given (float64, or np.longdouble for the
sensitivity check of tests/test_fbar_ref.py; elastoplastic materials: float64 only, their return mapping is the C oracle's).
"""
import numpy as np

import c3_ref as R
import hyper_ref as H
import mixed_nl_ref as MN
import tet_nl_ref as T
import yield_ref as Y
from tet_nl_ref import INFINITE, TOTALLAG, UPDATELAG  # noqa: F401

ELEMOPT_BBAR, ELEMOPT_FBAR = 2, 4


class TooSmall(ArithmeticError):
    """`stop 'Error in Update_C3D8Fbar: too small element volume'` / `too small average jacob` (:114-122, :449-457)"""


def _is_hyper(mat):
    return H.kind_of(mat) >= H.MOONEY and not Y.is_yield(mat)


def determinant33(m):
    """Determinant33 (utilities.f90)"""
    return (m[0, 0] * m[1, 1] * m[2, 2] + m[0, 1] * m[1, 2] * m[2, 0] + m[0, 2] * m[1, 0] * m[2, 1]
            - m[0, 2] * m[1, 1] * m[2, 0] - m[0, 1] * m[1, 0] * m[2, 2] - m[0, 0] * m[1, 2] * m[2, 1])


def _gderiv(ec, lc):
    """getGlobalDeriv of the 8-node hexahedron in the dtype of ec -> gderiv (8, 3), det"""
    dt = ec.dtype
    one, p = dt.type(1), [dt.type(v) for v in lc]
    dN = np.array([[dt.type(0.125) * sx * (one + sy * p[1]) * (one + sz * p[2]), dt.type(0.125) * sy * (one + sx * p[0]) * (one + sz * p[2]),
                    dt.type(0.125) * sz * (one + sx * p[0]) * (one + sy * p[1])] for sx, sy, sz in R.HEX_VERTS], dtype=dt)
    det, inv = R.jacobian(ec, dN)
    return dN @ inv, det


def _b0(gd):
    """BL0 (:151-162), c3_ref.b_matrix in the dtype of gd"""
    B = np.zeros((6, 24), dtype=gd.dtype)
    B[0, 0::3] = gd[:, 0]
    B[1, 1::3] = gd[:, 1]
    B[2, 2::3] = gd[:, 2]
    B[3, 0::3] = gd[:, 1]; B[3, 1::3] = gd[:, 0]
    B[4, 1::3] = gd[:, 2]; B[4, 2::3] = gd[:, 1]
    B[5, 0::3] = gd[:, 2]; B[5, 2::3] = gd[:, 0]
    return B


def _bl1(gd, F):
    """BL1 (:185-205), tet_nl_ref._bl1 in the dtype of gd; F = gdispderiv"""
    B1 = np.zeros((6, 24), dtype=gd.dtype)
    for c in range(3):
        B1[0, c::3] = F[c, 0] * gd[:, 0]
        B1[1, c::3] = F[c, 1] * gd[:, 1]
        B1[2, c::3] = F[c, 2] * gd[:, 2]
        B1[3, c::3] = F[c, 1] * gd[:, 0] + F[c, 0] * gd[:, 1]
        B1[4, c::3] = F[c, 1] * gd[:, 2] + F[c, 2] * gd[:, 1]
        B1[5, c::3] = F[c, 2] * gd[:, 0] + F[c, 0] * gd[:, 2]
    return B1


def _elastic_matrix(mat, dt):
    """calElasticMatrix in dt (tet_ref.elastic_matrix)"""
    E, nu, one, two = dt.type(mat.E), dt.type(mat.nu), dt.type(1), dt.type(2)
    D = np.zeros((6, 6), dtype=dt)
    D[:3, :3] = E * nu / (one - two * nu) / (one + nu)
    D[[0, 1, 2], [0, 1, 2]] = E * (one - nu) / (one - two * nu) / (one + nu)
    D[[3, 4, 5], [3, 4, 5]] = E / (one + nu) * dt.type(0.5)
    return D


def averages(ec, u, flag, second=False):
    """The volume averages over the eight points (:82-122, :418-457) -> V0, jacob_ave, Jratio (8), gderiv1_ave (8, 3) and, with
    `second`, gderiv2_ave (24, 24).  u (8, 3): the displacement the deformation gradient is taken from."""
    dt = ec.dtype
    V0 = jave = dt.type(0)
    jr = np.ones(8, dtype=dt)
    g1ave, g2ave = np.zeros((8, 3), dtype=dt), np.zeros((24, 24), dtype=dt)
    third = dt.type(1) / dt.type(3)
    for q in range(8):
        gd, det = _gderiv(ec, H.HEX8_POINTS[q])
        wg = det
        if flag == INFINITE:
            jacob, g1 = dt.type(1), gd
        else:
            jacob = determinant33(np.eye(3, dtype=dt) + u.T @ gd)
            jr[q] = jacob ** (-third)
            g1, _ = _gderiv(ec + u, H.HEX8_POINTS[q])
            if second:
                pq = np.einsum("pi,qj->piqj", g1, g1).reshape(24, 24)
                g2ave += jacob * wg * (pq - np.einsum("qi,pj->piqj", g1, g1).reshape(24, 24))
        g1ave += jacob * wg * g1
        V0 += wg
        jave += jacob * wg
    if not abs(V0) > 1.0e-12:
        raise TooSmall("too small element volume")
    if abs(jave) < 1.0e-12:
        raise TooSmall("too small average jacob")
    jave = jave / V0
    jr = jave ** third * jr
    return V0, jave, jr, g1ave / (V0 * jave), g2ave / (V0 * jave)


def _fbar_strain(Fbar):
    half, one = Fbar.dtype.type(0.5), Fbar.dtype.type(1)
    return np.array([half * (Fbar[:, 0] @ Fbar[:, 0] - one), half * (Fbar[:, 1] @ Fbar[:, 1] - one), half * (Fbar[:, 2] @ Fbar[:, 2] - one),
                     Fbar[:, 0] @ Fbar[:, 1], Fbar[:, 1] @ Fbar[:, 2], Fbar[:, 2] @ Fbar[:, 0]], dtype=Fbar.dtype)


def _bl2(e, Z):
    """B2 of the total Lagrange branch (:214-223, :717-726): row r is c(r) Z over every node"""
    two, one = e.dtype.type(2), e.dtype.type(1)
    c = np.array([two * e[0] + one, two * e[1] + one, two * e[2] + one, two * e[3], two * e[4], two * e[5]], dtype=e.dtype)
    return np.outer(c, Z.ravel())


def _bl_infinite(gd, g1ave):
    """BL0 + BL2 of the INFINITE branch (:165-177, :675-689): the dilatational rows get (gderiv1_ave - gderiv) / 3"""
    B = _b0(gd)
    h = (g1ave - gd) / gd.dtype.type(3)
    for r in range(3):
        for c in range(3):
            B[r, c::3] += h[:, c]
    return B


def _material_matrix(mat, latch, strain, stress, istat, fstat, dt):
    if _is_hyper(mat):
        return H.tangent(mat, np.asarray(strain, dtype=dt))
    if mat.plastic and not latch and istat != 0:
        return Y.matl_matrix(mat, latch, stress, istat, fstat)
    return _elastic_matrix(mat, dt)


def stf_c3d8fbar(ec, u, mat, latch, strain, stress, istat, fstat):
    """STF_C3D8Fbar with flag INFINITE / TOTALLAG: (24, 24).  u (8, 3) = unode + dunode; strain, stress (8, 6), istat, fstat (8,):
    the points' stored values."""
    flag = mat.nlgeom
    if flag == UPDATELAG:
        raise ValueError("Update_C3D8Fbar's UPDATELAG branch reads Fbar unassigned (static_LIB_Fbar.f90:600-602): not restated")
    dt = np.result_type(ec, u)
    ec, u = np.asarray(ec, dtype=dt), np.asarray(u, dtype=dt)
    stress = np.asarray(stress, dtype=dt)
    three, I3 = dt.type(3), np.eye(3, dtype=dt)
    _, _, jr, g1ave, g2ave = averages(ec, u, flag, second=True)
    K = np.zeros((24, 24), dtype=dt)
    for q in range(8):
        gd, det = _gderiv(ec, H.HEX8_POINTS[q])
        D = _material_matrix(mat, latch, strain[q], stress[q], istat[q], fstat[q], dt)
        wg = det
        if flag == INFINITE:
            B = _bl_infinite(gd, g1ave)
            K += (B.T @ (D @ B)) * wg
            continue
        g = u.T @ gd
        Fbar = jr[q] * (I3 + g)
        g1, _ = _gderiv(ec + u, H.HEX8_POINTS[q])
        e = _fbar_strain(Fbar)
        Z = (g1ave - g1) / three
        B = jr[q] * jr[q] * (_b0(gd) + _bl1(gd, g)) + _bl2(e, Z)
        K += (B.T @ (D @ B)) * wg
        # initial stress matrix (1): dFbar*dFbar*Stress (:253-302)
        s = stress[q]
        coeff, sff = jr[q], s @ e
        BN = np.zeros((9, 24), dtype=dt)
        for j in range(8):
            for d in range(3):
                for i in range(3):
                    BN[3 * d + i, 3 * j + i] = coeff * gd[j, d]
                    BN[3 * d + i, 3 * j:3 * j + 3] += Fbar[i, d] * Z[j]
        S = np.array([[s[0], s[3], s[5]], [s[3], s[1], s[4]], [s[5], s[4], s[2]]], dtype=dt)
        Smat = np.kron(S, I3)
        K += (BN.T @ (Smat @ BN)) * wg
        # initial stress matrix (2): d(dFbar)*Stress (:304-330)
        FS = Fbar @ S
        GFS = coeff * gd @ FS.T                       # (8, 3): GFS of every node
        for i in range(8):
            for j in range(8):
                dd = np.outer(Z[i], Z[j])
                dd = dd + (g2ave[3 * i:3 * i + 3, 3 * j:3 * j + 3] - np.outer(g1ave[i], g1ave[j])) / three
                dd = dd + np.outer(g1[j], g1[i]) / three            # gderiv1(i,q) gderiv1(j,p) at (p, q)
                dd = sff * dd + np.outer(Z[i], GFS[j]) + np.outer(GFS[i], Z[j])
                K[3 * i:3 * i + 3, 3 * j:3 * j + 3] += dd * wg
    return K


def update_c3d8fbar(ec, u, ddu, mat, plstrain, istat, fstat):
    """Update_C3D8Fbar with flag INFINITE / TOTALLAG -> qf (24), stress (8, 6), strain (8, 6), istat, fstat"""
    flag = mat.nlgeom
    if flag == UPDATELAG:
        raise ValueError("Update_C3D8Fbar's UPDATELAG branch reads Fbar unassigned (static_LIB_Fbar.f90:600-602): not restated")
    dt = np.result_type(ec, u, ddu)
    ec, total = np.asarray(ec, dtype=dt), np.asarray(u, dtype=dt) + np.asarray(ddu, dtype=dt)
    three, I3 = dt.type(3), np.eye(3, dtype=dt)
    _, _, jr, g1ave, _ = averages(ec, total, flag)
    qf, stress, strain = np.zeros(24, dtype=dt), np.zeros((8, 6), dtype=dt), np.zeros((8, 6), dtype=dt)
    istat, fstat = np.array(istat, dtype=np.int32).copy(), np.array(fstat, dtype=np.float64).copy()
    for q in range(8):
        gd, det = _gderiv(ec, H.HEX8_POINTS[q])
        g = total.T @ gd
        if flag == INFINITE:
            dvol = total[:, 0] @ g1ave[:, 0] + total[:, 1] @ g1ave[:, 1] + total[:, 2] @ g1ave[:, 2]
            dvol = (dvol - (g[0, 0] + g[1, 1] + g[2, 2])) / three
            de = np.array([g[0, 0] + dvol, g[1, 1] + dvol, g[2, 2] + dvol, g[0, 1] + g[1, 0], g[1, 2] + g[2, 1], g[2, 0] + g[0, 2]], dtype=dt)
            B = _bl_infinite(gd, g1ave)
        else:
            Fbar = jr[q] * (I3 + g)
            de = _fbar_strain(Fbar)
            g1, _ = _gderiv(ec + total, H.HEX8_POINTS[q])
            B = jr[q] * jr[q] * (_b0(gd) + _bl1(gd, g)) + _bl2(de, (g1ave - g1) / three)
        strain[q] = de
        stress[q] = H.stress_update(mat, de) if _is_hyper(mat) else _elastic_matrix(mat, dt) @ de
        if mat.plastic:
            stress[q], istat[q], fstat[q] = Y.point_update(mat, stress[q], plstrain[q], istat[q], fstat[q])
        qf += (stress[q] @ B) * det          # WG is taken before gderiv1 is formed (:674): the reference configuration's
    return qf, stress, strain, istat, fstat


class Model(H.Model):
    """fstr_solid of one mesh of F-bar hexahedra whose sections are ELASTIC, Mises, hyperelastic, Mohr-Coulomb or Drucker-Prager under
    INFINITE or TOTALLAG: hyper_ref.Model's state and steps on this module's element routines."""

    def __init__(self, coord, conn, mats, elem_mat=None):
        super().__init__(361, coord, conn, mats, elem_mat)

    def element_tangents(self):
        u = (self.unode + self.dunode).reshape(-1, 3)
        s = self.st
        return np.array([stf_c3d8fbar(self.coord[nd], u[nd], self.mat(e), self.latch, s["strain"][e], s["stress"][e], s["istat"][e],
                                      s["fstat"][e]) for e, nd in enumerate(self.conn - 1)])

    def element_update(self, order=None):
        u, du = self.unode.reshape(-1, 3), self.dunode.reshape(-1, 3)
        s = self.st
        qf = np.zeros((self.conn.shape[0], 24))
        for e, nd in enumerate(self.conn - 1):
            qf[e], s["stress"][e], s["strain"][e], s["istat"][e], s["fstat"][e] = update_c3d8fbar(
                self.coord[nd], u[nd], du[nd], self.mat(e), s["plstrain"][e], s["istat"][e], s["fstat"][e])
        if any(m.plastic for m in self.mats):
            self.latch = 1
        return qf


class MixedModel(MN.Model):
    """mixed_nl_ref.Model whose groups carry their elemopt: a 361 group with elemopt 4 is F-bar, every other group what
    mixed_nl_ref makes of it."""

    def __init__(self, coord, groups, mats):
        super().__init__(coord, groups, mats)
        for p, g in zip(self.parts, groups):
            p["fbar"] = p["etype"] == 361 and len(g) > 2 and g[2] == ELEMOPT_FBAR

    def element_tangents(self):
        out = super().element_tangents()
        u = (self.unode + self.dunode).reshape(-1, 3)
        for p, ke in zip(self.parts, out):
            if p["fbar"]:
                s = p["st"]
                for e, nd in enumerate(p["conn"] - 1):
                    ke[e] = stf_c3d8fbar(self.coord[nd], u[nd], self.mat_of(p, e), self.latch, s["strain"][e], s["stress"][e], s["istat"][e],
                                         s["fstat"][e])
        return out

    def element_update(self, order=None):
        u, du = self.unode.reshape(-1, 3), self.dunode.reshape(-1, 3)
        before = [{k: v.copy() for k, v in p["st"].items()} if p["fbar"] else None for p in self.parts]
        out = super().element_update(order)
        for p, qf, st0 in zip(self.parts, out, before):
            if not p["fbar"]:
                continue
            s = p["st"]
            for e, nd in enumerate(p["conn"] - 1):
                qf[e], s["stress"][e], s["strain"][e], s["istat"][e], s["fstat"][e] = update_c3d8fbar(
                    self.coord[nd], u[nd], du[nd], self.mat_of(p, e), st0["plstrain"][e], st0["istat"][e], st0["fstat"][e])
        return out


# ---- inputs of the comparisons -----------------------------------------------------------------------------------------------------------
# The mesh is hyper_ref.gpu_mesh(361) throughout (the skewed 2^3 cube plus one collapsed hexahedron), the displacement fields are
# hyper_ref.random_displacement at the amplitudes the B-bar comparisons use: hyper_ref.GPU_AMP for ELASTIC and hyperelastic materials,
# yield_ref.GPU_AMP on yield_ref's elastic constants for the elastoplastic ones.  The cohesion / yield stress and the seed of a plastic
# case were chosen on the CPU (search_plastic_case) so that the margins of yield_ref hold at every point of the F-bar trial stresses under
# both flags: no point sits on a branch edge of the return mapping, at least a quarter are plastic and a tenth elastic.
PLASTIC_CASES = {"mises": (1, 726.0), "drucker": (1, 413.0), "mohr": (1, 420.0)}      # family -> (seed, c or yield stress), from search_plastic_case


def gpu_material(family, nlgeom, c):
    from oracle.refrun import Material
    if family == "mises":
        return Material(Y.GPU_E, Y.GPU_NU, plastic=True, harden=0, plconst=(c, Y.GPU_H, 0.0), nlgeom=nlgeom)
    return Y.gpu_material(family, nlgeom, c)


def trial_stresses(family, nlgeom, seed, mesh=None):
    """The trial stresses of a plastic case's first update: the same update with a yield surface no point reaches.  mesh: another
    mesh than hyper_ref.gpu_mesh(361)"""
    m = H.gpu_mesh(361) if mesh is None else mesh
    ref = Model(m.coord, m.conn, gpu_material(family, nlgeom, 1.0e12))
    ref.unode[:], ref.dunode[:] = H.random_displacement(m.coord, seed, Y.GPU_AMP)
    ref.element_update()
    assert not ref.st["istat"].any()
    return ref.st["stress"].reshape(-1, 6)


def margins_hold(family, mat, trial):
    if family == "mises":
        f = Y.mises_f(trial, mat.plconst[0])
        return bool(np.all(np.abs(np.abs(f) - Y.TOL) >= 10 * Y.TOL) and (f > 0).mean() >= 0.25 and (f < 0).mean() >= 0.10)
    return Y.margins_hold(mat, Y.point_report(mat, trial))


def search_plastic_case(family, seeds=range(1, 200), mesh=None, elems=None):
    """How PLASTIC_CASES was filled (yield_ref.search_gpu_case on the F-bar trial stresses, flags INFINITE and TOTALLAG).  mesh, elems:
    on another mesh, at the points of those of its elements (SHAPE_CASES)"""
    for seed in seeds:
        trial = {g: trial_stresses(family, g, seed, mesh) for g in (INFINITE, TOTALLAG)}
        if elems is not None:
            trial = {g: t.reshape(-1, 8, 6)[elems].reshape(-1, 6) for g, t in trial.items()}
        if family == "mises":
            crit = T.mises(trial[INFINITE])
        else:
            probe = Y.gpu_material(family, INFINITE, 0.0)
            k = np.cos(probe.plconst[2]) if family == "mohr" else probe.plconst4
            crit = np.array([Y.cal_yield_func(probe, s, 0.0) for s in trial[INFINITE]]) / k
        for q in (45, 40, 50, 35, 55, 30, 60):
            c = float(np.round(np.percentile(crit, q), 0))
            if c <= 1.0:
                continue
            if all(margins_hold(family, gpu_material(family, g, c), trial[g]) for g in trial):
                return seed, c
    raise RuntimeError("no case found")


def plastic_case(family, nlgeom):
    """(mesh, material, unode, dunode) of one plastic comparison"""
    seed, c = PLASTIC_CASES[family]
    m = H.gpu_mesh(361)
    unode, dunode = H.random_displacement(m.coord, seed, Y.GPU_AMP)
    return m, gpu_material(family, nlgeom, c), unode, dunode


def elastic_case(name, nlgeom=TOTALLAG, seed=17):
    """(mesh, material, unode, dunode) of an ELASTIC (name 'elastic': E = 2.5, nu = 0.3, the second section of the hyperelastic decks) or
    hyperelastic (hyper_ref.TEST_MATERIALS) comparison"""
    from oracle.refrun import Material
    m = H.gpu_mesh(361)
    mat = Material(2.5, 0.3, nlgeom=nlgeom) if name == "elastic" else H.TEST_MATERIALS[name]()
    unode, dunode = H.random_displacement(m.coord, seed, H.GPU_AMP)
    return m, mat, unode, dunode


# ---- the reference program's own runs: tests/golden/nl_fbar_decks.npz (tests/golden/make_nl_fbar_golden.py) -----------------------------
DECK_SUBSTEPS, DECK_CONVERG, DECK_N = 3, 1.0e-3, 2
# name -> (MAT1 of scripts/fistr1_cube_deck.py --nl-material, stretch, two sections); TYPE=361, n = 2, --form361 FBAR
GOLDEN_DECKS = {"f361_elastic_tl": ("elastic_tl", 0.005, False), "f361_neohooke": ("neohooke", 0.1, False),
                "f361_mooney": ("mooney", 0.1, False), "f361_arruda": ("arruda", 0.1, False), "f361_mooney_two": ("mooney", 0.1, True)}


def deck_args(name):
    """The arguments of scripts/fistr1_cube_deck.py after the directory"""
    mat, stretch, two = GOLDEN_DECKS[name]
    return ([str(DECK_N), str(DECK_SUBSTEPS), "CG", "1", str(stretch), "--nl-material", mat, "--form361", "FBAR"]
            + (["--two-sections"] if two else []))


def golden_deck(name):
    """(mesh, materials, elem_mat or None, bc) of one recorded cube deck, as fistr1_cube_deck.py writes it: z = 0 clamped, the top face
    moved by the stretch in z and a fifth of that in x; with two sections the second half of the elements is ELASTIC 2.5 / 0.3, total
    Lagrange."""
    from frontistr_amd.mesh import CubeMesh
    from oracle.refrun import Material
    mat, stretch, two = GOLDEN_DECKS[name]
    m = CubeMesh(DECK_N)
    m.etype = 361
    mats, em = (Material(206900.0, 0.29, nlgeom=TOTALLAG) if mat == "elastic_tl" else H.TEST_MATERIALS[mat]()), None
    if two:
        mats = [mats, Material(2.5, 0.3, nlgeom=TOTALLAG)]
        em = np.where(np.arange(m.n_elem) < m.n_elem // 2, 1, 2).astype(np.int32)
    node, dof, val = m.dirichlet()
    t = m.top_nodes
    bc = (np.concatenate([node, t, t]).astype(np.int32),
          np.concatenate([dof, np.full(t.size, 3), np.full(t.size, 1)]).astype(np.int32),
          np.concatenate([val, np.full(t.size, stretch * DECK_N), np.full(t.size, 0.2 * stretch * DECK_N)]))
    return m, mats, em, bc


summary = H.summary


# The reference's own examples/static/FbarElement/T01_BEAM_HYPERELASTIC (committed copy: tests/golden/decks/static/FbarElement): a
# cantilever of five unit cubes along x, Mooney-Rivlin 1 / 0.923 / 0.24, the face x = 0 clamped, -0.01 in y on two nodes of the tip;
# one sub-step, CONVERG = 1e-10: seven Newton iterations, which the tangent has to be right for.
T01_CONVERG, T01_MAXITER = 1.0e-10, 12


def t01_deck():
    """(coord, conn, material, bc, cload) of T01_BEAM_HYPERELASTIC, read from the committed mesh file"""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decks", "static", "FbarElement", "T01_BEAM_HYPERELASTIC.msh")
    coord, conn, card = [], [], None
    with open(path) as fh:
        for line in fh:
            if line.startswith("!"):
                card = line.split(",")[0].strip().upper()
                continue
            a = [v.strip() for v in line.split(",")]
            if card == "!NODE":
                coord.append([float(v) for v in a[1:4]])
            elif card == "!ELEMENT":
                conn.append([int(v) for v in a[1:9]])
    coord, conn = np.array(coord), np.array(conn, dtype=np.int32)
    fixed = np.arange(21, 25)                                    # SET-1
    bc = (np.repeat(fixed, 3).astype(np.int32), np.tile([1, 2, 3], fixed.size).astype(np.int32), np.zeros(3 * fixed.size))
    cload = np.zeros(3 * coord.shape[0])
    for nd in (1, 3):                                            # SET-2, dof 2
        cload[3 * (nd - 1) + 1] = -0.01
    return coord, conn, H.mooney_rivlin(1.0, 0.923, 0.24), bc, cload
