"""The material point of the nonlinear loop ON its branch edges: a numpy restatement of the reference's Mises point for the four
hardening laws in the dtype of the stress it is given, and the table of trial stresses and histories that put each branch of the three
return mappings (Mises here, Mohr-Coulomb / Drucker-Prager in yield_ref.py) on the quadrature points of tests/test_gpu_point_edges.py.

Mises point, fistr1/src/lib/physics/Elastoplastic.f90 as it is written: calCurrYield :254-292, calHardenCoeff :175-220 with
GetTableData / GetTableGrad (lib/utilities/ttable.f90:320-335, :221-235), the Mises branch of BackwardEuler :351-459 and of
calElastoPlasticMatrix :16-117.  In float64 it computes what the C oracle (oracle/fstr_nl_oracle.c) computes; tests/test_point_ref.py
holds it to that on every Mises case.  Each routine takes an optional `info` dict, as yield_ref.backward_euler does: the exit taken
(`band`, `elastic`, `reset`, `converged`, `exhausted`), the iterations begun, and `lookups`, one (kind, segment, on_breakpoint) per table
lookup in the order they were made, kind in `below` (a < first abscissa), `beyond` (a >= last), `segment`.

The cases.  Under UPDATELAG with dunode = 0 every update kernel hands the point function trial = stress_bak bit for bit, so a case is
(material, trial stress, plstrain, incoming istat, incoming fstat) and the exit it was built for.  SENTINEL is the incoming fstat of the
cases whose exit must not write it.  CASES[material name] lists them; `tangent_states()` adds the hand-set states of the tangent
comparison.  What a case claims -- the exit, the iteration count, the table rows read, maxp / minp / mm, its margin to the edge it sits
beside -- is asserted on the CPU, in float64 and np.longdouble, by tests/test_point_ref.py; that is the condition under which a GPU
comparison at 1e-11 means something.

Cases that sit BESIDE an edge and not on it state their margin: `f` at 0.9 tol and 1.1 tol is 1e-4 away from the |f| < tol test, about
1e6 times the rounding of f at stresses of the order 1e3 (eps * 1e3 = 2e-13, a handful of operations); the ends of the Drucker-Prager
reset band are missed by 1e-4 of sqrt(J2), RAMBERG-OSGOOD's p > pl(1) by 1e-6 of pl(1).

Branches left out, and why:
  * the `fabs(hd) + od == fabs(hd)` arm of the Jacobi rotation (utilities.f90:158-159): it needs an off-diagonal term that is
    significant against both eigenvalues (100 |b| changes them) yet lost against their difference -- no stress of the magnitudes here.
  * a Mises return through `dlambda < 0`: the loop is entered with f > tol and the first step divides by 3 G + H > 0; later steps add
    f / (3 G + H) with H the slope at the current iterate: for a concave hardening curve (every material here) the residual is convex
    in dlambda, Newton's iterates approach the root from below and f stays positive.
  * a Mohr-Coulomb return through `dlambda < 0`: f > tol, and the denominator 4 G (1 + sf ss / 3) + 4 K sf ss + 4 H cf^2 is positive
    for |ss| <= 1/2 at the constants used; the second step adds the remaining half of the first (see yield_ref), never a negative one.
  * cos(phi) == 0 (`Math error in return mapping`): no double reaches it, as tests/test_gpu_yield.py notes.
  * the `stop` of |sin 3 theta| > 1: tests/test_gpu_yield.py (STOP_STRESS) runs it.
"""
import numpy as np

import tet_nl_ref as T
import yield_ref as Y
from tet_nl_ref import INFINITE, TOTALLAG, UPDATELAG  # noqa: F401

TOL, MAXITER = Y.TOL, Y.MAXITER
SENTINEL = -7.0
EXITS = ("band", "elastic", "reset", "converged", "exhausted")


# ---- ttable.f90 --------------------------------------------------------------------------------------------------------------------------
def _lt(a, b, as_le):
    return a <= b if as_le else a < b


def _ge(a, b, as_gt):
    return a > b if as_gt else a >= b


def _table_row(table, a, info, lt_as_le, ge_as_gt):
    """The branch GetTableData :320-335 and GetTableGrad :221-235 share -> ('below' | 'beyond' | 'segment' | 'none', i).  `none`
    is the fall-through behind the loop, which no number reaches with the reference's comparisons."""
    t = table[:, 1]
    n = t.shape[0]
    on = bool(np.any(t == a))
    if _lt(a, t[0], lt_as_le):
        row = ("below", 0)
    elif _ge(a, t[n - 1], ge_as_gt):
        row = ("beyond", n - 1)
    else:
        row = ("none", n - 1)
        for i in range(n - 1):
            if _ge(a, t[i], ge_as_gt) and _lt(a, t[i + 1], lt_as_le):
                row = ("segment", i)
                break
    if info is not None:
        info.setdefault("lookups", []).append(row + (on,))
    return row


def table_value(table, a, info=None, *, lt_as_le=False, ge_as_gt=False):
    """GetTableData of a 1-D table with rows (value, abscissa)"""
    n = a.dtype.type
    kind, i = _table_row(table, a, info, lt_as_le, ge_as_gt)
    if kind == "below":
        return table[0, 0]
    if kind != "segment":
        return table[-1, 0]
    lam = (a - table[i, 1]) / (table[i + 1, 1] - table[i, 1])
    return (n(1) - lam) * table[i, 0] + lam * table[i + 1, 0]


def table_grad(table, a, info=None, *, lt_as_le=False, ge_as_gt=False):
    """GetTableGrad"""
    kind, i = _table_row(table, a, info, lt_as_le, ge_as_gt)
    if kind != "segment":
        return a.dtype.type(0)
    return (table[i + 1, 0] - table[i, 0]) / (table[i + 1, 1] - table[i, 1])


# ---- Elastoplastic.f90, Mises ------------------------------------------------------------------------------------------------------------
def _pl(mat, dt):
    return [dt.type(v) for v in mat.plconst], np.asarray(mat.table, dtype=np.float64).reshape(-1, 2).astype(dt)


def curr_yield(mat, p, info=None, **lookup):
    """calCurrYield :254-292; p carries the dtype"""
    p = np.asarray(p)[()]
    n = p.dtype.type
    pl, tab = _pl(mat, p.dtype)
    if mat.harden == 0:
        return pl[0] + pl[1] * p
    if mat.harden == 1:
        return table_value(tab, p, info, **lookup)
    if mat.harden == 2:
        return pl[1] * (pl[0] + p) ** pl[2]
    if info is not None:
        info.setdefault("ramberg", []).append("flat" if p <= pl[0] else "power")
    return pl[1] if p <= pl[0] else pl[1] * (p / pl[0]) ** (n(1) / pl[2])


def harden_coeff(mat, p, info=None, **lookup):
    """calHardenCoeff :175-220"""
    p = np.asarray(p)[()]
    n = p.dtype.type
    pl, tab = _pl(mat, p.dtype)
    if mat.harden == 0:
        return pl[1]
    if mat.harden == 1:
        return table_grad(tab, p, info, **lookup)
    if mat.harden == 2:
        return pl[1] * pl[2] * (pl[0] + p) ** (pl[2] - n(1))
    ef = curr_yield(mat, p, info)
    return pl[1] * (ef / pl[1]) ** (n(1) - pl[2]) / (pl[0] * pl[2])


def _deviator(s):
    n = s.dtype.type
    J1 = (s[0] + s[1] + s[2]) / n(3)
    dv = s.copy()
    dv[:3] -= J1
    J2 = n(0.5) * (dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]) + (dv[3] * dv[3] + dv[4] * dv[4] + dv[5] * dv[5])
    return J1, dv, J2


def backward_euler(mat, stress, plstrain, istat, fstat1, info=None, *, maxiter=MAXITER, reset_istat=0, exits_write_fstat=False,
                   lt_as_le=False, ge_as_gt=False):
    """BackwardEuler, Mises (:351-459, :557) -> (stress, istat, fstat(1)) in the dtype of the stress.  The keyword parameters default
    to what the reference does (see yield_ref.backward_euler); lt_as_le / ge_as_gt replace every `<` / `>=` of the table lookups."""
    s = np.array(stress)
    n = s.dtype.type
    lookup = dict(lt_as_le=lt_as_le, ge_as_gt=ge_as_gt)
    plstrain = n(plstrain)
    tol = n(TOL)
    J1, dv, J2 = _deviator(s)
    yd = np.sqrt(n(3) * J2)
    f = yd - curr_yield(mat, plstrain, info, **lookup)
    if info is not None:
        info.update(f=float(f), iterations=0)
    if abs(f) < tol or f < 0:
        ist = 1 if abs(f) < tol else 0
        if info is not None:
            info["exit"] = "band" if ist else "elastic"
        return s, ist, (plstrain if exits_write_fstat else fstat1)
    G = n(mat.E) / (n(2) * (n(1) + n(mat.nu)))
    dl, ist, how, it = n(0), 1, "exhausted", 0
    for it in range(1, maxiter + 1):
        Hd = harden_coeff(mat, plstrain + dl, info, **lookup)
        dl = dl + f / (n(3) * G + Hd)
        if dl < 0:
            dl, ist, how = n(0), reset_istat, "reset"
            break
        f = yd - n(3) * G * dl - curr_yield(mat, plstrain + dl, info, **lookup)
        if abs(f) < tol * tol:
            how = "converged"
            break
    fac = n(1) - n(3) * dl * G / yd
    out = fac * dv
    out[:3] += J1
    if info is not None:
        info.update(exit=how, iterations=it, residual=float(f))
    return out, ist, plstrain + dl


def elastoplastic_matrix(mat, stress, istat, fstat1, info=None, **lookup):
    """calElastoPlasticMatrix :16-117, Mises.  info['branch']: 'edge' where the hardening coefficient is GetTableGrad's zero outside
    the table (below the first row, at and beyond the last: the perfectly plastic tangent), 'interior' otherwise."""
    s = np.asarray(stress)
    dt = s.dtype
    n = dt.type
    De = Y.elastic_matrix(mat, dt)
    if istat == 0:
        return De
    J1 = s[0] + s[1] + s[2]
    d = np.array([s[0] - J1 / n(3), s[1] - J1 / n(3), s[2] - J1 / n(3), s[3], s[4], s[5]], dtype=dt)
    J2 = n(0.5) * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + (d[3] * d[3] + d[4] * d[4] + d[5] * d[5])
    dj2 = np.array([d[0], d[1], d[2], n(2) * d[3], n(2) * d[4], n(2) * d[5]], dtype=dt) / (n(2) * np.sqrt(J2))
    mine = {}
    Hd = harden_coeff(mat, n(fstat1), mine, **lookup)
    if info is not None:
        info.update(mine)
        info["branch"] = "edge" if mat.harden == 1 and mine["lookups"][-1][0] != "segment" else "interior"
    a = np.sqrt(n(3)) * dj2
    da = De @ a
    dum = Hd + n(0) + da @ a
    return De - np.outer(da, da) / dum


# ---- any elastoplastic material ----------------------------------------------------------------------------------------------------------
_YIELD_KW = ("maxiter", "first_of_ties", "mm_rule", "reset_istat", "exits_write_fstat", "zeroing")
_MISES_KW = ("maxiter", "reset_istat", "exits_write_fstat", "lt_as_le", "ge_as_gt")


def point(mat, stress, plstrain, istat, fstat1, info=None, **kw):
    """BackwardEuler of a point of any elastoplastic material in the dtype of the stress; keywords a family does not have are dropped"""
    keys, f = (_YIELD_KW, Y.backward_euler) if Y.is_yield(mat) else (_MISES_KW, backward_euler)
    with np.errstate(all="ignore"):          # the apex: the reference divides by zero and goes on
        return f(mat, stress, plstrain, istat, fstat1, info, **{k: v for k, v in kw.items() if k in keys})


def tangent(mat, stress, istat, fstat1, info=None, **kw):
    """calElastoPlasticMatrix of a point of any elastoplastic material (keywords: the table comparisons, Mises only)"""
    if Y.is_yield(mat):
        return Y.elastoplastic_matrix(mat, np.asarray(stress), istat, fstat1, info)
    return elastoplastic_matrix(mat, np.asarray(stress), istat, fstat1, info, **{k: v for k, v in kw.items() if k in ("lt_as_le", "ge_as_gt")})


# ---- the materials -------------------------------------------------------------------------------------------------------------------------
# Mohr-Coulomb / Drucker-Prager: the constants of yield_ref's GPU comparisons with c = 300.  RAMBERG-OSGOOD: the constants of the
# reference's own examples/static/1elem/ramberg deck.  MULTILINEAR: the table of the recorded decks (tet_nl_ref.DECK_TABLE).
MATERIAL_NAMES = ("bilinear", "multilinear", "swift", "ramberg", "drucker", "mohr")
E0, NU0, C0, PHI0, H0 = Y.GPU_E, Y.GPU_NU, 300.0, Y.GPU_PHI, Y.GPU_H
TABLE = T.DECK_TABLE


def material(name, nlgeom=UPDATELAG):
    from oracle.refrun import Material
    if name == "mohr":
        return Y.mohr_coulomb(E0, NU0, C0, PHI0, H0, nlgeom=nlgeom)
    if name == "drucker":
        return Y.drucker_prager(E0, NU0, C0, PHI0, H0, nlgeom=nlgeom)
    if name == "bilinear":
        return Material(E0, NU0, plastic=True, harden=0, plconst=(500.0, H0, 0.0), nlgeom=nlgeom)
    if name == "multilinear":
        return Material(206900.0, 0.29, plastic=True, harden=1, table=TABLE, nlgeom=nlgeom)
    if name == "swift":
        return Material(E0, NU0, plastic=True, harden=2, plconst=(0.002, 900.0, 0.2), nlgeom=nlgeom)
    if name == "ramberg":
        return Material(8.0e4, 0.3, plastic=True, harden=3, plconst=(0.01, 800.0, 12.0), nlgeom=nlgeom)
    raise KeyError(name)


def family(name):
    return name if name in ("mohr", "drucker") else "mises"


def out_of_reach(name, nlgeom=UPDATELAG):
    """The material with a cohesion / yield stress no point reaches"""
    from oracle.refrun import Material
    if name == "mohr":
        return Y.mohr_coulomb(E0, NU0, 1.0e12, PHI0, H0, nlgeom=nlgeom)
    if name == "drucker":
        return Y.drucker_prager(E0, NU0, 1.0e12, PHI0, H0, nlgeom=nlgeom)
    m = material(name, nlgeom)
    if name == "multilinear":
        return Material(m.E, m.nu, plastic=True, harden=1, table=TABLE * np.array([1.0e9, 1.0]), nlgeom=nlgeom)
    pl = {"bilinear": (1.0e12, H0, 0.0), "swift": (0.002, 1.0e12, 0.2), "ramberg": (0.01, 1.0e12, 12.0)}[name]
    return Material(m.E, m.nu, plastic=True, harden=m.harden, plconst=pl, nlgeom=nlgeom)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
class Case:
    """One trial stress and history.  exit: the exit it is built for.  expect: what else test_point_ref.py asserts of `info` (keys
    iterations, triple = (maxp, minp, mm), first / last = the first / last table lookup, ramberg = the arm of its first lookup, snapped =
    sin 3 theta within 1e-8 of +-1, and of eigen3 rotated = rotations made (exactly 0 or 1, else at least), skipped).  margin: None, or
    (kind, size) of a case that sits beside an edge.  apex: the reference computes non-finite numbers here and goes on."""

    def __init__(self, name, mat, stress, plstrain=0.0, istat=0, fstat=None, exit=None, margin=None, apex=False, **expect):
        self.name, self.mat, self.stress = name, mat, np.array(stress, dtype=np.float64)
        self.plstrain, self.istat, self.exit, self.margin, self.apex, self.expect = float(plstrain), int(istat), exit, margin, apex, expect
        self.fstat = (SENTINEL if exit in ("band", "elastic") else float(plstrain)) if fstat is None else float(fstat)

    def run(self, dtype=np.float64, info=None, **kw):
        return point(material(self.mat), self.stress.astype(dtype), dtype(self.plstrain), self.istat, dtype(self.fstat), info, **kw)


DIR = np.array([0.9, -0.2, -0.7, 0.35, -0.25, 0.15])       # a deviator direction with separated principal values, |sin 3 theta| = 0.53


def shaped(direction, root_j2, p):
    """The stress of mean p whose deviator has the given direction and sqrt(J2)"""
    d = np.array(direction, dtype=np.float64)
    d[:3] -= d[:3].mean()
    j2 = 0.5 * (d[:3] @ d[:3]) + d[3:] @ d[3:]
    return d * (root_j2 / np.sqrt(j2)) + np.array([p, p, p, 0.0, 0.0, 0.0])


def _f(name, s, plstrain):
    mat = material(name)
    if Y.is_yield(mat):
        return float(Y.cal_yield_func(mat, s, plstrain))
    return float(T.mises(s) - curr_yield(mat, np.float64(plstrain)))


def at_f(name, target, p, plstrain=0.0, direction=DIR):
    """The stress of mean p along `direction` at which the material's yield function is `target`: f is linear in the size of the
    deviator for a fixed direction, so two secant steps land within rounding (the test asserts where they landed)."""
    r0, r1 = 100.0, 200.0
    f0, f1 = _f(name, shaped(direction, r0, p), plstrain), _f(name, shaped(direction, r1, p), plstrain)
    for _ in range(4):
        if f1 == target or f1 == f0:
            break
        r0, r1, f0 = r1, r1 + (target - f1) * (r1 - r0) / (f1 - f0), f1
        f1 = _f(name, shaped(direction, r1, p), plstrain)
    return shaped(direction, r1, p)


def diag(a, b, c, s12=0.0, s23=0.0, s31=0.0):
    return np.array([a, b, c, s12, s23, s31], dtype=np.float64)


def _build():
    cases = {k: [] for k in MATERIAL_NAMES}

    def add(name, mat, stress, **kw):
        cases[mat].append(Case(name, mat, stress, **kw))

    # ---- Mohr-Coulomb.  Both the linearised return and its start (calYieldFunc's f is half the principal-stress f) make every
    # return here end in its second iteration.
    hi, mid, lo = 600.0, 100.0, -900.0
    for perm, triple in (((hi, mid, lo), (0, 2, 1)), ((hi, lo, mid), (0, 1, 2)), ((mid, hi, lo), (1, 2, 2)), ((lo, hi, mid), (1, 0, 2)),
                         ((mid, lo, hi), (2, 1, 2)), ((lo, mid, hi), (2, 0, 1))):
        add("order_%d%d%d" % triple, "mohr", diag(*perm), exit="converged", iterations=2, triple=triple)
    a, b = 500.0, -900.0
    for tag, x, y in (("hi", a, b), ("lo", b, a)):           # two equal doubles: an exact tie on the device too
        for k, (perm, triple) in enumerate((((x, x, y), (0, 2, 1) if x > y else (2, 0, 1)), ((x, y, x), (0, 1, 2) if x > y else (1, 0, 2)),
                                            ((y, x, x), (1, 0, 2) if x > y else (0, 1, 2)))):
            add("tie_%s_%d" % (tag, k), "mohr", diag(*perm), exit="converged", iterations=2, triple=triple, snapped=True)
    add("shear_zeroed", "mohr", diag(hi, mid, lo, 5.0e-11), exit="converged", triple=(0, 2, 1), rotated=0)
    add("shear_kept", "mohr", diag(hi, mid, lo, 2.0e-10), exit="converged", triple=(0, 2, 1), rotated=1, skipped=2)
    # the zeroing decides a tie: (0, 5e-11, -2000) is (0, 0, -2000) behind :476-478, maximum at 0; without it the maximum is at 1
    add("zeroed_tie", "mohr", diag(0.0, 5.0e-11, -2000.0), exit="converged", triple=(0, 2, 1), rotated=0, snapped=True)
    add("full_max1", "mohr", diag(mid, hi, lo, 80.0, -60.0, 50.0), exit="converged", triple=(1, 2, 2), rotated=3)
    add("full_max2", "mohr", diag(lo, mid, hi, 80.0, -60.0, 50.0), exit="converged", triple=(2, 0, 1), rotated=3)
    add("band_0.9tol", "mohr", at_f("mohr", 0.9 * TOL, -200.0), exit="band", margin=("f", 1.0e-4))
    add("out_1.1tol", "mohr", at_f("mohr", 1.1 * TOL, -200.0), exit="converged", margin=("f", 1.0e-4))
    add("unloading", "mohr", at_f("mohr", -100.0, -200.0, 2.0e-3), plstrain=2.0e-3, istat=1, exit="elastic")
    add("apex", "mohr", diag(3000.0, 3000.0, 3000.0), exit="exhausted", apex=True)

    # ---- Drucker-Prager.  calYieldFunc takes the trace, the return the mean stress: with mean stress p > 0 the first step overshoots,
    # and for xi c - 3 eta p < sqrt(J2) < xi c - eta p the second one makes dlambda negative.
    m = material("drucker")
    c, _, eta = m.plconst
    xi, p = m.plconst4, 400.0
    lo_end, hi_end = xi * c - 3.0 * eta * p, xi * c - eta * p
    add("reset_mid", "drucker", diag(p, p, p, 0.5 * (lo_end + hi_end)), exit="reset", iterations=2)
    add("reset_generic", "drucker", shaped(DIR, 0.5 * (lo_end + hi_end), p), plstrain=0.0, exit="reset", iterations=2)
    add("below_band", "drucker", shaped(DIR, lo_end * (1.0 - 1.0e-4), p), exit="elastic", margin=("band", 1.0e-6))
    add("inside_low_end", "drucker", shaped(DIR, lo_end * (1.0 + 1.0e-4) + 1.1 * TOL, p), exit="reset", iterations=2, margin=("band", 1.0e-6))
    add("inside_high_end", "drucker", shaped(DIR, hi_end * (1.0 - 1.0e-4), p), exit="reset", iterations=2, margin=("band", 1.0e-6))
    add("above_band", "drucker", shaped(DIR, hi_end * (1.0 + 1.0e-4), p), exit="converged", iterations=2, margin=("band", 1.0e-6))
    add("band_0.9tol", "drucker", at_f("drucker", 0.9 * TOL, -200.0), exit="band", margin=("f", 1.0e-4))
    add("out_1.1tol", "drucker", at_f("drucker", 1.1 * TOL, -200.0), exit="converged", margin=("f", 1.0e-4))
    add("unloading", "drucker", at_f("drucker", -100.0, -200.0, 2.0e-3), plstrain=2.0e-3, istat=1, exit="elastic")
    add("apex", "drucker", diag(3000.0, 3000.0, 3000.0), exit="converged", apex=True)

    # ---- Mises, BILINEAR
    for tag, mult, ex in (("band_0.9tol", 0.9, "band"), ("band_-0.9tol", -0.9, "band"), ("out_1.1tol", 1.1, "converged"), ("in_-2tol", -2.0, "elastic")):
        add(tag, "bilinear", at_f("bilinear", mult * TOL, 150.0, 1.0e-3), plstrain=1.0e-3, exit=ex, margin=("f", 1.0e-4) if abs(mult) < 2 else None)
    add("unloading", "bilinear", at_f("bilinear", -100.0, 150.0, 2.0e-3), plstrain=2.0e-3, istat=1, exit="elastic")
    add("plastic", "bilinear", at_f("bilinear", 200.0, 150.0, 1.0e-3), plstrain=1.0e-3, istat=1, exit="converged", iterations=1)

    # ---- Mises, MULTILINEAR: rows (yield stress, plastic strain), breakpoints at 0, 0.05, 0.1, 0.2, ...; the last row is 0.5.  A
    # return inside one segment is exact after its first iteration.
    seg, below, beyond = (lambda i, on=False: ("segment", i, on)), ("below", 0, False), (lambda on: ("beyond", 6, on))
    add("first_row", "multilinear", at_f("multilinear", 90.0, 150.0, 0.0), plstrain=0.0, exit="converged", iterations=1, first=seg(0, True))
    add("on_breakpoint", "multilinear", at_f("multilinear", 90.0, 150.0, 0.05), plstrain=0.05, exit="converged", iterations=1, first=seg(1, True))
    add("on_breakpoint_band", "multilinear", at_f("multilinear", 0.5 * TOL, 150.0, 0.1), plstrain=0.1, exit="band", first=seg(2, True))
    add("below_first_row", "multilinear", at_f("multilinear", 90.0, 150.0, -1.0e-3), plstrain=-1.0e-3, exit="converged", first=below)
    add("on_last_row", "multilinear", at_f("multilinear", 90.0, 150.0, 0.5), plstrain=0.5, exit="converged", iterations=1, first=beyond(True))
    add("beyond_last_row", "multilinear", at_f("multilinear", 90.0, 150.0, 0.6), plstrain=0.6, exit="converged", iterations=1, first=beyond(False))
    add("crossing", "multilinear", at_f("multilinear", 400.0, 150.0, 0.0499), plstrain=0.0499, exit="converged", iterations=2,
        first=seg(0), last=seg(1))

    # ---- Mises, SWIFT and RAMBERG-OSGOOD
    add("from_p0", "swift", at_f("swift", 300.0, 150.0, 0.0), plstrain=0.0, exit="converged")
    # below pl(1) the law is flat but calHardenCoeff is not zero: the iteration contracts by H / (3 G + H) = 0.067 a step and runs out
    add("p0", "ramberg", at_f("ramberg", 300.0, 150.0, 0.0), plstrain=0.0, exit="exhausted", iterations=5, ramberg="flat")
    add("p0_small_step", "ramberg", at_f("ramberg", 2.0 * TOL, 150.0, 0.0), plstrain=0.0, exit="converged", iterations=3, ramberg="flat")
    add("p_is_pl1", "ramberg", at_f("ramberg", 300.0, 150.0, 0.01), plstrain=0.01, exit="converged", ramberg="flat")
    add("p_above_pl1", "ramberg", at_f("ramberg", 300.0, 150.0, 0.01 * (1.0 + 1.0e-6)), plstrain=0.01 * (1.0 + 1.0e-6), exit="converged",
        ramberg="power", margin=("ramberg", 1.0e-6))
    # the constants of the reference's 1elem/ramberg deck, a uniaxial trial stress of 1500 from plstrain = 0: the loop is left after its
    # fifth iteration with a residual of 9.7e-4 against tol^2 = 1e-6
    add("exhausted", "ramberg", diag(1500.0, 0.0, 0.0), plstrain=0.0, exit="exhausted", iterations=5)
    return cases


CASES = _build()


def all_cases():
    return [c for k in MATERIAL_NAMES for c in CASES[k]]


_RESULTS = {}


def result(case):
    """(stress, istat, fstat, info) of the float64 restatement, computed once"""
    key = (case.mat, case.name)
    if key not in _RESULTS:
        info = {}
        s, ist, fs = case.run(np.float64, info)
        _RESULTS[key] = (np.asarray(s, dtype=np.float64), int(ist), float(fs), info)
    return _RESULTS[key]


# ---- the mutants of the discrimination check ------------------------------------------------------------------------------------------------
MUTANTS = {"last of ties": dict(first_of_ties=False), "mm is the remaining index": dict(mm_rule=False), "four iterations": dict(maxiter=4),
           "six iterations": dict(maxiter=6), "reset leaves istat = 1": dict(reset_istat=1), "early exits write fstat": dict(exits_write_fstat=True),
           "<= for < in the tables": dict(lt_as_le=True), "> for >= in the tables": dict(ge_as_gt=True), "no zeroing": dict(zeroing=False)}


# ---- the states of the tangent comparison ----------------------------------------------------------------------------------------------------
class State:
    """(material, stress, istat, fstat) of one point of the tangent comparison; branch: 'edge', 'trig' or 'interior' where the state
    was set by hand for it, None where it is the outcome of a case"""

    def __init__(self, name, mat, stress, istat, fstat, branch=None, sin3=None):
        self.name, self.mat, self.stress, self.istat, self.fstat = name, mat, np.array(stress, dtype=np.float64), int(istat), float(fstat)
        self.branch, self.sin3 = branch, sin3


def tangent_states():
    """{material name: [State]}: the returned (stress, istat, fstat) of every case whose point ended plastic with finite numbers, and
    the hand-set edge states: sin 3 theta = -1 (uniaxial tension, and an (a, b, b) diagonal with a > b) and +1 (uniaxial compression)
    for Mohr-Coulomb; plastic strains on the edges of the hardening table and laws for Mises."""
    out = {k: [] for k in MATERIAL_NAMES}
    for c in all_cases():
        s, ist, fs, _ = result(c)
        if ist and not c.apex and np.isfinite(fs):
            out[c.mat].append(State("after " + c.name, c.mat, s, ist, fs))
    for name, st, sign in (("uniaxial_tension", diag(700.0, 0.0, 0.0), -1.0), ("diagonal_abb", diag(400.0, -350.0, -350.0), -1.0),
                           ("uniaxial_compression", diag(-700.0, 0.0, 0.0), 1.0), ("diagonal_aab", diag(400.0, 400.0, -350.0), 1.0)):
        out["mohr"].append(State(name, "mohr", st, 1, 2.0e-3, "edge", sign))
        out["drucker"].append(State(name, "drucker", st, 1, 2.0e-3))
    out["mohr"].append(State("generic", "mohr", shaped(DIR, 400.0, -200.0), 1, 2.0e-3, "trig"))
    gen = shaped(DIR, 600.0, 150.0)
    for name, fs, br in (("first_row", 0.0, "interior"), ("on_breakpoint", 0.05, "interior"), ("inside", 0.07, "interior"),
                         ("below_first_row", -1.0e-3, "edge"), ("on_last_row", 0.5, "edge"), ("beyond_last_row", 0.6, "edge")):
        out["multilinear"].append(State(name, "multilinear", gen, 1, fs, br))
    out["bilinear"].append(State("hand_set", "bilinear", gen, 1, 1.0e-3))
    out["swift"].append(State("p0", "swift", gen, 1, 0.0))
    for name, fs in (("p0", 0.0), ("p_is_pl1", 0.01), ("p_above_pl1", 0.01 * (1.0 + 1.0e-6)), ("p_large", 0.05)):
        out["ramberg"].append(State(name, "ramberg", gen, 1, fs))
    return out


# ---- dealing cases out over the quadrature points of a mesh ----------------------------------------------------------------------------------
def edge_mesh(etype, items_per_section, nq):
    """(mesh, elem_mat) whose section k (1-based ids in elem_mat) has at least twice items_per_section[k] quadrature points:
    hyper_ref.gpu_mesh(etype) where it is large enough, else the smallest skewed cube of that type that is (at 361 with the collapsed
    hexahedron of gpu_mesh added).  Elements are dealt to the sections in turn, each section until its need is met, the rest
    cyclically."""
    import hyper_ref as H
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    need = [max(1, -(-2 * k // nq)) for k in items_per_section]
    m = H.gpu_mesh(etype)
    n = 2
    while m.n_elem < sum(need):
        n += 1
        if etype == 361:
            m = CubeMesh(n, skew=0.1)
            c = m.conn[-1]
            m.conn = np.ascontiguousarray(np.vstack([m.conn, [[c[0], c[1], c[2], c[2], c[4], c[5], c[6], c[6]]]]).astype(np.int32))
            m.n_elem += 1
        else:
            m = solid_mesh(n, etype, skew=0.1, **({"curve": 0.03} if etype in (342, 352, 362) else {}))
        m.etype = etype
    left, em, k = list(need), np.zeros(m.n_elem, dtype=np.int32), 0
    for e in range(m.n_elem):
        for _ in range(len(need)):
            if left[k] > 0 or not any(left):
                break
            k = (k + 1) % len(need)
        em[e] = k + 1
        left[k] = max(0, left[k] - 1)
        k = (k + 1) % len(need)
    return m, em


def deal(elem_mat, nq, items_per_section):
    """(n_elem, nq) item index per point: within a section the items go round by flat point index (element by element, point by
    point), so that 2 n points hold each of n items twice.  Where the number of items is a multiple of the points per element an item
    would keep landing on the same quadrature index: the round is shifted by one item after every lcm(n, nq) points."""
    idx = np.zeros((len(elem_mat), nq), dtype=np.int64)
    for k, n in enumerate(items_per_section):
        el = np.flatnonzero(np.asarray(elem_mat) == k + 1)
        flat = np.arange(el.size * nq)
        idx[el] = ((flat + flat // np.lcm(n, nq)) % n).reshape(el.size, nq)
    return idx


# ---- the cases with a margin, through INFINITE / TOTALLAG / F-bar updates ---------------------------------------------------------------------
# trial = stress_bak exists only under UPDATELAG (and F-bar refuses UPDATELAG).  Under the other flags a case reaches the point function
# as D . strain of a displacement field, rounded: only cases whose branch survives that, by the margin asserted in check_affine, go here.
AFFINE_CASES = (("drucker", "reset_mid"), ("drucker", "reset_generic"), ("drucker", "unloading"), ("ramberg", "exhausted"),
                ("multilinear", "crossing"), ("bilinear", "unloading"), ("mohr", "unloading")) + tuple(
                    ("mohr", c.name) for c in CASES["mohr"] if c.name.startswith("order_"))
AFFINE_NAMES = ("drucker", "ramberg", "multilinear", "bilinear", "mohr")
AFFINE_RUNS = [(361, INFINITE, 2), (361, INFINITE, 4), (342, INFINITE, 2), (352, INFINITE, 2), (361, TOTALLAG, 2), (361, TOTALLAG, 4)]


def affine_model(etype, nlgeom, elemopt=2, reach=True):
    """(mesh, elem_mat, cases per element, state, restated Model with that state and dunode set) of a mesh of disconnected unit cells,
    one per case of AFFINE_CASES, each with its own nodes (one hexahedron, or the tetrahedra / wedges of one cube), under the affine
    displacement whose small strain is D^-1 . trial: the elements reproduce affine fields, so every point of the cell sees the case
    (under TOTALLAG: the Green-Lagrange strain of that field).  reach=False: the yield surfaces out of reach, for the trial stresses."""
    from types import SimpleNamespace
    import fbar_ref as FB
    import hyper_ref as H
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    cell = CubeMesh(1) if etype == 361 else solid_mesh(1, etype)
    nn, ne = cell.coord.shape[0], cell.conn.shape[0]
    nq = H.POINTS[etype]
    picked = [next(c for c in CASES[k] if c.name == name) for k, name in AFFINE_CASES]
    coord, conn, em, dun, per_elem = [], [], [], [], []
    for k, c in enumerate(picked):
        mat = material(c.mat, nlgeom)
        de = np.linalg.solve(Y.elastic_matrix(mat, np.dtype(np.float64)), c.stress)
        G = np.array([[de[0], de[3] / 2, de[5] / 2], [de[3] / 2, de[1], de[4] / 2], [de[5] / 2, de[4] / 2, de[2]]])
        coord.append(cell.coord + np.array([2.0 * k, 0.0, 0.0]))
        conn.append(cell.conn + k * nn)
        dun.append(cell.coord @ G.T)
        em += [1 + AFFINE_NAMES.index(c.mat)] * ne
        per_elem += [c] * ne
    m = SimpleNamespace(coord=np.vstack(coord), conn=np.ascontiguousarray(np.vstack(conn), dtype=np.int32), etype=etype)
    m.n_node, m.n_elem = m.coord.shape[0], m.conn.shape[0]
    em = np.array(em, dtype=np.int32)
    mats = [material(k, nlgeom) if reach else out_of_reach(k, nlgeom) for k in AFFINE_NAMES]
    ref = FB.Model(m.coord, m.conn, mats, em) if elemopt == 4 else Y.Model(etype, m.coord, m.conn, mats, em)
    ref.dunode[:] = np.vstack(dun).ravel()
    for e, c in enumerate(per_elem):
        ref.st["plstrain"][e], ref.st["istat"][e], ref.st["fstat"][e] = c.plstrain, c.istat, c.fstat
    st = {k: ref.st[k].copy() for k in ("plstrain", "istat", "fstat")}
    return m, em, per_elem, st, ref


def check_affine(etype, nlgeom, elemopt=2):
    """The condition of the comparison, on the CPU: every point of every element takes the branch of its case, with the margins of
    tests/test_point_ref.py (1e-4 in f around tol, 1e-6 of sqrt(J2) to the ends of the reset band, 1e-6 of the largest principal stress
    between principal stresses, 1e-6 in plastic strain to a breakpoint, a residual ten times tol^2 where the loop runs out), and
    float64 and long double agree to 1e-12 of the largest entry.  -> the trial stresses (n_elem, nq, 6)"""
    m, em, per_elem, st, ref = affine_model(etype, nlgeom, elemopt, reach=False)
    ref.element_update()
    assert not ref.st["istat"].any()
    trial = ref.st["stress"].copy()
    wide = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    for e, c in enumerate(per_elem):
        mat = material(c.mat, nlgeom)
        assert np.abs(trial[e] - c.stress).max() <= (1e-12 if nlgeom == INFINITE else 0.1) * np.abs(c.stress).max(), (c.name, trial[e][0], c.stress)
        for s in trial[e]:
            info = {}
            out, ist, fs = point(mat, s, np.float64(c.plstrain), c.istat, np.float64(c.fstat), info)
            tag = (etype, nlgeom, elemopt, c.mat, c.name, info)
            assert info["exit"] == c.exit and abs(abs(info["f"]) - TOL) >= 1.0e-4, tag
            for key in ("iterations", "triple"):
                if key in c.expect:
                    assert (info[key] if key == "iterations" else (info["maxp"], info["minp"], info["mm"])) == c.expect[key], tag
            if c.exit == "reset":
                cc, _, eta = mat.plconst
                p, root = (s[0] + s[1] + s[2]) / 3.0, float(T.mises(s)) / np.sqrt(3.0)
                assert min(abs(root - x) / x for x in (mat.plconst4 * cc - 3.0 * eta * p, mat.plconst4 * cc - eta * p)) >= 1.0e-6, tag
            if c.exit == "exhausted":
                assert abs(info["residual"]) >= 10.0 * TOL ** 2, tag
            if "principal" in info:
                pr = np.sort(info["principal"])
                assert min(pr[1] - pr[0], pr[2] - pr[1]) >= 1.0e-6 * np.abs(pr).max(), tag
            if c.name == "crossing":
                assert info["lookups"][0][:2] == ("segment", 0) and info["lookups"][-1][:2] == ("segment", 1), tag
                assert min(abs(fs - TABLE[1, 1]), abs(c.plstrain - TABLE[1, 1])) >= 1.0e-6, tag
            if wide and c.exit not in ("band", "elastic"):
                ol, il, fl = point(mat, s.astype(np.longdouble), np.longdouble(c.plstrain), c.istat, np.longdouble(c.fstat))
                assert il == ist and float(np.abs(ol - out).max()) <= 1e-12 * np.abs(out).max() and abs(float(fl) - fs) <= 1e-12 * max(abs(fs), 1e-3), tag
    return trial
