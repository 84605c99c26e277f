"""Heat conduction (!SOLUTION, TYPE=HEAT) on the device: the material tables of heat_init_material and the steady and the
transient loop of fistr1/src/analysis/heat/heat_solve_SS.f90 / heat_solve_TRAN.f90, with the element loops
(heat_mat_ass_conductivity, heat_mat_ass_capacity) in fx_heat_assemble_groups and the linear system in hecmw_solve (NDOF = 1).

!FIXTEMP and !CFLUX at constant amplitude; solid elements TYPE=341, 342, 351, 352, 361, 362 in any mix of groups.  Surface terms
(!FILM, !RADIATE, !DFLUX), amplitude tables and the automatic time step are not here.
"""
import numpy as np

from . import hecmw


class tHeatMaterial:
    """One material's three tables as heat_init_material (heat_init.f90:197-231) leaves them in fstrHEAT: per property
    (ntab, temp[ntab], funcA[ntab + 1], funcB[ntab + 1]) from rows [(value, temperature), ...]; cp and rho may be left out of a
    steady analysis."""

    def __init__(self, cond, cp=None, rho=None):
        self.cond = self.table(cond)
        self.cp = None if cp is None else self.table(cp)
        self.rho = None if rho is None else self.table(rho)

    @staticmethod
    def table(rows):
        rows = [(float(v), float(t)) for v, t in rows]
        n = len(rows)
        if n < 1:
            raise ValueError("a material table needs at least one row")
        temp = np.array([t for _, t in rows])
        fA, fB = np.zeros(n + 1), np.zeros(n + 1)
        fB[0] = rows[0][0]
        for k in range(1, n):
            bb = rows[k][0] - rows[k - 1][0]
            aa = rows[k][1] - rows[k - 1][1]
            fA[k] = bb / aa
            fB[k] = -(bb / aa) * rows[k - 1][1] + rows[k - 1][0]
        fB[n] = rows[n - 1][0]
        return n, temp, fA, fB


def heat_matrix(n_node, groups):
    """The scalar matrix (NDOF = 1) of a mesh of element groups [(etype, conn, ...)]: profile from hecmw_mat_con_groups,
    D, AL, AU, B, X zero."""
    mesh = hecmw.hecmwST_local_mesh(n_node=int(n_node))
    m = hecmw.hecmw_mat_con_groups(mesh, hecmw.hecmwST_matrix(), groups)
    m.NDOF = 1
    m.D, m.AL, m.AU = np.zeros(m.NP), np.zeros(max(m.NPL, 1))[:m.NPL], np.zeros(max(m.NPU, 1))[:m.NPU]
    m.B, m.X = np.zeros(m.NP), np.zeros(m.NP)
    return mesh, m


def _solver(hecMAT, resid, maxit, precond):
    hecMAT.Iarray[0], hecMAT.Iarray[1], hecMAT.Iarray[2] = int(maxit), 1, int(precond)
    hecMAT.Rarray[0] = float(resid)


def _solve(ctx, hecMESH, hecMAT):
    hecMAT.Iarray[96] = 1        # hecMAT%Iarray(97) = 1: need numerical factorization
    code = hecmw.hecmw_solve(hecMESH, hecMAT, ctx=ctx, want_history=False)
    if code not in (0, hecmw.HECMW_SOLVER_ERROR_ZERO_RHS):
        raise hecmw.HecmwSolverError(code, "the linear solver did not converge")


def heat_solve_SS(ctx, coord, groups, mats, temp, fix=None, flux=None, eps=1.0e-6, itmax=20, resid=1.0e-8, maxit=10000, precond=1,
                  matrix=None):
    """heat_solve_SS: BETA = 1, X = 0 before every solve, TEMPC <- TEMP <- X, CHK = sqrt(sum dT^2) < eps ends it, iterALL >= itmax
    without convergence raises (the reference aborts).  temp: the initial temperatures (n_node); fix = (nodes 1-based, values);
    flux (n_node).  -> (TEMP, [(iterALL, CHK), ...])"""
    coord = np.ascontiguousarray(coord, dtype=np.float64).reshape(-1, 3)
    hecMESH, hecMAT = heat_matrix(coord.shape[0], groups) if matrix is None else matrix
    _solver(hecMAT, resid, maxit, precond)
    TEMP = np.array(temp, dtype=np.float64)
    BETA, iterALL, hist = 1.0, 0, []
    while True:
        iterALL += 1
        hecMAT.X[:] = 0.0
        ctx.heat_assemble_groups(coord, groups, mats, hecMAT, TEMP, TEMP, beta=BETA, dtime=0.0, flux=flux, fix=fix)
        _solve(ctx, hecMESH, hecMAT)
        TEMPC = TEMP
        TEMP = hecMAT.X.copy()
        CHK = float(np.sqrt(np.sum((TEMP - TEMPC) ** 2)))
        hist.append((iterALL, CHK))
        if CHK < eps:
            return TEMP, hist
        if iterALL >= itmax:
            raise RuntimeError("ITERATION COUNT OVER : MAX = %d" % itmax)


def heat_solve_TRAN(ctx, coord, groups, mats, temp0, dtime, eetime, fix=None, flux=None, eps=1.0e-6, itmax=20, delmin=0.0,
                    resid=1.0e-8, maxit=10000, precond=1, matrix=None, keep=None):
    """heat_solve_TRAN with fixed steps: BETA = 0.5, X = 0 once before the loop, the last step clipped by
    TT + DTIME * 1.0000001 >= EETIME, per step the iteration on TEMP with TEMP0 held, iterALL > itmax without convergence raises,
    then TEMP0 <- TEMP.  keep: a list that receives every step's temperatures (what `!WRITE,RESULT` writes per step).
    -> (TEMP, [[(iterALL, CHK), ...] per step], [time per step])"""
    if delmin > 0.0:
        raise NotImplementedError("the automatic time step (DELMIN > 0) is not restated")
    coord = np.ascontiguousarray(coord, dtype=np.float64).reshape(-1, 3)
    hecMESH, hecMAT = heat_matrix(coord.shape[0], groups) if matrix is None else matrix
    _solver(hecMAT, resid, maxit, precond)
    TEMP0 = np.array(temp0, dtype=np.float64)
    TEMP = TEMP0.copy()
    TT, DTIME, EETIME, BETA = 0.0, float(dtime), float(eetime), 0.5
    hecMAT.X[:] = 0.0
    steps, times = [], []
    while True:
        if TT + DTIME * 1.0000001 >= EETIME:
            DTIME = EETIME - TT
            TT = EETIME
            iend = 1
        else:
            TT = TT + DTIME
            iend = 0
        iterALL, hist = 0, []
        while True:
            iterALL += 1
            ctx.heat_assemble_groups(coord, groups, mats, hecMAT, TEMP, TEMP0, beta=BETA, dtime=DTIME, flux=flux, fix=fix)
            _solve(ctx, hecMESH, hecMAT)
            TEMPC = TEMP
            TEMP = hecMAT.X.copy()
            CHK = float(np.sqrt(np.sum((TEMP - TEMPC) ** 2)))
            hist.append((iterALL, CHK))
            if CHK < eps:
                break
            if iterALL > itmax:
                raise RuntimeError("ITERATION COUNT OVER : MAX = %d" % itmax)
        TEMP0 = TEMP.copy()
        steps.append(hist)
        times.append(TT)
        if keep is not None:
            keep.append(TEMP.copy())
        if iend:
            return TEMP, steps, times
