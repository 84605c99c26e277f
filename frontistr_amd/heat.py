"""Heat conduction (!SOLUTION, TYPE=HEAT) on the device: the material tables of heat_init_material, the amplitude tables of
heat_init_amplitude and the steady and the transient loop of fistr1/src/analysis/heat/heat_solve_SS.f90 / heat_solve_TRAN.f90,
with the element loops (heat_mat_ass_conductivity, heat_mat_ass_capacity) and the surface terms of heat_mat_ass_boundary
(heat_mat_ass_bc_DFLUX with the body flux, _FILM, _RADIATE) in fx_heat_assemble_groups / fx_heat_assemble_groups_bc and the linear
system in hecmw_solve (NDOF = 1).

!FIXTEMP, !CFLUX, !DFLUX (S1.. and BF), !FILM and !RADIATE, each with an optional !AMPLITUDE; solid elements TYPE=341, 342, 351,
352, 361, 362 in any mix of groups.  The weld line of !DFLUX, shells, planes and interface elements, and the automatic time step
are not here.
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


class tHeatAmplitude:
    """One !AMPLITUDE as heat_init_amplitude (heat_init.f90:30-86) leaves it in fstrHEAT -- AMPLtab, AMPLtime, AMPLfuncA, AMPLfuncB --
    from rows [(value, time), ...]; calling it is heat_get_amplitude: the first value before the first row, the last from the last
    row on, the row's line in between."""

    def __init__(self, rows):
        rows = [(float(v), float(t)) for v, t in rows]
        nn = len(rows)
        if nn < 1:
            raise ValueError("an amplitude needs at least one row")
        self.AMPLtab = nn
        self.AMPL = np.array([v for v, _ in rows])
        self.AMPLtime = np.array([t for _, t in rows])
        self.AMPLfuncA, self.AMPLfuncB = np.zeros(nn + 1), np.zeros(nn + 1)
        self.AMPLfuncB[0] = self.AMPL[0]
        for k in range(1, nn):
            x1, y1, x2, y2 = self.AMPLtime[k - 1], self.AMPL[k - 1], self.AMPLtime[k], self.AMPL[k]
            self.AMPLfuncA[k] = (y2 - y1) / (x2 - x1)
            self.AMPLfuncB[k] = -(y2 - y1) / (x2 - x1) * x1 + y1
        self.AMPLfuncB[nn] = self.AMPL[nn - 1]

    def __call__(self, TT):
        nn = self.AMPLtab
        if TT < self.AMPLtime[0]:
            ii = 0
        elif TT >= self.AMPLtime[nn - 1]:
            ii = nn
        else:
            ii = 1
            for ikk in range(nn - 1):
                if self.AMPLtime[ikk] <= TT < self.AMPLtime[ikk + 1]:
                    ii = ikk + 1
                    break
        return float(self.AMPLfuncA[ii] * TT + self.AMPLfuncB[ii])


def heat_get_amplitude(amplitude, TT):
    """QQ of heat_get_amplitude: 1 for "no amplitude" (id = 0)"""
    return 1.0 if amplitude is None else amplitude(TT)


def surface_of_egroup(groups, elems, face, val, sink=None, amplitude=None, sink_amplitude=None):
    """A card on an element group -- `!DFLUX EGRP, S2, v`, `!FILM EGRP, F1, h, sink` -- as the tuple heat_solve_SS / heat_solve_TRAN
    take: elems are 0-based positions in the concatenation of the groups (the order of hecMESH); face is the number behind S, F or
    R, or 0 for BF.  -> (group, elem, face, val[, sink], amplitude[, sink_amplitude])"""
    elems = np.asarray(elems, dtype=np.int64).ravel()
    start = np.concatenate([[0], np.cumsum([np.asarray(g[1]).shape[0] for g in groups])])
    grp = np.searchsorted(start, elems, side="right") - 1
    if elems.size and (elems.min() < 0 or elems.max() >= start[-1]):
        raise ValueError("element position out of range")
    head = (grp.astype(np.int32), (elems - start[grp]).astype(np.int32), np.full(elems.size, int(face), dtype=np.int32),
            np.full(elems.size, float(val)))
    if sink is None:
        return head + (amplitude,)
    return head + (np.full(elems.size, float(sink)), amplitude, sink_amplitude)


def _at_time(lst, nval, TT):
    """(group, elem, face, nval values, up to nval amplitudes) -> the list at time TT, values times QQ"""
    if lst is None:
        return None
    amps = list(lst[3 + nval:]) + [None] * nval
    return tuple(lst[:3]) + tuple(np.asarray(v, dtype=np.float64) * heat_get_amplitude(a, TT) for v, a in zip(lst[3:3 + nval], amps))


def _boundary_at(TT, fix, flux, fix_amplitude, flux_amplitude, dflux, film, radiate, tzero):
    """the boundary arguments of heat_assemble_groups at CTIME = TT: every value times its amplitude (heat_mat_ass_bc_*)"""
    kw = dict(fix=fix, flux=flux)
    if fix is not None and fix_amplitude is not None:
        kw["fix"] = (fix[0], np.asarray(fix[1], dtype=np.float64) * fix_amplitude(TT))
    if flux is not None and flux_amplitude is not None:
        kw["flux"] = np.asarray(flux, dtype=np.float64) * flux_amplitude(TT)
    if dflux is not None or film is not None or radiate is not None:
        kw.update(dflux=_at_time(dflux, 1, TT), film=_at_time(film, 2, TT), radiate=_at_time(radiate, 2, TT), tzero=tzero)
    return kw


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
                  matrix=None, dflux=None, film=None, radiate=None, tzero=0.0, fix_amplitude=None, flux_amplitude=None):
    """heat_solve_SS: BETA = 1, X = 0 before every solve, TEMPC <- TEMP <- X, CHK = sqrt(sum dT^2) < eps ends it, iterALL >= itmax
    without convergence raises (the reference aborts).  temp: the initial temperatures (n_node); fix = (nodes 1-based, values);
    flux (n_node); dflux = (group, elem, face, val[, amplitude]), film and radiate = (group, elem, face, val, sink[, amplitude[,
    sink amplitude]]) as surface_of_egroup makes them; tzero: !ZERO.  Amplitudes (tHeatAmplitude) are taken at CTIME = STIME + ETIME
    = 0 (heat_solve_SS.f90:59).  -> (TEMP, [(iterALL, CHK), ...])"""
    coord = np.ascontiguousarray(coord, dtype=np.float64).reshape(-1, 3)
    hecMESH, hecMAT = heat_matrix(coord.shape[0], groups) if matrix is None else matrix
    _solver(hecMAT, resid, maxit, precond)
    TEMP = np.array(temp, dtype=np.float64)
    BETA, iterALL, hist = 1.0, 0, []
    bnd = _boundary_at(0.0, fix, flux, fix_amplitude, flux_amplitude, dflux, film, radiate, tzero)
    while True:
        iterALL += 1
        hecMAT.X[:] = 0.0
        ctx.heat_assemble_groups(coord, groups, mats, hecMAT, TEMP, TEMP, beta=BETA, dtime=0.0, **bnd)
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
                    resid=1.0e-8, maxit=10000, precond=1, matrix=None, keep=None, dflux=None, film=None, radiate=None, tzero=0.0,
                    fix_amplitude=None, flux_amplitude=None):
    """heat_solve_TRAN with fixed steps: BETA = 0.5, X = 0 once before the loop, the last step clipped by
    TT + DTIME * 1.0000001 >= EETIME, per step the iteration on TEMP with TEMP0 held, iterALL > itmax without convergence raises,
    then TEMP0 <- TEMP.  keep: a list that receives every step's temperatures (what `!WRITE,RESULT` writes per step).
    dflux, film, radiate, tzero and the amplitudes as in heat_solve_SS; they are taken at CTIME = TT + ST with ST = 0, the first
    step of an analysis (heat_solve_TRAN.f90:137).
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
        bnd = _boundary_at(TT, fix, flux, fix_amplitude, flux_amplitude, dflux, film, radiate, tzero)
        while True:
            iterALL += 1
            ctx.heat_assemble_groups(coord, groups, mats, hecMAT, TEMP, TEMP0, beta=BETA, dtime=DTIME, **bnd)
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
