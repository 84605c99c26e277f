"""Host-side mirror of the reference's solver interface on top of the C ABI
(include/fistr_hip.h -> frontistr_amd/libfistr_hip.so).

The reference's host language is Fortran; the production binding is the shim
frontistr_amd/shim/hecmw_solver_hip.f90.  This module is
the same boundary for Python callers, tests and bench.py, with the reference's
names and argument meaning:

    hecmwST_matrix       hecmw1/src/common/hecmw_util_f.F90:433-468
    hecmwST_local_mesh   (communication part) hecmw_util_f.F90:298-310
    hecmw_mat_init       hecmw1/src/solver/matrix/hecmw_matrix_misc.f90:142-182
    hecmw_mat_con        hecmw1/src/solver/matrix/hecmw_mat_con.f90:23
    hecmw_solve          hecmw1/src/solver/hecmw_solver.f90:9
    hecmw_matvec         hecmw1/src/solver/las/hecmw_solver_las.f90:57
    fstr_StiffMatrix     fistr1/src/analysis/static/fstr_StiffMatrix.f90:18 (+ hecmw_mat_ass_bc)

There is NO CPU fallback: a missing library or GPU raises.
"""
import ctypes as C
import os

import numpy as np

from .mesh import C3_NODES as _C3_NODES, C3_POINTS as _C3_POINTS      # nodes and quadrature points of the six solid types

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(_HERE, "libfistr_hip.so")
_lib = None

# hecmw_solve_error.f90:9-15
HECMW_SOLVER_ERROR_INCONS_PC = 1001
HECMW_SOLVER_ERROR_ZERO_DIAG = 2001
HECMW_SOLVER_ERROR_ZERO_RHS = 2002
HECMW_SOLVER_ERROR_NOCONV_MAXIT = 3001
HECMW_SOLVER_ERROR_DIVERGE_MAT = 3002
HECMW_SOLVER_ERROR_DIVERGE_PC = 3003

FX_UP_PROFILE, FX_UP_VALUES, FX_UP_RHS, FX_UP_X, FX_UP_ALL = 1, 2, 4, 8, 15


class HecmwSolverError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("HEC-MW-SOLVER %d: %s" % (code, msg))
        self.code = code


class _MatrixView(C.Structure):
    _fields_ = [("N", C.c_int32), ("NP", C.c_int32), ("NPL", C.c_int32), ("NPU", C.c_int32), ("NDOF", C.c_int32),
                ("indexL", C.c_void_p), ("itemL", C.c_void_p), ("indexU", C.c_void_p), ("itemU", C.c_void_p),
                ("D", C.c_void_p), ("AL", C.c_void_p), ("AU", C.c_void_p), ("B", C.c_void_p), ("X", C.c_void_p)]


class _CommView(C.Structure):
    _fields_ = [("my_rank", C.c_int32), ("PETOT", C.c_int32), ("nn_internal", C.c_int32), ("n_node", C.c_int32),
                ("n_neighbor_pe", C.c_int32),
                ("neighbor_pe", C.c_void_p), ("import_index", C.c_void_p), ("import_item", C.c_void_p),
                ("export_index", C.c_void_p), ("export_item", C.c_void_p)]


class _SolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("method", C.c_int32), ("precond", C.c_int32), ("ncolor", C.c_int32),
                ("n_hist", C.c_int32), ("resid", C.c_double), ("rel_resid", C.c_double),
                ("time_setup", C.c_double), ("time_sol", C.c_double), ("time_comm", C.c_double),
                ("time_matvec", C.c_double), ("time_precond", C.c_double)]


class _MeshView(C.Structure):
    _fields_ = [("n_node", C.c_int32), ("n_elem", C.c_int32), ("coord", C.c_void_p), ("conn", C.c_void_p)]


class _ElemGroup(C.Structure):      # fx_elem_group
    _fields_ = [("etype", C.c_int32), ("elemopt", C.c_int32), ("n_elem", C.c_int32), ("conn", C.c_void_p),
                ("elem_mat", C.c_void_p)]


class _ThermalView(C.Structure):    # fx_thermal_view
    _fields_ = [("temp", C.c_void_p), ("temp0", C.c_void_p), ("ref_temp", C.c_double), ("alpha", C.c_void_p)]


class _HeatTable(C.Structure):      # fx_heat_table
    _fields_ = [("ntab", C.c_int32), ("temp", C.c_void_p), ("funcA", C.c_void_p), ("funcB", C.c_void_p)]


class _HeatMaterialView(C.Structure):   # fx_heat_material_view
    _fields_ = [("cond", _HeatTable), ("cp", _HeatTable), ("rho", _HeatTable)]


class _HeatView(C.Structure):       # fx_heat_view
    _fields_ = [("temp", C.c_void_p), ("temp0", C.c_void_p), ("beta", C.c_double), ("dtime", C.c_double)]


class _HeatSurface(C.Structure):    # fx_heat_surface
    _fields_ = [("n", C.c_int32), ("group", C.c_void_p), ("elem", C.c_void_p), ("face", C.c_void_p), ("val", C.c_void_p),
                ("sink", C.c_void_p)]


class _HeatBc(C.Structure):         # fx_heat_bc
    _fields_ = [("dflux", _HeatSurface), ("film", _HeatSurface), ("radiate", _HeatSurface), ("tzero", C.c_double)]


class _Dload(C.Structure):          # fx_dload
    _fields_ = [("n", C.c_int32), ("group", C.c_void_p), ("elem", C.c_void_p), ("ltype", C.c_void_p), ("params", C.c_void_p),
                ("held", C.c_void_p)]


class _NodalResult(C.Structure):    # fx_nodal_result
    _fields_ = [("n_node", C.c_int32), ("n_elem", C.c_int32)] + [(k, C.POINTER(C.c_double)) for k in (
        "strain", "stress", "mises", "estrain", "estress", "emises", "pstress", "pstress_vect", "pstrain", "pstrain_vect",
        "epstress", "epstress_vect", "epstrain", "epstrain_vect")]


# make_principal's flag bits (fstr_NodalStress.f90:889-980)
PRINC_NSTRESS, PRINCV_NSTRESS, PRINC_NSTRAIN, PRINCV_NSTRAIN = 1, 2, 4, 8
PRINC_ESTRESS, PRINCV_ESTRESS, PRINC_ESTRAIN, PRINCV_ESTRAIN = 16, 32, 64, 128


class NodalStress:
    """What fstr_NodalStress3D leaves in fstrSOLID: copies of the arrays of an fx_nodal_result.  strain, stress (n_node, 6),
    mises (n_node), estrain, estress (n_elem, 6), emises (n_elem); the eight principal arrays -- values (n, 3) in descending
    order, vectors (n, 3, 3) indexed [item, vector, component], each vector scaled by its value -- or None where the flag of
    ``principal`` was off.  ms: the kernels' milliseconds."""
    _SHAPES = (("strain", 0, (6,)), ("stress", 0, (6,)), ("mises", 0, ()), ("estrain", 1, (6,)), ("estress", 1, (6,)),
               ("emises", 1, ()), ("pstress", 0, (3,)), ("pstress_vect", 0, (3, 3)), ("pstrain", 0, (3,)),
               ("pstrain_vect", 0, (3, 3)), ("epstress", 1, (3,)), ("epstress_vect", 1, (3, 3)), ("epstrain", 1, (3,)),
               ("epstrain_vect", 1, (3, 3)))
    COMPONENTS = ("11", "22", "33", "12", "23", "31")

    def __init__(self, res, ms=0.0):
        self.n_node, self.n_elem, self.ms = int(res.n_node), int(res.n_elem), float(ms)
        for name, per_elem, tail in self._SHAPES:
            p = getattr(res, name)
            shape = ((self.n_elem if per_elem else self.n_node),) + tail
            setattr(self, name, np.ctypeslib.as_array(p, shape=shape).copy() if p and shape[0] > 0 else
                    (np.zeros(shape) if p else None))

    def summary(self, unode=None):
        """The `Global Summary` block of 0.log as oracle/fistr1_run.read_log returns one step of it: {'Node': {name: (max,
        min)}, 'Element': {...}} with the five digits the program prints (1PE11.4).  unode (3 * n_node): adds U1..U3."""
        ext = lambda v: (float("%.4E" % v.max()), float("%.4E" % v.min()))
        node, elem = {}, {}
        if unode is not None:
            U = np.asarray(unode, dtype=np.float64).reshape(-1, 3)
            node.update({"U%d" % (c + 1): ext(U[:, c]) for c in range(3)})
        for k, c in enumerate(self.COMPONENTS):
            node["E" + c], node["S" + c] = ext(self.strain[:, k]), ext(self.stress[:, k])
            elem["E" + c], elem["S" + c] = ext(self.estrain[:, k]), ext(self.estress[:, k])
        node["SMS"], elem["SMS"] = ext(self.mises), ext(self.emises)
        return {"Node": node, "Element": elem}


def lib():
    """Load libfistr_hip.so (built by `make -C frontistr_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBPATH):
            raise ImportError("%s missing: run `make -C frontistr_amd/csrc` (hipcc, gfx950). "
                              "There is no CPU fallback." % LIBPATH)
        L = C.CDLL(LIBPATH)
        L.fx_last_error.restype = C.c_char_p
        L.fx_version.restype = C.c_char_p
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _chk(code, allow=()):
    if code == 0 or code in allow:
        return code
    raise HecmwSolverError(code, lib().fx_last_error().decode(errors="replace"))


class hecmwST_matrix:
    """Same members as the reference type; index arrays are int32, items 1-based."""

    def __init__(self):
        self.N = self.NP = self.NPL = self.NPU = 0
        self.NDOF = 3
        self.indexL = self.itemL = self.indexU = self.itemU = None
        self.D = self.AL = self.AU = self.B = self.X = None
        self.Iarray = np.zeros(100, dtype=np.int32)
        self.Rarray = np.zeros(100, dtype=np.float64)
        hecmw_mat_init(self)

    @classmethod
    def from_arrays(cls, N, NP, indexL, itemL, indexU, itemU, D, AL, AU, B=None, X=None, NDOF=3):
        m = cls()
        m.N, m.NP, m.NDOF = int(N), int(NP), int(NDOF)
        m.indexL = np.ascontiguousarray(indexL, dtype=np.int32)
        m.itemL = np.ascontiguousarray(itemL, dtype=np.int32)
        m.indexU = np.ascontiguousarray(indexU, dtype=np.int32)
        m.itemU = np.ascontiguousarray(itemU, dtype=np.int32)
        m.NPL, m.NPU = int(m.itemL.size), int(m.itemU.size)
        m.D = None if D is None else np.ascontiguousarray(D, dtype=np.float64)
        m.AL = None if AL is None else np.ascontiguousarray(AL, dtype=np.float64)
        m.AU = None if AU is None else np.ascontiguousarray(AU, dtype=np.float64)
        m.B = np.zeros(m.NDOF * m.NP) if B is None else np.ascontiguousarray(B, dtype=np.float64)
        m.X = np.zeros(m.NDOF * m.NP) if X is None else np.ascontiguousarray(X, dtype=np.float64)
        return m

    def view(self):
        v = _MatrixView(self.N, self.NP, self.NPL, self.NPU, self.NDOF, _ptr(self.indexL), _ptr(self.itemL),
                        _ptr(self.indexU), _ptr(self.itemU), _ptr(self.D), _ptr(self.AL), _ptr(self.AU),
                        _ptr(self.B), _ptr(self.X))
        v._keep = self
        return v


def hecmw_mat_init(hecMAT):
    """hecmw_matrix_misc.f90:142-182 defaults (1-based slot k lives at index k-1)."""
    I, R = hecMAT.Iarray, hecMAT.Rarray
    I[:] = 0
    R[:] = 0.0
    I[0] = 100      # iter
    I[1] = 1        # method  CG
    I[2] = 1        # precond SSOR
    I[4] = 1        # iterPREmax
    I[5] = 10       # nrest
    I[33] = 10      # ncolor_in
    I[34] = 3       # maxrecycle_precond
    I[12] = 3       # mpc_method
    I[96] = 1       # flag_numfact
    I[97] = 1       # flag_symbfact
    I[98] = 1       # solver_type: iterative
    R[0] = 1.0e-8   # resid
    R[1] = 1.0      # sigma_diag
    R[3] = 0.10     # thresh
    R[4] = 0.10     # filter
    R[10] = 1.0e4   # penalty


class hecmwST_local_mesh:
    """Only what the hot path reads (hecmw_util_f.F90:298-310) + mesh arrays for assembly."""

    def __init__(self, n_node=0, nn_internal=None):
        self.n_node = n_node
        self.nn_internal = n_node if nn_internal is None else nn_internal
        self.my_rank, self.PETOT, self.zero = 0, 1, 0
        self.n_neighbor_pe = 0
        self.neighbor_pe = np.zeros(0, dtype=np.int32)
        self.import_index = np.zeros(1, dtype=np.int32)
        self.import_item = np.zeros(0, dtype=np.int32)
        self.export_index = np.zeros(1, dtype=np.int32)
        self.export_item = np.zeros(0, dtype=np.int32)
        self.node = None            # 3*n_node coordinates
        self.elem_node_item = None  # flattened connectivity, 1-based
        self.nn_elem = 8            # nodes per element of elem_node_item (8: TYPE=361, 4: 341, 10: 342, 6: 351, 15: 352, 20: 362)
        self.n_elem = 0

    def comm_view(self):
        v = _CommView(self.my_rank, self.PETOT, self.nn_internal, self.n_node, self.n_neighbor_pe,
                      _ptr(self.neighbor_pe), _ptr(self.import_index), _ptr(self.import_item),
                      _ptr(self.export_index), _ptr(self.export_item))
        v._keep = self
        return v


def _bc_arrays(bc, load):
    """(bc_node, bc_dof, bc_val, load) as the assembly entry points take them: bc = (nodes, dofs, values) or None."""
    bn, bd, bv = ((), (), ()) if bc is None else bc
    return (np.ascontiguousarray(bn, dtype=np.int32), np.ascontiguousarray(bd, dtype=np.int32),
            np.ascontiguousarray(bv, dtype=np.float64), None if load is None else np.ascontiguousarray(load, dtype=np.float64))


def _material_arrays(E, nu, elem_mat=None):
    """(E[], nu[], elem_mat[] or None): scalars become one-entry tables; elem_mat is 1-based per element."""
    return (np.atleast_1d(np.asarray(E, dtype=np.float64)).copy(), np.atleast_1d(np.asarray(nu, dtype=np.float64)).copy(),
            None if elem_mat is None else np.ascontiguousarray(elem_mat, dtype=np.int32))


def _staged(p, n_elem, nq):
    """A copy (n_elem, nq, 6) of one result in the context's pinned staging, which the next update on the context overwrites."""
    if n_elem == 0:
        return np.zeros((0, nq, 6))
    return np.ctypeslib.as_array(p, shape=(6 * nq * n_elem,)).reshape(-1, nq, 6).copy()


class SolverContext:
    """Device state the reference keeps in module-level `save` variables."""

    def __init__(self, device=-1):
        self.h = C.c_void_p()
        _chk(lib().fx_create(device, C.byref(self.h)))
        self.info = None
        self.history = None
        self.messages = []

    def close(self):
        if self.h:
            lib().fx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- staged device-resident API -------------------------------------
    def upload(self, hecMAT, hecMESH=None, what=FX_UP_ALL):
        mv = hecMAT.view()
        cv = hecMESH.comm_view() if hecMESH is not None else None
        _chk(lib().fx_upload(self.h, C.byref(mv), C.byref(cv) if cv is not None else None, what))

    def precond_setup(self, hecMAT):
        _chk(lib().fx_precond_setup(self.h, _ptr(hecMAT.Iarray), _ptr(hecMAT.Rarray)))

    def set_option(self, name, value):
        """Tuning knob of the live context (the FX_* names of csrc/fx_internal.h)."""
        f = lib().fx_set_option
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        _chk(f(self.h, name.encode(), float(value)))

    def placement_report(self):
        """Where the value arrays of the sliced layouts live (fx_placement_report): the context's value arena."""
        out = (C.c_double * 9)()
        _chk(lib().fx_placement_report(self.h, out))
        return {"arena_bytes": int(out[0]), "arena_used_bytes": int(out[1]), "arrays_in_arena": int(out[2]),
                "spmv_values_in_arena": bool(out[3]), "lower_values_in_arena": bool(out[4]), "upper_values_in_arena": bool(out[5]),
                "spmv_value_bytes": int(out[6]), "arenas_timed": int(out[7]), "kept_ms": float(out[8])}

    def march_report(self):
        """The plane march of the level-scheduled sweeps of this context (fx_march_report)."""
        out = (C.c_double * 16)()
        _chk(lib().fx_march_report(self.h, out))
        keys = ("built", "chunk_rows", "chunks", "pair_waves", "rounds_fwd", "rounds_bwd", "near_blocks", "far_blocks",
                "far_same_chunk", "est_us", "est_level_us", "build_s", "applies", "grid", "max_round_rows", "levels")
        d = {k: float(out[i]) for i, k in enumerate(keys)}
        for k in keys:
            if k not in ("est_us", "est_level_us", "build_s"):
                d[k] = int(d[k])
        return d

    def march_trace(self):
        """Diagnostics: one traced march apply (fx_debug_march_trace) -> array [chunks, 8]: forward start / end, backward start / end
        in microseconds, rounds that waited and polls, forward / backward."""
        n = self.march_report()["chunks"]
        out = np.zeros(8 * max(n, 1))
        nch = C.c_int32(0)
        f = lib().fx_debug_march_trace
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        _chk(f(self.h, _ptr(out), out.size, C.byref(nch)))
        a = out.reshape(-1, 8)
        a[:, :4] = np.where(a[:, :4] >= 0, a[:, :4] * 0.01, -1.0)
        return a

    def march_rounds(self, chunk):
        """Diagnostics: when each round of one chunk's forward sweep passed its barrier (us; negative = the round waited)."""
        out = np.zeros(1 << 16)
        n = C.c_int32(0)
        f = lib().fx_debug_march_rounds
        f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        _chk(f(self.h, int(chunk), _ptr(out), out.size, C.byref(n)))
        return out[:n.value].copy()

    def solve_resident(self, hecMAT, want_history=True):
        info = _SolveInfo()
        maxit = int(hecMAT.Iarray[0])
        hist = np.zeros(max(maxit, 1) + 1) if want_history else None   # GMRES logs MAXIT+1 lines when it runs out
        code = lib().fx_solve_resident(self.h, _ptr(hecMAT.Iarray), _ptr(hecMAT.Rarray), C.byref(info),
                                       _ptr(hist), 0 if hist is None else hist.size)
        self._finish(code, info, hist)
        return code

    def download_x(self, hecMAT):
        _chk(lib().fx_download_x(self.h, _ptr(hecMAT.X), hecMAT.X.size))
        return hecMAT.X

    def download_matrix(self, hecMAT):
        for k, n in (("D", 9 * hecMAT.NP), ("AL", 9 * hecMAT.NPL), ("AU", 9 * hecMAT.NPU)):
            if getattr(hecMAT, k) is None:
                setattr(hecMAT, k, np.zeros(max(n, 1)))
        _chk(lib().fx_download_matrix(self.h, _ptr(hecMAT.D), _ptr(hecMAT.AL), _ptr(hecMAT.AU), _ptr(hecMAT.B)))

    def matvec_resident_ms(self, nrepeat=10):
        ms = C.c_float(0)
        _chk(lib().fx_matvec_resident(self.h, nrepeat, C.byref(ms)))
        return ms.value

    def spmv_resident_ms(self, variant=1, nrepeat=10):
        """variant 0 plain, 1 with the fused x.y partial (the CG loop's launch), 2 residual + r.r partial."""
        ms = C.c_float(0)
        _chk(lib().fx_spmv_resident(self.h, int(variant), nrepeat, C.byref(ms)))
        return ms.value

    def precond_apply_ms(self, nrepeat=5):
        ms = C.c_float(0)
        _chk(lib().fx_precond_apply_resident(self.h, nrepeat, C.byref(ms)))
        return ms.value

    def stream_ceiling_gbs(self, nrepeat=5):
        out = C.c_double(0)
        _chk(lib().fx_stream_ceiling(self.h, nrepeat, C.byref(out)))
        return out.value

    def stats(self):
        out = (C.c_int64 * 16)()
        _chk(lib().fx_get_stats(self.h, out))
        keys = ("N", "NP", "NPL", "NPU", "M_pairs", "M_blocks", "M_slices", "ncolor", "L_pairs", "L_blocks",
                "U_pairs", "U_blocks", "ssor_slices", "wg_interior", "wg_boundary", "eisenstat")
        st = {k: int(out[i]) for i, k in enumerate(keys)}
        v = st["eisenstat"]
        st["ssor_natural"] = (v >> 1) & 1     # PRECOND = 1 resident as the natural-order (level-scheduled) SSOR
        st["df_mode"] = (v >> 2) & 3            # 0: one launch per colour / level; 1: dataflow ILU(0) sweeps; 2: also SSOR
        st["df_fallbacks"] = (v >> 8) & 0xFF    # timed-out dataflow sweeps that made the context fall back to df_mode 0
        st["df_grid"] = v >> 16                 # workgroups of the last dataflow launch (after the co-residency clamp)
        st["eisenstat"] = v & 1
        return st

    def eis_tail_stats(self):
        """The dataflow tail of the Eisenstat sweeps (fx_eis_tail_stats): first tail colour of the last iteration (== ncolor: none),
        its slices, workgroups of the backward tail launch, tail launches enqueued or captured so far, colours, co-resident grid."""
        out = (C.c_int64 * 6)()
        _chk(lib().fx_eis_tail_stats(self.h, out))
        keys = ("color0", "slices", "grid", "launches", "ncolor", "grid_max")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def krylov_begin(self, hecMAT):
        _chk(lib().fx_krylov_begin(self.h, _ptr(hecMAT.Iarray), _ptr(hecMAT.Rarray)))

    def krylov_steps(self, nsteps):
        it, st, rs = C.c_int32(0), C.c_int32(0), C.c_double(0)
        _chk(lib().fx_krylov_steps(self.h, int(nsteps), C.byref(it), C.byref(st), C.byref(rs)))
        return it.value, st.value, rs.value

    def comm_ledger(self):
        """What this rank asked of the transport since it was set up (fx_comm_ledger): dict with ops, seq_hash, allreduces,
        allreduce_bytes, halos, own_halo_comm and peers = {rank: (sends, send_bytes, recvs, recv_bytes)}."""
        n = C.c_int32(0)
        _chk(lib().fx_comm_ledger(self.h, None, 0, C.byref(n)))
        out = (C.c_int64 * max(n.value, 1))()
        _chk(lib().fx_comm_ledger(self.h, out, n.value, C.byref(n)))
        v = list(out)[:n.value]
        peers = {int(v[7 + 5 * k]): tuple(int(x) for x in v[8 + 5 * k:12 + 5 * k]) for k in range(int(v[5]))}
        return {"ops": int(v[0]), "seq_hash": int(v[1]) & 0xFFFFFFFFFFFFFFFF, "allreduces": int(v[2]), "allreduce_bytes": int(v[3]),
                "halos": int(v[4]), "own_halo_comm": bool(v[6]), "peers": peers}

    def krylov_history(self):
        """RESID per iteration of the staged loop since krylov_begin (the reference's ITERLOG lines, hecmw_solver_CG.f90:245)."""
        n = C.c_int32(0)
        _chk(lib().fx_krylov_history(self.h, None, 0, C.byref(n)))
        h = np.zeros(max(n.value, 1))
        _chk(lib().fx_krylov_history(self.h, _ptr(h), n.value, C.byref(n)))
        return h[:n.value]

    def nn_precond_apply(self, hecMAT, r, hecMESH=None):
        """NDOF != 3: hecmw_precond_setup + hecmw_precond_apply -- uploads hecMAT, sets up (or reuses) the preconditioner its
        Iarray / Rarray select, returns z = M^-1 r (NDOF*NP doubles, halo part 0).  Iarray(97) / (98) are cleared as a set-up does."""
        mv = hecMAT.view()
        cv = hecMESH.comm_view() if hecMESH is not None else None
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert r.size == hecMAT.NDOF * hecMAT.NP
        z = np.zeros_like(r)
        _chk(lib().fx_nn_precond_apply(self.h, C.byref(mv), C.byref(cv) if cv is not None else None, _ptr(hecMAT.Iarray),
                                       _ptr(hecMAT.Rarray), _ptr(r), _ptr(z)))
        return z

    def nn_precond_apply_ms(self, nrepeat=10):
        """Timed applies of the resident NDOF != 3 preconditioner (ms per apply)."""
        ms = C.c_float(0)
        _chk(lib().fx_nn_precond_apply_resident(self.h, int(nrepeat), C.byref(ms)))
        return ms.value

    def nn_precond_stats(self):
        out = (C.c_int64 * 10)()
        _chk(lib().fx_nn_precond_stats(self.h, out))
        keys = ("kind", "levels", "slices", "max_row_blocks", "factor_lanes", "L_blocks", "U_blocks", "setup_us", "dataflow")
        st = {k: int(out[i]) for i, k in enumerate(keys)}
        st["df_grid"], st["df_fallbacks"] = int(out[9]) & 0xFFFFFFFF, int(out[9]) >> 32
        return st

    def solve_attempts(self):
        """(method, SIGMA_DIAG, ITERLOG lines) of every pass of the last solve's retry loop."""
        n = C.c_int32(0)
        _chk(lib().fx_solve_attempts(self.h, 0, C.byref(n), None, None, None))
        k = n.value
        meth = np.zeros(max(k, 1), dtype=np.int32)
        sig = np.zeros(max(k, 1))
        nh = np.zeros(max(k, 1), dtype=np.int32)
        _chk(lib().fx_solve_attempts(self.h, k, C.byref(n), _ptr(meth), _ptr(sig), _ptr(nh)))
        return [(int(meth[i]), float(sig[i]), int(nh[i])) for i in range(k)]

    def precond_apply(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        _chk(lib().fx_precond_apply_host(self.h, _ptr(r), _ptr(z)))
        return z

    def dot(self, x, y):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        out = C.c_double(0)
        _chk(lib().fx_dot_host(self.h, _ptr(x), _ptr(y), C.byref(out)))
        return out.value

    def assemble_c3d8(self, coord, conn, E, nu, elemopt=1, load=None, bc=None, sections=None):
        """fstr_StiffMatrix + fstr_AddBC on the device.  sections = (E[], nu[], elem_mat[] 1-based): several materials."""
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        mv = _MeshView(coord.shape[0], conn.shape[0], _ptr(coord), _ptr(conn))
        bn, bd, bv, load = _bc_arrays(bc, load)
        ms = C.c_float(0)
        if sections is not None:
            Es, nus, em = _material_arrays(*sections)
            _chk(lib().fx_assemble_c3d8_sections(self.h, C.byref(mv), int(Es.size), _ptr(Es), _ptr(nus), _ptr(em), int(elemopt),
                                                 _ptr(load), int(bn.size), _ptr(bn), _ptr(bd), _ptr(bv), C.byref(ms)))
            return ms.value
        _chk(lib().fx_assemble_c3d8(self.h, C.byref(mv), C.c_double(E), C.c_double(nu), int(elemopt), _ptr(load),
                                    int(bn.size), _ptr(bn), _ptr(bd), _ptr(bv), C.byref(ms)))
        return ms.value

    def update_c3d8_linear(self, coord, conn, E, nu, disp, elemopt=1, elem_mat=None):
        """fstr_UpdateNewton of a linear static analysis on the device (fx_update_c3d8_linear): strain, stress (n_elem, 8, 6) at the
        quadrature points and QFORCE (3 * n_node) from the total displacement; E, nu scalars or per-material arrays with
        elem_mat (1-based).  Returns (strain, stress, qforce, kernel ms)."""
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        disp = np.ascontiguousarray(disp, dtype=np.float64)
        Es, nus, em = _material_arrays(E, nu, elem_mat)
        mv = _MeshView(coord.shape[0], conn.shape[0], _ptr(coord), _ptr(conn))
        ps, pt = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
        qf = np.zeros(3 * coord.shape[0])
        ms = C.c_float(0)
        _chk(lib().fx_update_c3d8_linear(self.h, C.byref(mv), int(Es.size), _ptr(Es), _ptr(nus), _ptr(em), int(elemopt), _ptr(disp),
                                         C.byref(ps), C.byref(pt), _ptr(qf), C.byref(ms)))
        return _staged(ps, conn.shape[0], 8), _staged(pt, conn.shape[0], 8), qf, ms.value

    def element_stiffness(self, elemopt, ecoord, E, nu):
        ec = np.ascontiguousarray(ecoord, dtype=np.float64).reshape(8, 3)
        k = np.zeros((24, 24))
        _chk(lib().fx_element_stiffness_c3d8(self.h, int(elemopt), _ptr(ec), C.c_double(E), C.c_double(nu), _ptr(k)))
        return k

    def assemble_c3(self, coord, conn, etype, E, nu, load=None, bc=None, elem_mat=None):
        """fstr_StiffMatrix + fstr_AddBC on the device for the elements of STF_C3 (fx_assemble_c3): etype 341 (conn (n_elem, 4)),
        342 (n_elem, 10), 351 (n_elem, 6), 352 (n_elem, 15) or 362 (n_elem, 20), FrontISTR's node order.  E, nu scalars, or
        per-material arrays with elem_mat (1-based per element).  Returns the kernel milliseconds."""
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        Es, nus, em = _material_arrays(E, nu, elem_mat)
        mv = _MeshView(coord.shape[0], conn.shape[0], _ptr(coord), _ptr(conn))
        bn, bd, bv, load = _bc_arrays(bc, load)
        ms = C.c_float(0)
        _chk(lib().fx_assemble_c3(self.h, C.byref(mv), int(etype), int(Es.size), _ptr(Es), _ptr(nus), _ptr(em), _ptr(load),
                                  int(bn.size), _ptr(bn), _ptr(bd), _ptr(bv), C.byref(ms)))
        return ms.value

    def update_c3_linear(self, coord, conn, etype, E, nu, disp, elem_mat=None):
        """fstr_UpdateNewton of a linear static analysis on the device for the elements of UPDATE_C3 (fx_update_c3_linear):
        strain, stress (n_elem, nq, 6) with nq = 1 (341), 4 (342), 2 (351), 9 (352) or 27 (362), QFORCE (3 * n_node) from the
        total displacement.  Returns (strain, stress, qforce, kernel ms)."""
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        disp = np.ascontiguousarray(disp, dtype=np.float64)
        Es, nus, em = _material_arrays(E, nu, elem_mat)
        mv = _MeshView(coord.shape[0], conn.shape[0], _ptr(coord), _ptr(conn))
        ps, pt = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
        qf = np.zeros(3 * coord.shape[0])
        ms = C.c_float(0)
        _chk(lib().fx_update_c3_linear(self.h, C.byref(mv), int(etype), int(Es.size), _ptr(Es), _ptr(nus), _ptr(em), _ptr(disp),
                                       C.byref(ps), C.byref(pt), _ptr(qf), C.byref(ms)))
        nq = _C3_POINTS.get(int(etype), 1)
        return _staged(ps, conn.shape[0], nq), _staged(pt, conn.shape[0], nq), qf, ms.value

    def element_stiffness_c3(self, etype, ecoord, E, nu):
        """One element's (3 nn, 3 nn) stiffness through the device kernel (fx_element_stiffness_c3): etype 341, 342, 351, 352
        or 362."""
        nn = _C3_NODES.get(int(etype), 4)
        ec = np.ascontiguousarray(ecoord, dtype=np.float64).reshape(nn, 3)
        k = np.zeros((3 * nn, 3 * nn))
        _chk(lib().fx_element_stiffness_c3(self.h, int(etype), _ptr(ec), C.c_double(E), C.c_double(nu), _ptr(k)))
        return k

    @staticmethod
    def _group_table(groups):
        """fx_elem_group[] of [(etype, conn, elemopt, elem_mat)] (elemopt and elem_mat may be left out); the arrays are kept
        alive by the second return value."""
        keep, tab = [], (_ElemGroup * max(len(groups), 1))()
        for g, grp in enumerate(groups):
            etype, conn = int(grp[0]), np.ascontiguousarray(grp[1], dtype=np.int32)
            elemopt = int(grp[2]) if len(grp) > 2 and grp[2] is not None else 1
            em = None if len(grp) < 4 or grp[3] is None else np.ascontiguousarray(grp[3], dtype=np.int32)
            nn = _C3_NODES.get(etype, 0)
            n_elem = conn.size // nn if nn else (conn.shape[0] if conn.ndim == 2 else 0)
            keep += [conn, em]
            tab[g] = _ElemGroup(etype, elemopt, n_elem, _ptr(conn), _ptr(em))
        return tab, keep

    def assemble_groups(self, coord, groups, E, nu, load=None, bc=None):
        """fstr_StiffMatrix + fstr_AddBC on the device for a mesh of several solid element types (fx_assemble_groups):
        ``groups`` = [(etype, conn, elemopt, elem_mat)], etype 361 (elemopt 1 IC, 2 B-bar, 3 FI), 341, 342, 351, 352 or 362,
        all into the one resident matrix; E, nu scalars, or per-material arrays with every group's elem_mat (1-based).
        Returns the kernel milliseconds."""
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        Es, nus, _ = _material_arrays(E, nu)
        tab, keep = self._group_table(groups)
        bn, bd, bv, load = _bc_arrays(bc, load)
        ms = C.c_float(0)
        _chk(lib().fx_assemble_groups(self.h, int(coord.shape[0]), _ptr(coord), len(groups), tab, int(Es.size), _ptr(Es), _ptr(nus),
                                      _ptr(load), int(bn.size), _ptr(bn), _ptr(bd), _ptr(bv), C.byref(ms)))
        del keep
        return ms.value

    @staticmethod
    def _thermal_view(thermal):
        """fx_thermal_view of ``thermal`` = (temp, temp0, ref_temp, alpha): node temperatures now and in the reference state
        (n_node each), !REFTEMP, one expansion coefficient per material.  A None entry is passed on as NULL (refused)."""
        temp, temp0, ref_temp, alpha = thermal
        arr = [None if a is None else np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64) for a in (temp, temp0, alpha)]
        return _ThermalView(_ptr(arr[0]), _ptr(arr[1]), float(ref_temp), _ptr(arr[2])), arr

    def thermal_load_groups(self, coord, groups, E, nu, thermal, load=None):
        """The thermal load vector of fstr_ass_load for the solid element groups (fx_thermal_load_groups), added to ``load``
        (3 * n_node, zeros when None).  groups, E, nu as assemble_groups; thermal = (temp, temp0, ref_temp, alpha).  Returns
        (the vector, kernel ms); ``load`` itself is not changed."""
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        Es, nus, _ = _material_arrays(E, nu)
        tab, keep = self._group_table(groups)
        tv, keep_t = self._thermal_view(thermal)
        out = np.zeros(3 * coord.shape[0]) if load is None else np.array(load, dtype=np.float64).ravel()
        ms = C.c_float(0)
        _chk(lib().fx_thermal_load_groups(self.h, int(coord.shape[0]), _ptr(coord), len(groups), tab, int(Es.size), _ptr(Es), _ptr(nus),
                                          C.byref(tv), _ptr(out), C.byref(ms)))
        del keep, keep_t
        return out, ms.value

    def thermal_load(self, mesh, E, nu, thermal, elemopt=1, elem_mat=None, load=None):
        """thermal_load_groups for one of mesh.py's meshes (a single-type mesh is one group; mesh.mesh_groups)."""
        from .mesh import mesh_groups
        return self.thermal_load_groups(mesh.coord, mesh_groups(mesh, elemopt, elem_mat), E, nu, thermal, load=load)

    def update_linear(self, mesh, E, nu, disp, elemopt=1, elem_mat=None, thermal=None):
        """update_groups_linear for one of mesh.py's meshes (a single-type mesh is one group; mesh.mesh_groups)."""
        from .mesh import mesh_groups
        return self.update_groups_linear(mesh.coord, mesh_groups(mesh, elemopt, elem_mat), E, nu, disp, thermal=thermal)

    def update_groups_linear(self, coord, groups, E, nu, disp, thermal=None):
        """fstr_UpdateNewton of a linear static analysis on the device for the same groups (fx_update_groups_linear; with
        thermal = (temp, temp0, ref_temp, alpha) fx_update_groups_linear_thermal: stress = D (strain - thermal strain)).
        Returns ([strain per group (n_elem, nq, 6)], [stress per group], qforce (3 * n_node) summed over the groups, kernel ms)."""
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        disp = np.ascontiguousarray(disp, dtype=np.float64)
        Es, nus, _ = _material_arrays(E, nu)
        tab, keep = self._group_table(groups)
        ng = len(groups)
        ps, pt = (C.POINTER(C.c_double) * max(ng, 1))(), (C.POINTER(C.c_double) * max(ng, 1))()
        qf = np.zeros(3 * coord.shape[0])
        ms = C.c_float(0)
        if thermal is None:
            _chk(lib().fx_update_groups_linear(self.h, int(coord.shape[0]), _ptr(coord), ng, tab, int(Es.size), _ptr(Es), _ptr(nus),
                                               _ptr(disp), ps, pt, _ptr(qf), C.byref(ms)))
        else:
            tv, keep_t = self._thermal_view(thermal)
            _chk(lib().fx_update_groups_linear_thermal(self.h, int(coord.shape[0]), _ptr(coord), ng, tab, int(Es.size), _ptr(Es),
                                                       _ptr(nus), C.byref(tv), _ptr(disp), ps, pt, _ptr(qf), C.byref(ms)))
            del keep_t
        nqs = [_C3_POINTS[tab[g].etype] for g in range(ng)]
        strain = [_staged(ps[g], tab[g].n_elem, nqs[g]) for g in range(ng)]
        stress = [_staged(pt[g], tab[g].n_elem, nqs[g]) for g in range(ng)]
        del keep
        return strain, stress, qf, ms.value

    def nodal_stress_groups(self, n_node, groups, strain, stress, principal=0):
        """fstr_NodalStress3D on the device (fx_nodal_stress_groups) from the quadrature-point arrays of a linear update:
        ``groups`` as assemble_groups takes them, ``strain`` / ``stress`` the per-group lists update_groups_linear returns (or
        one flat array, the groups one after the other, [elem][point][6]).  principal: make_principal's bit mask (PRINC_*).
        Returns a NodalStress.  A connectivity whose row length (or, flat, whose size) does not fit the type's node count is refused
        here with the code of an unknown type: fx_elem_group carries no row length, so the library cannot see it."""
        for grp in groups:
            nn = _C3_NODES.get(int(grp[0]), 0)
            conn = np.asarray(grp[1])
            if nn and (conn.shape[1] != nn if conn.ndim == 2 else conn.size % nn):     # flat arrays pass as in assemble_groups
                raise HecmwSolverError(-2, "nodal_stress_groups: TYPE=%d has %d nodes per element, the connectivity has shape %s"
                                       % (int(grp[0]), nn, conn.shape))
        tab, keep = self._group_table(groups)
        flat = lambda v: np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in v])
                                              if isinstance(v, (list, tuple)) else v, dtype=np.float64).ravel()
        st, ss = flat(strain), flat(stress)
        nqs = [_C3_POINTS.get(tab[g].etype, 0) for g in range(len(groups))]
        want = 6 * sum(q * tab[g].n_elem for g, q in enumerate(nqs))
        if all(nqs) and (st.size != want or ss.size != want):
            raise ValueError("nodal_stress_groups: the point arrays hold %d / %d doubles, the groups need %d" % (st.size, ss.size, want))
        res, ms = _NodalResult(), C.c_float(0)
        _chk(lib().fx_nodal_stress_groups(self.h, int(n_node), len(groups), tab, _ptr(st), _ptr(ss), int(principal), C.byref(res),
                                          C.byref(ms)))
        del keep
        return NodalStress(res, ms.value)

    def nodal_stats(self):
        """fx_nodal_get_stats: lists built (linear, nonlinear), entries, records, workgroup size of the node kernel, elements per
        workgroup of the element kernel by type."""
        out = (C.c_int64 * 12)()
        _chk(lib().fx_nodal_get_stats(self.h, out))
        v = list(out)
        return {"lists": v[0], "lists_nl": v[1], "entries": v[2], "records": v[3], "node_bs": v[4],
                "elems_per_wg": dict(zip((341, 342, 351, 352, 361, 362), v[5:11]))}

    # --- heat conduction (frontistr_amd/heat.py drives these) ----------
    @staticmethod
    def _heat_materials(mats):
        """fx_heat_material_view[] of heat.tHeatMaterial objects (anything with .cond / .cp / .rho = (ntab, temp, funcA, funcB) or
        None); the arrays are kept alive by the second return value."""
        mats = list(mats) if isinstance(mats, (list, tuple)) else [mats]
        tab, keep = (_HeatMaterialView * max(len(mats), 1))(), []
        for k, m in enumerate(mats):
            views = []
            for t in (m.cond, m.cp, m.rho):
                if t is None:
                    views.append(_HeatTable(0, None, None, None))
                    continue
                arr = [np.ascontiguousarray(a, dtype=np.float64) for a in t[1:]]
                keep += arr
                views.append(_HeatTable(int(t[0]), _ptr(arr[0]), _ptr(arr[1]), _ptr(arr[2])))
            tab[k] = _HeatMaterialView(*views)
        return tab, keep, len(mats)

    @staticmethod
    def _heat_surface(lst, with_sink):
        """fx_heat_surface of (group, elem, face, val[, sink]) (0-based group and element positions, values with their amplitude
        applied; a scalar value serves every entry); the arrays are kept alive by the second return value."""
        if lst is None:
            return _HeatSurface(0, None, None, None, None, None), []
        idx = [np.ascontiguousarray(a, dtype=np.int32).ravel() for a in lst[:3]]
        n = idx[0].size
        if idx[1].size != n or idx[2].size != n or len(lst) < (5 if with_sink else 4):
            raise ValueError("a surface list is (group, elem, face, val%s) of one length" % (", sink" if with_sink else ""))
        vals = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)))
                for v in lst[3:5 if with_sink else 4]] + [None]
        keep = idx + vals
        return _HeatSurface(n, _ptr(idx[0]), _ptr(idx[1]), _ptr(idx[2]), _ptr(vals[0]), _ptr(vals[1])), keep

    def heat_assemble_groups(self, coord, groups, mats, hecMAT, temp, temp0=None, beta=1.0, dtime=0.0, flux=None, fix=None,
                             dflux=None, film=None, radiate=None, tzero=0.0):
        """heat_mat_ass_conductivity + heat_mat_ass_capacity (+ !CFLUX, !FIXTEMP) on the device (fx_heat_assemble_groups):
        ``groups`` = [(etype, conn, None, elem_mat)] of TYPE=341, 342, 351, 352, 361, 362; ``mats`` heat.tHeatMaterial objects;
        ``hecMAT`` a scalar matrix (NDOF = 1) whose D, AL, AU, B receive the result; temp / temp0 node temperatures;
        flux (n_node) or None; fix = (nodes 1-based, values) or None.  With any of dflux = (group, elem, face, val), film or
        radiate = (group, elem, face, val, sink) -- 0-based positions of the group and of the element in it, face = LTYPE of the
        routine (0 in dflux: the body flux), values with their amplitudes applied -- the surface terms are added on the device
        (fx_heat_assemble_groups_bc; tzero is !ZERO).  Returns the kernel milliseconds."""
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        tab, keep = self._group_table(groups)
        mt, keep_m, n_mat = self._heat_materials(mats)
        temp = np.ascontiguousarray(temp, dtype=np.float64)
        temp0 = None if temp0 is None else np.ascontiguousarray(temp0, dtype=np.float64)
        flux = None if flux is None else np.ascontiguousarray(flux, dtype=np.float64)
        fn, fv = ((), ()) if fix is None else fix
        fn, fv = np.ascontiguousarray(fn, dtype=np.int32), np.ascontiguousarray(fv, dtype=np.float64)
        hv = _HeatView(_ptr(temp), _ptr(temp0), float(beta), float(dtime))
        mv = hecMAT.view()
        ms = C.c_float(0)
        if dflux is None and film is None and radiate is None:
            _chk(lib().fx_heat_assemble_groups(self.h, int(coord.shape[0]), _ptr(coord), len(groups), tab, n_mat, mt, C.byref(hv),
                                               C.byref(mv), _ptr(flux), int(fn.size), _ptr(fn), _ptr(fv), C.byref(ms)))
        else:
            (sd, kd), (sf, kf), (sr, kr) = self._heat_surface(dflux, False), self._heat_surface(film, True), self._heat_surface(radiate, True)
            bc = _HeatBc(sd, sf, sr, float(tzero))
            _chk(lib().fx_heat_assemble_groups_bc(self.h, int(coord.shape[0]), _ptr(coord), len(groups), tab, n_mat, mt, C.byref(hv),
                                                  C.byref(mv), _ptr(flux), int(fn.size), _ptr(fn), _ptr(fv), C.byref(bc), C.byref(ms)))
            del kd, kf, kr
        del keep, keep_m
        return ms.value

    def heat_face(self, etype, kind, face, ecoord, val, sink=0.0, tt=None, tzero=0.0):
        """One face of one element through the device kernels (fx_heat_face).  kind: "dflux", "film" or "radiate" (or 0, 1, 2);
        face: LTYPE of the routine (0 with dflux: the body flux); ecoord (nn, 3) and tt (nn, radiate only) of the whole element.
        -> (TERM1 (mm, mm), TERM2 (mm), NOD (mm, 1-based)), or for dflux (None, VECT (nn), NOD)."""
        kind = {"dflux": 0, "film": 1, "radiate": 2}.get(kind, kind)
        ec = np.ascontiguousarray(ecoord, dtype=np.float64)
        nn = ec.size // 3
        tt = None if tt is None else np.ascontiguousarray(tt, dtype=np.float64)
        t1, t2, nsuf, mm = np.zeros(64), np.zeros(20), np.zeros(20, dtype=np.int32), C.c_int32(0)
        _chk(lib().fx_heat_face(self.h, int(etype), int(kind), int(face), _ptr(ec), _ptr(tt), C.c_double(val), C.c_double(sink),
                                C.c_double(tzero), _ptr(t1), _ptr(t2), _ptr(nsuf), C.byref(mm)))
        m = mm.value
        if kind == 0:
            return None, t2[:nn].copy(), nsuf[:m].copy()
        return t1[:m * m].reshape(m, m).copy(), t2[:m].copy(), nsuf[:m].copy()

    def heat_bc_stats(self):
        """fx_heat_get_bc_stats as a dict."""
        out = (C.c_int64 * 8)()
        _chk(lib().fx_heat_get_bc_stats(self.h, out))
        keys = ("face_colourings", "face_maps", "elem_us", "surf_us", "lanes_per_face", "faces_per_workgroup")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    @staticmethod
    def _dload(dload):
        """fx_dload of a fstr.tDload, or of (group, elem, ltype, params[, held]): 0-based positions of the group and of the
        element in it, DL_C3's LTYPE (1..5, 10 * face), PARAMS(0:6) per entry (n, 7) with the amplitude applied, and optionally
        the flags of the entries that take factor 1.  The arrays are kept alive by the second return value."""
        lst = dload.arrays() if hasattr(dload, "arrays") else dload
        idx = [np.ascontiguousarray(a, dtype=np.int32).ravel() for a in lst[:3]]
        n = idx[0].size
        par = np.ascontiguousarray(lst[3], dtype=np.float64).reshape(-1)
        held = None if len(lst) < 5 or lst[4] is None else np.ascontiguousarray(lst[4], dtype=np.uint8).ravel()
        if idx[1].size != n or idx[2].size != n or par.size != 7 * n or (held is not None and held.size != n):
            raise ValueError("a dload list is (group, elem, ltype, params (n, 7)[, held]) of one length")
        keep = idx + [par, held]
        return _Dload(n, _ptr(idx[0]), _ptr(idx[1]), _ptr(idx[2]), _ptr(par), _ptr(held)), keep

    def dload_groups(self, coord, groups, rho, dload, factor=1.0, disp=None, load=None):
        """The DLOAD block of fstr_ass_load for the solid element groups (fx_dload_groups): factor * DL_C3 of every entry of
        ``dload`` (a fstr.tDload, or the tuple of _dload), taken on coord (+ disp), added to ``load`` (3 * n_node, zeros when
        None).  groups as assemble_groups; rho a density or one per material (None: the list has neither GRAV nor CENT).
        Returns (the vector, kernel ms); ``load`` itself is not changed."""
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        tab, keep = self._group_table(groups)
        rho = None if rho is None else np.ascontiguousarray(np.atleast_1d(rho), dtype=np.float64)
        dv, keep_d = self._dload(dload)
        disp = None if disp is None else np.ascontiguousarray(disp, dtype=np.float64).ravel()
        if disp is not None and disp.size != 3 * coord.shape[0]:
            raise ValueError("disp must hold 3 * n_node values")
        out = np.zeros(3 * coord.shape[0]) if load is None else np.array(load, dtype=np.float64).ravel()
        if out.size != 3 * coord.shape[0]:
            raise ValueError("load must hold 3 * n_node values")
        ms = C.c_float(0)
        _chk(lib().fx_dload_groups(self.h, int(coord.shape[0]), _ptr(coord), len(groups), tab, 0 if rho is None else int(rho.size),
                                   _ptr(rho), C.byref(dv), C.c_double(factor), _ptr(disp), _ptr(out), C.byref(ms)))
        del keep, keep_d
        return out, ms.value

    def dload_element(self, etype, ltype, ecoord, params, rho=0.0):
        """One element through the device kernels (fx_dload_element): DL_C3's VECT (3 * nn) for ecoord (nn, 3), LTYPE and
        PARAMS(0:6)."""
        ec = np.ascontiguousarray(ecoord, dtype=np.float64)
        par = np.ascontiguousarray(params, dtype=np.float64).ravel()
        if par.size != 7:
            raise ValueError("params is PARAMS(0:6)")
        nn = _C3_NODES.get(int(etype), 8)
        if ec.size != 3 * nn:
            raise ValueError("ecoord must be (%d, 3) for TYPE=%d" % (nn, etype))
        vect = np.zeros(3 * nn)
        _chk(lib().fx_dload_element(self.h, int(etype), int(ltype), _ptr(ec), C.c_double(rho), _ptr(par), _ptr(vect)))
        return vect

    def dload_stats(self):
        """fx_dload_get_stats as a dict."""
        out = (C.c_int64 * 8)()
        _chk(lib().fx_dload_get_stats(self.h, out))
        keys = ("tri_entries", "quad_entries", "body_entries", "grav_entries", "cent_entries", "face_us", "vol_us", "lanes_per_face")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def heat_element(self, etype, ecoord, tt, mat, tt0=None, dtime=0.0):
        """One element through the device kernels (fx_heat_element) -> (SS (nn, nn) at tt, S0 (nn) at tt0 or None)."""
        ec = np.ascontiguousarray(ecoord, dtype=np.float64)
        nn = ec.size // 3
        tt = np.ascontiguousarray(tt, dtype=np.float64)
        tt0 = None if tt0 is None else np.ascontiguousarray(tt0, dtype=np.float64)
        mt, keep_m, _ = self._heat_materials([mat])
        ss, s0 = np.zeros((nn, nn)), np.zeros(nn)
        _chk(lib().fx_heat_element(self.h, int(etype), _ptr(ec), _ptr(tt), _ptr(tt0), mt, C.c_double(dtime), _ptr(ss), _ptr(s0)))
        del keep_m
        return ss, (s0 if dtime > 0 else None)

    def heat_stats(self):
        """fx_heat_get_stats as a dict."""
        out = (C.c_int64 * 8)()
        _chk(lib().fx_heat_get_stats(self.h, out))
        keys = ("colourings", "maps", "profiles", "calls", "copy_us", "lanes_per_element", "elements_per_workgroup")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        _chk(lib().fx_comm_init(self.h, buf, rank, nranks))

    def comm_size(self):
        """(ranks, device) as the transport itself reports them (ncclCommCount / ncclCommCuDevice)."""
        n, d = C.c_int32(0), C.c_int32(0)
        _chk(lib().fx_comm_size(self.h, C.byref(n), C.byref(d)))
        return n.value, d.value

    def synchronize(self):
        _chk(lib().fx_device_synchronize(self.h))

    def _finish(self, code, info, hist):
        self.info = info
        self.history = None if hist is None else hist[:info.n_hist].copy()
        if code < 0 or code in (HECMW_SOLVER_ERROR_INCONS_PC, HECMW_SOLVER_ERROR_ZERO_DIAG):
            # E-codes abort in the reference (hecmw_solve_error.f90:50-83)
            raise HecmwSolverError(code, lib().fx_last_error().decode(errors="replace"))
        if code:
            self.messages.append("#### HEC-MW-SOLVER-W-%d" % code)


def comm_unique_id():
    buf = (C.c_ubyte * 128)()
    _chk(lib().fx_comm_unique_id(buf))
    return bytes(buf)


_default_ctx = None


def _ctx(ctx):
    global _default_ctx
    if ctx is not None:
        return ctx
    if _default_ctx is None:
        _default_ctx = SolverContext()
    return _default_ctx


def hecmw_mat_con(hecMESH, hecMAT):
    """CRS block profile from hecMESH%elem_node_item: hecMESH.nn_elem nodes per element when the mesh sets it (4 at TYPE=341,
    10 at 342, 6 at 351, 15 at 352, 20 at 362), else 8 (TYPE=361)."""
    nn = int(getattr(hecMESH, "nn_elem", 8))
    conn = np.ascontiguousarray(hecMESH.elem_node_item, dtype=np.int32).reshape(-1, nn)
    NP = hecMESH.n_node
    indexL = np.zeros(NP + 1, dtype=np.int32)
    indexU = np.zeros(NP + 1, dtype=np.int32)
    _chk(lib().fx_mat_con(NP, conn.shape[0], nn, _ptr(conn), _ptr(indexL), _ptr(indexU), None, None))
    itemL = np.zeros(max(int(indexL[NP]), 1), dtype=np.int32)
    itemU = np.zeros(max(int(indexU[NP]), 1), dtype=np.int32)
    _chk(lib().fx_mat_con(NP, conn.shape[0], nn, _ptr(conn), _ptr(indexL), _ptr(indexU), _ptr(itemL), _ptr(itemU)))
    hecMAT.N, hecMAT.NP = hecMESH.nn_internal, NP
    hecMAT.indexL, hecMAT.indexU = indexL, indexU
    hecMAT.itemL, hecMAT.itemU = itemL[:indexL[NP]], itemU[:indexU[NP]]       # exact-size arrays (views when nothing is cut)
    hecMAT.NPL, hecMAT.NPU = int(indexL[NP]), int(indexU[NP])
    hecMAT.B = np.zeros(3 * NP)
    hecMAT.X = np.zeros(3 * NP)
    return hecMAT


def hecmw_mat_con_groups(hecMESH, hecMAT, groups):
    """hecmw_mat_con for a mesh of several element types: the CRS block profile of the union of the groups' elements
    (``groups`` = [(etype, conn, ...)], conn (n_elem, nn) 1-based).  Host only (numpy): the node pairs of the elements, made
    unique slice by slice and then together."""
    NP = int(hecMESH.n_node)
    parts = []
    for grp in groups:
        conn = np.asarray(grp[1], dtype=np.int64)
        if conn.size == 0:
            continue
        nn = conn.shape[1]
        step = max(1, (1 << 24) // (nn * nn))
        for a in range(0, conn.shape[0], step):          # in slices: nn^2 pairs per element
            c = conn[a:a + step] - 1
            parts.append(np.unique((c[:, :, None] * NP + c[:, None, :]).ravel()))
    keys = np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64)
    row, col = keys // NP, keys % NP
    lower, upper = col < row, col > row
    indexL = np.zeros(NP + 1, dtype=np.int32)
    indexU = np.zeros(NP + 1, dtype=np.int32)
    indexL[1:] = np.cumsum(np.bincount(row[lower], minlength=NP))
    indexU[1:] = np.cumsum(np.bincount(row[upper], minlength=NP))
    hecMAT.N, hecMAT.NP = hecMESH.nn_internal, NP
    hecMAT.indexL, hecMAT.indexU = indexL, indexU
    hecMAT.itemL = np.ascontiguousarray(col[lower] + 1, dtype=np.int32)      # keys are sorted by (row, col)
    hecMAT.itemU = np.ascontiguousarray(col[upper] + 1, dtype=np.int32)
    hecMAT.NPL, hecMAT.NPU = int(indexL[NP]), int(indexU[NP])
    hecMAT.B = np.zeros(3 * NP)
    hecMAT.X = np.zeros(3 * NP)
    return hecMAT


def march_plan(hecMAT, chunk, waves):
    """Host-only: the two plane-march programs of hecMAT's profile (fx_march_plan), replayed on the host."""
    out = (C.c_double * 8)()
    f = lib().fx_march_plan
    f.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    iL, jL = np.ascontiguousarray(hecMAT.indexL, dtype=np.int32), np.ascontiguousarray(hecMAT.itemL, dtype=np.int32)
    iU, jU = np.ascontiguousarray(hecMAT.indexU, dtype=np.int32), np.ascontiguousarray(hecMAT.itemU, dtype=np.int32)
    _chk(f(int(hecMAT.N), _ptr(iL), _ptr(jL), _ptr(iU), _ptr(jU), int(chunk), int(waves), out))
    keys = ("admitted", "chunks", "rounds_fwd", "rounds_bwd", "near_blocks", "far_blocks", "max_round_rows", "levels")
    return {k: int(out[i]) for i, k in enumerate(keys)}


def hecmw_solve(hecMESH, hecMAT, ctx=None, want_history=True):
    """subroutine hecmw_solve(hecMESH, hecMAT): solves hecMAT in place (X, Iarray flags).
    Returns the reference's status code (0, or a W-code such as 3001 / 2002)."""
    ctx = _ctx(ctx)
    mv = hecMAT.view()
    cv = hecMESH.comm_view() if hecMESH is not None else None
    info = _SolveInfo()
    maxit = int(hecMAT.Iarray[0])
    hist = np.zeros(max(maxit, 1) + 1) if want_history else None   # GMRES logs MAXIT+1 lines when it runs out
    code = lib().fx_solve(ctx.h, C.byref(mv), C.byref(cv) if cv is not None else None, _ptr(hecMAT.Iarray),
                          _ptr(hecMAT.Rarray), C.byref(info), _ptr(hist), 0 if hist is None else hist.size)
    ctx._finish(code, info, hist)
    return code


def hecmw_matvec(hecMESH, hecMAT, X, Y, ctx=None):
    """subroutine hecmw_matvec(hecMESH, hecMAT, X, Y, COMMtime): Y(1:3N) = A X; returns COMMtime."""
    ctx = _ctx(ctx)
    mv = hecMAT.view()
    cv = hecMESH.comm_view() if hecMESH is not None else None
    assert X.dtype == np.float64 and Y.dtype == np.float64 and X.flags.c_contiguous and Y.flags.c_contiguous
    t = C.c_double(0.0)
    _chk(lib().fx_matvec(ctx.h, C.byref(mv), C.byref(cv) if cv is not None else None, _ptr(X), _ptr(Y), C.byref(t)))
    return t.value
