"""Host-side mirror of the reference's nonlinear static loop on top of the C ABI
(include/fistr_hip.h, "nonlinear static loop" section).  Same names and argument meaning as

    tMaterial            fistr1/src/lib/physics/material.f90:135-149  (+ !ELASTIC / !PLASTIC cards,
                         fistr1/src/common/fstr_ctrl_material.f90:60-106, :341-480)
    fstr_solid           fistr1/src/lib/m_fstr.f90 (unode, dunode, QFORCE, elements(:)%gausses(:))
    fstr_StiffMatrix     fistr1/src/analysis/static/fstr_StiffMatrix.f90:18
    fstr_AddBC           fistr1/src/analysis/static/fstr_AddBC.f90:17
    fstr_UpdateNewton    fistr1/src/analysis/static/fstr_Update.f90:25
    fstr_Update_NDForce  fistr1/src/analysis/static/fstr_Residual.f90:23
    fstr_UpdateState     fistr1/src/analysis/static/fstr_Update.f90:296
    fstr_NodalStress3D   fistr1/src/analysis/static/fstr_NodalStress.f90:13
    fstr_cutback_save / _load  fistr1/src/analysis/static/fstr_Cutback.f90:108-198
    tDload / set_dload   the !DLOAD cards of fstr_ass_load (fistr1/src/analysis/static/fstr_ass_load.f90:138-257, DL_C3)
    fstr_Newton          fistr1/src/analysis/static/fstr_solve_NonLinear.f90:29
    fstr_solve_NLGEOM    fistr1/src/analysis/static/fstr_solve_NLGEOM.f90:32 (sub-step loop, linear load ramp)

for one TYPE=361 B-bar or F-bar group (fstr_solid(..., elemopt=2 | 4); F-bar: `!SECTION, FORM361=FBAR`, INFINITE and TOTALLAG materials),
or one group of tetrahedra TYPE=341 / 342, wedges TYPE=351 / 352 or 20-node hexahedra TYPE=362
(fstr_solid(..., etype=341 | 342 | 351 | 352 | 362): STF_C3 / UPDATE_C3), or a mesh of several groups of these types
(fstr_solid(ctx, coord, None, materials, groups=[...]): fx_nl_init_groups),
with one isotropic (elastic; Mises, Mohr-Coulomb or Drucker-Prager elastoplastic: tMaterial.mohr_coulomb / .drucker_prager;
hyperelastic: tMaterial.neohooke / .mooney_rivlin / .arruda_boyce; viscoelastic: tMaterial.viscoelastic; or NORTON creep:
tMaterial.norton) material per section.  Everything is resident on the GPU; there is NO CPU
fallback.
"""
import ctypes as C

import numpy as np

from . import hecmw
from .hecmw import _chk, _ptr, lib
from .mesh import C3_NODES, C3_POINTS, C3_SUBFACE

INFINITE, TOTALLAG, UPDATELAG = 0, 1, 2
BILINEAR, MULTILINEAR, SWIFT, RAMBERG_OSGOOD = 0, 1, 2, 3
ELASTIC, MISES, MOONEYRIVLIN, ARRUDABOYCE = 0, 1, 2, 3      # fx_material_view::plastic, the material kind (NEOHOOKE is MOONEYRIVLIN with C01 = 0)
MOHRCOULOMB, DRUCKERPRAGER = 4, 5                           # !PLASTIC, YIELD=MOHR-COULOMB | DRUCKER-PRAGER
VISCOELASTIC = 7                                            # !VISCOELASTIC: table = the Prony rows (g, tau)
NORTON = 8                                                  # !CREEP, TYPE=NORTON: plconst = A, n, m
_PLASTICITY_PI = 3.14159265358979                           # fstr_ctrl_get_PLASTICITY's own PI (fstr_ctrl_material.f90:355)


class _MaterialView(C.Structure):
    _fields_ = [("E", C.c_double), ("nu", C.c_double), ("plastic", C.c_int32), ("harden", C.c_int32),
                ("nlgeom", C.c_int32), ("ntab", C.c_int32), ("plconst", C.c_double * 3), ("tab", C.c_void_p),
                ("plconst4", C.c_double)]


class _StateView(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat",
                                          "istat", "unode", "dunode", "qforce")] + [("latch", C.c_int32)]


class _NlThermalView(C.Structure):
    _fields_ = [("ref_temp", C.c_double), ("temp_init", C.c_void_p), ("alpha", C.c_void_p), ("alpha_tab", C.c_void_p),
                ("alpha_rows", C.c_void_p), ("elastic_tab", C.c_void_p), ("elastic_rows", C.c_void_p)]


class tMaterial:
    """!ELASTIC E, nu; optional !PLASTIC, YIELD=MISES, HARDEN=<harden> with `plconst` (BILINEAR: yield0, H;
    SWIFT / RAMBERG-OSGOOD: the three constants) or `table` rows (yield stress, plastic strain) for MULTILINEAR.
    nlgeom_flag defaults to UPDATELAG as !PLASTIC does (KIRCHHOFF -> TOTALLAG, INFINITE -> INFINITE).
    Hyperelastic materials come from the named constructors neohooke / mooney_rivlin / arruda_boyce; they default to TOTALLAG, the
    only flag the device loop serves for them.  Mohr-Coulomb and Drucker-Prager materials come from mohr_coulomb / drucker_prager.
    Thermal strain (fstr_solid.set_thermal): ``expansion`` is !EXPANSION_COEFF's constant; ``expansion_table`` (rows alpha, T) and
    ``elastic_table`` (rows E, nu, T) are the DEPENDENCIES=1 forms of !EXPANSION_COEFF and !ELASTIC, ascending in T.  They are
    attributes: set them on the material before fstr_solid.set_thermal."""

    expansion = 0.0
    expansion_table = None
    elastic_table = None

    def __init__(self, E, nu, plastic=False, harden=BILINEAR, plconst=(0.0, 0.0, 0.0), table=None, nlgeom_flag=UPDATELAG):
        self.E, self.nu, self.plastic, self.harden = float(E), float(nu), bool(plastic), int(harden)
        self.plconst = tuple(float(v) for v in plconst)
        self.table = np.zeros((0, 2)) if table is None else np.ascontiguousarray(table, dtype=np.float64).reshape(-1, 2)
        self.nlgeom_flag = int(nlgeom_flag)
        self.kind = MISES if self.plastic else ELASTIC
        self.plconst4 = 0.0
        if self.plastic and self.harden == MULTILINEAR:
            if self.table.shape[0] < 1 or self.table[0, 1] != 0.0:
                raise ValueError("Multilinear hardening: First plastic strain must be zero")   # fstr_ctrl_material.f90:416
            if (self.table[:, 1] < 0).any():
                raise ValueError("Multilinear hardening: Error in plastic strain definition")

    @classmethod
    def _hyperelastic(cls, kind, plconst, nlgeom_flag):
        m = cls(0.0, 0.0, plconst=plconst, nlgeom_flag=nlgeom_flag)
        m.kind = kind
        return m

    @classmethod
    def neohooke(cls, C10, D1, nlgeom_flag=TOTALLAG):
        """!HYPERELASTIC, TYPE=NEOHOOKE: C10, D1 (fstr_ctrl_material.f90:166-255: Mooney-Rivlin with C01 = 0)."""
        return cls._hyperelastic(MOONEYRIVLIN, (C10, 0.0, D1), nlgeom_flag)

    @classmethod
    def mooney_rivlin(cls, C10, C01, D1, nlgeom_flag=TOTALLAG):
        """!HYPERELASTIC, TYPE=MOONEY-RIVLIN: C10, C01, D1."""
        return cls._hyperelastic(MOONEYRIVLIN, (C10, C01, D1), nlgeom_flag)

    @classmethod
    def arruda_boyce(cls, mu, lam, D, nlgeom_flag=TOTALLAG):
        """!HYPERELASTIC, TYPE=ARRUDA-BOYCE: mu, lambda_m, D."""
        return cls._hyperelastic(ARRUDABOYCE, (mu, lam, D), nlgeom_flag)

    @classmethod
    def mohr_coulomb(cls, E, nu, c, phi_deg, H=0.0, nlgeom_flag=UPDATELAG):
        """!PLASTIC, YIELD=MOHR-COULOMB with the data line c, phi [degrees], H: M_PLCONST1..3 = c, H, phi in radians, computed as
        fstr_ctrl_get_PLASTICITY does (fstr_ctrl_material.f90:451-469, with its own 15-digit PI), so the material equals the parsed
        one bit for bit."""
        m = cls(E, nu, plastic=True, harden=BILINEAR, plconst=(c, H, float(phi_deg) * _PLASTICITY_PI / 180.0), nlgeom_flag=nlgeom_flag)
        m.kind = MOHRCOULOMB
        return m

    @classmethod
    def drucker_prager(cls, E, nu, c, phi_deg, H=0.0, nlgeom_flag=UPDATELAG):
        """!PLASTIC, YIELD=DRUCKER-PRAGER with the data line c, phi [degrees], H: M_PLCONST1..4 = c, H, eta, xi with
        eta = 2 sin(phi) / (sqrt(3) (3 + sin(phi))), xi = 6 cos(phi) / (sqrt(3) (3 + sin(phi))) (fstr_ctrl_material.f90:460-465)."""
        dum = float(phi_deg) * _PLASTICITY_PI / 180.0
        eta = 2.0 * np.sin(dum) / (np.sqrt(3.0) * (3.0 + np.sin(dum)))
        xi = 6.0 * np.cos(dum) / (np.sqrt(3.0) * (3.0 + np.sin(dum)))
        m = cls(E, nu, plastic=True, harden=BILINEAR, plconst=(c, H, float(eta)), nlgeom_flag=nlgeom_flag)
        m.kind = DRUCKERPRAGER
        m.plconst4 = float(xi)
        return m

    @classmethod
    def viscoelastic(cls, E, nu, prony, nlgeom_flag=TOTALLAG):
        """!ELASTIC E, nu with !VISCOELASTIC: ``prony`` rows (g_n, tau_n), one per term.  The card's flag is TOTALLAG, or INFINITE
        with its INFINITE parameter (fstr_ctrl_material.f90:277-279).  Time-dependent: fstr_solid.set_time / the tincr arguments."""
        m = cls(E, nu, table=prony, nlgeom_flag=nlgeom_flag)
        m.kind = VISCOELASTIC
        return m

    @classmethod
    def norton(cls, E, nu, A, n, m, nlgeom_flag=UPDATELAG):
        """!ELASTIC E, nu with !CREEP, TYPE=NORTON: A, n, m of the law  d(eps_cr)/dt = A q**n t**m.  The card's flag is UPDATELAG
        (TOTALLAG with KIRCHHOFF, which the device loop refuses; fstr_ctrl_material.f90:502-504).  Time-dependent."""
        mat = cls(E, nu, plconst=(A, n, m), nlgeom_flag=nlgeom_flag)
        mat.kind = NORTON
        return mat

    def view(self):
        kind = self.kind if self.kind >= MOONEYRIVLIN else int(self.plastic)
        v = _MaterialView(self.E, self.nu, kind, self.harden, self.nlgeom_flag, self.table.shape[0],
                          (C.c_double * 3)(*self.plconst), _ptr(self.table) if self.table.size else None, self.plconst4)
        v._keep = self.table
        return v


class tDload:
    """A list of distributed loads, one entry per (element, LTYPE) of fstr_ass_load's loop over the !DLOAD cards
    (fstr_ass_load.f90:157-256); values carry their amplitude.  ``group`` is the position of the element group (0 for a
    single-type mesh) and ``elems`` the 0-based elements in it.  held=True marks a card whose load group was active in the step
    before: its entries take factor 1 (:141-142).  SolverContext.dload_groups and fstr_solid.set_dload take the object."""

    LTYPE = {"BX": 1, "BY": 2, "BZ": 3, "GRAV": 4, "CENT": 5}
    SUBFACE = C3_SUBFACE        # getSubFace: the nodes of face f, 1-based positions in the element

    def __init__(self):
        self.group, self.elem, self.ltype, self.params, self.held = [], [], [], [], []

    def __len__(self):
        return len(self.group)

    def add(self, group, elems, ltype, params, held=False):
        """Entries (group, e, ltype) for every e of ``elems`` with PARAMS(0:6) = params (7 values)."""
        par = [float(v) for v in params]
        if len(par) != 7:
            raise ValueError("params is PARAMS(0:6)")
        for e in np.atleast_1d(np.asarray(elems, dtype=np.int64)).ravel():
            self.group.append(int(group)); self.elem.append(int(e)); self.ltype.append(int(ltype))
            self.params.append(par); self.held.append(1 if held else 0)
        return self

    def body(self, group, elems, direction, val, held=False):
        """!DLOAD BX | BY | BZ: a force per volume (not multiplied by the density)."""
        if direction not in ("BX", "BY", "BZ"):
            raise ValueError("body: direction is BX, BY or BZ")
        return self.add(group, elems, self.LTYPE[direction], (val, 0, 0, 0, 0, 0, 0), held)

    def gravity(self, group, elems, val, direction, held=False):
        """!DLOAD GRAV: acceleration val along ``direction`` (normalised by DL_C3), times the element's density."""
        return self.add(group, elems, 4, (val,) + tuple(direction) + (0, 0, 0), held)

    def centrifugal(self, group, elems, omega, point, axis, held=False):
        """!DLOAD CENT: angular velocity omega about the axis through ``point`` along ``axis``."""
        return self.add(group, elems, 5, (omega,) + tuple(point) + tuple(axis), held)

    def pressure(self, group, elems, face, val, held=False):
        """!DLOAD P<face>: val times SurfaceNormal of getSubFace's face, which points into the element: a positive value presses.
        ``face`` a number, or one per element."""
        elems = np.atleast_1d(np.asarray(elems, dtype=np.int64)).ravel()
        for e, f in zip(elems, np.broadcast_to(np.asarray(face, dtype=np.int64), elems.shape)):
            self.add(group, [e], 10 * int(f), (val, 0, 0, 0, 0, 0, 0), held)
        return self

    def arrays(self):
        """(group, elem, ltype, params (n, 7), held) as SolverContext._dload takes them."""
        return (np.array(self.group, dtype=np.int32), np.array(self.elem, dtype=np.int32), np.array(self.ltype, dtype=np.int32),
                np.array(self.params, dtype=np.float64).reshape(-1, 7), np.array(self.held, dtype=np.uint8))


def dload_faces(coord, groups, node_mask):
    """The (group, element, face) triples -- 0-based group and element, 1-based face of getSubFace -- whose face nodes all lie in
    ``node_mask`` (n_node booleans): what a surface group of a !DLOAD card resolves to.  groups: [(etype, conn, ...)]."""
    mask = np.asarray(node_mask, dtype=bool)
    if mask.shape != (np.asarray(coord).shape[0],):
        raise ValueError("node_mask: one flag per node")
    out = []
    for g, grp in enumerate(groups):
        etype, conn = int(grp[0]), np.asarray(grp[1])
        conn = conn.reshape(-1, fstr_solid.NODES[etype])
        for f, nod in enumerate(tDload.SUBFACE[etype]):
            hit = mask[conn[:, np.array(nod) - 1] - 1].all(axis=1)
            out += [(g, int(e), f + 1) for e in np.nonzero(hit)[0]]
    return sorted(out)


class fstr_solid:
    """The resident nonlinear state of one context (created by fx_nl_init)."""

    NODES, POINTS = C3_NODES, C3_POINTS     # nodes and quadrature points (NumOfQuadPoints) per element

    def __init__(self, ctx, hecMESH_coord, hecMESH_conn, material, elem_mat=None, etype=361, groups=None, elemopt=2):
        """material: one tMaterial, or a list of them with elem_mat (1-based material id per element = the section's
        material, hecMESH%section_ID -> fstrSOLID%materials).  etype: 361 (B-bar), 341 / 342 (fx_nl_init_c3), or 351 / 352 / 362
        (fx_nl_init_type with the row length of hecMESH_conn).  elemopt (etype 361 only): 2 B-bar, 4 F-bar; any value but 2 goes
        through fx_nl_init_groups with one group, which makes the same single-type context and refuses what is not served.

        A mesh of several solid element types (fx_nl_init_groups): hecMESH_conn = None and groups = [(etype, conn, elemopt,
        elem_mat), ...], the tuples of SolverContext.assemble_groups / mesh.mesh_groups; a 361 group is B-bar (elemopt 2, also
        taken when left out or None) or F-bar (elemopt 4), elem_mat of every group is 1-based into the one list ``material``.  The state arrays and
        the element outputs are then flat, the groups one after the other (point_offsets, elem_offsets; group_slices cuts them
        into per-group views)."""
        self.ctx = ctx
        self._timed = False         # set_time has been called: a later STATIC step sets tincr = 0 again
        self.coord = np.ascontiguousarray(hecMESH_coord, dtype=np.float64)
        self.material = material
        self.n_node = self.coord.shape[0]
        if groups is not None:
            if hecMESH_conn is not None:
                raise ValueError("fstr_solid: give hecMESH_conn or groups, not both")
            self._init_groups(groups, material)
            return
        self.etype = int(etype)
        self.nn, self.nq = self.NODES.get(self.etype, 0), self.POINTS.get(self.etype, 0)
        self.conn = np.ascontiguousarray(hecMESH_conn, dtype=np.int32)
        self.n_elem = self.conn.shape[0]
        self._set_parts([(self.etype, self.n_elem)])
        mats, arr, self.elem_mat = self._materials(material, elem_mat, self.n_elem)
        mv = hecmw._MeshView(self.n_node, self.n_elem, _ptr(self.coord), _ptr(self.conn))
        head, tail = (ctx.h, C.byref(mv)), (len(mats), arr, _ptr(self.elem_mat))
        if self.etype == 361 and int(elemopt) != 2:
            tab, keep = hecmw.SolverContext._group_table([(361, self.conn, int(elemopt), self.elem_mat)])
            _chk(lib().fx_nl_init_groups(ctx.h, self.n_node, _ptr(self.coord), 1, tab, len(mats), arr))
            del keep
        elif self.etype in (351, 352, 362):
            nn_elem = self.conn.shape[1] if self.conn.ndim == 2 else 0
            _chk(lib().fx_nl_init_type(*head, self.etype, nn_elem, *tail))
        elif self.etype != 361:
            _chk(lib().fx_nl_init_c3(*head, self.etype, *tail))
        elif isinstance(material, (list, tuple)):
            _chk(lib().fx_nl_init_sections(*head, *tail))
        else:
            _chk(lib().fx_nl_init(*head, arr))

    @staticmethod
    def _materials(material, elem_mat=None, n_elem=None):
        """(mats, the _MaterialView array the entry points take, elem_mat as int32 or None).  n_elem given (one group): several
        materials need one id per element."""
        mats = list(material) if isinstance(material, (list, tuple)) else [material]
        arr = (_MaterialView * len(mats))(*[m.view() for m in mats])
        elem_mat = None if elem_mat is None else np.ascontiguousarray(elem_mat, dtype=np.int32)
        if n_elem is not None and len(mats) > 1 and (elem_mat is None or elem_mat.shape != (n_elem,)):
            raise ValueError("elem_mat: one material id per element")
        return mats, arr, elem_mat

    def _set_parts(self, parts):
        """parts: [(etype, n_elem)] in the context's order -> the offsets of the flat layouts (fx_nl_init_groups)."""
        self.parts = [(int(et), int(ne), self.NODES.get(int(et), 0), self.POINTS.get(int(et), 0)) for et, ne in parts]
        cum = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
        self.elem_offsets = cum([ne for _, ne, _, _ in self.parts])
        self.point_offsets = cum([ne * q for _, ne, _, q in self.parts])            # P_g of the per-point arrays
        self.tangent_offsets = cum([ne * 9 * nn * nn for _, ne, nn, _ in self.parts])  # doubles, element tangents
        self.force_offsets = cum([ne * 3 * nn for _, ne, nn, _ in self.parts])         # doubles, element internal forces
        self.n_point = int(self.point_offsets[-1])

    def _init_groups(self, groups, material):
        mats, arr, _ = self._materials(material)
        groups = [(g[0], g[1], 2 if len(g) < 3 or g[2] is None else g[2], g[3] if len(g) > 3 else None) for g in groups]
        tab, keep = hecmw.SolverContext._group_table(groups)
        self.groups = groups
        self.etype = self.nn = self.nq = self.conn = None       # no single type: see parts
        self._set_parts([(tab[g].etype, tab[g].n_elem) for g in range(len(groups))])
        self.n_elem = int(self.elem_offsets[-1])
        _chk(lib().fx_nl_init_groups(self.ctx.h, self.n_node, _ptr(self.coord), len(groups), tab, len(mats), arr))
        del keep

    def group_slices(self, name, array):
        """Per-group views of a flat array of a context of several groups: ``name`` a state array ("stress", ..., "istat":
        views (n_elem_g, nq_g[, 6])), "tangents" ((n_elem_g, 3 nn_g, 3 nn_g)) or "forces" ((n_elem_g, 3 nn_g))."""
        a = np.asarray(array).ravel()
        out = []
        for g, (et, ne, nn, q) in enumerate(self.parts):
            if name == "tangents":
                out.append(a[self.tangent_offsets[g]:self.tangent_offsets[g + 1]].reshape(ne, 3 * nn, 3 * nn))
            elif name == "forces":
                out.append(a[self.force_offsets[g]:self.force_offsets[g + 1]].reshape(ne, 3 * nn))
            elif name in ("plstrain", "fstat", "istat"):
                out.append(a[self.point_offsets[g]:self.point_offsets[g + 1]].reshape(ne, q))
            elif name in ("stress", "strain", "stress_bak", "strain_bak"):
                out.append(a[6 * self.point_offsets[g]:6 * self.point_offsets[g + 1]].reshape(ne, q, 6))
            else:
                raise ValueError("group_slices: %r is no per-point or per-element array" % (name,))
        return out

    # ---- distributed loads (fx_nl_set_dload)
    def set_dload(self, dload, rho=None, follow=True):
        """The !DLOAD cards of the step as a tDload (None clears them): from now on every sub-step adds factor * DLOAD to its
        nodal load, and with follow (DLOAD_follow, the default; False is `!DLOAD, FOLLOW=NO`) takes it on the current
        configuration and rebuilds it in every Newton iteration.  rho: one density per material (GRAV and CENT need it).
        The factor is the load factor at the end of the sub-step (fstr_Newton's factor[1]).  In a `!STEP, TYPE=VISCO` step
        fstr_solve_NLGEOM hands fstr_Newton the factors (0, 1) and scales the nodal load itself, so there the distributed load
        is applied whole in every sub-step, like a nodal load with load_held; it is not ramped."""
        if dload is None:
            _chk(lib().fx_nl_set_dload(self.ctx.h, 0, None, None, 0))
            return
        rho = None if rho is None else np.ascontiguousarray(np.atleast_1d(rho), dtype=np.float64)
        dv, keep = hecmw.SolverContext._dload(dload)
        _chk(lib().fx_nl_set_dload(self.ctx.h, 0 if rho is None else int(rho.size), _ptr(rho), C.byref(dv), int(bool(follow))))
        del keep

    def set_dload_factor(self, factor):
        """fstrSOLID%factor(2) for a caller that drives fx_nl_begin_substep itself (fstr_Newton sets it)."""
        _chk(lib().fx_nl_set_dload_factor(self.ctx.h, C.c_double(factor)))

    def get_load(self):
        """fstrSOLID%GL (3 * n_node) as the device holds it."""
        gl = np.zeros(3 * self.n_node)
        _chk(lib().fx_nl_get_load(self.ctx.h, _ptr(gl)))
        return gl

    # ---- thermal strain (fx_nl_set_thermal)
    thermal = False

    def set_thermal(self, ref_temp, temp_init=None):
        """Switch the thermal branches of the update routines on: !REFTEMP, the initial condition (n_node, None = 0; last_temp
        starts from it) and every material's expansion / expansion_table / elastic_table.  ref_temp = None switches them off."""
        if ref_temp is None:
            _chk(lib().fx_nl_set_thermal(self.ctx.h, None))
            self.thermal = False
            return
        mats = list(self.material) if isinstance(self.material, (list, tuple)) else [self.material]
        t0 = None if temp_init is None else np.ascontiguousarray(temp_init, dtype=np.float64)
        if t0 is not None and t0.shape != (self.n_node,):
            raise ValueError("temp_init: one temperature per node")
        alpha = np.array([float(m.expansion) for m in mats])

        def tables(name, ncol):
            tabs = [None if getattr(m, name) is None else np.ascontiguousarray(getattr(m, name), dtype=np.float64).reshape(-1, ncol)
                    for m in mats]
            if all(t is None for t in tabs):
                return None, None, tabs
            ptrs = (C.c_void_p * len(mats))(*[None if t is None else t.ctypes.data for t in tabs])
            rows = np.array([0 if t is None else t.shape[0] for t in tabs], dtype=np.int32)
            return ptrs, rows, tabs

        ap, ar, akeep = tables("expansion_table", 2)
        ep, er, ekeep = tables("elastic_table", 3)
        v = _NlThermalView(float(ref_temp), _ptr(t0), _ptr(alpha), None if ap is None else C.cast(ap, C.c_void_p), _ptr(ar),
                           None if ep is None else C.cast(ep, C.c_void_p), _ptr(er))
        _chk(lib().fx_nl_set_thermal(self.ctx.h, C.byref(v)))
        del akeep, ekeep
        self.thermal = True
        self._temperature = np.full(self.n_node, float(ref_temp)) if t0 is None else t0.copy()

    def temperature_at_step_start(self):
        """temp_bak of fstr_solve_NLGEOM.f90:92: the temperature last set, or what set_thermal left (the initial condition, or
        ref_temp without one)"""
        return self._temperature.copy()

    def set_temperature(self, temp):
        """fstrSOLID%temperature (n_node) of the coming sub-step or call."""
        t = None if temp is None else np.ascontiguousarray(temp, dtype=np.float64)
        if t is not None and t.shape != (self.n_node,):
            raise ValueError("temperature: one value per node")
        _chk(lib().fx_nl_set_temperature(self.ctx.h, _ptr(t)))
        self._temperature = t.copy()

    # ---- time (fx_nl_set_time) and the history of time-dependent materials
    def set_time(self, time, tincr):
        """ctime and tincr of the coming sub-step or call (fstr_solve_NonLinear.f90:74, :100, :162); (0, 0) after construction."""
        _chk(lib().fx_nl_set_time(self.ctx.h, C.c_double(time), C.c_double(tincr)))
        self._timed = True

    def history_width(self):
        w = C.c_int32(0)
        _chk(lib().fx_nl_get_history(self.ctx.h, None, C.byref(w)))
        return int(w.value)

    def get_history(self):
        """fstatus(1..W) of every point, (n_point, W); W = 0 without a time-dependent material."""
        w = self.history_width()
        out = np.zeros((self.n_point, w))
        if w:
            _chk(lib().fx_nl_get_history(self.ctx.h, _ptr(out), None))
        return out

    def set_history(self, hist):
        h = np.ascontiguousarray(hist, dtype=np.float64).reshape(self.n_point, -1)
        _chk(lib().fx_nl_set_history(self.ctx.h, _ptr(h) if h.size else None, int(h.shape[1])))

    # ---- state transfer (tests, restart, output)
    def get_state(self, names=("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat", "istat",
                               "unode", "dunode", "qforce")):
        """``last_temp`` may be named too (thermal strain on); it is not among the defaults."""
        want_last = "last_temp" in names
        names = tuple(k for k in names if k != "last_temp")
        ne, nn, q = self.n_elem, self.n_node, self.nq
        if self.etype is None:      # several groups: flat, the groups one after the other
            p6, p1 = (self.n_point, 6), (self.n_point,)
        else:
            p6, p1 = (ne, q, 6), (ne, q)
        shapes = {"stress": p6, "strain": p6, "stress_bak": p6, "strain_bak": p6,
                  "plstrain": p1, "fstat": p1, "istat": p1, "unode": (3 * nn,), "dunode": (3 * nn,),
                  "qforce": (3 * nn,)}
        out = {k: np.zeros(shapes[k], dtype=np.int32 if k == "istat" else np.float64) for k in names}
        v = _StateView(*[_ptr(out.get(k)) for k in shapes], 0)
        _chk(lib().fx_nl_get_state(self.ctx.h, C.byref(v)))
        out["latch"] = int(v.latch)
        if want_last:
            out["last_temp"] = np.zeros(nn)
            _chk(lib().fx_nl_get_last_temp(self.ctx.h, _ptr(out["last_temp"])))
        return out

    def set_state(self, state, latch=-1):
        keys = ("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat", "istat", "unode", "dunode", "qforce")
        arrs = {}
        for k in keys:
            if k in state and state[k] is not None:
                arrs[k] = np.ascontiguousarray(state[k], dtype=np.int32 if k == "istat" else np.float64)
        v = _StateView(*[_ptr(arrs.get(k)) for k in keys], int(latch))
        _chk(lib().fx_nl_set_state(self.ctx.h, C.byref(v)))
        if state.get("last_temp") is not None:
            _chk(lib().fx_nl_set_last_temp(self.ctx.h, _ptr(np.ascontiguousarray(state["last_temp"], dtype=np.float64))))

    def nodal_stress(self, principal=0):
        """fstr_NodalStress3D over the resident stress and strain of this context (fx_nl_nodal_stress): a hecmw.NodalStress; only
        the results cross the bus.  principal: make_principal's bit mask (hecmw.PRINC_*)."""
        res, ms = hecmw._NodalResult(), C.c_float(0)
        _chk(lib().fx_nl_nodal_stress(self.ctx.h, int(principal), C.byref(res), C.byref(ms)))
        return hecmw.NodalStress(res, ms.value)

    def element_tangents(self):
        ke = np.zeros(int(self.tangent_offsets[-1])) if self.etype is None else np.zeros((self.n_elem, 3 * self.nn, 3 * self.nn))
        _chk(lib().fx_nl_element_tangents(self.ctx.h, _ptr(ke)))
        return ke

    def element_update(self):
        qf = np.zeros(int(self.force_offsets[-1])) if self.etype is None else np.zeros((self.n_elem, 3 * self.nn))
        _chk(lib().fx_nl_element_update(self.ctx.h, _ptr(qf)))
        return qf


def _bc_arrays(bc):
    if bc is None:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)
    return (np.ascontiguousarray(bc[0], dtype=np.int32), np.ascontiguousarray(bc[1], dtype=np.int32),
            np.ascontiguousarray(bc[2], dtype=np.float64))


def fstr_StiffMatrix(fstrSOLID, bc=None):
    """fstr_StiffMatrix + fstr_AddBC: tangent of the current state into the resident matrix, Dirichlet
    elimination with the increments bc = (node, dof, value).  Returns the kernel time in ms."""
    bn, bd, bv = _bc_arrays(bc)
    ms = C.c_float(0)
    _chk(lib().fx_nl_stiffness(fstrSOLID.ctx.h, int(bn.size), _ptr(bn), _ptr(bd), _ptr(bv), C.byref(ms)))
    return ms.value


def fstr_UpdateNewton(fstrSOLID):
    """dunode += X; fstr_UpdateNewton; fstr_Update_NDForce.  Returns (res, xnrm, qnrm, dunrm_all) and the
    kernel time in ms."""
    out = (C.c_double * 4)()
    ms = C.c_float(0)
    _chk(lib().fx_nl_update(fstrSOLID.ctx.h, out, C.byref(ms)))
    return tuple(float(np.sqrt(v)) for v in out), ms.value


def fstr_UpdateState(fstrSOLID):
    _chk(lib().fx_nl_commit(fstrSOLID.ctx.h))


def fstr_NodalStress3D(fstrSOLID, principal=0):
    """fstr_NodalStress3D (fstr_NodalStress.f90:13-272): sets fstrSOLID.STRAIN, .STRESS, .MISES, .ESTRAIN, .ESTRESS, .EMISES and,
    where ``principal`` asks for them, .PSTRESS, .PSTRESS_VECT, .PSTRAIN, .PSTRAIN_VECT, .EPSTRESS, .EPSTRESS_VECT, .EPSTRAIN,
    .EPSTRAIN_VECT (None otherwise) from the resident state.  Returns the hecmw.NodalStress they come from."""
    r = fstrSOLID.nodal_stress(principal)
    for name, _, _ in r._SHAPES:
        setattr(fstrSOLID, name.upper(), getattr(r, name))
    return r


def fstr_cutback_save(fstrSOLID):
    """fstr_Cutback.f90:108-152 for the device-resident quadrature-point history."""
    _chk(lib().fx_nl_snapshot(fstrSOLID.ctx.h, 0))


def fstr_cutback_load(fstrSOLID):
    """fstr_Cutback.f90:155-198: back to the state of the last fstr_cutback_save."""
    _chk(lib().fx_nl_snapshot(fstrSOLID.ctx.h, 1))


def fstr_Newton(fstrSOLID, hecMAT, factor, bc, cload, max_iter, converg, commit_unconverged=False, temperature=None,
                time=None, tincr=None):
    """One substep of fstr_Newton.  factor = (FACTOR(1), FACTOR(2)); bc / cload are the values at load factor 1.
    temperature: fstrSOLID%temperature of this sub-step (fstr_solid.set_thermal first); None keeps the one last set.
    time, tincr: ctime and tincr of this sub-step (fstr_solid.set_time); both None keeps what was last set.
    Returns (converged, log) with log rows (iter, solver iterations, solver code, |B|, |X|, |QFORCE|, |dunode|)."""
    if temperature is not None:
        fstrSOLID.set_temperature(temperature)
    if time is not None or tincr is not None:
        fstrSOLID.set_time(0.0 if time is None else time, 0.0 if tincr is None else tincr)
    bn, bd, bv = _bc_arrays(bc)
    cl = None if cload is None else np.ascontiguousarray(cload, dtype=np.float64)
    log = np.zeros((max_iter, 7))
    nit = C.c_int32(0)
    code = lib().fx_newton_substep(fstrSOLID.ctx.h, C.c_double(factor[0]), C.c_double(factor[1]), int(bn.size), _ptr(bn),
                                   _ptr(bd), _ptr(bv), _ptr(cl), int(max_iter), C.c_double(converg), _ptr(hecMAT.Iarray),
                                   _ptr(hecMAT.Rarray), _ptr(log), C.byref(nit), int(commit_unconverged))
    _chk(code, allow=(hecmw.HECMW_SOLVER_ERROR_NOCONV_MAXIT, FX_NEWTON_MAXRES))
    fstrSOLID.last_code = code
    return code == 0, log[:nit.value].copy()


FX_NEWTON_MAXRES = 4002


def fstr_set_step_control(fstrSOLID, maxres=1.0e10, is_linear=False):
    """step_ctrl(cstep)%maxres (m_step.f90:31, :78) and fstr_Newton's isLinear (.not. fstrPR%nlgeom)."""
    _chk(lib().fx_nl_set_step_control(fstrSOLID.ctx.h, C.c_double(maxres), int(is_linear)))


def fstr_solve_NLGEOM(fstrSOLID, hecMAT, bc, cload, substeps, max_iter, converg, commit_unconverged=True, temperature=None,
                      tincr=None, start_time=0.0, load_held=False):
    """The sub-step loop of fstr_solve_NLGEOM with the default linear load-factor ramp (table_nlsta without
    amplitude).  temperature: the nodal temperature at load factor 1 (fstr_solid.set_thermal first), ramped as
    fstr_ass_load.f90:291-300 ramps it from temp_bak, the temperature at the start of the step (fstr_solve_NLGEOM.f90:92) -- in
    a first step the initial condition given to set_thermal or, without one, ref_temp (fstr_setup.f90:780):
    temperature(sub) = temp_bak + (temperature - temp_bak) * factor; and as the program calls fstr_UpdateState at the start of
    the step (:96), last_temp starts the step as that temperature.  tincr: the time increment of every sub-step of a `!STEP,
    TYPE=VISCO` step (None: a STATIC step, which sets tincr = 0 as fstr_Newton does for one, fstr_solve_NonLinear.f90:60-61, unless
    the context holds no time yet); sub-step k runs at the time of its start, start_time + (k - 1) tincr
    (fstr_solve_NLGEOM.f90:129-130: fstr_get_time() before fstr_proceed_time), which is what iso_creep and update_iso_creep document
    for ttime.  In a VISCO step the prescribed displacements are not ramped: fstr_AddBC gives the first sub-step the whole value and
    every later one nothing (fstr_AddBC.f90:44-47), while the nodal load follows the load factor as in a STATIC step -- or, with
    load_held, stays whole in every sub-step, which is what fstr_ass_load does for a load group that was active in the step before
    (fstr_ass_load.f90:69-70).  Returns the concatenated Newton log with the substep number
    in front."""
    logs = []
    if temperature is not None:
        temperature = np.asarray(temperature, dtype=np.float64)
        temp_bak = fstrSOLID.temperature_at_step_start()
        fstrSOLID.set_temperature(temp_bak)
        fstr_UpdateState(fstrSOLID)
    if tincr is None and fstrSOLID._timed:
        fstrSOLID.set_time(start_time, 0.0)         # a STATIC step after a VISCO one
    for sub in range(1, substeps + 1):
        tsub = None if temperature is None else temp_bak + (temperature - temp_bak) * (sub / substeps)
        f0, f1 = (sub - 1) / substeps, sub / substeps
        bcs, cl = bc, cload
        if tincr is not None:    # step and hold: fx_newton_substep forms bc * (factor1 - factor0) and cload * factor1, so factor (0, 1)
            if bc is not None and sub > 1:
                bcs = (bc[0], bc[1], np.zeros(len(bc[2])))
            if cload is not None and not load_held:
                cl = np.asarray(cload, dtype=np.float64) * f1
            f0, f1 = 0.0, 1.0
        ok, log = fstr_Newton(fstrSOLID, hecMAT, (f0, f1), bcs, cl, max_iter, converg,
                              commit_unconverged, temperature=tsub,
                              time=None if tincr is None else start_time + (sub - 1) * tincr, tincr=tincr)
        logs.append(np.concatenate([np.full((log.shape[0], 1), float(sub)), log], axis=1))
    return np.concatenate(logs, axis=0)
