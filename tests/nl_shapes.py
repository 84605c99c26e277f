"""The sizes at which the nonlinear element kernels are compared with their restatements (tests/test_gpu_nl_shapes.py), and a
restatement of what the host launches on them (tests/test_nl_shapes.py asserts that the cases reach what they are there for).

Kernel table: read from the sources, not written down here -- NL_GROUPS (fx_internal.h), nl_group_flag (fx_nl_point.h), nl_group_visco /
nl_group_creep (fx_visco.h), nl_fbar_group / nl_thermal_group (fx_nonlinear_host.h), FXN_BLOCK, FXF_BLOCK and the lanes-per-element
table of fx_c3_element.h.  A family is an element type and formulation: 361 B-bar, 361 F-bar ("361f"), 341, 342, 351, 352, 362.

Launch restatement: nl_part_lists (fx_nonlinear_host.h) -- elements grouped by the group of their material, inside a group colour
by colour (frontistr_amd.mesh.color_elements), 361 elements that name a node twice in their own list when the mesh is coloured --
and the launches of nl_launch_stiffness_group / nl_launch_update_group on those lists: one per non-empty (group, colour) range for
the coloured scatter, one per group for element matrices out, for the atomic scatter and for the update.

Cases: the smallest skewed meshes on which a group's own element list gives the launches of test_nl_shapes.CONDITIONS."""
import os
import re

import numpy as np

import hyper_ref as H
import visco_ref as V
from tet_nl_ref import INFINITE, TOTALLAG, UPDATELAG

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "frontistr_amd", "csrc")
FAMILIES = ("361", "361f", "341", "342", "351", "352", "362")


def family_type(fam):
    return int(fam[:3])


# ---- the kernel table, from the sources ----------------------------------------------------------------------------------------------
def _text(name):
    with open(os.path.join(SRC, name)) as f:
        return f.read()


def _c_expr(expr):
    """A C expression of ints, comparisons, !, &&, || and ?: (right-associative) as a Python one"""
    expr = expr.strip()
    depth = 0
    for i, ch in enumerate(expr):           # the first '?' outside parentheses and its ':'
        depth += ch == "("
        depth -= ch == ")"
        if ch == "?" and depth == 0:
            level, d2 = 0, 0
            for j in range(i + 1, len(expr)):
                d2 += expr[j] == "("
                d2 -= expr[j] == ")"
                if d2:
                    continue
                if expr[j] == "?":
                    level += 1
                elif expr[j] == ":":
                    if level == 0:
                        return "((%s) if (%s) else (%s))" % (_c_expr(expr[i + 1:j]), _c_expr(expr[:i]), _c_expr(expr[j + 1:]))
                    level -= 1
            raise ValueError(expr)
    if expr.startswith("(") and expr.endswith(")") and _balanced(expr[1:-1]):
        return "(" + _c_expr(expr[1:-1]) + ")"
    return re.sub(r"!(?!=)", " not ", expr.replace("&&", " and ").replace("||", " or "))


def _balanced(s):
    d = 0
    for ch in s:
        d += ch == "("
        d -= ch == ")"
        if d < 0:
            return False
    return d == 0


def _c_function(name, files, env):
    """`constexpr ... name(int G) { return EXPR; }` of one of the files as a Python function of G"""
    for f in files:
        m = re.search(r"constexpr\s+(?:int|bool)\s+%s\(int G\)\s*\{\s*return\s+(.*?);\s*\}" % name, _text(f))
        if m:
            code = _c_expr(m.group(1))
            return lambda G: eval(code, dict(env), {"G": G})       # noqa: S307 -- the project's own header, ints only
    raise LookupError(name)


def kernel_facts():
    """-> dict: n_groups, flag(G), visco(G), creep(G), fbar(G), thermal(G), epb[family] = (tangent, update)"""
    n_groups = int(re.search(r"constexpr int NL_GROUPS = (\d+);", _text("fx_internal.h")).group(1))
    env = {}
    env["nl_group_flag"] = _c_function("nl_group_flag", ["fx_nl_point.h"], env)
    env["nl_group_visco"] = _c_function("nl_group_visco", ["fx_visco.h"], env)
    env["nl_group_creep"] = _c_function("nl_group_creep", ["fx_visco.h"], env)
    env["nl_fbar_group"] = _c_function("nl_fbar_group", ["fx_nonlinear_host.h"], env)
    env["nl_thermal_group"] = _c_function("nl_thermal_group", ["fx_nonlinear_host.h"], env)
    fxn = int(re.search(r"#define FXN_BLOCK (\d+)", _text("fx_nonlinear.h")).group(1))
    fxf = int(re.search(r"#define FXF_BLOCK (\d+)", _text("fx_nonlinear_fbar.h")).group(1))
    c3 = _text("fx_c3_element.h")
    bs = int(re.search(r"static constexpr int BS = (\d+);", c3).group(1))
    rows = {int(a): (int(l), int(u)) for a, l, u in re.findall(r"\{(\d+), \d+, \d+, (\d+), (\d+)\}", c3)}
    epb = {"361": (fxn // 8, fxn // 8), "361f": (fxf // 8, fxn // 8)}      # k_nl_update_fbar runs in FXN_BLOCK lanes
    for et in (341, 342, 351, 352, 362):
        lpe, ulpe = rows[et]
        epb[str(et)] = ((bs // 64) * (64 // lpe) if lpe < 64 else bs // lpe, bs // ulpe)       # C3El::EPB, C3El::UEPB
    return dict(n_groups=n_groups, flag=env["nl_group_flag"], visco=env["nl_group_visco"], creep=env["nl_group_creep"],
                fbar=lambda G: bool(env["nl_fbar_group"](G)), thermal=lambda G: bool(env["nl_thermal_group"](G)), epb=epb)


def instantiated(facts=None):
    """every (family, group, TH) the host instantiates a tangent and an update kernel for"""
    k = kernel_facts() if facts is None else facts
    out = []
    for fam in FAMILIES:
        for g in range(k["n_groups"]):
            if fam == "361f" and not k["fbar"](g):
                continue
            out.append((fam, g, 0))
            if k["thermal"](g):
                out.append((fam, g, 1))
    return out


def material_group(mat):
    """NlMat::group of a material (nl_init_parts): the NLGEOM flag for ELASTIC and Mises, 3 hyperelastic, 4 + flag Mohr-Coulomb /
    Drucker-Prager, 7 + flag viscoelastic, 9 NORTON"""
    import yield_ref as Y
    if V.is_creep(mat):
        return 9
    if V.is_visco(mat):
        return 7 + mat.nlgeom
    if Y.is_yield(mat):
        return 4 + mat.nlgeom
    if H.kind_of(mat) in (H.MOONEY, H.ARRUDA):
        return 3
    return mat.nlgeom


# ---- nl_part_lists and the launchers -------------------------------------------------------------------------------------------------
def part_lists(conn, n_node, elem_group, n_groups, force_atomic=False):
    """nl_part_lists -> dict(order, dup, grp_off, dup_off, atomic, n_elem, colour_of): the lists are element ids (0-based)"""
    from frontistr_amd.mesh import color_elements
    conn = np.asarray(conn)
    ne, nn = conn.shape
    col = None if force_atomic else color_elements(conn, n_node)
    coloured = col is not None
    if coloured:
        order = np.argsort(col, kind="stable")
        off = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=int(col.max()) + 1))]).tolist()
    else:
        order, off = np.arange(ne), [0, ne]
    twice = [len(set(c)) < nn for c in conn.tolist()]
    grouped, dups, grp_off, dup_off = [], [], {}, {}
    for g in range(n_groups):
        go, doff, found = [], [len(dups)], False
        for k in range(len(off) - 1):
            before = len(grouped)
            for q in range(off[k], off[k + 1]):
                e = int(order[q])
                if elem_group[e] == g:
                    (dups if coloured and twice[e] else grouped).append(e)
            doff.append(len(dups))
            if len(grouped) > before or found:
                if not found:
                    go.append(before)
                found = True
                go.append(len(grouped))
        grp_off[g] = go
        dup_off[g] = doff if doff[-1] > doff[0] else []
    return dict(order=grouped, dup=dups, grp_off=grp_off, dup_off=dup_off, atomic=not coloured, n_elem=ne, colour_of=col)


def _launch(what, walk, e0, e1, epb):
    wg = (e1 - e0 + epb - 1) // epb
    return dict(what=what, walk=walk, e0=e0, e1=e1, workgroups=wg, last=(e1 - e0) - (wg - 1) * epb, epb=epb)


def _colour_ranges(off, one_range):
    """for_colour_ranges (fx_assemble_host.h)"""
    out = []
    for k in range(len(off) - 1):
        e0, e1 = (off[0], off[-1]) if one_range else (off[k], off[k + 1])
        if e1 > e0:
            out.append((e0, e1))
        if one_range:
            break
    return out


def tangent_launches(lists, g, epb, matrices_out):
    """nl_launch_stiffness_group of group g: `out` (element matrices out: one launch over the group's colours), `atomic` (the same with
    atomics where the mesh is not coloured), `colour` (one per non-empty colour range), `dup` (the group's collapsed elements) and
    `add` (k_add_elem_blocks, 64 per workgroup, per colour of the collapsed elements)"""
    one = matrices_out or lists["atomic"]
    what = "out" if matrices_out else ("atomic" if lists["atomic"] else "colour")
    out = [_launch(what, "order", e0, e1, epb) for e0, e1 in _colour_ranges(lists["grp_off"][g], one)]
    doff = lists["dup_off"][g]
    if doff:
        out.append(_launch("dup", "dup", doff[0], doff[-1], epb))
        if not matrices_out:
            out += [_launch("add", "dup", p0, p1, 64) for p0, p1 in _colour_ranges(doff, False)]
    return out


def update_launches(lists, g, epb):
    """nl_launch_update_group of group g: `update` over the group's list -- in element order where the group is the whole part -- and
    `dup` over its collapsed elements"""
    out = []
    off = lists["grp_off"][g]
    if off and off[-1] > off[0]:
        whole = off[0] == 0 and off[-1] == lists["n_elem"]
        out.append(_launch("update", "elements" if whole else "order", off[0], off[-1], epb))
    doff = lists["dup_off"][g]
    if doff:
        out.append(_launch("dup", "dup", doff[0], doff[-1], epb))
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
SKEW, CURVE = 0.1, 0.03


def _with_collapsed(m):
    """hyper_ref.gpu_mesh's collapsed hexahedron (a prism that names two nodes twice) on the nodes of the last cell"""
    c = m.conn[-1]
    m.conn = np.ascontiguousarray(np.vstack([m.conn, [[c[0], c[1], c[2], c[2], c[4], c[5], c[6], c[6]]]]).astype(np.int32))
    m.n_elem += 1
    return m


def mesh_of(name):
    from frontistr_amd.mesh import CubeMesh, PieMesh, renumber, solid_mesh
    if name == "gpu352":
        return H.gpu_mesh(352)
    if name == "gpu362":
        return H.gpu_mesh(362)
    if name == "pie24":
        return PieMesh(24, 2, 2)
    if name == "pie33":
        return PieMesh(33, 1, 2)
    if name == "renum7":
        return renumber(CubeMesh(7, skew=SKEW), 11)
    kind, n = name[:-1], int(name[-1])
    if kind == "cube":
        return CubeMesh(n, skew=SKEW)
    if kind == "cubedup":
        return _with_collapsed(CubeMesh(n, skew=SKEW))
    et = int(kind)
    return solid_mesh(n, et, skew=SKEW, **({"curve": CURVE} if et in (342, 352, 362) else {}))


def _ref(E, nu, flag):
    from oracle.refrun import Material
    return Material(E, nu, nlgeom=flag)


# materials by name: the constants of the existing GPU comparisons
MATERIALS = {
    "el_inf": lambda: _ref(2.5, 0.3, INFINITE), "el_tl": lambda: _ref(2.5, 0.3, TOTALLAG),          # the hyperelastic cases' partners
    "mooney": H.TEST_MATERIALS["mooney"], "arruda": H.TEST_MATERIALS["arruda"],
    "visco_inf": lambda: V.gpu_material("one", INFINITE), "visco_tl": lambda: V.gpu_material("two", TOTALLAG),
    "cvisco_inf": lambda: V.Material(206900.0, 0.29, V.PRONY["one"], INFINITE),                    # beside NORTON: its E, its amplitude
    "cvisco_tl": lambda: V.Material(206900.0, 0.29, V.PRONY["two"], TOTALLAG),
    "norton": V.creep_material, "el_ul": lambda: _ref(70000.0, 0.33, UPDATELAG),
}


class Case:
    """One context: family, mesh (mesh_of), materials (MATERIALS) dealt over the elements by `deal` (a function of the mesh
    -> 1-based material ids; None: `1 + e % k`), and the helper that makes displacement, history and time: "hyper" (zero state,
    hyper_ref.random_displacement at GPU_AMP), "visco" (visco_ref.gpu_case), "creep" (visco_ref.creep_case), "yield" (yield_ref.gpu_case
    with the seed and cohesion of yield_ref.SHAPE_CASES[yield_key]).  scatter: the assembled matrix is compared too (the coloured
    scatter, or the atomic one where the mesh cannot be coloured)."""

    def __init__(self, fam, mesh, mats, helper, deal=None, scatter=True, atomic_child=False, yield_key=None):
        self.fam, self.mesh, self.mats, self.helper, self.deal, self.scatter = fam, mesh, tuple(mats), helper, deal, scatter
        self.atomic_child = atomic_child
        self.th = 0
        self.yield_key = (mesh, "all") if yield_key is None else yield_key

    def materials(self):
        import yield_ref as Y
        out = []
        for x in self.mats:
            flag = {"inf": INFINITE, "tl": TOTALLAG, "ul": UPDATELAG}.get(x.split("_")[-1])
            if x.startswith("dp_") or x.startswith("mc_"):      # Drucker-Prager / Mohr-Coulomb on yield_ref's constants, the cohesion of this mesh
                out.append(Y.gpu_material("drucker" if x.startswith("dp_") else "mohr", flag, Y.SHAPE_CASES[self.yield_key][1]))
            elif x.startswith("mises_"):        # Mises BILINEAR on the same constants, the yield stress of this case
                from oracle.refrun import Material
                out.append(Material(Y.GPU_E, Y.GPU_NU, plastic=True, harden=0, plconst=(Y.SHAPE_CASES[self.yield_key][1], Y.GPU_H, 0.0), nlgeom=flag))
            elif x == "yel_inf":
                out.append(_ref(Y.GPU_E, Y.GPU_NU, INFINITE))
            else:
                out.append(MATERIALS[x]())
        return out

    @property
    def etype(self):
        return family_type(self.fam)

    def elem_mat(self, m):
        if len(self.mats) == 1:
            return None
        if self.deal is not None:
            return np.asarray(self.deal(m), dtype=np.int32)
        return (1 + np.arange(m.conn.shape[0]) % len(self.mats)).astype(np.int32)

    def amplitude(self):
        import yield_ref as Y
        return {"creep": V.CREEP_AMP, "yield": Y.GPU_AMP}.get(self.helper, H.GPU_AMP)

    def single_precision(self):
        """UPDATELAG at an STF_C3 type: UPDATE_C3 rounds the stress increment to default real (static_LIB_3d.f90:718)"""
        return self.etype != 361 and any(x.nlgeom == UPDATELAG for x in self.materials())

    def build(self):
        """-> (mesh, visco_ref.Model with displacement, history and time set)"""
        m = mesh_of(self.mesh)
        mats = self.materials()
        em = self.elem_mat(m)
        fbar = self.fam == "361f"
        if self.helper == "creep":
            assert not fbar
            return V.creep_case(self.etype, mats=mats, elem_mat=em, mesh=m)
        if self.helper == "visco":
            return V.gpu_case(self.etype, fbar=fbar, mats=mats, elem_mat=em, mesh=m)
        model = V.Model(self.etype, m.coord, m.conn, mats, em, fbar=fbar)
        seed = 17
        if self.helper == "yield":
            import yield_ref as Y
            seed = Y.SHAPE_CASES[self.yield_key][0]
        model.unode[:], model.dunode[:] = H.random_displacement(m.coord, seed, self.amplitude())
        return m, model

    def elem_groups(self, m):
        g = [material_group(x) for x in self.materials()]
        em = self.elem_mat(m)
        return np.full(m.conn.shape[0], g[0]) if em is None else np.array(g)[em - 1]


class ThermalCase(Case):
    """A context with thermal strain on (the TH = 1 kernels): materials (kind of nl_thermal_ref.material, NLGEOM flag) with the
    !ELASTIC and !EXPANSION_COEFF tables -- the tangent kernels take their thermal variant only with an elastic table --, node
    temperatures, initial condition and last_temp as nl_thermal_ref.gpu_case makes them, displacement fields of its amplitude."""
    def __init__(self, fam, mesh, kinds, deal=None):
        Case.__init__(self, fam, mesh, ["%s_%d" % k for k in kinds], "thermal", deal)
        self.kinds, self.th = tuple(kinds), 1

    cid, cohesion = None, None          # cohesion: set by the search that filled nl_thermal_ref.SHAPE_COHESION

    def materials(self):
        import nl_thermal_ref as NT
        c = NT.SHAPE_COHESION.get(self.cid) if self.cohesion is None else self.cohesion
        return [NT.material(kind, self.fam, True, flag, c=c if kind in ("drucker", "mohr") else None) for kind, flag in self.kinds]

    def amplitude(self):
        import nl_thermal_ref as NT
        return NT.AMP

    def build(self):
        """-> the case dict of nl_thermal_ref.model_of"""
        import nl_thermal_ref as NT
        m = mesh_of(self.mesh)
        return NT.gpu_case(self.fam, "tables", mesh=m, mats=self.materials(), elem_mat=self.elem_mat(m))


def _colour_to_first(*colours):
    """deal: the elements of the given colours of the mesh ("largest": of its largest colour) to material 1, every other element to
    material 2"""
    def deal(m):
        from frontistr_amd.mesh import color_elements
        col = color_elements(m.conn, m.n_node)
        return np.where(np.isin(col, [int(np.argmax(np.bincount(col))) if k == "largest" else k for k in colours]), 1, 2)
    return deal


def _counts(*counts):
    """deal: counts[k] elements to material k + 1, spread over the mesh with a stride of 7 (the element counts here have no factor 7)"""
    def deal(m):
        n = m.conn.shape[0]
        assert sum(counts) == n and n % 7, (counts, n)
        em = np.zeros(n, dtype=np.int32)
        em[(np.arange(n) * 7) % n] = np.repeat(np.arange(1, len(counts) + 1), counts)
        return em
    return deal


def _cases():
    c = {}
    # the mesh of a family's one-material cases: more than one workgroup of both kernels with a partly filled last one where the
    # element count allows, colours of more than one tangent workgroup
    solo_mesh = {"361": "cube7", "361f": "cube5", "341": "3414", "342": "3423", "351": "3514", "352": "gpu352", "362": "gpu362"}
    # 64 hexahedra where the restatement is dear: the hyperelastic one takes 12 ms an element, F-bar's total Lagrange 25 to 40 ms
    hyper_solo = dict(solo_mesh, **{"361": "cube4", "361f": "cube4"})
    for fam in FAMILIES:
        s = solo_mesh[fam]
        tl = hyper_solo[fam] if fam == "361f" else s
        c["%s_solo_el_inf" % fam] = Case(fam, s, ["el_inf"], "hyper")
        c["%s_solo_el_tl" % fam] = Case(fam, tl, ["el_tl"], "hyper")
        c["%s_solo_mooney" % fam] = Case(fam, hyper_solo[fam], ["mooney"], "hyper")
        c["%s_solo_visco_inf" % fam] = Case(fam, s, ["visco_inf"], "visco")
        c["%s_solo_visco_tl" % fam] = Case(fam, tl, ["visco_tl"], "visco")
        if fam != "361f":
            c["%s_solo_el_ul" % fam] = Case(fam, s, ["el_ul"], "creep")
            c["%s_solo_norton" % fam] = Case(fam, s, ["norton"], "creep")
        # several groups in one context: every list is walked through colors.order
        # (a deal in turn gives 352's tangent, two elements per workgroup, lists of even length, and 341's lists of 96 = 4 x 24)
        c["%s_mix_hyper" % fam] = Case(fam, hyper_solo[fam] if fam != "361" else "cubedup4", ["el_inf", "el_tl", "mooney"], "hyper",
                                       deal=_counts(19, 17, 18) if fam == "352" else None, atomic_child=True)
        if fam == "361f":
            c["361f_mix_visco"] = Case(fam, s, ["visco_inf", "visco_tl"], "visco")
        else:
            # 351: four lists of more than one update workgroup (32) take the 250 wedges of the 5^3 cube
            c["%s_mix_creep" % fam] = Case(fam, {"361": "cubedup4", "351": "3515"}.get(fam, s), ["cvisco_inf", "cvisco_tl", "norton", "el_ul"],
                                           "creep", deal={"341": _counts(154, 77, 77, 76), "352": _counts(15, 13, 13, 13)}.get(fam))
    # Drucker-Prager under the three flags (groups 4..6), B-bar and the STF_C3 types
    for fam in FAMILIES:
        if fam == "361f":
            continue
        s = solo_mesh[fam] if fam != "361" else "cube4"
        for flag in ("inf", "tl", "ul"):
            c["%s_solo_dp_%s" % (fam, flag)] = Case(fam, s, ["dp_" + flag], "yield")
        c["%s_mix_dp" % fam] = Case(fam, s if fam != "361" else "cubedup4", ["dp_inf", "dp_tl", "dp_ul"], "yield",
                                    deal=_counts(19, 17, 18) if fam == "352" else None)
    c["352_mix_dp_2"] = Case("352", "gpu352", ["dp_inf", "dp_tl", "dp_ul"], "yield", deal=_counts(18, 17, 19))
    # 361 B-bar: the 48 elements of cube7's second colour (no seed of the first 39 keeps all 2744 points of the cube off the edges)
    for flag in ("inf", "tl", "ul"):
        c["361_mix_dp_%s_colour" % flag] = Case("361", "cube7", ["dp_" + flag, "yel_inf"], "yield", deal=_colour_to_first(1),
                                                yield_key=("cube7", "colour1"))
    # thermal strain on (TH = 1): ELASTIC under the three flags and Mooney-Rivlin, all with tables
    for fam in FAMILIES:
        s = solo_mesh[fam]
        hs = hyper_solo[fam]
        flags = (("inf", INFINITE), ("tl", TOTALLAG)) + ((("ul", UPDATELAG),) if fam != "361f" else ())
        for name, flag in flags:
            c["%s_th_solo_el_%s" % (fam, name)] = ThermalCase(fam, hs if fam == "361f" and name == "tl" else s, [("elastic", flag)])
        c["%s_th_solo_mooney" % fam] = ThermalCase(fam, hs, [("hyper", TOTALLAG)])
        c["%s_th_mix" % fam] = ThermalCase(fam, {"361": "cubedup4", "351": "3515", "361f": "cube4"}.get(fam, s),
                                           [("elastic", f) for _, f in flags] + [("hyper", TOTALLAG)],
                                           deal={"341": _counts(154, 77, 77, 76), "352": _counts(15, 13, 13, 13)}.get(fam))
    c["361_th_mix_mooney_colour"] = ThermalCase("361", "cube7", [("hyper", TOTALLAG), ("elastic", TOTALLAG)], deal=_colour_to_first(1))
    for kind in ("elastic", "hyper"):
        c["361f_th_mix_%s_colour" % kind] = ThermalCase("361f", "cube5", [(kind, TOTALLAG), ("elastic", INFINITE)], deal=_colour_to_first(1, 2))
    for fam in ("341", "342", "351"):       # the hyperelastic group alone in the largest colour: 25, 14 and 14 elements
        c["%s_th_mix_mooney_colour" % fam] = ThermalCase(fam, solo_mesh[fam], [("hyper", TOTALLAG), ("elastic", TOTALLAG)],
                                                         deal=_colour_to_first("largest"))
    # thermal strain on, Drucker-Prager with E(T), nu(T) inside the return mapping (TH = 1 of groups 4..6): the contexts of the
    # Drucker-Prager cases above; the cohesion of each is nl_thermal_ref.SHAPE_COHESION
    for fam in FAMILIES:
        flags = (("inf", INFINITE), ("tl", TOTALLAG)) + ((("ul", UPDATELAG),) if fam != "361f" else ())
        s = {"361": "cube4", "361f": "cube4"}.get(fam, solo_mesh[fam])
        for name, flag in flags:
            c["%s_th_solo_dp_%s" % (fam, name)] = ThermalCase(fam, s, [("drucker", flag)])
            if fam in ("361", "361f"):
                big, cols = ("cube7", (1,)) if fam == "361" else ("cube5", (1, 2))
                c["%s_th_mix_dp_%s_colour" % (fam, name)] = ThermalCase(fam, big, [("drucker", flag), ("elastic", INFINITE)],
                                                                        deal=_colour_to_first(*cols))
        c["%s_th_mix_dp" % fam] = ThermalCase(fam, s if fam != "361" else "cubedup4", [("drucker", f) for _, f in flags],
                                              deal=_counts(19, 17, 18) if fam == "352" else None)
    c["352_th_mix_dp_2"] = ThermalCase("352", "gpu352", [("drucker", f) for f in (INFINITE, TOTALLAG, UPDATELAG)], deal=_counts(18, 17, 19))
    c["352_th_mix_2"] = ThermalCase("352", "gpu352", [("hyper", TOTALLAG), ("elastic", TOTALLAG)])
    # Mohr-Coulomb and Mises under the three flags (F-bar: two): the return mappings of groups 4..6 and, in groups 0..2, everything
    # behind the kernels' `plastic` test, on lists of more than one workgroup
    for fam in FAMILIES:
        flags = ("inf", "tl") + (("ul",) if fam != "361f" else ())
        s = {"361": "cube4", "361f": "cube4"}.get(fam, solo_mesh[fam])
        if fam in ("342", "362"):       # dealt in three, a section of these meshes misses the shares (23 % and 98 % plastic): one flag a case
            for f in flags:
                c["%s_solo_mc_%s" % (fam, f)] = Case(fam, s, ["mc_" + f], "yield", yield_key=(s, "mohr"))
        else:
            c["%s_mix_mohr" % fam] = Case(fam, s, ["mc_" + f for f in flags], "yield", yield_key=(s, "fbar mohr" if fam == "361f" else "mohr"),
                                          deal=_counts(19, 17, 18) if fam == "352" else None)
        s = {"361": "cube7", "361f": "cube4"}.get(fam, solo_mesh[fam])
        c["%s_mix_mises" % fam] = Case(fam, s, ["mises_" + f for f in flags], "yield", yield_key=(s, "fbar mises" if fam == "361f" else "mises"),
                                       deal=_counts(19, 17, 18) if fam == "352" else None)
    # F-bar: no UPDATELAG; seed and cohesion from fbar_ref.search_plastic_case on the F-bar trial stresses
    for flag in ("inf", "tl"):
        c["361f_solo_dp_%s" % flag] = Case("361f", "cube4", ["dp_" + flag], "yield", yield_key=("cube4", "fbar"))
        c["361f_mix_dp_%s_colour" % flag] = Case("361f", "cube5", ["dp_" + flag, "yel_inf"], "yield", deal=_colour_to_first(1, 2),
                                                 yield_key=("cube5", "fbar colours 1, 2"))
    c["361f_mix_dp"] = Case("361f", "cube4", ["dp_inf", "dp_tl"], "yield", yield_key=("cube4", "fbar"))
    c["352_mix_mooney"] = Case("352", "gpu352", ["mooney", "el_tl"], "hyper")          # 27 and 27: three odd lists do not make 54
    # 361 B-bar: the hyperelastic group with a colour of more than one workgroup.  343 hyperelastic elements are too dear for the
    # restatement: the 48 elements of cube7's second colour are hyperelastic, the others ELASTIC
    c["361_mix_mooney_colour"] = Case("361", "cube7", ["mooney", "el_tl"], "hyper", deal=_colour_to_first(1))
    # F-bar's total-Lagrange groups the same way on cube5: the 36 elements of its second and third colour beside a cheap partner of
    # a lower group, so that two update workgroups, a partly filled last one and a colour of more than one tangent workgroup are theirs
    c["361f_mix_el_tl_colour"] = Case("361f", "cube5", ["el_tl", "el_inf"], "hyper", deal=_colour_to_first(1, 2))
    c["361f_mix_mooney_colour"] = Case("361f", "cube5", ["mooney", "el_inf"], "hyper", deal=_colour_to_first(1, 2))
    c["361f_mix_visco_tl_colour"] = Case("361f", "cube5", ["visco_tl", "visco_inf"], "visco", deal=_colour_to_first(1, 2))
    # irregular 361 meshes
    c["361_pie24"] = Case("361", "pie24", ["el_inf", "el_tl", "mooney"], "hyper")
    c["361f_pie24"] = Case("361f", "pie24", ["el_inf", "el_tl", "mooney"], "hyper")
    c["361_pie24_creep"] = Case("361", "pie24", ["cvisco_tl", "norton", "el_ul"], "creep")
    c["361_pie33"] = Case("361", "pie33", ["el_inf", "el_tl", "mooney"], "hyper")
    c["361_renum7"] = Case("361", "renum7", ["el_tl", "visco_tl"], "visco")
    for cid, case in c.items():
        case.cid = cid
    return c


CASES = _cases()

def case_launches(case, facts=None, force_atomic=False):
    """-> {group: dict(out=[...], scatter=[...], update=[...])} of the launches a case's context makes"""
    k = kernel_facts() if facts is None else facts
    m = mesh_of(case.mesh)
    eg = case.elem_groups(m)
    lists = part_lists(m.conn, m.n_node, eg, k["n_groups"], force_atomic)
    tep, uep = k["epb"][case.fam]
    out = {}
    for g in sorted(set(eg.tolist())):
        out[int(g)] = dict(out=tangent_launches(lists, g, tep, True), scatter=tangent_launches(lists, g, tep, False),
                           update=update_launches(lists, g, uep))
    return out, lists
