"""The host path of the nonlinear context (csrc/fx_nonlinear_host.h): the five fx_nl_init* entry points run one set-up driver, and
fx_nl_stiffness and fx_mat_ass_bc one Dirichlet elimination.  What the single-type entry points refuse, with which code, under
whose name, and that a refusal leaves the context that was there untouched; that a one-material call does not read elem_mat;
that the elimination is the same arithmetic from both callers.  Every comparison is bit for bit: the inputs are the same and the
kernels are the same, so is every number.

Meshes: the 2 x 2 x 2 cube of each type (CubeMesh(2), solid_mesh(2, etype): 8 to 48 elements).  The collapsed hexahedra behind a
single-type entry point are a parameter of test_gpu_mixed_nonlinear.test_one_group_is_the_single_type_context_bitwise."""
import ctypes as C

import numpy as np
import pytest

import mixed_nl_ref as M
from oracle.refrun import Material
from test_gpu_mixed_nonlinear import _fmat

pytestmark = pytest.mark.gpu
FX_ERROR_UNSUPPORTED, FX_ERROR_RUNTIME = -2, -1
E0, NU0 = 206900.0, 0.29
ENTRIES = [("fx_nl_init", 361), ("fx_nl_init_sections", 361), ("fx_nl_init_c3", 341), ("fx_nl_init_c3", 342),
           ("fx_nl_init_type", 351), ("fx_nl_init_type", 352), ("fx_nl_init_type", 362)]


def _mesh(etype):
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    return CubeMesh(2, skew=0.1) if etype == 361 else solid_mesh(2, etype, skew=0.1)


def _context(hip, m):
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    return ctx, hecMAT


def _init(hip, ctx, entry, etype, coord, conn, mats, elem_mat, n_node=None, n_elem=None, n_mat=None):
    """the entry point through ctypes -> (return code, message); mats: oracle materials, None: a null pointer"""
    from frontistr_amd import fstr
    coord, conn = np.ascontiguousarray(coord, dtype=np.float64), np.ascontiguousarray(conn, dtype=np.int32)
    mv = hip._MeshView(coord.shape[0] if n_node is None else n_node, conn.shape[0] if n_elem is None else n_elem, hip._ptr(coord),
                       hip._ptr(conn))
    arr = None if mats is None else (fstr._MaterialView * len(mats))(*[_fmat(x).view() for x in mats])
    n_mat = (0 if mats is None else len(mats)) if n_mat is None else n_mat
    em = None if elem_mat is None else np.ascontiguousarray(elem_mat, dtype=np.int32)
    L, head = hip.lib(), (ctx.h, C.byref(mv))
    if entry == "fx_nl_init":
        code = L.fx_nl_init(*head, arr)
    elif entry == "fx_nl_init_sections":
        code = L.fx_nl_init_sections(*head, n_mat, arr, hip._ptr(em))
    elif entry == "fx_nl_init_c3":
        code = L.fx_nl_init_c3(*head, etype, n_mat, arr, hip._ptr(em))
    else:
        code = L.fx_nl_init_type(*head, etype, conn.shape[1], n_mat, arr, hip._ptr(em))
    return code, L.fx_last_error().decode()


def _materials(entry):
    """what the context is built with: two sections where the entry point takes them"""
    if entry == "fx_nl_init":
        return [Material(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=M.UPDATELAG)]
    return [Material(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=M.UPDATELAG), Material(70000.0, 0.33, nlgeom=M.TOTALLAG)]


@pytest.mark.parametrize("entry,etype", ENTRIES, ids=["%s-%d" % e for e in ENTRIES])
def test_refusals_of_the_single_type_entry_points(hip, entry, etype):
    """Codes as the set-up has always returned them: FX_ERROR_RUNTIME for ids out of range, missing materials, an empty mesh, a
    mesh that is not the profile's, no profile and a degenerate element; FX_ERROR_UNSUPPORTED for a hardening law that is not
    served.  The message names the entry point called, and the context built before returns the tangents it returned before."""
    from frontistr_amd import fstr
    m = _mesh(etype)
    mats = _materials(entry)
    two = len(mats) > 1
    em = (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32) if two else None
    groups = [(etype, m.conn, 2, em)]
    unode, dunode, st = M.random_case(m, groups, mats, 5)
    ctx, hecMAT = _context(hip, m)
    fm = [_fmat(x) for x in mats]
    solid = fstr.fstr_solid(ctx, m.coord, m.conn, fm if entry != "fx_nl_init" else fm[0], elem_mat=em, etype=etype)
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    want = np.asarray(solid.element_tangents()).copy()
    code, msg = _init(hip, ctx, entry, etype, m.coord, m.conn, mats, em)       # the call itself is one the entry point accepts
    assert code == 0, msg
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    assert np.array_equal(np.asarray(solid.element_tangents()), want)

    def conn_with(e, k, v):
        c = m.conn.copy()
        c[e, k] = v
        return c

    def em_with(e, v):
        a = em.copy()
        a[e] = v
        return a
    nn = m.conn.shape[1]
    R, U = FX_ERROR_RUNTIME, FX_ERROR_UNSUPPORTED
    cases = [("node id 0", R, "", dict(conn=conn_with(1, 0, 0))),
             ("node id n_node + 1", R, "", dict(conn=conn_with(m.n_elem - 1, nn - 1, m.n_node + 1))),
             ("n_elem = 0", R, "", dict(n_elem=0)),
             ("n_node is not the profile's", R, "", dict(coord=np.vstack([m.coord, m.coord[-1:] + 1.0]))),
             ("harden = 4", U, "", dict(mats=[Material(E0, NU0, plastic=True, harden=4, plconst=(450.0, 2000.0, 0.0))] + mats[1:]))]
    if entry == "fx_nl_init":
        cases.append(("no material", R, "", dict(mats=None)))
    else:
        cases += [("material id 0", R, "", dict(elem_mat=em_with(2, 0))),
                  ("material id n_mat + 1", R, "", dict(elem_mat=em_with(m.n_elem - 1, 3))),
                  ("two materials, no elem_mat", R, "", dict(elem_mat=None)),
                  ("n_mat = 0", R, "", dict(n_mat=0))]
    if etype != 361:
        cases.append(("a node named twice", R, "twice", dict(conn=conn_with(1, nn - 1, m.conn[1, 0]))))
    for name, want_code, text, kw in cases:
        args = dict(coord=m.coord, conn=m.conn, mats=mats, elem_mat=em)
        args.update(kw)
        code, msg = _init(hip, ctx, entry, etype, **args)
        print("%s: %d %s" % (name, code, msg))
        assert code == want_code, (name, code, msg)
        assert (entry + ":") in msg and text in msg, (name, msg)
        assert np.array_equal(np.asarray(solid.element_tangents()), want), name + ": the context changed"
    ctx2 = hip.SolverContext()                   # a context without a profile
    code, msg = _init(hip, ctx2, entry, etype, m.coord, m.conn, mats, em)
    assert code == FX_ERROR_RUNTIME and (entry + ":") in msg, (code, msg)
    ctx2.close()
    assert np.array_equal(np.asarray(solid.element_tangents()), want)
    ctx.close()


@pytest.mark.parametrize("entry,etype", [("fx_nl_init_sections", 361), ("fx_nl_init_c3", 342), ("fx_nl_init_type", 352)])
def test_one_material_does_not_read_elem_mat(hip, entry, etype):
    """n_mat = 1 with an elem_mat of zeros -- ids that are out of range -- succeeds and gives the numbers of a null elem_mat."""
    from frontistr_amd import fstr
    m = _mesh(etype)
    mats = _materials("fx_nl_init")
    unode, dunode, st = M.random_case(m, [(etype, m.conn, 2, None)], mats, 7)
    ctx, hecMAT = _context(hip, m)
    solid = fstr.fstr_solid(ctx, m.coord, m.conn, [_fmat(mats[0])], etype=etype)
    res = []
    for em in (None, np.zeros(m.n_elem, dtype=np.int32)):
        code, msg = _init(hip, ctx, entry, etype, m.coord, m.conn, mats, em)
        assert code == 0, msg
        solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
        out = [np.asarray(solid.element_tangents()).copy(), np.asarray(solid.element_update()).copy()]
        s = solid.get_state()
        out += [np.asarray(s[k]).copy() for k in M.STATE6 + M.STATE1] + [np.array([s["latch"]])]
        out.append(np.asarray(solid.element_tangents()).copy())
        res.append(out)
    assert res[0][-2][0] == 1                     # the Mises update has set the latch: the second tangent is another one
    for i, (a, b) in enumerate(zip(*res)):
        assert np.array_equal(a, b), "output %d differs with an elem_mat of zeros" % i
    ctx.close()


def test_dirichlet_elimination_is_one_for_both_callers(hip):
    """fx_nl_stiffness with prescribed dofs and non-zero increments against fx_nl_stiffness_at followed by fx_mat_ass_bc with the
    same list, on the same state and right-hand side: D, AL, AU and B bit for bit."""
    from frontistr_amd import fstr
    m = _mesh(361)
    mats = _materials("fx_nl_init_sections")
    em = (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32)
    unode, dunode, st = M.random_case(m, [(361, m.conn, 2, em)], mats, 9)
    rng = np.random.default_rng(3)
    GL, qforce = rng.standard_normal(3 * m.n_node), rng.standard_normal(3 * m.n_node)
    node, dof, _ = m.dirichlet()
    node, dof = np.concatenate([node, [m.n_node]]).astype(np.int32), np.concatenate([dof, [2]]).astype(np.int32)   # and a dof of the top face
    val = 1e-3 * (1.0 + np.cos(np.arange(node.size)))
    ctx, hecMAT = _context(hip, m)
    solid = fstr.fstr_solid(ctx, m.coord, m.conn, [_fmat(x) for x in mats], elem_mat=em)
    res = []
    for how in ("fx_nl_stiffness", "fx_mat_ass_bc"):
        solid.set_state(dict(st, unode=unode, dunode=dunode, qforce=qforce), latch=0)
        hip._chk(hip.lib().fx_nl_begin_substep(ctx.h, hip._ptr(GL)))                # B = GL - QFORCE (and dunode = 0)
        if how == "fx_nl_stiffness":
            fstr.fstr_StiffMatrix(solid, (node, dof, val))
        else:
            hip._chk(hip.lib().fx_nl_stiffness_at(ctx.h, None, None, None))
            hip._chk(hip.lib().fx_mat_ass_bc(ctx.h, int(node.size), hip._ptr(node), hip._ptr(dof), hip._ptr(val)))
        ctx.download_matrix(hecMAT)
        res.append([np.array(getattr(hecMAT, k)) for k in ("D", "AL", "AU", "B")])
    assert np.abs(res[0][3]).max() > 0 and not np.array_equal(res[0][3], GL - qforce)   # the elimination moved the right-hand side
    for k, a, b in zip(("D", "AL", "AU", "B"), *res):
        assert np.array_equal(a, b), k
    ctx.close()
