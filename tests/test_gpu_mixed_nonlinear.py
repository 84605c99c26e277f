"""GPU parity of the nonlinear static loop on meshes of several solid element types (fx_nl_init_groups; fstr_solid(...,
groups=[...])) through the C ABI and frontistr_amd/fstr.py against the composed restatement tests/mixed_nl_ref.py.

Meshes (mixed_nl_ref._mesh): MixedMesh(2, order), MixedMesh(3, order, skew=0.1, curve=0.03 at order 2) and the renumbered
MixedMesh(2, order), order 1 (361 + 351 + 341) and 2 (362 + 352 + 342): 2 or 3 hexahedra, 8 or 24 wedges, 12 or 72 tetrahedra,
nq = 8 / 2 / 1 and 27 / 9 / 4 -- every group starts at another point offset.  Group lists (mixed_nl_ref.group_list): the three
groups in mesh order, the wedge group cut in two (one type twice), an empty group in the middle; the variant of a case is
(kind + NLGEOM flag) mod 3, so every mesh, kind and flag meets all three.  Materials: the KINDS of test_gpu_c3_nonlinear.py, the
two-section ones with that test's (arange * 7 // 3) % 2 pattern cut into the groups, on every mesh under all three NLGEOM
flags (a case takes a few tenths of a second).  Beside them one hyperelastic case (Neo-Hooke beside an
ELASTIC TOTALLAG section) and one Drucker-Prager case (TOTALLAG, beside a Mises UPDATELAG section).

Tolerances, the project's own: 1e-11 relative to the largest entry of the compared array for INFINITE and TOTALLAG and for
everything of a 361 group.  Quantities that depend on an UPDATELAG stress of an STF_C3 type (`real()` of the stress increment,
static_LIB_3d.f90:718): at most 2 x 2^-23 relative to the group's largest stress increment (quantities linear in the stress: to
their largest entry), and at most 1 % of the components above 1e-11; tests/test_mixed_nl_ref.py shows that the restatement alone,
its nodes summed in two orders on these inputs, stays inside that cap.  Arrays are compared group by group (group_slices).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import c3_ref as R
import hyper_ref as H
import mixed_nl_ref as M
import test_gpu_c3_nonlinear as C3T
import yield_ref as Y
from oracle.refrun import Material

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX_ERROR_UNSUPPORTED, FX_ERROR_RUNTIME = -2, -1
SINGLE = 2.0 * 2.0 ** -23
E0, NU0 = C3T.E0, C3T.NU0
KINDS = C3T.KINDS
NLGEOM = (M.INFINITE, M.TOTALLAG, M.UPDATELAG)
NLNAME = ("infinite", "totallag", "updatelag")


def materials(kind, nlgeom):
    """-> (material list, two sections?)"""
    if kind == "neohooke":          # hyperelastic: TOTALLAG only; beside an ELASTIC section of its own stiffness scale
        return [H.neohooke(0.1486, 0.0789), Material(1.0, 0.3, nlgeom=M.TOTALLAG)], True
    if kind == "drucker":
        return [Y.drucker_prager(E0, NU0, 300.0, 20.0, 2000.0, nlgeom=M.TOTALLAG),
                Material(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=M.UPDATELAG)], True
    mat, emf = C3T.materials(kind, nlgeom)
    return (mat if isinstance(mat, list) else [mat]), emf is not None


def _cases():
    out = []
    for order in (1, 2):
        for mesh in M.MESHES:
            for ki, kind in enumerate(KINDS):
                for ni, nlgeom in enumerate(NLGEOM):
                    variant = M.VARIANTS[(ki + ni) % 3]
                    out.append(pytest.param(order, mesh, variant, kind, nlgeom, id="o%d-%s-%s-%s-%s" % (order, mesh, variant, kind, NLNAME[ni])))
    for kind in ("neohooke", "drucker"):
        out.append(pytest.param(1, "n2", "split_wedges", kind, M.TOTALLAG, id="o1-n2-split_wedges-%s" % kind))
        out.append(pytest.param(2, "n3", "empty_middle", kind, M.TOTALLAG, id="o2-n3-empty_middle-%s" % kind))
    return out


def _fmat(mat):
    from frontistr_amd import fstr
    if Y.is_yield(mat):
        fm = fstr.tMaterial(mat.E, mat.nu, plastic=True, harden=0, plconst=mat.plconst, nlgeom_flag=mat.nlgeom)
        fm.kind, fm.plconst4 = (fstr.MOHRCOULOMB if mat.kind == Y.MOHR else fstr.DRUCKERPRAGER), mat.plconst4
        return fm
    if H.kind_of(mat) == H.ARRUDA:
        return fstr.tMaterial.arruda_boyce(*mat.plconst)
    if H.kind_of(mat) == H.MOONEY:
        return fstr.tMaterial.mooney_rivlin(*mat.plconst)
    return fstr.tMaterial(mat.E, mat.nu, plastic=mat.plastic, harden=mat.harden, plconst=mat.plconst,
                          table=mat.table if mat.table.size else None, nlgeom_flag=mat.nlgeom)


def _profile(hip, mesh, groups, ctx=None):
    hm = hip.hecmwST_local_mesh(n_node=mesh.n_node)
    hecMAT = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)
    if ctx is None:
        ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    return ctx, hecMAT


def _solid(hip, mesh, groups, mats, ctx=None):
    from frontistr_amd import fstr
    ctx, hecMAT = _profile(hip, mesh, groups, ctx)
    return ctx, hecMAT, fstr.fstr_solid(ctx, mesh.coord, None, [_fmat(x) for x in mats], groups=groups)


def _close(a, b, tol, tag, scale=None):
    if np.asarray(b).size == 0:
        assert np.asarray(a).size == 0, tag
        return
    scale = max(np.abs(b).max(), 1e-300) if scale is None else scale
    err = np.abs(a - b).max() / scale
    print("%s: %.3e (bound %.1e)" % (tag, err, tol))
    assert err < tol, "%s: %.3e" % (tag, err)


def _close_ul(a, b, tag, scale=None):
    """the two-tier rule of the module docstring"""
    scale = max(np.abs(b).max(), 1e-300) if scale is None else scale
    d = np.abs(a - b) / scale
    share = (d > 1e-11).mean()
    print("%s: max %.3e (bound %.3e), share above 1e-11: %.5f" % (tag, d.max(), SINGLE, share))
    assert d.max() <= SINGLE, "%s: %.3e" % (tag, d.max())
    assert share <= 0.01, "%s: %.4f of the components differ by more than 1e-11" % (tag, share)


def _cmp(a, b, ul, tag, scale=None):
    (_close_ul(a, b, tag, scale) if ul else _close(a, b, 1e-11, tag, scale))


def _ul_groups(ref):
    """per group: does it hold an element of an STF_C3 type with an UPDATELAG material?"""
    return [p["etype"] != 361 and any(ref.mat_of(p, e).nlgeom == M.UPDATELAG for e in range(p["conn"].shape[0])) for p in ref.parts]


def _model(mesh, groups, mats, unode, dunode, st, latch=0):
    ref = M.Model(mesh.coord, groups, mats)
    ref.set_flat(st)
    ref.unode[:], ref.dunode[:] = unode, dunode
    ref.latch = latch
    return ref


def _matrix(ctx, hecMAT):
    ctx.download_matrix(hecMAT)
    return [np.array(getattr(hecMAT, k)) for k in ("D", "AL", "AU")]


@pytest.mark.parametrize("order,mesh,variant,kind,nlgeom", _cases())
def test_elements_state_matrix_and_qforce(hip, oracle, order, mesh, variant, kind, nlgeom):
    from frontistr_amd import fstr
    mats, two = materials(kind, nlgeom)
    m, groups, unode, dunode, st = M.gpu_case(mesh, order, variant, mats, two)
    ref = _model(m, groups, mats, unode, dunode, st)
    uls = _ul_groups(ref)
    tag = lambda g, what: "group %d (TYPE=%d) %s" % (g + 1, ref.parts[g]["etype"], what)
    ctx, hecMAT, solid = _solid(hip, m, groups, mats)
    assert [p[1] for p in solid.parts] == [p["conn"].shape[0] for p in ref.parts]
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    # tangents before the latch
    for g, (a, b) in enumerate(zip(solid.group_slices("tangents", solid.element_tangents()), ref.element_tangents())):
        _close(a, b, 1e-11, tag(g, "tangent before the first update"))
    # the assembled matrix with boundary conditions, twice: bitwise repeatable
    bc = m.dirichlet()
    bc = (bc[0], bc[1], 1e-3 * np.cos(np.arange(bc[0].size)))
    Kd, fd = R.apply_bc(ref.stiffness(), np.zeros(3 * m.n_node), bc)
    got = []
    for _ in range(2):
        fstr.fstr_StiffMatrix(solid, bc)
        got.append(_matrix(ctx, hecMAT))
    for x, y in zip(*got):
        assert np.array_equal(x, y), "two assemblies of the same state differ"
    scale = np.abs(Kd).max()
    for k, x, y in zip(("D", "AL", "AU"), got[0], R.to_blocks(Kd, hecMAT)):
        _close(x, y, 1e-11, "assembled " + k, scale)
    # stress update, internal forces, state
    qf = solid.group_slices("forces", solid.element_update())
    rqf = ref.element_update()
    s = solid.get_state()
    assert s["latch"] == ref.latch
    cut = lambda name: solid.group_slices(name, s[name])
    plastic = [x for x in mats if x.plastic]
    for g, p in enumerate(ref.parts):
        ul, rs = uls[g], p["st"]
        if p["conn"].shape[0] == 0:
            continue
        ds = max(np.abs(ref.dstress[g]).max(), 1e-300)
        _cmp(cut("stress")[g], rs["stress"], ul, tag(g, "stress"), ds if ul else None)
        _cmp(qf[g], rqf[g], ul, tag(g, "element internal force"))
        _close(cut("strain")[g], rs["strain"], 1e-11, tag(g, "strain"))
        if ref.latch:
            assert np.array_equal(cut("istat")[g], rs["istat"]), tag(g, "istat")
            if ul:      # as test_gpu_c3_nonlinear.py: fstatus(1) follows the stress at 1 / (3 G)
                G = min(x.E / (2.0 * (1.0 + x.nu)) for x in plastic)
                _close_ul(cut("fstat")[g], rs["fstat"], tag(g, "fstatus(1)"), ds / G)
            else:
                _close(cut("fstat")[g], rs["fstat"], 1e-11, tag(g, "fstatus(1)"), max(np.abs(rs["fstat"]).max(), 1e-3))
    for k in ("plstrain", "stress_bak", "strain_bak"):      # the element update leaves them alone
        assert np.array_equal(s[k].ravel(), st[k]), k
    # tangents after the update: latched in EVERY group, new stress in the geometric terms
    for g, (a, b) in enumerate(zip(solid.group_slices("tangents", solid.element_tangents()), ref.element_tangents())):
        _cmp(a, b, uls[g], tag(g, "tangent after the update"))
    # QFORCE: the scattered internal force of all groups (fp64 atomics)
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    q = np.zeros(3 * m.n_node)
    hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(dunode), hip._ptr(q), None))
    ref = _model(m, groups, mats, unode, dunode, st)
    _cmp(q, ref.update(), any(uls), "QFORCE")
    # fstr_UpdateState group by group: the _bak copies, plstrain of the elastoplastic elements only
    fstr.fstr_UpdateState(solid)
    ref.commit()
    s = solid.get_state()
    assert np.array_equal(s["stress_bak"], s["stress"]) and np.array_equal(s["strain_bak"], s["strain"])
    for g, p in enumerate(ref.parts):
        pl = np.array([bool(ref.mat_of(p, e).plastic) for e in range(p["conn"].shape[0])], dtype=bool)
        got_pl, got_fs, old = (solid.group_slices("plstrain", a)[g] for a in (s["plstrain"], s["fstat"], st["plstrain"]))
        assert np.array_equal(got_pl[pl], got_fs[pl]) and np.array_equal(got_pl[~pl], old[~pl]), tag(g, "plstrain after the commit")
    ctx.close()


@pytest.mark.parametrize("order", [1, 2])
def test_newton_substeps_with_mises(hip, oracle, order):
    """A whole fstr_Newton sub-step loop (fx_newton_substep around CG + SSOR to 1e-12) on the two-section mesh, Mises BILINEAR
    beside ELASTIC, both TOTALLAG (nothing is rounded to single precision, so device and restatement differ by the linear solves
    alone): the Newton counts are equal and the norms agree to rtol 1e-6 / atol 1e-9 as in test_gpu_nonlinear.py.  The solves
    are converged to 1e-12 of their right-hand side, the previous residual: six orders below the bound unless one Newton
    iteration gains more than six orders (after the first plastic update the latched elastic tangent converges linearly, ten
    and more iterations per sub-step to CONVERG = 1e-3)."""
    from frontistr_amd import fstr
    from oracle.refrun import default_params
    mats = [Material(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=M.TOTALLAG), Material(70000.0, 0.33, nlgeom=M.TOTALLAG)]
    m, groups, _, _, st = M.gpu_case("n2", order, "split_wedges", mats, True, history=False)
    node, dof, val = m.dirichlet()
    t = m.top_nodes
    bc = (np.concatenate([node, t, t]).astype(np.int32), np.concatenate([dof, np.full(t.size, 3), np.full(t.size, 1)]).astype(np.int32),
          np.concatenate([val, np.full(t.size, 0.01), np.full(t.size, 0.002)]))
    ref = M.Model(m.coord, groups, mats)
    ctx, hecMAT, solid = _solid(hip, m, groups, mats)
    I, Rr = default_params(method=1, precond=1, maxit=5000, tol=1e-12)
    hecMAT.Iarray[:] = I
    hecMAT.Rarray[:] = Rr
    nsub = 3
    for sub in range(1, nsub + 1):
        f = ((sub - 1) / nsub, sub / nsub)
        ok, it = ref.newton_substep(f[0], f[1], bc, None, 50, 1e-3)
        assert ok
        okd, log = fstr.fstr_Newton(solid, hecMAT, f, bc, None, 50, 1e-3)
        want = np.array(ref.newton_log)
        print("sub-step %d: Newton iterations %d (restatement %d)\n%s\n%s" % (sub, log.shape[0], it, log[:, 3:], want[:, 1:]))
        assert okd and log.shape[0] == it
        np.testing.assert_allclose(log[:, 3:], want[:, 1:], rtol=1e-6, atol=1e-9)
    assert (ref.flat("plstrain") > 0).any(), "no plastic point"
    s = solid.get_state()
    _close(s["unode"], ref.unode, 1e-9, "unode")
    assert np.array_equal(s["istat"], ref.flat("istat"))
    _close(s["plstrain"], ref.flat("plstrain"), 1e-8, "plstrain", 1.0)
    ctx.close()


@pytest.mark.parametrize("order", [1, 2])
def test_newton_substeps_with_a_follower_load(hip, oracle, order):
    """The same loop driven by a distributed load alone (mixed_nl_ref.follower_case: the bottom clamped, nothing prescribed at the
    top, follower pressure on the top side and gravity, the materials of test_newton_substeps_with_mises; CG + SSOR to 1e-12)
    beside the restatement's loop with its load rebuilt in every iteration, sub-step by sub-step: equal Newton counts, the norms
    to rtol 1e-6 / atol 1e-9 and unode to 1e-9, the bounds of the test above for the reason given there.  Then once with
    FOLLOW=NO: other counts or norms.  tests/test_dload_nl_ref.py asserts that the restatement alone converges on these values
    and leaves a plastic point."""
    from frontistr_amd import fstr
    from oracle.refrun import default_params
    F = M.FOLLOWER
    m, groups, mats, bc, dl = M.follower_case(order)
    nsub = F["nsub"]
    logs = {}
    for follow in (True, False):
        ref = M.Model(m.coord, groups, mats)
        ctx, hecMAT, solid = _solid(hip, m, groups, mats)
        I, Rr = default_params(method=1, precond=1, maxit=5000, tol=1e-12)
        hecMAT.Iarray[:] = I
        hecMAT.Rarray[:] = Rr
        solid.set_dload(dl, F["rho"], follow=follow)
        logs[follow] = []
        for sub in range(1, nsub + 1):
            f = ((sub - 1) / nsub, sub / nsub)
            ok, it = ref.newton_substep(f[0], f[1], bc, None, F["max_iter"], F["converg"], dload=(dl.arrays(), F["rho"], follow))
            assert ok
            okd, log = fstr.fstr_Newton(solid, hecMAT, f, bc, None, F["max_iter"], F["converg"])
            want = np.array(ref.newton_log)
            print("follow %s sub-step %d: Newton iterations %d (restatement %d)\n%s\n%s" % (follow, sub, log.shape[0], it, log[:, 3:], want[:, 1:]))
            assert okd and log.shape[0] == it
            np.testing.assert_allclose(log[:, 3:], want[:, 1:], rtol=1e-6, atol=1e-9)
            logs[follow].append(log[:, 3:].copy())
        assert (ref.flat("plstrain") > 0).any(), "no plastic point"
        s = solid.get_state()
        _close(s["unode"], ref.unode, 1e-9, "unode, follow %s" % follow)
        assert np.array_equal(s["istat"], ref.flat("istat"))
        ctx.close()
    same = all(a.shape == b.shape and np.allclose(a, b, rtol=1e-6, atol=1e-9) for a, b in zip(logs[True], logs[False]))
    assert not same, "FOLLOW=NO gave the follower run's counts and norms"


def test_snapshot_restores_every_group_bitwise(hip, oracle):
    from frontistr_amd import fstr
    mats, two = materials("two_sections", M.UPDATELAG)
    m, groups, unode, dunode, st = M.gpu_case("n3", 2, "split_wedges", mats, two)
    ctx, hecMAT, solid = _solid(hip, m, groups, mats)
    solid.set_state(dict(st, unode=unode, dunode=np.zeros_like(dunode)), latch=0)
    before = solid.get_state()
    fstr.fstr_cutback_save(solid)
    solid.set_state(dict(dunode=dunode))
    solid.element_update()
    fstr.fstr_UpdateState(solid)
    mid = solid.get_state()
    for g, (a, b) in enumerate(zip(solid.group_slices("stress", mid["stress"]), solid.group_slices("stress", before["stress"]))):
        assert not np.array_equal(a, b), "group %d did not move" % (g + 1)
    fstr.fstr_cutback_load(solid)
    after = solid.get_state()
    for k in M.STATE6 + M.STATE1:
        assert np.array_equal(after[k], before[k]), k
    ctx.close()


def test_collapsed_hexahedra_in_a_361_group(hip, oracle):
    """Two 361 groups (the second one after the wedges, so that its element matrices sit behind another part's) whose hexahedra
    each name a node twice (a hexahedron collapsed to a wedge along one edge): served as in the single-type context
    (colors.dup), every block of the repeated node added."""
    from frontistr_amd import fstr
    mats, two = materials("two_sections", M.UPDATELAG)
    m = M._mesh("n3", 1)
    et, conn, opt, _ = m.groups_with(2)[0]
    conn = conn.copy()
    conn[:, 7] = conn[:, 4]
    conn[:, 6] = conn[:, 5]      # the edge 7-8 onto the edge 5-6: a wedge; the mesh no longer conforms, the algebra does not care
    groups = m.groups_with(2, (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32))
    ghex = groups[0]
    groups = [(et, conn[:2], opt, ghex[3][:2]), groups[1], (et, conn[2:], opt, ghex[3][2:]), groups[2]]
    unode, dunode, st = M.random_case(m, groups, mats, 23)
    ref = _model(m, groups, mats, unode, dunode, st)
    ctx, hecMAT, solid = _solid(hip, m, groups, mats)
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    for g, (a, b) in enumerate(zip(solid.group_slices("tangents", solid.element_tangents()), ref.element_tangents())):
        _close(a, b, 1e-11, "group %d tangent" % (g + 1))
    bc = m.dirichlet()
    Kd, fd = R.apply_bc(ref.stiffness(), np.zeros(3 * m.n_node), bc)
    got = []
    for _ in range(2):
        fstr.fstr_StiffMatrix(solid, bc)
        got.append(_matrix(ctx, hecMAT))
    for x, y in zip(*got):
        assert np.array_equal(x, y), "two assemblies of the same state differ"
    for k, x, y in zip(("D", "AL", "AU"), got[0], R.to_blocks(Kd, hecMAT)):
        _close(x, y, 1e-11, "assembled " + k, np.abs(Kd).max())
    qf = solid.group_slices("forces", solid.element_update())
    rqf = ref.element_update()
    s = solid.get_state()
    for g in (0, 2):             # the 361 groups: 1e-11 whatever the flag
        _close(qf[g], rqf[g], 1e-11, "group %d internal force" % (g + 1))
        _close(solid.group_slices("stress", s["stress"])[g], ref.parts[g]["st"]["stress"], 1e-11, "group %d stress" % (g + 1))
        assert np.array_equal(solid.group_slices("istat", s["istat"])[g], ref.parts[g]["st"]["istat"])
    ctx.close()


def _state_and_matrix(hip, ctx, hecMAT, solid, st, unode, dunode, bc):
    """tangents, assembled matrix, update, state, tangents again: everything a context computes"""
    from frontistr_amd import fstr
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    out = [np.asarray(solid.element_tangents()).ravel()]
    fstr.fstr_StiffMatrix(solid, bc)
    out += _matrix(ctx, hecMAT)
    out.append(np.asarray(solid.element_update()).ravel())
    s = solid.get_state()
    out += [np.asarray(s[k]).ravel() for k in M.STATE6 + M.STATE1]
    out.append(np.asarray(solid.element_tangents()).ravel())
    fstr.fstr_UpdateState(solid)
    out.append(np.asarray(solid.get_state(("plstrain",))["plstrain"]).ravel())
    return out


@pytest.mark.parametrize("etype", [361, 352, 341, "361_collapsed"])
def test_one_group_is_the_single_type_context_bitwise(hip, oracle, etype):
    """fx_nl_init_groups with one group (also: with empty groups around it) against fx_nl_init_sections (361) / fx_nl_init_type /
    fx_nl_init_c3 on the same mesh, two sections: every number equal bit for bit.  361_collapsed: two of the hexahedra, one of
    each section, name two nodes twice (the collapsed-element tail of the tangent and update launchers, with its own room for
    the element matrices)."""
    from frontistr_amd import fstr
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    collapsed, etype = etype == "361_collapsed", 361 if etype == "361_collapsed" else etype
    m = CubeMesh(3, skew=0.1) if etype == 361 else solid_mesh(2, etype, skew=0.1)
    mats, _ = materials("two_sections", M.UPDATELAG)
    em = (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32)
    conn = m.conn.copy()
    if collapsed:
        hexes = [4, 18]
        assert em[4] != em[18]
        conn[hexes, 7], conn[hexes, 6] = conn[hexes, 4], conn[hexes, 5]      # the edge 7-8 onto the edge 5-6: a wedge
    groups = [(etype, conn, 2, em)]
    unode, dunode, st = M.random_case(m, groups, mats, 5)
    bc = m.dirichlet()
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = conn.shape[1]
    hm.elem_node_item = conn.ravel()
    res = []
    empty = (342, np.zeros((0, 10), dtype=np.int32), 2, np.zeros(0, dtype=np.int32))
    for how in ("single", "groups", "groups_with_empty"):
        hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
        ctx = hip.SolverContext()
        ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
        fm = [_fmat(x) for x in mats]
        if how == "single":
            solid = fstr.fstr_solid(ctx, m.coord, conn, fm, elem_mat=em, etype=etype)
        else:
            solid = fstr.fstr_solid(ctx, m.coord, None, fm, groups=groups if how == "groups" else [empty] + groups + [empty])
        res.append(_state_and_matrix(hip, ctx, hecMAT, solid, st, unode, dunode, bc))
        ctx.close()
    for other in res[1:]:
        assert len(other) == len(res[0])
        for i, (a, b) in enumerate(zip(res[0], other)):
            assert np.array_equal(a, b), "output %d differs from the single-type context" % i


def _init_groups(hip, ctx, mesh, groups, mats):
    """fx_nl_init_groups -> (return code, message)"""
    from frontistr_amd import fstr
    tab, keep = hip.SolverContext._group_table(groups)
    views = [_fmat(x).view() for x in mats]
    arr = (fstr._MaterialView * max(len(views), 1))(*views)
    coord = np.ascontiguousarray(mesh.coord)
    code = hip.lib().fx_nl_init_groups(ctx.h, mesh.n_node, hip._ptr(coord), len(groups), tab, len(views), arr if views else None)
    return code, hip.lib().fx_last_error().decode()


def test_refusals_leave_the_context_usable(hip, oracle):
    mats, two = materials("two_sections", M.TOTALLAG)
    m, groups, unode, dunode, st = M.gpu_case("n2", 1, "mesh_order", mats, two)
    ctx, hecMAT, solid = _solid(hip, m, groups, mats)
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    want = np.asarray(solid.element_tangents()).copy()

    def swap(g, **kw):
        et, conn, opt, em = groups[g]
        d = dict(etype=et, conn=conn, elemopt=opt, em=em)
        d.update(kw)
        return groups[:g] + [(d["etype"], d["conn"], d["elemopt"], d["em"])] + groups[g + 1:]

    def bad(a, idx, v):
        a = a.copy()
        a[idx] = v
        return a
    hyper = [H.neohooke(0.1486, 0.0789), mats[0]]
    yhyper = [H.neohooke(0.1486, 0.0789), Y.drucker_prager(E0, NU0, 300.0, 20.0, 2000.0)]
    cases = [("IC hexahedra", swap(0, elemopt=1), mats, FX_ERROR_UNSUPPORTED, "group 1"),
             ("FI hexahedra", swap(0, elemopt=3), mats, FX_ERROR_UNSUPPORTED, "group 1"),
             ("unknown type", swap(1, etype=371), mats, FX_ERROR_UNSUPPORTED, "group 2"),
             ("node id", swap(2, conn=bad(groups[2][1], (3, 1), m.n_node + 1)), mats, FX_ERROR_RUNTIME, "group 3, element 4"),
             ("material id", swap(1, em=bad(groups[1][3], 2, 3)), mats, FX_ERROR_RUNTIME, "group 2, element 3"),
             ("degenerate wedge", swap(1, conn=bad(groups[1][1], (4, 5), groups[1][1][4, 0])), mats, FX_ERROR_RUNTIME, "element 5 names a node twice"),
             ("no elem_mat", swap(2, em=None), mats, FX_ERROR_RUNTIME, "group 3"),
             ("no group", [], mats, FX_ERROR_RUNTIME, "n_group"),
             ("no material", groups, [], FX_ERROR_RUNTIME, "materials missing"),
             ("Mises beside hyperelastic", groups, hyper, FX_ERROR_UNSUPPORTED, "hyperelastic"),
             ("Drucker-Prager beside hyperelastic", groups, yhyper, FX_ERROR_UNSUPPORTED, "hyperelastic"),
             ("material kind", groups, [mats[0], Material(E0, NU0, plastic=True, harden=7)], FX_ERROR_UNSUPPORTED, "fx_nl_init")]
    for name, grp, mt, code, text in cases:
        got, msg = _init_groups(hip, ctx, m, grp, mt)
        print("%s: %d %s" % (name, got, msg))
        assert got == code and text in msg, (name, got, msg)
        assert "fx_nl_init" in msg
        assert np.array_equal(np.asarray(solid.element_tangents()), want), name + ": the context changed"
    # only empty groups: nothing to build
    got, msg = _init_groups(hip, ctx, m, [(g[0], g[1][:0], g[2], g[3][:0]) for g in groups], mats)
    assert got == FX_ERROR_RUNTIME and "empty mesh" in msg, (got, msg)
    # a context without a profile
    ctx2 = hip.SolverContext()
    got, msg = _init_groups(hip, ctx2, m, groups, mats)
    assert got == FX_ERROR_RUNTIME and "profile" in msg, (got, msg)
    ctx2.close()
    # both a connectivity and groups
    from frontistr_amd import fstr
    with pytest.raises(ValueError):
        fstr.fstr_solid(ctx, m.coord, groups[0][1], [_fmat(x) for x in mats], groups=groups)
    assert np.array_equal(np.asarray(solid.element_tangents()), want)
    ctx.close()


def test_contexts_replace_each_other_on_one_fx_context(hip, oracle):
    """group context -> single-type fx_nl_init (361, the oracle's numbers) -> group context again, all on one fx_context"""
    from frontistr_amd import fstr
    import test_gpu_nonlinear as G
    mats, two = materials("two_sections", M.UPDATELAG)
    m, groups, unode, dunode, st = M.gpu_case("n2", 2, "mesh_order", mats, two)
    ctx, hecMAT, solid = _solid(hip, m, groups, mats)
    first = _state_and_matrix(hip, ctx, hecMAT, solid, st, unode, dunode, m.dirichlet())
    T = G._T()
    hmat, hm, hu, hdu, hst = T.element_case("mises_bilinear_ul", seed=11)
    ke0, qf, ke1, ost = oracle.nl_elements(hmat, hm.coord, hm.conn, hu, hdu, hst)
    hx = hip.hecmwST_local_mesh(n_node=hm.n_node)
    hx.elem_node_item = hm.conn.ravel()
    ctx.upload(hip.hecmw_mat_con(hx, hip.hecmwST_matrix()), what=hip.FX_UP_PROFILE)
    hsolid = fstr.fstr_solid(ctx, hm.coord, hm.conn, G._fmat(hmat))
    hsolid.set_state(dict(hst, unode=hu, dunode=hdu), latch=0)
    _close(hsolid.element_tangents(), ke0, 1e-11, "361 ke0")
    _close(hsolid.element_update(), qf, 1e-11, "361 qf")
    _close(hsolid.get_state()["stress"], ost["stress"], 1e-11, "361 stress")
    _close(hsolid.element_tangents(), ke1, 1e-11, "361 ke1")
    ctx, hecMAT, solid = _solid(hip, m, groups, mats, ctx=ctx)
    again = _state_and_matrix(hip, ctx, hecMAT, solid, st, unode, dunode, m.dirichlet())
    for i, (a, b) in enumerate(zip(first, again)):      # the matrix too: no atomics on the coloured path
        assert np.array_equal(a, b), "output %d" % i
    ctx.close()


# ---- FX_ASM_ATOMIC=1 is read once per process -> child processes
def compute_paths(path):
    from frontistr_amd import fstr, hecmw as hip
    from oracle import pyoracle
    pyoracle.build()
    out = {}
    for order in (1, 2):
        mats, two = materials("two_sections", M.UPDATELAG)
        m, groups, unode, dunode, st = M.gpu_case("n3", order, "split_wedges", mats, two)
        ctx, hecMAT, solid = _solid(hip, m, groups, mats)
        solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
        fstr.fstr_StiffMatrix(solid, m.dirichlet())
        for k, a in zip(("D", "AL", "AU"), _matrix(ctx, hecMAT)):
            out["%d/%s" % (order, k)] = a
        ctx.close()
    np.savez(path, **out)


def test_atomic_scatter_agrees(tmp_path):
    res = {}
    for name, env in (("default", {}), ("atomic", {"FX_ASM_ATOMIC": "1"})):
        out = str(tmp_path / (name + ".npz"))
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_mixed_nonlinear as T; T.compute_paths(%r)" % (HERE, ROOT, out)
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
        assert p.returncode == 0, "scatter path %s: child exited with %d\n%s" % (name, p.returncode, p.stdout[-3000:])
        res[name] = dict(np.load(out))
    for k, want in res["default"].items():      # equal to rounding: 1e-12 of the diagonal, as test_gpu_c3_nonlinear.py
        scale = max(np.abs(res["default"][k.split("/")[0] + "/D"]).max(), 1e-300)
        assert np.abs(res["atomic"][k] - want).max() <= 1e-12 * scale, ("atomic", k)
