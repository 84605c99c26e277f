"""Distributed loads in the device nonlinear loop (fx_nl_set_dload, csrc/fx_dload.h): the resident load vector GL against the numpy
restatement of DL_C3 (tests/dload_ref.py) on the configurations fstr_ass_load takes it on, and whole NLSTATIC runs against the
unmodified reference program's (tests/golden/dload_nl.npz, recorded by tests/golden/make_dload_nl_golden.py from the decks of
tests/dload_nl_decks.py), with and without `FOLLOW=NO`.

Bounds: GL is summed with atomics: 1e-11 of its largest entry.  The recorded runs: the same Newton count in every sub-step and the
Global summaries at the printed decimals (hyper_ref.within_1e4)."""
import ctypes as C
import json

import numpy as np
import pytest

import dload_nl_decks as D
import dload_ref as R
from frontistr_amd.mesh import CubeMesh, solid_mesh

pytestmark = pytest.mark.gpu


def _solid(hip, etype, coord, conn, mat, elemopt=2):
    from frontistr_amd import fstr
    hm = hip.hecmwST_local_mesh(n_node=coord.shape[0])
    hm.nn_elem = conn.shape[1]
    hm.elem_node_item = conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    return ctx, hecMAT, fstr.fstr_solid(ctx, coord, conn, mat, etype=etype, elemopt=elemopt)


def _begin(hip, solid, cload):
    cl = np.ascontiguousarray(cload, dtype=np.float64)
    hip._chk(hip.lib().fx_nl_begin_substep(solid.ctx.h, hip._ptr(cl)))


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("etype", [361, 342])
def test_resident_load_vector(hip, etype):
    from frontistr_amd import fstr
    from oracle.refrun import default_params
    m = CubeMesh(3) if etype == 361 else solid_mesh(3, etype)
    groups = [(etype, m.conn)]
    ctx, hecMAT, solid = _solid(hip, etype, m.coord, m.conn, fstr.tMaterial(1000.0, 0.3, nlgeom_flag=fstr.TOTALLAG))
    # a finite rotation about y and a stretch of the whole mesh
    a = 0.35
    F = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]) @ np.diag([1.15, 0.95, 1.1])
    U = ((m.coord - 1.5) @ F.T + 1.5 - m.coord).ravel()
    top = m.coord[:, 2] == 3.0
    faces = fstr.dload_faces(m.coord, groups, top)
    dl = fstr.tDload()
    for g, e, f in faces:
        dl.pressure(g, [e], f, 2.0)
    dl.gravity(0, np.arange(m.conn.shape[0]), 9.8, (0.2, 0.0, -1.0))
    rho, factor = 0.4, 0.7
    cload = np.sin(np.arange(3 * m.n_node) * 0.23)

    # without a list the load is the nodal load it was handed, bit for bit
    solid.set_state({"unode": U})
    _begin(hip, solid, cload)
    assert np.array_equal(solid.get_load(), cload)

    want_u = cload + R.assemble(m.coord, groups, rho, dl.arrays(), factor=factor, disp=U)
    want_0 = cload + R.assemble(m.coord, groups, rho, dl.arrays(), factor=factor)
    assert np.abs(want_u - want_0).max() > 1e-3 * np.abs(want_u).max()
    solid.set_dload(dl, rho, follow=True)
    solid.set_dload_factor(factor)
    _begin(hip, solid, cload)
    got = solid.get_load()
    print("TYPE=%d follow: %.3e" % (etype, _rel(got, want_u)))
    assert _rel(got, want_u) <= 1e-11
    solid.set_dload(dl, rho, follow=False)
    _begin(hip, solid, cload)
    got = solid.get_load()
    print("TYPE=%d fixed: %.3e" % (etype, _rel(got, want_0)))
    assert _rel(got, want_0) <= 1e-11
    assert ctx.dload_stats()["grav_entries"] == m.conn.shape[0]

    # one Newton iteration: the follower load is rebuilt on coord + unode + dunode
    solid.set_dload(dl, rho, follow=True)
    I, Rr = default_params(method=1, precond=3, maxit=5000, tol=1e-10)
    hecMAT.Iarray[:] = I
    hecMAT.Rarray[:] = Rr
    fix = m.bottom_nodes
    bc = (np.repeat(fix, 3).astype(np.int32), np.tile(np.array([1, 2, 3], dtype=np.int32), fix.size), np.zeros(3 * fix.size))
    ok, log = fstr.fstr_Newton(solid, hecMAT, (0.0, factor), bc, cload, 1, 1.0e-12, commit_unconverged=False)
    assert not ok and log.shape[0] == 1
    st = solid.get_state(("unode", "dunode"))
    assert np.array_equal(st["unode"], U) and np.abs(st["dunode"]).max() > 1e-6
    want = factor * cload + R.assemble(m.coord, groups, rho, dl.arrays(), factor=factor, disp=st["unode"] + st["dunode"])
    got = solid.get_load()
    print("TYPE=%d after one iteration: %.3e" % (etype, _rel(got, want)))
    assert _rel(got, want) <= 1e-11

    # cleared again: the nodal load alone
    solid.set_dload(None)
    _begin(hip, solid, cload)
    assert np.array_equal(solid.get_load(), cload)
    ctx.close()


def _deck(hip, name, follow):
    from frontistr_amd import fstr
    from oracle.refrun import default_params
    etype = D.ETYPE[name]
    coord, conn = D.cantilever(etype)
    if name == "c342":
        mat = fstr.tMaterial(D.E, D.NU, plastic=True, harden=fstr.BILINEAR, plconst=(D.YIELD0, D.HARDEN, 0.0), nlgeom_flag=fstr.UPDATELAG)
    else:
        mat = fstr.tMaterial(D.E, D.NU, nlgeom_flag=fstr.TOTALLAG)
    ctx, hecMAT, solid = _solid(hip, etype, coord, conn, mat)
    I, Rr = default_params(method=1, precond=1, maxit=5000, tol=1e-10)
    hecMAT.Iarray[:] = I
    hecMAT.Rarray[:] = Rr
    dl = fstr.tDload()
    for e, f in D.top_faces(etype, coord, conn):
        dl.pressure(0, [e], f, D.PRESSURE[name])
    if name == "c342":
        dl.gravity(0, np.arange(conn.shape[0]), D.GRAV[0], D.GRAV[1:])
    solid.set_dload(dl, D.RHO if name == "c342" else None, follow=follow)
    fix = D.fix_nodes(coord)
    bc = (np.repeat(fix, 3).astype(np.int32), np.tile(np.array([1, 2, 3], dtype=np.int32), fix.size), np.zeros(3 * fix.size))
    return ctx, hecMAT, solid, bc


@pytest.mark.parametrize("follow", [True, False], ids=["follow", "fixed"])
@pytest.mark.parametrize("name", D.NAMES)
def test_against_the_unmodified_program(hip, name, follow):
    from frontistr_amd import fstr
    from hyper_ref import within_1e4
    g = np.load(D.GOLDEN)
    t = D.tag(name, follow)
    rlog, newton = json.loads(str(g[t + "/log"])), [int(x) for x in g[t + "/newton"]]
    nsub = D.SUBSTEPS
    # sub-step by sub-step: every step's summary
    ctx, hecMAT, solid, bc = _deck(hip, name, follow)
    got = []
    for sub in range(1, nsub + 1):
        ok, log = fstr.fstr_Newton(solid, hecMAT, ((sub - 1) / nsub, sub / nsub), bc, None, D.MAX_ITER, D.CONVERG)
        assert ok, (sub, log)
        got.append(log.shape[0])
        summary = solid.nodal_stress().summary(solid.get_state(("unode",))["unode"])
        bad = within_1e4(summary, rlog[len(rlog) - nsub + sub - 1])
        print(t, "sub-step", sub, "U3", summary["Node"]["U3"], "reference", rlog[len(rlog) - nsub + sub - 1]["Node"]["U3"])
        assert bad == [], (sub, bad)
    print(t, "Newton iterations per sub-step", got, "reference", newton)
    assert got == newton
    ctx.close()
    # the sub-step loop itself
    ctx, hecMAT, solid, bc = _deck(hip, name, follow)
    log = fstr.fstr_solve_NLGEOM(solid, hecMAT, bc, None, nsub, D.MAX_ITER, D.CONVERG)
    assert [int((log[:, 0] == s).sum()) for s in range(1, nsub + 1)] == newton
    summary = solid.nodal_stress().summary(solid.get_state(("unode",))["unode"])
    assert within_1e4(summary, rlog[-1]) == []
    ctx.close()
