"""GPU parity of the nonlinear element kernels at more than one workgroup: every case of tests/nl_shapes.py through
frontistr_amd/fstr.py and the C ABI against the numpy restatements (visco_ref.Model, which hands the sections that are not
viscoelastic or NORTON to hyper_ref, yield_ref and fbar_ref).

Per case: element tangents before the update and after it (the latch and the history change them), the stress update (element
forces, stress, strain, fstat, istat, plstrain, history, latch), the assembled D / AL / AU with boundary conditions before and after
the update -- twice, bit-identical, on the coloured path --, QFORCE of fx_nl_update_at, and the state fstr_UpdateState commits.
tests/test_nl_shapes.py shows on the CPU which launches each case makes (full and partly filled workgroups, coloured launches
behind the head of the list, both ways of walking a list) and that the inputs determine the restated numbers to 1e-12.

Bounds, the project's own: 1e-11 of the largest entry of the compared array; istat and latch exact; the elements of an UPDATELAG
section at the STF_C3 types (the stress increment is rounded to default real), and the sums that hold them (assembled matrix,
QFORCE), the two-tier rule of test_gpu_c3_nonlinear._close_ul -- the other sections of such a context keep 1e-11; the mesh that cannot be
coloured (PieMesh(33, 1, 2), atomics) 1e-12 of the largest diagonal entry for the assembled matrix.  One case per family runs again
in a child process with FX_ASM_ATOMIC=1 (the variable is read once per process).

Reference times (one CPU core; the numpy models are the cost, each case's reference is computed once per module and shared by the
parity test and the forced-atomic one): 343 hexahedra ELASTIC 0.7 .. 1.1 s, viscoelastic 0.7 .. 1.6 s, NORTON 2.0 s; 64 hyperelastic
hexahedra 1.3 s, the 48 hyperelastic of 343 2.8 s; F-bar total Lagrange 64 hexahedra 2.5 .. 4.8 s (125 would be 5 .. 9 s: they get two
colours of the 5^3 cube instead, 1.4 .. 2.7 s); 384 tetrahedra 0.1 .. 1.1 s; 162 ten-node tetrahedra 0.1 .. 2.9 s; 27 twenty-node
hexahedra 0.1 .. 2.5 s; the pies 0.5 .. 4.4 s.  With an MI355X and its host no test of this module takes more than 1.7 s."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import c3_ref as R
import hyper_ref as H
import nl_shapes as S
import test_gpu_c3_nonlinear as GC
import test_gpu_hyperelastic as GH
import test_gpu_visco as GV
import test_gpu_yield as GY
import visco_ref as V
import yield_ref as Y

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL = 1e-11
POINT = ("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat", "istat")


def _fmat(mat):
    if Y.kind_of(mat) in (Y.MOHR, Y.DRUCKER):
        return GY._fmat(mat)
    if H.kind_of(mat) == H.ARRUDA:
        return GH._fmat(mat)
    return GV._fmat(mat)


def _solid(hip, m, model):
    from frontistr_amd import fstr
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    fm = [_fmat(x) for x in model.mats]
    several = len(fm) > 1
    solid = fstr.fstr_solid(ctx, m.coord, m.conn, fm if several else fm[0], elem_mat=model.elem_mat.astype(np.int32) if several else None,
                            etype=model.etype, elemopt=4 if model.fbar else 2)
    assert solid.history_width() == model.width
    state = {k: model.st[k] for k in POINT}
    state.update(unode=model.unode, dunode=model.dunode)
    solid.set_state(state, latch=0)
    if model.width:
        solid.set_history(model.hist.reshape(-1, model.width))
    solid.set_time(model.time, model.tincr)
    return ctx, hecMAT, solid


def _close(a, b, tag, scale=None, tol=TOL):
    b = np.asarray(b)
    a = np.asarray(a).reshape(b.shape)
    scale = np.abs(b).max() if scale is None else scale
    if scale == 0.0:
        print("%s: the restatement holds zeros" % tag)
        assert not a.any(), "%s: not zero" % tag
        return
    err = np.abs(a - b).max() / scale
    print("%s: %.3e (bound %.1e)" % (tag, err, tol))
    assert err < tol, "%s: %.3e" % (tag, err)


def _dense(conn, ke, n_node):
    K = np.zeros((3 * n_node, 3 * n_node))
    for e, k in enumerate(ke):
        dofs = (3 * (conn[e][:, None] - 1) + np.arange(3)).ravel()
        np.add.at(K, (dofs[:, None], dofs[None, :]), k)
    return K


def _bc(m):
    bc = m.dirichlet()
    return bc[0], bc[1], 1e-3 * np.cos(np.arange(bc[0].size))


_REFERENCE = {}


def reference(cid):
    """The restatement's numbers of one case, computed once: tangents before the update, the update, tangents after it, the commit"""
    if cid in _REFERENCE:
        return _REFERENCE[cid]
    t0 = time.perf_counter()
    m, ref = S.CASES[cid].build()
    out = dict(mesh=m, model0=ref)
    import copy
    ref = copy.deepcopy(ref)
    out["ke0"] = ref.element_tangents()
    out["qf"] = ref.element_update()
    out["after"] = {k: ref.st[k].copy() for k in POINT}
    out["hist1"], out["latch"] = ref.hist.copy(), ref.latch
    out["ke1"] = ref.element_tangents()
    q = np.zeros(3 * m.n_node)
    for e, nd in enumerate(ref.conn - 1):
        np.add.at(q, (3 * nd[:, None] + np.arange(3)).ravel(), out["qf"][e])
    out["qforce"] = q
    ref.commit()
    out["committed"] = {k: ref.st[k].copy() for k in POINT}
    out["hist2"], out["unode2"] = ref.hist.copy(), ref.unode.copy()
    print("%s: %d elements, reference %.2f s" % (cid, ref.conn.shape[0], time.perf_counter() - t0))
    _REFERENCE[cid] = out
    return out


def _assembled(hip, case, ctx, hecMAT, solid, m, ke, tag, later, coloured):
    from frontistr_amd import fstr
    bc = _bc(m)
    Kd, _ = R.apply_bc(_dense(m.conn, ke, m.n_node), np.zeros(3 * m.n_node), bc)
    got = []
    for _ in range(2):
        fstr.fstr_StiffMatrix(solid, bc)
        ctx.download_matrix(hecMAT)
        got.append([np.array(getattr(hecMAT, k)) for k in ("D", "AL", "AU")])
    want = R.to_blocks(Kd, hecMAT)
    diag = np.abs(want[0]).max()
    for k, x, y, z in zip(("D", "AL", "AU"), got[0], got[1], want):
        if coloured:
            assert np.array_equal(x, y), "two assemblies of the same state differ (%s)" % k
            later(x, z, "assembled %s %s" % (k, tag), np.abs(Kd).max())
        else:       # atomics: 1e-12 of the largest diagonal entry, between two assemblies and against the restatement
            _close(x, y, "assembled %s %s, two atomic assemblies" % (k, tag), diag, tol=1e-12)
            _close(x, z, "assembled %s %s (atomic)" % (k, tag), diag, tol=1e-12)


def _by_section(case, mats, elem_mat, n_elem):
    """The comparison of an array whose first axis is the element (or, flat, its points in element order) after the update: 1e-11,
    but for the elements of an UPDATELAG section at an STF_C3 type, whose stress increment UPDATE_C3 rounds to default real -- they
    alone are held to the two-tier rule of test_gpu_c3_nonlinear._close_ul, on the scale of the whole array"""
    if not case.single_precision():
        return _close
    flags = np.array([x.nlgeom for x in mats])
    ul = (flags[0] if elem_mat is None else flags[np.asarray(elem_mat) - 1]) == S.UPDATELAG
    ul = np.broadcast_to(ul, (n_elem,))

    def close(a, b, tag):
        b = np.asarray(b)
        b = b.reshape(n_elem, -1)
        a = np.asarray(a).reshape(b.shape)
        scale = np.abs(b).max()
        if (~ul).any():
            _close(a[~ul], b[~ul], tag + ", the sections that are not UPDATELAG", scale)
        GC._close_ul(a[ul], b[ul], tag + ", the UPDATELAG sections", scale)
    return close


def _check(hip, cid):
    from frontistr_amd import fstr
    case = S.CASES[cid]
    want = reference(cid)
    m, ref = want["mesh"], want["model0"]
    W = ref.width
    launches, lists = S.case_launches(case)
    coloured = not lists["atomic"]
    # UPDATELAG at an STF_C3 type: what depends on the updated stress is compared by the two-tier single-precision rule
    later = GC._close_ul if case.single_precision() else _close        # the assembled matrix and QFORCE: sums over all sections
    sec = _by_section(case, ref.mats, ref.elem_mat if len(ref.mats) > 1 else None, ref.conn.shape[0])
    ctx, hecMAT, solid = _solid(hip, m, ref)
    _close(solid.element_tangents(), want["ke0"], "tangent before the update")
    if case.scatter:
        _assembled(hip, case, ctx, hecMAT, solid, m, want["ke0"], "before the update", _close, coloured)
    qf = solid.element_update()
    s = solid.get_state()
    a = want["after"]
    assert s["latch"] == want["latch"]
    assert np.array_equal(np.asarray(s["istat"]).reshape(a["istat"].shape), a["istat"])
    assert np.abs(a["strain"]).max() > {"creep": 1e-3, "yield": 5e-3}.get(case.helper, 0.02)
    _close(s["strain"], a["strain"], "stored strain")
    sec(s["stress"], a["stress"], "stress")
    sec(qf, want["qf"], "element internal force")
    for k in ("plstrain", "fstat"):
        if a[k].any():
            sec(s[k], a[k], k)
        else:
            assert not np.asarray(s[k]).any(), k
    for k in ("stress_bak", "strain_bak"):
        assert np.array_equal(np.asarray(s[k]).reshape(a[k].shape), a[k]), k
    if W:
        sec(solid.get_history(), want["hist1"], "history after the update")
    sec(solid.element_tangents(), want["ke1"], "tangent after the update")
    if case.scatter:
        _assembled(hip, case, ctx, hecMAT, solid, m, want["ke1"], "after the update", later, coloured)
    q = np.zeros(3 * m.n_node)
    hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(ref.dunode.copy()), hip._ptr(q), None))
    later(q, want["qforce"], "QFORCE")
    fstr.fstr_UpdateState(solid)
    s = solid.get_state()
    c = want["committed"]
    assert np.array_equal(s["strain_bak"], s["strain"]) and np.array_equal(s["stress_bak"], s["stress"])
    _close(s["unode"], want["unode2"], "unode after the commit")
    for k in ("stress_bak", "plstrain", "fstat"):
        if c[k].any():
            sec(s[k], c[k], "%s after the commit" % k)
        else:
            assert not np.asarray(s[k]).any(), k
    assert np.array_equal(np.asarray(s["istat"]).reshape(c["istat"].shape), c["istat"])
    if W:
        sec(solid.get_history(), want["hist2"], "history after the commit")
    ctx.close()


@pytest.mark.parametrize("cid", [c for c in S.CASES if not S.CASES[c].th])
def test_kernels_match_the_restatement(hip, oracle, cid):
    _check(hip, cid)


# ---- thermal strain on: the TH = 1 kernels --------------------------------------------------------------------------------------------
def _check_thermal(hip, cid):
    """nl_thermal_ref.Model against the context with fx_nl_set_thermal: tangents (the elastic table at the points' temperatures),
    the assembled matrix on the coloured path, the update, QFORCE, the commit of last_temp"""
    import nl_thermal_ref as NT
    import test_gpu_nl_thermal as GT
    from frontistr_amd import fstr
    case = S.CASES[cid]
    d = case.build()
    m = d["mesh"]
    t0 = time.perf_counter()
    ref = NT.model_of(d)
    ke0 = ref.element_tangents()[0]
    rqf = ref.element_update()[0]
    ke1 = ref.element_tangents()[0]
    rq = np.zeros(3 * m.n_node)
    for e, nd in enumerate(m.conn - 1):
        np.add.at(rq, (3 * nd[:, None] + np.arange(3)).ravel(), rqf[e])
    print("%s: %d elements, reference %.2f s" % (cid, m.conn.shape[0], time.perf_counter() - t0))
    st = ref.parts[0]["st"]
    plastic = any(NT.is_elastoplastic(x) for x in d["mats"])
    assert ref.latch == (1 if plastic else 0) and st["istat"].any() == plastic
    later = (lambda a, b, tag, sc=None: GT._close_ul(a, b, tag, np.abs(b).max() if sc is None else sc)) if case.single_precision() else _close
    sec = _by_section(case, d["mats"], d["elem_mats"][0], m.conn.shape[0])
    ctx, hecMAT, solid = GT._solid(hip, d)
    launches, lists = S.case_launches(case)
    assert not lists["atomic"]
    _close(solid.element_tangents(), ke0, "tangent before the update")
    _assembled(hip, case, ctx, hecMAT, solid, m, ke0, "before the update", _close, True)
    qf = solid.element_update()
    s = solid.get_state()
    assert s["latch"] == ref.latch and np.array_equal(np.asarray(s["istat"]).reshape(st["istat"].shape), st["istat"])
    _close(s["strain"], st["strain"], "stored strain")
    sec(s["stress"], st["stress"], "stress")
    sec(qf, rqf, "element internal force")
    if plastic:
        sec(s["fstat"], st["fstat"], "fstatus(1)")
    sec(solid.element_tangents(), ke1, "tangent after the update")
    _assembled(hip, case, ctx, hecMAT, solid, m, ke1, "after the update", later, True)
    # QFORCE from the zero history again, as test_gpu_nl_thermal does
    solid.set_state({k: np.zeros_like(v) for k, v in s.items() if k in ("stress", "strain", "fstat", "istat")}, latch=0)
    q = np.zeros(3 * m.n_node)
    hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(d["dunode"].copy()), hip._ptr(q), None))
    later(q, rq, "QFORCE")
    fstr.fstr_UpdateState(solid)
    s = solid.get_state(("stress", "strain", "stress_bak", "strain_bak", "last_temp"))
    assert np.array_equal(s["strain_bak"], s["strain"]) and np.array_equal(s["stress_bak"], s["stress"])
    assert np.array_equal(s["last_temp"], d["temperature"])
    ctx.close()


@pytest.mark.parametrize("cid", [c for c in S.CASES if S.CASES[c].th])
def test_thermal_kernels_match_the_restatement(hip, oracle, cid):
    _check_thermal(hip, cid)


# ---- FX_ASM_ATOMIC=1: one case per family in a child process -----------------------------------------------------------------------------
ATOMIC = [c for c in S.CASES if S.CASES[c].atomic_child]


def compute_paths(cid, path):
    """What one process computes for the comparison of the scatter paths: tangents and update through the lists of this process (one
    range per group and no list of collapsed elements under FX_ASM_ATOMIC=1), the assembled matrix after the update"""
    from frontistr_amd import fstr, hecmw as hip
    m, ref = S.CASES[cid].build()
    ctx, hecMAT, solid = _solid(hip, m, ref)
    out = dict(ke0=solid.element_tangents(), qf=solid.element_update())
    out["stress"] = solid.get_state(("stress",))["stress"]
    out["ke1"] = solid.element_tangents()
    fstr.fstr_StiffMatrix(solid, _bc(m))
    ctx.download_matrix(hecMAT)
    for k in ("D", "AL", "AU"):
        out[k] = np.array(getattr(hecMAT, k))
    ctx.close()
    np.savez(path, **out)


@pytest.mark.parametrize("cid", ATOMIC)
def test_forced_atomic_scatter(hip, oracle, cid, tmp_path):
    want = reference(cid)
    res = {}
    for name, env in (("default", {}), ("atomic", {"FX_ASM_ATOMIC": "1"})):     # one after the other, each under its own time limit
        out = str(tmp_path / (name + ".npz"))
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_nl_shapes as T; T.compute_paths(%r, %r)" % (HERE, ROOT, cid, out)
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=300)
        assert p.returncode == 0, "scatter path %s: child exited with %d\n%s" % (name, p.returncode, p.stdout[-3000:])
        res[name] = dict(np.load(out))
    got = res["atomic"]
    later = GC._close_ul if S.CASES[cid].single_precision() else _close
    _close(got["ke0"], want["ke0"], "atomic lists: tangent before the update")
    later(got["qf"], want["qf"], "atomic lists: element internal force")
    later(got["stress"].reshape(want["after"]["stress"].shape), want["after"]["stress"], "atomic lists: stress")
    later(got["ke1"], want["ke1"], "atomic lists: tangent after the update")
    diag = np.abs(res["default"]["D"]).max()
    for k in ("D", "AL", "AU"):
        _close(got[k], res["default"][k], "atomic scatter %s against the coloured one" % k, diag, tol=1e-12)
