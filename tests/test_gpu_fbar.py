"""GPU parity of the F-bar hexahedron (TYPE=361, elemopt 4: csrc/fx_nonlinear_fbar.h) in the nonlinear static loop through
frontistr_amd/fstr.py against the numpy restatement tests/fbar_ref.py, one case per instantiated group of the element kernels:

    group 0   ELASTIC INFINITE, Mises INFINITE          group 4   Mohr-Coulomb INFINITE, Drucker-Prager INFINITE
    group 1   ELASTIC TOTALLAG, Mises TOTALLAG          group 5   Mohr-Coulomb TOTALLAG, Drucker-Prager TOTALLAG
    group 3   Neo-Hooke, Mooney-Rivlin, Arruda-Boyce

For each: element tangents before any update and after one (elastoplastic cases: with the latch the update has set, and the
elastoplastic tangent with the latch cleared by hand), stored strain / stress / plstrain / istat / fstat, element internal forces, the
assembled D / AL / AU (coloured: two assemblies bitwise equal; FX_ASM_ATOMIC=1 in a child process), QFORCE of fx_nl_update_at.  Then a
two-section context, a context of an F-bar group beside a B-bar group and a 342 group, the sub-step loops of the recorded cube decks,
snapshot / commit, the refusals, the device error word.

Mesh: hyper_ref.gpu_mesh(361), the skewed 2^3 cube plus one collapsed hexahedron (9 elements: two workgroups of the tangent kernel,
the second one partly idle; the `dup` path).  Tolerance: the project's nonlinear 1e-11 of the largest entry of the compared array;
tests/test_fbar_ref.py shows that these inputs determine the restated numbers to 1e-12 on that scale and keep every plastic point off
the edges of its return mapping; istat is compared exactly.  The reference of a case is computed once (_reference) and shared."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import c3_ref as R
import fbar_ref as F
import hyper_ref as H
import mixed_nl_ref as M
import yield_ref as Y

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX_ERROR_RUNTIME, FX_ERROR_UNSUPPORTED = -1, -2
TOL = 1e-11
FBAR = F.ELEMOPT_FBAR

# name -> inputs (mesh, material, unode, dunode)
CASES = {"elastic_infinite": lambda: F.elastic_case("elastic", F.INFINITE), "mises_infinite": lambda: F.plastic_case("mises", F.INFINITE),
         "elastic_totallag": lambda: F.elastic_case("elastic", F.TOTALLAG), "mises_totallag": lambda: F.plastic_case("mises", F.TOTALLAG),
         "neohooke": lambda: F.elastic_case("neohooke"), "mooney": lambda: F.elastic_case("mooney"), "arruda": lambda: F.elastic_case("arruda"),
         "mohr_infinite": lambda: F.plastic_case("mohr", F.INFINITE), "drucker_infinite": lambda: F.plastic_case("drucker", F.INFINITE),
         "mohr_totallag": lambda: F.plastic_case("mohr", F.TOTALLAG), "drucker_totallag": lambda: F.plastic_case("drucker", F.TOTALLAG)}


def _two_sections():
    """Mooney-Rivlin beside ELASTIC TOTALLAG, the elements dealt out irregularly: groups 3 and 1 in one assembly"""
    from oracle.refrun import Material
    m, mat, unode, dunode = F.elastic_case("mooney")
    em = (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32)
    return m, [mat, Material(2.5, 0.3, nlgeom=F.TOTALLAG)], unode, dunode, em


def _inputs(name):
    if name == "two_sections":
        return _two_sections()
    return CASES[name]() + (None,)


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
    return fstr.tMaterial(mat.E, mat.nu, plastic=mat.plastic, harden=mat.harden, plconst=mat.plconst, nlgeom_flag=mat.nlgeom)


def _solid(hip, m, mat, elem_mat=None, elemopt=FBAR, ctx=None):
    from frontistr_amd import fstr
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    if ctx is None:
        ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    fm = [_fmat(x) for x in mat] if isinstance(mat, (list, tuple)) else _fmat(mat)
    return ctx, hecMAT, fstr.fstr_solid(ctx, m.coord, m.conn, fm, elem_mat=elem_mat, etype=361, elemopt=elemopt)


def _close(a, b, tag, scale=None, tol=TOL):
    scale = max(np.abs(b).max(), 1e-300) if scale is None else scale
    err = np.abs(np.asarray(a).reshape(np.shape(b)) - b).max() / scale
    print("%s: %.3e (bound %.1e)" % (tag, err, tol))
    assert err < tol, "%s: %.3e" % (tag, err)


def _bc(m):
    bc = m.dirichlet()
    return (bc[0], bc[1], 1e-3 * np.cos(np.arange(bc[0].size)))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """What fbar_ref gives for a case, step by step as _check_parity walks the device through it"""
    m, mat, unode, dunode, em = _inputs(name)
    ref = F.Model(m.coord, m.conn, mat, em)
    ref.unode[:], ref.dunode[:] = unode, dunode
    plastic = any(x.plastic for x in ref.mats)
    bc = _bc(m)
    dense = lambda: R.apply_bc(ref.stiffness(), np.zeros(3 * m.n_node), bc)[0]
    out = dict(plastic=plastic, k0=ref.element_tangents(), K0=dense())
    out["qf"] = ref.element_update()
    out["state"] = {k: v.copy() for k, v in ref.st.items()}
    out["k1"], out["K1"] = ref.element_tangents(), dense()            # with the latch, if the update set it
    if plastic:
        ref.latch = 0
        out["k_ep"], out["K_ep"] = ref.element_tangents(), dense()
        ref.latch = 1
    out["Q"] = ref.update().copy()
    return out


def _assembled(hip, ctx, hecMAT, solid, bc, twice=True):
    from frontistr_amd import fstr
    got = []
    for _ in range(2 if twice else 1):
        fstr.fstr_StiffMatrix(solid, bc)
        ctx.download_matrix(hecMAT)
        got.append([np.array(getattr(hecMAT, k)) for k in ("D", "AL", "AU")])
    if twice:
        for x, y in zip(*got):
            assert np.array_equal(x, y), "two assemblies of the same state differ"
    return got[0]


def _check_parity(hip, name):
    m, mat, unode, dunode, em = _inputs(name)
    assert any(len(set(c)) < 8 for c in m.conn.tolist()), "no collapsed hexahedron in the mesh"
    ref = _reference(name)
    ctx, hecMAT, solid = _solid(hip, m, mat, em)
    solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
    bc = _bc(m)

    def assembled(key, tag):
        for k, x, y in zip(("D", "AL", "AU"), _assembled(hip, ctx, hecMAT, solid, bc), R.to_blocks(ref[key], hecMAT)):
            _close(x, y, "assembled %s %s" % (k, tag), np.abs(ref[key]).max())

    _close(solid.element_tangents(), ref["k0"], "tangent before any update")
    assembled("K0", "before any update")
    qf = solid.element_update()
    s, rs = solid.get_state(), ref["state"]
    assert s["latch"] == int(ref["plastic"])
    assert np.array_equal(s["istat"], rs["istat"]), "istat"
    if ref["plastic"]:
        share = rs["istat"].mean()
        print("%.0f %% of the points plastic" % (100 * share))
        assert share >= 0.25
        _close(s["fstat"], rs["fstat"], "fstat")
    else:
        assert not s["fstat"].any()
    _close(s["strain"], rs["strain"], "stored strain")
    _close(s["stress"], rs["stress"], "stress")
    _close(qf, ref["qf"], "element internal force")
    for k in ("plstrain", "stress_bak", "strain_bak"):
        assert not s[k].any(), k
    _close(solid.element_tangents(), ref["k1"], "tangent after the update")
    assembled("K1", "after the update")
    if ref["plastic"]:
        assert np.abs(ref["k_ep"] - ref["k1"]).max() > 1e-3 * np.abs(ref["k1"]).max(), "the plastic state does not change the reference tangent"
        solid.set_state({}, latch=0)
        _close(solid.element_tangents(), ref["k_ep"], "elastoplastic tangent (latch cleared)")
        assembled("K_ep", "elastoplastic")
        solid.set_state({}, latch=1)
    q = np.zeros(3 * m.n_node)
    hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(dunode), hip._ptr(q), None))
    _close(q, ref["Q"], "QFORCE")
    ctx.close()


@pytest.mark.parametrize("name", list(CASES))
def test_elements_state_matrix_and_qforce(hip, name):
    _check_parity(hip, name)


def test_two_section_context(hip):
    _check_parity(hip, "two_sections")


# ---- FX_ASM_ATOMIC=1 is read once per process -> one child process for all cases
def compute_atomic(path):
    from frontistr_amd import fstr, hecmw as hip
    out = {}
    for name in list(CASES) + ["two_sections"]:
        m, mat, unode, dunode, em = _inputs(name)
        ctx, hecMAT, solid = _solid(hip, m, mat, em)
        solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
        for tag in ("K0", "K1"):
            for k, x in zip(("D", "AL", "AU"), _assembled(hip, ctx, hecMAT, solid, _bc(m), twice=False)):
                out["%s/%s/%s" % (name, tag, k)] = x
            solid.element_update()
        ctx.close()
    np.savez(path, **out)


def test_atomic_scatter_matches_the_reference(hip, tmp_path):
    out = str(tmp_path / "atomic.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_fbar as T; T.compute_atomic(%r)" % (HERE, ROOT, out)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FX_ASM_ATOMIC="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, "child exited with %d\n%s" % (p.returncode, p.stdout[-3000:])
    got = dict(np.load(out))
    for name in list(CASES) + ["two_sections"]:
        m, mat, _, _, em = _inputs(name)
        hm = hip.hecmwST_local_mesh(n_node=m.n_node)
        hm.nn_elem = m.conn.shape[1]
        hm.elem_node_item = m.conn.ravel()
        hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
        ref = _reference(name)
        for tag in ("K0", "K1"):
            for k, y in zip(("D", "AL", "AU"), R.to_blocks(ref[tag], hecMAT)):
                _close(got["%s/%s/%s" % (name, tag, k)], y, "atomic %s %s %s" % (name, tag, k), np.abs(ref[tag]).max())


# ---- an F-bar group beside a B-bar group and a 342 group
def _group_case():
    """MixedMesh(3, order 2), skewed and curved: the corner nodes of its three 20-node hexahedra as 361 elements -- two F-bar, one
    B-bar -- and its 72 ten-node tetrahedra, all over the one node set (the 361 elements do not conform with their neighbours'
    mid-edge nodes; the algebra does not care).  Neo-Hooke beside ELASTIC TOTALLAG, dealt out irregularly."""
    from oracle.refrun import Material
    mesh = M._mesh("n3", 2)
    em = (1 + (np.arange(mesh.n_elem) * 7 // 3) % 2).astype(np.int32)
    g = mesh.groups_with(2, em)
    assert g[0][0] == 362 and g[2][0] == 342
    hexes = np.ascontiguousarray(g[0][1][:, :8])
    groups = [(361, np.ascontiguousarray(hexes[:2]), FBAR, np.ascontiguousarray(g[0][3][:2])),
              (361, np.ascontiguousarray(hexes[2:]), F.ELEMOPT_BBAR, np.ascontiguousarray(g[0][3][2:])),
              (342, g[2][1], 2, g[2][3])]
    mats = [H.neohooke(0.1486, 0.0789), Material(1.0, 0.3, nlgeom=F.TOTALLAG)]
    unode, dunode = H.random_displacement(mesh.coord, 17, H.GPU_AMP)
    return mesh, groups, mats, unode, dunode


def test_group_context_with_bbar_and_tetrahedra(hip, oracle):
    from frontistr_amd import fstr
    mesh, groups, mats, unode, dunode = _group_case()
    ref = F.MixedModel(mesh.coord, groups, mats)
    ref.unode[:], ref.dunode[:] = unode, dunode
    hm = hip.hecmwST_local_mesh(n_node=mesh.n_node)
    hecMAT = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)
    ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    solid = fstr.fstr_solid(ctx, mesh.coord, None, [_fmat(x) for x in mats], groups=groups)
    solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
    bc = _bc(mesh)

    def tangents_and_matrix(tag):
        for g, (a, b) in enumerate(zip(solid.group_slices("tangents", solid.element_tangents()), ref.element_tangents())):
            _close(a, b, "group %d tangents %s" % (g + 1, tag))
        Kd = R.apply_bc(ref.stiffness(), np.zeros(3 * mesh.n_node), bc)[0]
        for k, x, y in zip(("D", "AL", "AU"), _assembled(hip, ctx, hecMAT, solid, bc), R.to_blocks(Kd, hecMAT)):
            _close(x, y, "assembled %s %s" % (k, tag), np.abs(Kd).max())

    tangents_and_matrix("before any update")
    qf, rqf = solid.element_update(), ref.element_update()
    for g, (a, b) in enumerate(zip(solid.group_slices("forces", qf), rqf)):
        _close(a, b, "group %d element internal force" % (g + 1))
    s = solid.get_state()
    assert solid.n_point == 8 * 3 + 4 * groups[2][1].shape[0]
    for k in ("strain", "stress"):          # the flat per-point layout: the groups one after the other
        _close(s[k], ref.flat(k), "flat " + k)
        for g, (a, p) in enumerate(zip(solid.group_slices(k, s[k]), ref.parts)):
            _close(a, p["st"][k], "group %d %s" % (g + 1, k))
    # the two 361 formulations differ on these inputs: a context that ran one family for both would not pass
    bb = F.MixedModel(mesh.coord, [(et, c, 2, e) for et, c, _, e in groups], mats)
    bb.unode[:], bb.dunode[:] = unode, dunode
    bb.element_update()
    assert np.abs(bb.parts[0]["st"]["stress"] - ref.parts[0]["st"]["stress"]).max() > 1e-6 * np.abs(ref.parts[0]["st"]["stress"]).max()
    tangents_and_matrix("after the update")
    q = np.zeros(3 * mesh.n_node)
    hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(dunode), hip._ptr(q), None))
    _close(q, ref.update(), "QFORCE")
    ctx.close()


@pytest.mark.parametrize("name", list(F.GOLDEN_DECKS))
def test_substeps_match_the_recorded_decks(hip, name):
    """fx_newton_substep (CG + SSOR to 1e-8, as the decks' !SOLVER card) on the recorded cube decks (tests/golden/nl_fbar_decks.npz, the
    unmodified reference program's runs with FORM361=FBAR): the Newton count of every sub-step is the reference's, the Global
    summaries of every step match at the reference harness's 1e-4."""
    from frontistr_amd import fstr
    from oracle import fistr1_run as f1
    from oracle.refrun import default_params
    g = np.load(os.path.join(HERE, "golden", "nl_fbar_decks.npz"))
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    m, mats, em, bc = F.golden_deck(name)
    nsub = F.DECK_SUBSTEPS
    ctx, hecMAT, solid = _solid(hip, m, mats, em)
    I, Rr = default_params(method=1, precond=1, maxit=5000, tol=1e-8)
    hecMAT.Iarray[:] = I
    hecMAT.Rarray[:] = Rr
    got = []
    for sub in range(1, nsub + 1):
        ok, log = fstr.fstr_Newton(solid, hecMAT, ((sub - 1) / nsub, sub / nsub), bc, None, 50, F.DECK_CONVERG)
        assert ok
        got.append(log.shape[0])
        st = solid.get_state(("unode", "strain", "stress"))
        summary = F.summary(361, m.conn, st["unode"], st["strain"], st["stress"])
        assert f1.compare_step(summary, rlog[len(rlog) - nsub + sub - 1]) == [], sub
    print(name, "Newton iterations per sub-step", got, "reference", newton)
    assert got == newton
    s = solid.get_state()
    assert np.array_equal(s["strain_bak"], s["strain"]) and np.array_equal(s["stress_bak"], s["stress"])
    ctx.close()


def test_snapshot_and_commit(hip):
    from frontistr_amd import fstr
    m, mat, unode, dunode = F.plastic_case("mises", F.TOTALLAG)
    ctx, hecMAT, solid = _solid(hip, m, mat)
    solid.set_state(dict(unode=unode, dunode=np.zeros_like(dunode)), latch=0)
    solid.element_update()
    fstr.fstr_UpdateState(solid)            # fx_nl_commit: stress -> stress_bak, fstat -> plstrain
    keys = ("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat", "istat")
    before = solid.get_state()
    assert before["stress"].any() and np.array_equal(before["stress_bak"], before["stress"])
    assert np.array_equal(before["strain_bak"], before["strain"]) and np.array_equal(before["plstrain"], before["fstat"])
    fstr.fstr_cutback_save(solid)
    solid.set_state(dict(dunode=dunode))
    solid.element_update()
    fstr.fstr_UpdateState(solid)
    assert not np.array_equal(solid.get_state()["strain"], before["strain"])
    fstr.fstr_cutback_load(solid)
    after = solid.get_state()
    for k in keys:
        assert np.array_equal(after[k], before[k]), k
    ctx.close()


def test_refusals_leave_the_context_usable(hip):
    from frontistr_amd import fstr
    from oracle.refrun import Material
    m, mat, unode, dunode = F.elastic_case("elastic", F.TOTALLAG)
    ctx, hecMAT, solid = _solid(hip, m, mat)
    solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
    want = solid.element_tangents().copy()
    ul = [fstr.tMaterial(2.5, 0.3, nlgeom_flag=fstr.TOTALLAG), fstr.tMaterial(2.5, 0.3, nlgeom_flag=fstr.UPDATELAG)]
    em = (1 + (np.arange(m.n_elem) == 4)).astype(np.int32)          # the fifth element alone is updated Lagrange
    with pytest.raises(hip.HecmwSolverError) as e:
        fstr.fstr_solid(ctx, m.coord, m.conn, ul, elem_mat=em, etype=361, elemopt=FBAR)
    assert e.value.code == FX_ERROR_UNSUPPORTED and "group 1" in str(e.value) and "UPDATELAG" in str(e.value) and "element 5" in str(e.value), str(e.value)
    with pytest.raises(hip.HecmwSolverError) as e:
        fstr.fstr_solid(ctx, m.coord, m.conn, ul[0], etype=361, elemopt=5)
    assert e.value.code == FX_ERROR_UNSUPPORTED and "elemopt 5" in str(e.value) and "4 (F-bar)" in str(e.value), str(e.value)
    for opt in (1, 3):          # IC and FI keep their refusal; the message now names 4 as served
        with pytest.raises(hip.HecmwSolverError) as e:
            fstr.fstr_solid(ctx, m.coord, m.conn, ul[0], etype=361, elemopt=opt)
        assert e.value.code == FX_ERROR_UNSUPPORTED and "group 1" in str(e.value), str(e.value)
    # the previous context is untouched
    assert np.array_equal(solid.element_tangents(), want)
    _close(want, _reference("elastic_totallag")["k0"], "F-bar tangent after the refusals")
    ctx.close()
    # elemopt 4 on a 342 group is ignored, as fx_elem_group documents
    t = H.gpu_mesh(342)
    el = Material(2.5, 0.3, nlgeom=F.TOTALLAG)
    u, du = H.random_displacement(t.coord, 17, H.GPU_AMP)
    res = []
    for opt in (2, FBAR):
        hm = hip.hecmwST_local_mesh(n_node=t.n_node)
        hm.nn_elem = t.conn.shape[1]
        hm.elem_node_item = t.conn.ravel()
        hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
        ctx = hip.SolverContext()
        ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
        s = fstr.fstr_solid(ctx, t.coord, None, [_fmat(el)], groups=[(342, t.conn, opt, None)])
        s.set_state(dict(unode=u, dunode=du), latch=0)
        res.append(np.asarray(s.element_tangents()).copy())
        ctx.close()
    assert np.array_equal(res[0], res[1])


def test_too_small_volume_comes_back_as_an_error(hip):
    """One well-shaped cube of edge 1e-5: V0 = 1e-15 <= 1e-12, the reference's `stop 'too small element volume'` -- an ordinary return
    path of the kernel (it sets the error word and completes), FX_ERROR_RUNTIME with that text; a sound context afterwards works."""
    from types import SimpleNamespace
    from oracle.refrun import Material
    mat = Material(2.5, 0.3, nlgeom=F.TOTALLAG)
    m = SimpleNamespace(coord=Y.ONE_ELEM_COORD * 1.0e-5, conn=Y.ONE_ELEM_CONN, n_node=8, n_elem=1)
    ctx, hecMAT, solid = _solid(hip, m, mat)
    z = np.zeros(24)
    code = hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(z), hip._ptr(z), None)
    msg = hip.lib().fx_last_error().decode()
    assert code == FX_ERROR_RUNTIME and "too small element volume" in msg, (code, msg)
    q = np.zeros(24)
    code = hip.lib().fx_nl_update_at(ctx.h, hip._ptr(z), hip._ptr(q), None)
    assert code == FX_ERROR_RUNTIME and "too small element volume" in hip.lib().fx_last_error().decode()
    ctx.close()
    m = SimpleNamespace(coord=Y.ONE_ELEM_COORD, conn=Y.ONE_ELEM_CONN, n_node=8, n_elem=1)
    ctx, hecMAT, solid = _solid(hip, m, mat)
    assert hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(z), hip._ptr(z), None) == 0
    ref = F.Model(m.coord, m.conn, mat)
    _close(solid.element_tangents(), ref.element_tangents(), "unit cube tangent after the error")
    ctx.close()
