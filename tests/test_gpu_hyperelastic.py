"""GPU parity of the hyperelastic materials (Neo-Hooke, Mooney-Rivlin, Arruda-Boyce; compile-time group 3 of the nonlinear element
kernels, csrc/fx_hyperelastic.h) through frontistr_amd/fstr.py against the numpy restatement tests/hyper_ref.py, for the six solid
types: element tangents before any update (stored strain zero) and after one, stored strain, stress, element internal forces, the
assembled D / AL / AU and QFORCE; two-section contexts (hyperelastic beside ELASTIC INFINITE and beside ELASTIC TOTALLAG: groups
0 / 1 and 3 in one assembly); the scatter fallbacks; the sub-step loops of the recorded cube decks; snapshot; the refusals; the latch.

Meshes: hyper_ref.gpu_mesh -- the distorted small meshes of the tet / wedge / hexahedron tests, at 361 with a collapsed hexahedron so
that the `dup` path of group 3 runs.  Tolerance: the project's nonlinear 1e-11 of the largest entry of the compared array;
tests/test_hyper_ref.py (test_gpu_inputs_are_well_conditioned) shows that these inputs and constants determine the restated numbers
to 1e-12 on that scale."""
import os
import subprocess
import sys

import numpy as np
import pytest

import c3_ref as R
import hyper_ref as H

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX_ERROR_UNSUPPORTED = -2
ETYPES = [361, 341, 342, 351, 352, 362]
NAMES = ["mooney", "neohooke", "arruda"]
TOL = 1e-11


def _fmat(mat):
    from frontistr_amd import fstr
    if H.kind_of(mat) == H.ARRUDA:
        return fstr.tMaterial.arruda_boyce(*mat.plconst)
    if H.kind_of(mat) == H.MOONEY:
        c10, c01, d1 = mat.plconst
        return fstr.tMaterial.neohooke(c10, d1) if c01 == 0.0 else fstr.tMaterial.mooney_rivlin(c10, c01, d1)
    return fstr.tMaterial(mat.E, mat.nu, nlgeom_flag=mat.nlgeom)


def _solid(hip, etype, m, mat, elem_mat=None, ctx=None):
    from frontistr_amd import fstr
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    if ctx is None:
        ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    fm = [_fmat(x) for x in mat] if isinstance(mat, (list, tuple)) else _fmat(mat)
    return ctx, hecMAT, fstr.fstr_solid(ctx, m.coord, m.conn, fm, elem_mat=elem_mat, etype=etype)


def _close(a, b, tag, scale=None, tol=TOL):
    scale = max(np.abs(b).max(), 1e-300) if scale is None else scale
    err = np.abs(a - b).max() / scale
    print("%s: %.3e (bound %.1e)" % (tag, err, tol))
    assert err < tol, "%s: %.3e" % (tag, err)


def _two_sections(etype, name, flag):
    """hyperelastic beside an ELASTIC section of the given NLGEOM flag, elements dealt out irregularly"""
    from oracle.refrun import Material
    m = H.gpu_mesh(etype)
    mats = [H.TEST_MATERIALS[name](), Material(2.5, 0.3, nlgeom=flag)]
    em = (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32)
    return m, mats, em


def _check_parity(hip, etype, m, mat, em):
    from frontistr_amd import fstr
    unode, dunode = H.random_displacement(m.coord, 17, H.GPU_AMP)
    ref = H.Model(etype, m.coord, m.conn, mat, em)
    ref.unode[:], ref.dunode[:] = unode, dunode
    ctx, hecMAT, solid = _solid(hip, etype, m, mat, em)
    solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
    bc = m.dirichlet()
    bc = (bc[0], bc[1], 1e-3 * np.cos(np.arange(bc[0].size)))

    def assembled(tag):
        Kd, _ = R.apply_bc(ref.stiffness(), np.zeros(3 * m.n_node), bc)
        got = []
        for _ in range(2):
            fstr.fstr_StiffMatrix(solid, bc)
            ctx.download_matrix(hecMAT)
            got.append([np.array(getattr(hecMAT, k)) for k in ("D", "AL", "AU")])
        for x, y in zip(*got):
            assert np.array_equal(x, y), "two assemblies of the same state differ"
        for k, x, y in zip(("D", "AL", "AU"), got[0], R.to_blocks(Kd, hecMAT)):
            _close(x, y, "assembled %s %s" % (k, tag), np.abs(Kd).max())

    _close(solid.element_tangents(), ref.element_tangents(), "tangent before any update (stored strain zero)")
    assembled("before any update")
    qf, rqf = solid.element_update(), ref.element_update()
    s = solid.get_state()
    assert s["latch"] == 0
    assert np.abs(ref.st["strain"]).max() > 0.02
    _close(s["strain"], ref.st["strain"], "stored strain")
    _close(s["stress"], ref.st["stress"], "stress")
    _close(qf, rqf, "element internal force")
    for k in ("plstrain", "fstat", "stress_bak", "strain_bak"):
        assert not s[k].any(), k
    assert not s["istat"].any()
    _close(solid.element_tangents(), ref.element_tangents(), "tangent after the update")
    assembled("after the update")
    q = np.zeros(3 * m.n_node)
    hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(dunode), hip._ptr(q), None))
    _close(q, ref.update(), "QFORCE")
    assert solid.get_state(("stress",))["latch"] == 0
    ctx.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("etype", ETYPES)
def test_elements_state_matrix_and_qforce(hip, etype, name):
    m = H.gpu_mesh(etype)
    if etype == 361:
        assert any(len(set(c)) < 8 for c in m.conn.tolist()), "no collapsed hexahedron in the 361 mesh"
    _check_parity(hip, etype, m, H.TEST_MATERIALS[name](), None)


@pytest.mark.parametrize("flag", [H.INFINITE, H.TOTALLAG], ids=["beside_infinite", "beside_totallag"])
@pytest.mark.parametrize("etype,name", [(361, "mooney"), (342, "arruda"), (352, "neohooke")])
def test_hyperelastic_section_beside_an_elastic_one(hip, etype, name, flag):
    m, mats, em = _two_sections(etype, name, flag)
    _check_parity(hip, etype, m, mats, em)


@pytest.mark.parametrize("name", list(H.GOLDEN_DECKS))
def test_substeps_match_the_recorded_decks(hip, name):
    """fx_newton_substep (CG + SSOR to 1e-8, as the decks' !SOLVER card) on the recorded cube decks (tests/golden/hyper_decks.npz, the
    unmodified reference program's runs): the Newton count of every sub-step is the reference's, the Global summaries of every step
    match at the reference harness's 1e-4; against the restatement's dense-solve loop the converged displacement agrees to 1e-6
    relative (the Krylov tolerance); no latch."""
    import json
    from frontistr_amd import fstr
    from oracle import fistr1_run as f1
    from oracle.refrun import default_params
    g = np.load(os.path.join(HERE, "golden", "hyper_decks.npz"))
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    m, mats, em, bc = H.golden_deck(name)
    nsub = H.DECK_SUBSTEPS
    ref = H.Model(m.etype, m.coord, m.conn, mats, em)
    for sub in range(1, nsub + 1):
        ok, it = ref.newton_substep((sub - 1) / nsub, sub / nsub, bc, None, 50, H.DECK_CONVERG)
        assert ok
    ctx, hecMAT, solid = _solid(hip, m.etype, m, mats, em)
    I, Rr = default_params(method=1, precond=1, maxit=5000, tol=1e-8)
    hecMAT.Iarray[:] = I
    hecMAT.Rarray[:] = Rr
    got = []
    for sub in range(1, nsub + 1):
        ok, log = fstr.fstr_Newton(solid, hecMAT, ((sub - 1) / nsub, sub / nsub), bc, None, 50, H.DECK_CONVERG)
        assert ok
        got.append(log.shape[0])
        st = solid.get_state(("unode", "strain", "stress"))
        summary = H.summary(m.etype, m.conn, st["unode"], st["strain"], st["stress"])
        assert f1.compare_step(summary, rlog[len(rlog) - nsub + sub - 1]) == [], sub
    print(name, "Newton iterations per sub-step", got, "reference", newton)
    assert got == newton
    s = solid.get_state()
    assert s["latch"] == 0
    _close(s["unode"], ref.unode, "unode", tol=1e-6)
    assert np.array_equal(s["strain_bak"], s["strain"]) and np.array_equal(s["stress_bak"], s["stress"])
    ctx.close()


def test_snapshot_restores_the_state_bitwise(hip):
    from frontistr_amd import fstr
    etype = 361
    m = H.gpu_mesh(etype)
    unode, dunode = H.random_displacement(m.coord, 3, H.GPU_AMP)
    ctx, hecMAT, solid = _solid(hip, etype, m, H.TEST_MATERIALS["arruda"]())
    solid.set_state(dict(unode=unode, dunode=np.zeros_like(dunode)), latch=0)
    solid.element_update()
    fstr.fstr_UpdateState(solid)
    keys = ("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat", "istat")
    before = solid.get_state()
    k0 = solid.element_tangents()
    fstr.fstr_cutback_save(solid)
    solid.set_state(dict(dunode=dunode))
    solid.element_update()
    fstr.fstr_UpdateState(solid)
    mid = solid.get_state()
    assert not np.array_equal(mid["strain"], before["strain"])
    fstr.fstr_cutback_load(solid)
    after = solid.get_state()
    for k in keys:
        assert np.array_equal(after[k], before[k]), k
    solid.set_state(dict(unode=before["unode"], dunode=before["dunode"]))
    assert np.array_equal(solid.element_tangents(), k0)
    ctx.close()


def test_refusals_leave_the_context_usable(hip):
    from frontistr_amd import fstr
    from oracle.refrun import Material
    T = fstr.tMaterial
    mises = T(206900.0, 0.29, plastic=True, plconst=(450.0, 2000.0, 0.0))
    cases = [("TOTALLAG", T.neohooke(0.15, 0.08, nlgeom_flag=fstr.UPDATELAG), None),
             ("TOTALLAG", T.arruda_boyce(0.71, 1.7, 0.14, nlgeom_flag=fstr.INFINITE), None),
             ("incompressible", T.mooney_rivlin(0.15, 0.48, 0.0), None),
             ("incompressible", T.arruda_boyce(0.71, 1.7, 0.0), None),
             ("lambda_m", T.arruda_boyce(0.71, 0.0, 0.14), None),
             ("Mises and a hyperelastic", [mises, T.neohooke(0.15, 0.08)], True),
             ("Mises and a hyperelastic", [T.arruda_boyce(0.71, 1.7, 0.14), mises], True)]
    for etype in (361, 342, 352):
        m = H.gpu_mesh(etype)
        hm = hip.hecmwST_local_mesh(n_node=m.n_node)
        hm.nn_elem = m.conn.shape[1]
        hm.elem_node_item = m.conn.ravel()
        hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
        ctx = hip.SolverContext()
        ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
        em = (1 + np.arange(m.n_elem) % 2).astype(np.int32)
        for word, mat, two in cases:
            with pytest.raises(hip.HecmwSolverError) as e:
                fstr.fstr_solid(ctx, m.coord, m.conn, mat, elem_mat=em if two else None, etype=etype)
            assert e.value.code == FX_ERROR_UNSUPPORTED and word in str(e.value), (etype, word, e.value.code, str(e.value))
        # an ELASTIC context on the same fx_context afterwards
        el = Material(2.5, 0.3, nlgeom=H.TOTALLAG)
        solid = fstr.fstr_solid(ctx, m.coord, m.conn, _fmat(el), etype=etype)
        unode, dunode = H.random_displacement(m.coord, 17, 2e-3)
        solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
        ref = H.Model(etype, m.coord, m.conn, el)
        ref.unode[:], ref.dunode[:] = unode, dunode
        _close(solid.element_tangents(), ref.element_tangents(), "%d elastic tangent after the refusals" % etype)
        ctx.close()


# ---- the scatter fallbacks: FX_ASM_ATOMIC=1, FX_ASM_MAP=0, FX_ASM_FIRST=0 are read once per process -> child processes
PATHS = {"default": {}, "first0": {"FX_ASM_FIRST": "0"}, "map0": {"FX_ASM_MAP": "0"}, "atomic": {"FX_ASM_ATOMIC": "1"}}


def compute_paths(path):
    from frontistr_amd import fstr, hecmw as hip
    out = {}
    for etype, name in ((361, "mooney"), (342, "arruda"), (352, "neohooke")):
        m, mats, em = _two_sections(etype, name, H.TOTALLAG)
        unode, dunode = H.random_displacement(m.coord, 17, H.GPU_AMP)
        ctx, hecMAT, solid = _solid(hip, etype, m, mats, em)
        solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
        solid.element_update()
        fstr.fstr_StiffMatrix(solid, m.dirichlet())
        ctx.download_matrix(hecMAT)
        for k in ("D", "AL", "AU"):
            out["%d/%s" % (etype, k)] = np.array(getattr(hecMAT, k))
        ctx.close()
    np.savez(path, **out)


def test_scatter_fallbacks_agree(tmp_path):
    res = {}
    for name, env in PATHS.items():
        out = str(tmp_path / (name + ".npz"))
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_hyperelastic as T; T.compute_paths(%r)" % (HERE, ROOT, out)
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
        assert p.returncode == 0, "scatter path %s: child exited with %d\n%s" % (name, p.returncode, p.stdout[-3000:])
        res[name] = dict(np.load(out))
    for k, want in res["default"].items():
        # the atomic-free fallbacks add the same contributions in the same colour order: bitwise; atomics: 1e-12 of the diagonal
        for name in ("first0", "map0"):
            assert np.array_equal(res[name][k], want), (name, k)
        scale = max(np.abs(res["default"][k.split("/")[0] + "/D"]).max(), 1e-300)
        assert np.abs(res["atomic"][k] - want).max() <= 1e-12 * scale, ("atomic", k)
