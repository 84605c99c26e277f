"""GPU parity of the Mohr-Coulomb and Drucker-Prager materials (compile-time groups 4..6 of the nonlinear element kernels,
csrc/fx_yield.h) through frontistr_amd/fstr.py against the numpy restatement tests/yield_ref.py, for the six solid types and the three
NLGEOM flags: the elastic tangent before any update, then stress / strain / fstat / istat / internal forces of the first update,
the elastoplastic tangent of that state with the latch cleared (it differs from the elastic one by more than 1e-3 of its largest
entry: a kernel that ignored istat fails), the assembled D / AL / AU, QFORCE, and the elastic tangent again once the latch is set;
both branches of the Mohr-Coulomb tangent; mixed sections; the sub-step loops of recorded cube decks; snapshot; the scatter
fallbacks; the refusals; the device error word.

Meshes: hyper_ref.gpu_mesh (distorted, at 361 with a collapsed hexahedron so that the `dup` path runs).  Tolerance: the project's
nonlinear 1e-11 of the largest entry of the compared array; tests/test_yield_ref.py shows that the inputs (yield_ref.gpu_case)
determine the restated numbers to 1e-12 on that scale and keep every point off every branch edge; istat is compared exactly.  The
edges themselves -- ties of principal stresses, |f| beside tol, the `dlambda < 0` reset, the apex, sin 3 theta = +-1 -- are run by
tests/test_gpu_point_edges.py on trial stresses chosen to the bit (tests/point_ref.py, tests/test_point_ref.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import c3_ref as R
import yield_ref as Y

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX_ERROR_RUNTIME, FX_ERROR_UNSUPPORTED = -1, -2
ETYPES = [361, 341, 342, 351, 352, 362]
FAMILIES = ["drucker", "mohr"]
TOL = 1e-11


def _fmat(mat):
    from frontistr_amd import fstr
    if Y.kind_of(mat) in (Y.MOHR, Y.DRUCKER):
        fm = fstr.tMaterial(mat.E, mat.nu, plastic=True, harden=0, plconst=mat.plconst, nlgeom_flag=mat.nlgeom)
        fm.kind, fm.plconst4 = (fstr.MOHRCOULOMB if mat.kind == Y.MOHR else fstr.DRUCKERPRAGER), mat.plconst4
        return fm
    return fstr.tMaterial(mat.E, mat.nu, plastic=mat.plastic, harden=mat.harden, plconst=mat.plconst, nlgeom_flag=mat.nlgeom)


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


def _check_parity(hip, etype, m, mat, em, unode, dunode):
    from frontistr_amd import fstr
    ref = Y.Model(etype, m.coord, m.conn, mat, em)
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

    k_el = ref.element_tangents()
    _close(solid.element_tangents(), k_el, "elastic tangent before any update")
    qf, rqf = solid.element_update(), ref.element_update()
    s = solid.get_state()
    assert s["latch"] == 1 and ref.latch == 1
    shape = ref.st["istat"].shape
    assert np.array_equal(s["istat"].reshape(shape), ref.st["istat"]), "istat"
    first = np.array([Y.is_yield(ref.mat(e)) for e in range(m.n_elem)])
    plastic = ref.st["istat"][first].mean()
    print("%.0f %% of the points of the Mohr-Coulomb / Drucker-Prager section plastic" % (100 * plastic))
    assert plastic >= 0.25 and 1.0 - plastic >= 0.10
    if not first.all() and any(x.plastic for x in ref.mats[1:]):
        other = ref.st["istat"][~first].mean()
        print("%.0f %% of the points of the Mises section plastic" % (100 * other))
        assert other >= 0.10 and 1.0 - other >= 0.10
    _close(s["strain"], ref.st["strain"], "strain")
    _close(s["stress"], ref.st["stress"], "stress")
    _close(s["fstat"].reshape(shape), ref.st["fstat"], "fstat")
    _close(qf, rqf, "element internal force")
    assert not s["plstrain"].any() and not s["stress_bak"].any()
    # the elastoplastic tangent of that state: the latch cleared by hand
    solid.set_state({}, latch=0)
    ref.latch = 0
    k_ep = ref.element_tangents()
    assert np.abs(k_ep - k_el).max() > 1e-3 * np.abs(k_el).max(), "the plastic state does not change the reference tangent"
    _close(solid.element_tangents(), k_ep, "elastoplastic tangent (latch cleared)")
    assembled("elastoplastic")
    q = np.zeros(3 * m.n_node)
    hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(dunode), hip._ptr(q), None))
    _close(q, ref.update(), "QFORCE")
    # with the latch every tangent is the elastic one again (of the current stress: GEOMAT_C3 and the initial-stress term)
    assert solid.get_state(("stress",))["latch"] == 1 and ref.latch == 1
    k_l = ref.element_tangents()
    assert np.abs(k_l - k_ep).max() > 1e-3 * np.abs(k_ep).max()
    _close(solid.element_tangents(), k_l, "elastic tangent with the latch set")
    ctx.close()


@pytest.mark.parametrize("nlgeom", [Y.INFINITE, Y.TOTALLAG, Y.UPDATELAG], ids=["infinite", "totallag", "updatelag"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("etype", ETYPES)
def test_elements_state_matrix_and_qforce(hip, etype, family, nlgeom):
    m, mat, unode, dunode = Y.gpu_case(etype, family, nlgeom)
    if etype == 361:
        assert any(len(set(c)) < 8 for c in m.conn.tolist()), "no collapsed hexahedron in the 361 mesh"
    _check_parity(hip, etype, m, mat, None, unode, dunode)


@pytest.mark.parametrize("generic", [False, True], ids=["sin3theta_is_1", "trigonometric"])
def test_mohr_coulomb_tangent_branches(hip, generic):
    """One unit cube, nu = 0, displacement along x (yield_ref.branch_case).  Exactly uniaxial: C1 = 0, C2 = sqrt 3, C3 = 0 -- the update
    leaves the uniaxial trial stress (the cohesion is out of reach) and the points are marked as yielded by hand; generic: the
    trigonometric branch on the returned stress of a real update."""
    from types import SimpleNamespace
    mat, dunode = Y.branch_case(generic)
    m = SimpleNamespace(coord=Y.ONE_ELEM_COORD, conn=Y.ONE_ELEM_CONN, n_node=8, n_elem=1)
    ref = Y.Model(361, m.coord, m.conn, mat)
    ref.dunode[:] = dunode
    ctx, hecMAT, solid = _solid(hip, 361, m, mat)
    solid.set_state(dict(dunode=dunode), latch=0)
    qf, rqf = solid.element_update(), ref.element_update()
    _close(qf, rqf, "element internal force")
    s = solid.get_state()
    assert np.array_equal(s["istat"].reshape(1, 8), ref.st["istat"]) and bool(ref.st["istat"].all()) == generic
    _close(s["stress"], ref.st["stress"], "stress")
    if not generic:
        assert not s["stress"].reshape(8, 6)[:, 1:].any() or np.abs(s["stress"].reshape(8, 6)[:, 1:]).max() < 1e-9
        ref.st["istat"][:] = 1
        ref.st["fstat"][:] = 2.0e-3
        solid.set_state(dict(istat=ref.st["istat"], fstat=ref.st["fstat"], stress=ref.st["stress"]))
    for st, fs in zip(ref.st["stress"][0], ref.st["fstat"][0]):
        info = {}
        Y.elastoplastic_matrix(mat, st, 1, fs, info)
        assert info["branch"] == ("trig" if generic else "edge")
    solid.set_state({}, latch=0)
    ref.latch = 0
    k_ep = ref.element_tangents()
    De = R.elastic_matrix(mat.E, mat.nu)
    assert np.abs(Y.elastoplastic_matrix(mat, ref.st["stress"][0, 0], 1, ref.st["fstat"][0, 0]) - De).max() > 1e-3 * De.max()
    _close(solid.element_tangents(), k_ep, "elastoplastic tangent")
    ctx.close()


@pytest.mark.parametrize("other", ["mises", "elastic"])
@pytest.mark.parametrize("etype", [361, 342, 352])
def test_drucker_prager_section_beside_another(hip, etype, other):
    """A Drucker-Prager section (updated Lagrange) beside a Mises one and beside an ELASTIC total-Lagrange one, elements dealt out
    irregularly (yield_ref.mixed_case; tests/test_yield_ref.py asserts the margins of both subsets): groups 6 and 2 / 1 of one
    context.  The latch comes from whichever section is plastic: beside the ELASTIC section only the Drucker-Prager one can set it,
    and it then holds for the ELASTIC elements' tangents too."""
    m, mats, em, unode, dunode = Y.mixed_case(etype, other)
    _check_parity(hip, etype, m, mats, em, unode, dunode)


DECKS_ON_THE_GPU = ["y361_drucker", "y342_mohr", "y352_drucker", "y362_mohr", "y361_drucker_two", "y342_mohr_two"]


@pytest.mark.parametrize("name", DECKS_ON_THE_GPU)
def test_substeps_match_the_recorded_decks(hip, name):
    """fx_newton_substep (CG + SSOR to 1e-12, as the decks' !SOLVER card) on recorded cube decks (tests/golden/yield_decks.npz, the
    unmodified reference program's runs), one per element family and yield function plus two with a Mises second section: the Newton
    count of every sub-step is the reference's, the Global summaries of every step match at the reference harness's 1e-4."""
    from frontistr_amd import fstr
    from oracle.refrun import default_params
    g = np.load(os.path.join(HERE, "golden", "yield_decks.npz"))
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    m, mats, em, bc = Y.golden_deck(name)
    nsub = Y.DECK_SUBSTEPS
    ctx, hecMAT, solid = _solid(hip, m.etype, m, mats, em)
    I, Rr = default_params(method=1, precond=1, maxit=5000, tol=1e-12)
    hecMAT.Iarray[:] = I
    hecMAT.Rarray[:] = Rr
    got = []
    for sub in range(1, nsub + 1):
        ok, log = fstr.fstr_Newton(solid, hecMAT, ((sub - 1) / nsub, sub / nsub), bc, None, 50, Y.DECK_CONVERG)
        assert ok
        got.append(log.shape[0])
        st = solid.get_state(("unode", "strain", "stress"))
        summary = Y.summary(m.etype, m.conn, st["unode"], st["strain"], st["stress"])
        bad = Y.within_1e4(summary, rlog[len(rlog) - nsub + sub - 1])
        assert bad == [], (sub, bad)
    print(name, "Newton iterations per sub-step", got, "reference", newton)
    assert got == newton
    s = solid.get_state()
    assert s["latch"] == 1 and s["istat"].any()
    assert np.array_equal(s["plstrain"], s["fstat"]) and np.array_equal(s["stress_bak"], s["stress"])
    ctx.close()


def test_snapshot_restores_the_state_bitwise(hip):
    from frontistr_amd import fstr
    etype = 361
    m, mat, unode, dunode = Y.gpu_case(etype, "mohr", Y.UPDATELAG)
    ctx, hecMAT, solid = _solid(hip, etype, m, mat)
    solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
    solid.element_update()
    fstr.fstr_UpdateState(solid)
    keys = ("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat", "istat")
    before = solid.get_state()
    assert before["istat"].any() and before["plstrain"].any()
    k0 = solid.element_tangents()
    fstr.fstr_cutback_save(solid)
    solid.set_state(dict(dunode=0.3 * dunode))
    solid.element_update()
    fstr.fstr_UpdateState(solid)
    mid = solid.get_state()
    assert not np.array_equal(mid["plstrain"], before["plstrain"]) and not np.array_equal(mid["stress"], before["stress"])
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

    def with_(mat, **kw):
        for k, v in kw.items():
            setattr(mat, k, v)
        return mat
    dp, mc = (lambda: T.drucker_prager(2.0e4, 0.3, 300.0, 25.0, 400.0)), (lambda: T.mohr_coulomb(2.0e4, 0.3, 300.0, 25.0, 400.0))
    # (the library also refuses cos(phi) == 0, the constant at which the reference's return would stop.  pi / 2 is no double and the
    #  cosine of the doubles next to it is 6e-17 and -1.6e-16, so no input reaches that line and nothing here tests it)
    cases = [("xi = 0", with_(dp(), plconst4=0.0), None),
             ("material kind 6", with_(dp(), kind=6), None),
             ("harden = 0", with_(mc(), harden=2), None),
             ("harden = 0", with_(dp(), harden=4), None),
             ("hyperelastic", [dp(), T.neohooke(0.15, 0.08)], True),
             ("hyperelastic", [T.arruda_boyce(0.71, 1.7, 0.14), mc()], True)]
    for etype in (361, 342, 352):
        m = Y.H.gpu_mesh(etype)
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
        el = Material(2.5, 0.3, nlgeom=Y.TOTALLAG)
        solid = fstr.fstr_solid(ctx, m.coord, m.conn, _fmat(el), etype=etype)
        unode, dunode = Y.H.random_displacement(m.coord, 17, 2e-3)
        solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
        ref = Y.Model(etype, m.coord, m.conn, el)
        ref.unode[:], ref.dunode[:] = unode, dunode
        _close(solid.element_tangents(), ref.element_tangents(), "%d elastic tangent after the refusals" % etype)
        ctx.close()


def test_device_error_word(hip):
    """A hand-set stress at which the reference would `stop` in calElastoPlasticMatrix (yield_ref.STOP_STRESS: J2**1.5 and J3 are
    subnormal and their quotient leaves [-1, 1] by 0.25): the kernels complete, the entry points return FX_ERROR_RUNTIME with the
    reference's text, and the context goes on working once the state is a sound one."""
    from frontistr_amd import fstr
    from frontistr_amd.mesh import CubeMesh
    m = CubeMesh(2)
    mat = Y.mohr_coulomb(1.0e5, 0.0, 500.0, 20.0, nlgeom=Y.INFINITE)
    with pytest.raises(Y.MathError):
        Y.elastoplastic_matrix(mat, Y.STOP_STRESS, 1, 0.0)
    ctx, hecMAT, solid = _solid(hip, 361, m, mat)
    npt = m.n_elem * 8
    stress = np.zeros((npt, 6))
    stress[5] = Y.STOP_STRESS
    istat = np.zeros(npt, dtype=np.int32)
    istat[5] = 1
    solid.set_state(dict(stress=stress, istat=istat), latch=0)
    for call in (lambda: solid.element_tangents(), lambda: fstr.fstr_StiffMatrix(solid, m.dirichlet())):
        with pytest.raises(hip.HecmwSolverError) as e:
            call()
        assert e.value.code == FX_ERROR_RUNTIME and "Math Error in Mohr-Coulomb calculation" in str(e.value), str(e.value)
    solid.set_state(dict(stress=np.zeros((npt, 6)), istat=np.zeros(npt, dtype=np.int32)), latch=0)
    ref = Y.Model(361, m.coord, m.conn, mat)
    _close(solid.element_tangents(), ref.element_tangents(), "tangent after the error")
    ctx.close()


@pytest.mark.parametrize("etype", [361, 342, 352])
def test_device_error_word_of_the_update(hip, etype):
    """The same `stop` on the update side (calYieldFunc :338): a displacement increment whose trial stress is STOP_STRESS at every
    point (nu = 0, u_x = eps x).  fx_nl_element_update and fx_nl_update_at return FX_ERROR_RUNTIME with the text, through the error
    word of the update kernels of all three kernel families; the context then serves a sound increment."""
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    m = CubeMesh(2) if etype == 361 else solid_mesh(2, etype)
    mat = Y.mohr_coulomb(1.0e5, 0.0, 500.0, 20.0, nlgeom=Y.INFINITE)
    bad = np.zeros_like(m.coord)
    bad[:, 0] = (Y.STOP_STRESS[0] / mat.E) * m.coord[:, 0]
    ref = Y.Model(etype, m.coord, m.conn, mat)
    ref.dunode[:] = bad.ravel()
    with pytest.raises(Y.MathError, match="Mohr-Coulomb"):
        ref.element_update()
    ctx, hecMAT, solid = _solid(hip, etype, m, mat)
    solid.set_state(dict(dunode=bad.ravel()), latch=0)
    q = np.zeros(3 * m.n_node)
    for call in (lambda: solid.element_update(),
                 lambda: hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(bad.ravel().copy()), hip._ptr(q), None))):
        with pytest.raises(hip.HecmwSolverError) as e:
            call()
        assert e.value.code == FX_ERROR_RUNTIME and "Math Error in Mohr-Coulomb calculation" in str(e.value), str(e.value)
    assert solid.get_state(("istat",))["latch"] == 0, "the update that stopped does not set the latch"
    good = np.zeros_like(m.coord)
    good[:, 0] = 0.012 * m.coord[:, 0] + 0.009 * m.coord[:, 1] + 0.004 * m.coord[:, 2]
    ref = Y.Model(etype, m.coord, m.conn, mat)
    ref.dunode[:] = good.ravel()
    solid.set_state(dict(dunode=good.ravel(), stress=np.zeros_like(ref.st["stress"]), strain=np.zeros_like(ref.st["strain"]),
                         istat=ref.st["istat"], fstat=ref.st["fstat"]), latch=0)
    qf, rqf = solid.element_update(), ref.element_update()
    _close(qf, rqf, "element internal force after the error")
    s2 = solid.get_state()
    assert s2["latch"] == 1 and np.array_equal(s2["istat"], ref.st["istat"]) and ref.st["istat"].any()
    _close(s2["stress"], ref.st["stress"], "stress after the error")
    ctx.close()


# ---- the scatter fallbacks: FX_ASM_ATOMIC=1, FX_ASM_MAP=0, FX_ASM_FIRST=0 are read once per process -> child processes
PATHS = {"default": {}, "first0": {"FX_ASM_FIRST": "0"}, "map0": {"FX_ASM_MAP": "0"}, "atomic": {"FX_ASM_ATOMIC": "1"}}


def compute_paths(path):
    from frontistr_amd import fstr, hecmw as hip
    out = {}
    for etype, family in ((361, "mohr"), (342, "drucker"), (352, "mohr")):
        m, mat, unode, dunode = Y.gpu_case(etype, family, Y.UPDATELAG)
        ctx, hecMAT, solid = _solid(hip, etype, m, mat)
        solid.set_state(dict(unode=unode, dunode=dunode), latch=0)
        solid.element_update()
        solid.set_state({}, latch=0)          # the elastoplastic tangent
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
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_yield as T; T.compute_paths(%r)" % (HERE, ROOT, out)
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
        assert p.returncode == 0, "scatter path %s: child exited with %d\n%s" % (name, p.returncode, p.stdout[-3000:])
        res[name] = dict(np.load(out))
    for k, want in res["default"].items():
        # the atomic-free fallbacks add the same contributions in the same colour order: bitwise; atomics: the 1e-11
        for name in ("first0", "map0"):
            assert np.array_equal(res[name][k], want), (name, k)
        scale = max(np.abs(res["default"][k.split("/")[0] + "/D"]).max(), 1e-300)
        assert np.abs(res["atomic"][k] - want).max() <= TOL * scale, ("atomic", k)
