"""GPU parity of the nonlinear wedges and 20-node hexahedra (TYPE=351, 352, 362; fx_nl_init_type, csrc/fx_nonlinear_c3.h) through
the C ABI and frontistr_amd/fstr.py against the numpy restatement tests/c3_nl_ref.py: the cases of test_gpu_tet_nonlinear.py --
element tangents before and after the latch, the stress update with its internal forces, the state, the assembled matrix with
boundary conditions, QFORCE, whole sub-step loops, snapshot, scatter fallbacks, errors.

Meshes: solid_mesh(2, etype) regular and skewed (curved edges at 352 / 362), and for 352 / 362 the skewed 3^3 cube: 54 wedges
or 27 hexahedra are no multiple of the elements per workgroup of the update kernels (8 / 2) or, at 362 and in the colours of
both, of the tangent kernels' (2 / 1); the 16 wedges of the 2^3 cube are no multiple of 351's 12 / 32.

Tolerances: the project's own from the tet tests.  INFINITE and TOTALLAG: 1e-11 relative to the largest entry of the compared
array.  UPDATELAG: the reference rounds the stress increment to single precision (`real()`, static_LIB_3d.f90:718, on every type
that goes through UPDATE_C3), so everything that depends on the updated stress is compared at 2 x 2^-23 relative to the largest
stress increment of the case (for quantities linear in the stress: to their largest entry), and at most 1 % of the components
may differ by more than 1e-11 relative.  The 1 % is a cap; tests/test_c3_nl_ref.py shows that the restatement alone, with the
element's nodes summed in two orders on these inputs, stays inside it (share 0.0000 at all three types).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import c3_nl_ref as N
import c3_ref as R
from frontistr_amd.mesh import solid_mesh
from oracle.refrun import Material

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAB = np.array([[450.0, 0.0], [608.0, 0.05], [679.0, 0.1], [732.0, 0.2]])
E0, NU0 = 206900.0, 0.29
FX_ERROR_UNSUPPORTED, FX_ERROR_RUNTIME = -2, -1
SINGLE = 2.0 * 2.0 ** -23


def materials(kind, nlgeom):
    """-> (material or list, elem_mat function or None)"""
    if kind == "elastic":
        return Material(E0, NU0, nlgeom=nlgeom), None
    if kind == "bilinear":
        return Material(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=nlgeom), None
    if kind == "multilinear":
        return Material(E0, NU0, plastic=True, harden=1, table=TAB, nlgeom=nlgeom), None
    if kind == "swift":
        return Material(E0, NU0, plastic=True, harden=2, plconst=(0.002, 900.0, 0.2), nlgeom=nlgeom), None
    if kind == "ramberg":
        return Material(E0, NU0, plastic=True, harden=3, plconst=(0.002, 450.0, 5.0), nlgeom=nlgeom), None
    # two sections with different flags: the given kinematics with Mises BILINEAR next to an elastic part of another flag
    other = N.TOTALLAG if nlgeom != N.TOTALLAG else N.UPDATELAG
    if kind == "two_sections_elastic_first":     # the latch must come from whichever section is elastoplastic
        return ([Material(70000.0, 0.33, nlgeom=other), Material(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=nlgeom)],
                lambda m: (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32))
    return ([Material(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=nlgeom), Material(70000.0, 0.33, nlgeom=other)],
            lambda m: (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32))


KINDS = ["elastic", "bilinear", "multilinear", "swift", "ramberg", "two_sections", "two_sections_elastic_first"]
ETYPES = [351, 352, 362]
_CURVE = lambda et: {"curve": 0.03} if et != 351 else {}
MESHES = {"regular": lambda et: solid_mesh(2, et), "skewed": lambda et: solid_mesh(2, et, skew=0.1, **_CURVE(et)),
          "skewed3": lambda et: solid_mesh(3, et, skew=0.1, **_CURVE(et))}
# (etype, mesh) of the element-level cases: the 3^3 cube where the 2^3 one fills the workgroups evenly
ELEMENT_CASES = [(et, mesh) for et in ETYPES for mesh in MESHES if mesh != "skewed3" or et != 351]


def _fmat(mat):
    from frontistr_amd import fstr
    return fstr.tMaterial(mat.E, mat.nu, plastic=mat.plastic, harden=mat.harden, plconst=mat.plconst,
                          table=mat.table if mat.table.size else None, nlgeom_flag=mat.nlgeom)


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


def _close(a, b, tol, tag, scale=None):
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


def _case(etype, kind, nlgeom, mesh, seed=17):
    m = MESHES[mesh](etype)
    mat, emf = materials(kind, nlgeom)
    em = emf(m) if emf else None
    first = next((x for x in mat if x.plastic), mat[0]) if isinstance(mat, list) else mat
    unode, dunode, st = N.random_case(etype, first, m, seed)
    return m, mat, em, unode, dunode, st


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nlgeom", [N.INFINITE, N.TOTALLAG, N.UPDATELAG], ids=["infinite", "totallag", "updatelag"])
@pytest.mark.parametrize("etype,mesh", ELEMENT_CASES)
def test_elements_state_matrix_and_qforce(hip, oracle, etype, nlgeom, kind, mesh):
    from frontistr_amd import fstr
    m, mat, em, unode, dunode, st = _case(etype, kind, nlgeom, mesh)
    ul = nlgeom == N.UPDATELAG or kind.startswith("two_sections")     # (the second section of two_sections is UPDATELAG when the first is TOTALLAG)
    ul = ul and any(x.nlgeom == N.UPDATELAG for x in (mat if isinstance(mat, list) else [mat]))
    ref = N.Model(etype, m.coord, m.conn, mat, em)
    ref.st = {k: v.copy() for k, v in st.items()}
    ref.unode[:], ref.dunode[:] = unode, dunode
    ctx, hecMAT, solid = _solid(hip, etype, m, mat, em)
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    # tangent before the latch (plastic points use calElastoPlasticMatrix)
    _close(solid.element_tangents(), ref.element_tangents(), 1e-11, "tangent before the first update")
    # the assembled matrix with boundary conditions, twice: bitwise repeatable
    bc = m.dirichlet()
    bc = (bc[0], bc[1], 1e-3 * np.cos(np.arange(bc[0].size)))
    Kd, fd = R.apply_bc(ref.stiffness(), np.zeros(3 * m.n_node), bc)
    got = []
    for _ in range(2):
        fstr.fstr_StiffMatrix(solid, bc)
        ctx.download_matrix(hecMAT)
        got.append([np.array(getattr(hecMAT, k)) for k in ("D", "AL", "AU")])
    for x, y in zip(*got):
        assert np.array_equal(x, y), "two assemblies of the same state differ"
    D, AL, AU = R.to_blocks(Kd, hecMAT)
    scale = np.abs(Kd).max()
    for k, x, y in zip(("D", "AL", "AU"), got[0], (D, AL, AU)):
        _close(x, y, 1e-11, "assembled " + k, scale)
    # stress update, internal forces, state
    qf = solid.element_update()
    rqf = ref.element_update()
    s = solid.get_state()
    assert s["latch"] == ref.latch
    if ul:
        ds = max(np.abs(ref.dstress).max(), 1e-300)
        _close_ul(s["stress"], ref.st["stress"], "stress", ds)
        _close_ul(qf, rqf, "element internal force")
    else:
        _close(s["stress"], ref.st["stress"], 1e-11, "stress")
        _close(qf, rqf, 1e-11, "element internal force")
    _close(s["strain"], ref.st["strain"], 1e-11, "strain")
    if ref.latch:
        assert np.array_equal(s["istat"], ref.st["istat"])
        if ul:
            # a stress perturbation d moves the Mises stress by at most sqrt(3/2) |d| and the plastic multiplier by that over 3 G + H:
            # with the stress at 2 x 2^-23 of the largest increment ds, fstatus(1) is within the same figure of sqrt(9) ds / (3 G)
            G = min(x.E / (2.0 * (1.0 + x.nu)) for x in (mat if isinstance(mat, list) else [mat]) if x.plastic)
            _close_ul(s["fstat"], ref.st["fstat"], "fstatus(1)", ds / G)
        else:
            _close(s["fstat"], ref.st["fstat"], 1e-11, "fstatus(1)", max(np.abs(ref.st["fstat"]).max(), 1e-3))
    for k in ("plstrain", "stress_bak", "strain_bak"):      # the element update leaves them alone
        assert np.array_equal(s[k], st[k]), k
    # tangent after the update (latched elastic matrix, new stress in the geometric terms)
    (_close_ul if ul else lambda a, b, t: _close(a, b, 1e-11, t))(solid.element_tangents(), ref.element_tangents(), "tangent after the update")
    # QFORCE: the scattered internal force (fp64 atomics)
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    q = np.zeros(3 * m.n_node)
    hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(dunode), hip._ptr(q), None))
    ref.st = {k: v.copy() for k, v in st.items()}
    ref.latch = 0
    rq = ref.update()
    (_close_ul if ul else lambda a, b, t: _close(a, b, 1e-11, t))(q, rq, "QFORCE")
    ctx.close()


@pytest.mark.parametrize("name", list(N.GOLDEN_DECKS))
def test_substeps_match_the_recorded_decks(hip, oracle, name):
    """fstr_solve_NLGEOM (fx_newton_substep around CG + SSOR to 1e-8, as the decks' !SOLVER card) on the recorded cube decks
    (tests/golden/nl_c3_decks.npz, the unmodified reference program's runs): the Newton count of every sub-step is the
    reference's, the summaries of every step (displacements, nodal and element strains, stresses, Mises stress)
    match at the reference harness's 1e-4; against the restatement's
    dense-solve loop the converged displacement agrees to 1e-6 relative (the Krylov tolerance) and the plastic flags are equal."""
    import json
    from frontistr_amd import fstr
    from oracle import fistr1_run as f1
    from oracle.refrun import default_params
    g = np.load(os.path.join(HERE, "golden", "nl_c3_decks.npz"))
    rlog, newton = json.loads(str(g[name + "/log"])), list(g[name + "/newton"])
    m, mats, em, bc = N.golden_deck(name)
    nsub = N.DECK_SUBSTEPS
    oracle.nl_reset_latch()
    ref = N.Model(m.etype, m.coord, m.conn, mats, em)
    for sub in range(1, nsub + 1):
        ok, it = ref.newton_substep((sub - 1) / nsub, sub / nsub, bc, None, 50, N.DECK_CONVERG)
        assert ok
    ctx, hecMAT, solid = _solid(hip, m.etype, m, mats, em)
    I, Rr = default_params(method=1, precond=1, maxit=5000, tol=1e-8)
    hecMAT.Iarray[:] = I
    hecMAT.Rarray[:] = Rr
    got = []
    for sub in range(1, nsub + 1):
        ok, log = fstr.fstr_Newton(solid, hecMAT, ((sub - 1) / nsub, sub / nsub), bc, None, 50, N.DECK_CONVERG)
        assert ok
        got.append(log.shape[0])
        st = solid.get_state(("unode", "strain", "stress"))
        summary = N.summary(m.etype, m.conn, st["unode"], st["strain"], st["stress"])
        assert f1.compare_step(summary, rlog[len(rlog) - nsub + sub - 1]) == [], sub
    print(name, "Newton iterations per sub-step", got, "reference", newton)
    assert got == [int(x) for x in newton]
    s = solid.get_state()
    _close(s["unode"], ref.unode, 1e-6, "unode")
    if "elastic" not in name:
        assert (ref.st["plstrain"] > 0).any(), "the plastic deck has no plastic point"
        assert np.array_equal(s["istat"], ref.st["istat"])
        assert np.abs(s["plstrain"] - ref.st["plstrain"]).max() < 1e-8
    ctx.close()


def test_snapshot_restores_the_state_bitwise(hip, oracle):
    from frontistr_amd import fstr
    etype = 352
    m, mat, em, unode, dunode, st = _case(etype, "bilinear", N.UPDATELAG, "skewed")
    ctx, hecMAT, solid = _solid(hip, etype, m, mat, em)
    solid.set_state(dict(st, unode=unode, dunode=np.zeros_like(dunode)), latch=0)
    keys = ("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat", "istat")
    before = solid.get_state()
    fstr.fstr_cutback_save(solid)
    solid.set_state(dict(dunode=dunode))
    solid.element_update()
    fstr.fstr_UpdateState(solid)
    mid = solid.get_state()
    assert not np.array_equal(mid["stress"], before["stress"])
    fstr.fstr_cutback_load(solid)
    after = solid.get_state()
    for k in keys:
        assert np.array_equal(after[k], before[k]), k
    ctx.close()


def _init_type(hip, m, etype, nn_elem, mat):
    """fx_nl_init_type on a fresh context with the profile of m -> (return code, message)"""
    import ctypes as C
    from frontistr_amd import fstr
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    coord, conn = np.ascontiguousarray(m.coord), np.ascontiguousarray(m.conn, dtype=np.int32)
    mv = hip._MeshView(m.n_node, m.n_elem, hip._ptr(coord), hip._ptr(conn))
    arr = (fstr._MaterialView * 1)(_fmat(mat).view())
    code = hip.lib().fx_nl_init_type(ctx.h, C.byref(mv), etype, nn_elem, 1, arr, None)
    msg = hip.lib().fx_last_error().decode()
    ctx.close()
    return code, msg


def test_errors(hip):
    mat = Material(E0, NU0, nlgeom=N.TOTALLAG)
    m = solid_mesh(1, 362)
    w6 = solid_mesh(1, 351)
    for etype in (361, 371):
        code, msg = _init_type(hip, m, etype, 20, mat)
        assert code == FX_ERROR_UNSUPPORTED and "fx_nl_init_type" in msg, (etype, code, msg)
    from frontistr_amd.mesh import CubeMesh
    cube = CubeMesh(1)
    code, msg = _init_type(hip, cube, 362, 8, mat)          # 362 stated for an 8-node connectivity
    assert code == FX_ERROR_UNSUPPORTED and "20 nodes" in msg, (code, msg)
    bad = solid_mesh(1, 352)
    bad.conn = bad.conn.copy()
    bad.conn[1, 14] = bad.conn[1, 2]
    with pytest.raises(hip.HecmwSolverError) as e:
        _solid(hip, 352, bad, mat)
    assert e.value.code == FX_ERROR_RUNTIME and "twice" in str(e.value)
    # fx_nl_init_c3 keeps its two types
    import ctypes as C
    from frontistr_amd import fstr
    ctx, hecMAT, _ = _solid(hip, 351, w6, mat)
    coord, conn = np.ascontiguousarray(w6.coord), np.ascontiguousarray(w6.conn, dtype=np.int32)
    mv = hip._MeshView(w6.n_node, w6.n_elem, hip._ptr(coord), hip._ptr(conn))
    arr = (fstr._MaterialView * 1)(_fmat(mat).view())
    assert hip.lib().fx_nl_init_c3(ctx.h, C.byref(mv), 351, 1, arr, None) == FX_ERROR_UNSUPPORTED
    ctx.close()


def test_hexahedra_after_20_node_hexahedra_on_one_context(hip, oracle):
    """A 361 fx_nl_init context created after a 362 context on the same fx_context gives the oracle's 361 results."""
    from frontistr_amd import fstr
    import test_gpu_nonlinear as G
    T = G._T()
    etype = 362
    m, mat, em, unode, dunode, st = _case(etype, "bilinear", N.UPDATELAG, "regular")
    ctx, hecMAT, solid = _solid(hip, etype, m, mat, em)
    solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
    solid.element_update()
    hmat, hm, hu, hdu, hst = T.element_case("mises_bilinear_ul", seed=11)
    ke0, qf, ke1, ost = oracle.nl_elements(hmat, hm.coord, hm.conn, hu, hdu, hst)
    hx = hip.hecmwST_local_mesh(n_node=hm.n_node)
    hx.elem_node_item = hm.conn.ravel()
    hecMAT2 = hip.hecmw_mat_con(hx, hip.hecmwST_matrix())
    ctx.upload(hecMAT2, what=hip.FX_UP_PROFILE)
    hsolid = fstr.fstr_solid(ctx, hm.coord, hm.conn, G._fmat(hmat))
    hsolid.set_state(dict(hst, unode=hu, dunode=hdu), latch=0)
    _close(hsolid.element_tangents(), ke0, 1e-11, "361 ke0")
    _close(hsolid.element_update(), qf, 1e-11, "361 qf")
    _close(hsolid.get_state()["stress"], ost["stress"], 1e-11, "361 stress")
    _close(hsolid.element_tangents(), ke1, 1e-11, "361 ke1")
    ctx.close()


# ---- the scatter fallbacks: FX_ASM_ATOMIC=1, FX_ASM_MAP=0, FX_ASM_FIRST=0 are read once per process -> child processes
PATHS = {"default": {}, "first0": {"FX_ASM_FIRST": "0"}, "map0": {"FX_ASM_MAP": "0"}, "atomic": {"FX_ASM_ATOMIC": "1"}}


def compute_paths(path):
    from frontistr_amd import fstr, hecmw as hip
    from oracle import pyoracle
    pyoracle.build()
    out = {}
    for etype in ETYPES:
        m, mat, em, unode, dunode, st = _case(etype, "two_sections", N.UPDATELAG, "skewed")
        ctx, hecMAT, solid = _solid(hip, etype, m, mat, em)
        solid.set_state(dict(st, unode=unode, dunode=dunode), latch=0)
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
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_c3_nonlinear as T; T.compute_paths(%r)" % (HERE, ROOT, out)
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
