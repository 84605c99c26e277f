"""GPU parity of thermal strain in the nonlinear loop (fx_nl_set_thermal, the TH variants of the four update kernel families and of
the tangent kernels) through the C ABI and frontistr_amd/fstr.py against the numpy restatement tests/nl_thermal_ref.py.

Cases (nl_thermal_ref.gpu_case / mixed_case) per type and formulation -- 361 B-bar, 361 F-bar, 341, 342, 351, 352, 362:
  one     one distorted element, a different temperature at each of its nodes
  cube    the smallest skewed cube that fills more than one workgroup of the family's update kernel and is no multiple of its
          elements per workgroup (nl_thermal_ref.update_elems_per_workgroup reads FXN_BLOCK and C3El<ET>::BS / ULPE from the headers)
  two     an ELASTIC and a Mises material in one group; last_temp, temp_init and ref_temp all different, so a tt0 taken by the
          wrong rule shows
  tables  the same with !ELASTIC and !EXPANSION_COEFF tables, node temperatures from below the first row to above the last;
          the tangent with the elastic table before and after the latch
and a context of an F-bar group, a wedge group and a tetrahedral group; further the material groups those cases do not reach
(INFINITE, Drucker-Prager with tables, hyperelastic, UPDATELAG at the STF_C3 types), the thermal first right-hand side after
fx_nl_begin_substep, and the Newton loop on the decks recorded from the reference program (tests/golden/nl_thermal_decks.npz).

Tolerance: the project's nonlinear bound, 1e-11 of the largest entry of the compared array, for stress, strain, fstatus, element
forces, QFORCE and tangents.  The Mises material is UPDATELAG at 361 B-bar and TOTALLAG elsewhere (nl_thermal_ref.mises_flag says
why: UPDATE_C3's UPDATELAG branch rounds to single precision and is compared at that precision by the families' own tests).
tests/test_nl_thermal_ref.py holds the conditions under which this bound means something.
"""
import numpy as np
import pytest

import nl_thermal_ref as NT

pytestmark = pytest.mark.gpu
FX_ERROR_UNSUPPORTED, FX_ERROR_RUNTIME = -2, -1
TOL = 1e-11


def _fmat(mat):
    from frontistr_amd import fstr
    import yield_ref as Y
    if NT._is_hyper(mat):
        m = fstr.tMaterial.mooney_rivlin(*mat.plconst)
    elif Y.is_yield(mat):
        m = fstr.tMaterial(mat.E, mat.nu, plastic=True, harden=0, plconst=mat.plconst, nlgeom_flag=mat.nlgeom)
        m.kind, m.plconst4 = (fstr.MOHRCOULOMB if mat.kind == Y.MOHR else fstr.DRUCKERPRAGER), mat.plconst4
    else:
        m = fstr.tMaterial(mat.E, mat.nu, plastic=mat.plastic, harden=mat.harden, plconst=mat.plconst,
                           table=mat.table if mat.table.size else None, nlgeom_flag=mat.nlgeom)
    m.expansion = getattr(mat, "expansion", 0.0)
    m.expansion_table = getattr(mat, "expansion_table", None)
    m.elastic_table = getattr(mat, "elastic_table", None)
    return m


def _solid(hip, case, thermal=True):
    from frontistr_amd import fstr
    m = case["mesh"]
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hecMAT = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), case["groups"])
    ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    solid = fstr.fstr_solid(ctx, m.coord, None, [_fmat(x) for x in case["mats"]], groups=case["groups"])
    solid.set_state(dict(unode=case["unode"], dunode=case["dunode"]), latch=0)
    if thermal:
        solid.set_thermal(case["ref_temp"], case["temp_init"])
        solid.set_state(dict(last_temp=case["last_temp"]))
        solid.set_temperature(case["temperature"])
    return ctx, hecMAT, solid


def _close(a, b, tag, scale=None):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    scale = max(np.abs(b).max(), 1e-300) if scale is None else scale
    err = np.abs(a - b).max() / scale
    print("%s: %.3e (bound %.1e)" % (tag, err, TOL))
    assert err < TOL, "%s: %.3e" % (tag, err)


SINGLE = 2.0 * 2.0 ** -23


def _close_ul(a, b, tag, scale):
    """UPDATE_C3's UPDATELAG branch rounds the stress increment to single precision (static_LIB_3d.f90:718): the two-tier rule of
    test_gpu_c3_nonlinear.py for everything that depends on the updated stress -- within 2 x 2^-23 of the largest stress increment
    (here the largest stress: the history is zero and the ELASTIC partner keeps its trial stress), at most 1 % of the components
    beyond 1e-11"""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    d = np.abs(a - b) / scale
    share = (d > TOL).mean()
    print("%s: max %.3e (bound %.3e), share above 1e-11: %.5f" % (tag, d.max(), SINGLE, share))
    assert d.max() <= SINGLE, "%s: %.3e" % (tag, d.max())
    assert share <= 0.01, "%s: %.4f of the components differ by more than 1e-11" % (tag, share)


def _flat(ref, key):
    return np.concatenate([p["st"][key].ravel() for p in ref.parts])


def _cat(per_group):
    return np.concatenate([np.asarray(x).ravel() for x in per_group])


def _compare(hip, case, tangents, single=False):
    """single: the case runs UPDATE_C3's UPDATELAG branch; what depends on the updated stress is held to _close_ul"""
    ref = NT.model_of(case)
    ctx, hecMAT, solid = _solid(hip, case)
    if tangents:
        _close(solid.element_tangents(), _cat(ref.element_tangents()), "tangent before the first update")
    qf, rqf = solid.element_update(), _cat(ref.element_update())
    s = solid.get_state()
    assert s["latch"] == ref.latch
    ds = np.abs(_flat(ref, "stress")).max()
    stressy = (lambda a, b, tag, scale=None: _close_ul(a, b, tag, ds if scale is None else scale)) if single else _close
    stressy(s["stress"], _flat(ref, "stress"), "stress")
    _close(s["strain"], _flat(ref, "strain"), "strain")
    stressy(qf, rqf, "element internal force", np.abs(rqf).max() if single else None)
    if ref.latch:
        assert np.array_equal(s["istat"].ravel(), _flat(ref, "istat"))
        assert _flat(ref, "istat").any(), "no point yields"
        G = min(x.E / (2.0 * (1.0 + x.nu)) for x in case["mats"] if NT.is_elastoplastic(x))
        stressy(s["fstat"], _flat(ref, "fstat"), "fstatus(1)", ds / G if single else max(np.abs(_flat(ref, "fstat")).max(), 1e-3))
    if tangents:
        kr = _cat(ref.element_tangents())
        stressy(solid.element_tangents(), kr, "tangent after the update", np.abs(kr).max() if single else None)
    # QFORCE: the scattered internal force, from the zero history again
    z = NT.model_of(case)
    solid.set_state({k: np.zeros_like(v) for k, v in s.items() if k in ("stress", "strain", "fstat", "istat")}, latch=0)
    q = np.zeros(3 * case["mesh"].n_node)
    hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(case["dunode"]), hip._ptr(q), None))
    rq = z.update()
    stressy(q, rq, "QFORCE", np.abs(rq).max() if single else None)
    ctx.close()


@pytest.mark.parametrize("variant", ["one", "cube", "two", "tables"])
@pytest.mark.parametrize("fam", NT.FAMILIES)
def test_update_and_tangent_against_the_restatement(hip, oracle, fam, variant):
    case = NT.gpu_case(fam, variant)
    if variant == "cube":
        epb = NT.update_elems_per_workgroup(fam)
        assert case["mesh"].n_elem > epb and case["mesh"].n_elem % epb != 0
    if variant == "tables":
        tc = case["temperature"]
        assert tc.min() < NT.ELASTIC_TAB[0, 2] and tc.max() > NT.ELASTIC_TAB[-1, 2] and ((tc > 0.0) & (tc < 300.0)).any()
    if variant in ("two", "tables"):
        assert not np.array_equal(case["last_temp"], case["temp_init"]) and np.all(case["temp_init"] != case["ref_temp"])
    _compare(hip, case, tangents=variant in ("two", "tables"))


# (UPDATELAG: 361 B-bar runs it in the `two` and `tables` cases above, F-bar serves none)
GROUP_CASES = [(f, v) for f in NT.FAMILIES for v in ("infinite", "yield", "mohr", "hyper", "updatelag") if v != "updatelag" or f not in ("361", "361f")]


@pytest.mark.parametrize("fam,variant", GROUP_CASES)
def test_every_material_group_with_thermal_strain(hip, oracle, fam, variant):
    """The groups the cases above do not reach: INFINITE (group 0; at F-bar its own branch of the strain), Drucker-Prager and
    Mohr-Coulomb with tables (groups 4..6: E(T), nu(T) inside yield_backward_euler), hyperelastic (group 3: tt0 is the initial condition, the stored
    strain dstrain + EPSTH), and UPDATELAG at the STF_C3 types (strain_bak + dstrain + EPSTH; single-precision stress increment)."""
    _compare(hip, NT.gpu_case(fam, variant), tangents=True, single=variant == "updatelag")


@pytest.mark.parametrize("fam,variant", [(f, v) for f in NT.FAMILIES for v in ("two", "tables", "yield", "hyper")] + [("mixed", "two")])
def test_thermal_first_right_hand_side(hip, oracle, fam, variant):
    """B after fx_nl_begin_substep with GL = 0 and a known QFORCE is -QFORCE plus the TLOAD vector of every element on coord +
    unode with TEMP0 = last_temp (not the initial condition, whatever the material), every 361 element as B-bar (F-bar included),
    coefficients and D of the point's temperatures where there are tables: against Model.thermal_load at 1e-11 of the largest entry."""
    case = NT.mixed_case() if fam == "mixed" else NT.gpu_case(fam, variant)
    ref = NT.model_of(case)
    ref.hyper_load = False          # the library adds no load for a hyperelastic element
    load = ref.thermal_load()
    assert np.abs(load).max() > 0 and not np.array_equal(case["last_temp"], case["temp_init"])
    q = np.random.default_rng(4).uniform(-1, 1, load.size) * np.abs(load).max()
    ctx, hecMAT, solid = _solid(hip, case)
    solid.set_state(dict(qforce=q))
    hip._chk(hip.lib().fx_nl_begin_substep(ctx.h, None))
    ctx.download_matrix(hecMAT)
    _close(np.array(hecMAT.B), load - q, "B = -QFORCE + thermal load")
    assert not solid.get_state(("dunode",))["dunode"].any()
    ctx.close()


def test_snapshot_from_before_set_thermal_is_not_loaded(hip, oracle):
    """A save that holds no last_temp of the present thermal set-up restores nothing: FX_ERROR_RUNTIME, last_temp as it was"""
    from frontistr_amd import fstr
    case = NT.gpu_case("341", "two")
    ctx, hecMAT, solid = _solid(hip, case, thermal=False)
    fstr.fstr_cutback_save(solid)
    solid.set_thermal(case["ref_temp"], case["temp_init"])
    with pytest.raises(hip.HecmwSolverError) as ei:
        fstr.fstr_cutback_load(solid)
    assert ei.value.code == FX_ERROR_RUNTIME and "last_temp" in str(ei.value)
    assert np.array_equal(solid.get_state(("last_temp",))["last_temp"], case["temp_init"])
    fstr.fstr_cutback_save(solid)
    solid.set_thermal(case["ref_temp"], case["temp_init"])          # a repeated set-up drops the saved last_temp too
    with pytest.raises(hip.HecmwSolverError):
        fstr.fstr_cutback_load(solid)
    ctx.close()


def test_mixed_context_with_fbar_c3_and_tet_groups(hip, oracle):
    case = NT.mixed_case()
    assert [g[0] for g in case["groups"]] == [361, 351, 341] and case["groups"][0][2] == 4
    _compare(hip, case, tangents=True)


def test_commit_and_snapshot_carry_last_temp(hip, oracle):
    from frontistr_amd import fstr
    case = NT.gpu_case("361", "two")
    ctx, hecMAT, solid = _solid(hip, case)
    assert np.array_equal(solid.get_state(("last_temp",))["last_temp"], case["last_temp"])
    fstr.fstr_cutback_save(solid)
    solid.element_update()
    fstr.fstr_UpdateState(solid)
    assert np.array_equal(solid.get_state(("last_temp",))["last_temp"], case["temperature"])
    fstr.fstr_cutback_load(solid)
    assert np.array_equal(solid.get_state(("last_temp",))["last_temp"], case["last_temp"])
    ctx.close()


def test_set_thermal_starts_last_temp_from_the_initial_condition(hip, oracle):
    case = NT.gpu_case("341", "one")
    ctx, hecMAT, solid = _solid(hip, case, thermal=False)
    solid.set_thermal(case["ref_temp"], case["temp_init"])
    assert np.array_equal(solid.get_state(("last_temp",))["last_temp"], case["temp_init"])
    solid.set_thermal(case["ref_temp"])
    assert not solid.get_state(("last_temp",))["last_temp"].any()
    ctx.close()


@pytest.mark.parametrize("fam", NT.FAMILIES)
def test_no_thermal_strain_is_the_non_thermal_update_bit_for_bit(hip, oracle, fam):
    """temp == temp_init == last_temp == ref_temp: stress, strain, history and element forces of the thermal variant equal those
    of the kernels without it, and two updates of the same state are bitwise equal"""
    case = NT.gpu_case(fam, "two")
    flat = np.full(case["mesh"].n_node, case["ref_temp"])
    case.update(temp_init=flat, last_temp=flat, temperature=flat)
    out = []
    for thermal in (False, True, True):
        ctx, hecMAT, solid = _solid(hip, case, thermal=thermal)
        qf = solid.element_update()
        s = solid.get_state()
        out.append((qf, s))
        ctx.close()
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]), "element forces"
        for k in ("stress", "strain", "fstat", "istat"):
            assert np.array_equal(out[0][1][k], other[1][k]), k


def test_two_updates_of_a_thermal_state_are_bitwise_equal(hip, oracle):
    case = NT.gpu_case("362", "tables")
    ctx, hecMAT, solid = _solid(hip, case)
    solid.element_update()
    a = solid.get_state()
    solid.set_state({k: np.zeros_like(a[k]) for k in ("stress", "strain", "fstat", "istat")})
    solid.element_update()
    b = solid.get_state()
    assert np.array_equal(a["stress"], b["stress"]) and np.array_equal(a["strain"], b["strain"])
    ctx.close()


def test_refusals(hip, oracle):
    from frontistr_amd import fstr
    case = NT.gpu_case("341", "two")
    ctx, hecMAT, solid = _solid(hip, case)
    before = solid.get_state(("last_temp",))["last_temp"]
    for name, tab in (("expansion_table", np.array([[1e-5, 0.0], [2e-5, 0.0]])), ("elastic_table", np.array([[2e5, 0.3, 50.0], [1e5, 0.3, 10.0]]))):
        setattr(solid.material[0], name, tab)
        with pytest.raises(hip.HecmwSolverError) as ei:
            solid.set_thermal(0.0, None)
        assert ei.value.code == FX_ERROR_UNSUPPORTED and "ascending" in str(ei.value)
        setattr(solid.material[0], name, None)
        assert np.array_equal(solid.get_state(("last_temp",))["last_temp"], before)      # the context is untouched
    with pytest.raises(hip.HecmwSolverError) as ei:
        solid.set_temperature(None)
    assert ei.value.code == FX_ERROR_RUNTIME
    ctx.close()
    # an elastic table on a hyperelastic material
    m = case["mesh"]
    hyper = fstr.tMaterial.neohooke(0.1486, 0.0789)
    hyper.elastic_table = NT.ELASTIC_TAB
    c2 = dict(case, mats=[], groups=[(341, m.conn, 2, None)])
    ctx, hecMAT, solid = _solid(hip, dict(c2, mats=[NT.material("elastic", "341")]), thermal=False)
    solid2 = fstr.fstr_solid(ctx, m.coord, None, [hyper], groups=c2["groups"])
    with pytest.raises(hip.HecmwSolverError) as ei:
        solid2.set_thermal(0.0)
    assert ei.value.code == FX_ERROR_UNSUPPORTED and "hyperelastic" in str(ei.value)
    ctx.close()


@pytest.mark.parametrize("name", list(NT.THERMAL_DECKS))
def test_newton_loop_reproduces_the_recorded_decks(hip, oracle, name):
    """fstr_solve_NLGEOM(..., temperature=...) on the recorded cube decks (tests/golden/nl_thermal_decks.npz, the unmodified
    reference program's runs; CG + SSOR to 1e-8 as the decks' !SOLVER card): the Newton count of every sub-step is the recorded one,
    and the Global summaries of every step match at the reference harness's 1e-4.  The Mooney-Rivlin deck is held to the counts
    only: the library adds no thermal load for a hyperelastic element, which moves its converged state
    within CONVERG = 1e-3 (one summary entry at 1.2e-3, printed)."""
    import json
    import os
    from frontistr_amd import fstr
    from oracle import fistr1_run as f1
    from oracle.refrun import default_params
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nl_thermal_decks.npz"))
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    d = NT.THERMAL_DECKS[name]
    model, bc, target = NT.golden_deck(name)
    p = model.parts[0]
    n = model.coord.shape[0]

    class _M:
        coord, n_node = model.coord, n
    case = dict(mesh=_M, groups=[(p["etype"], p["conn"], 4 if p["fbar"] else 2, None)], mats=model.mats, unode=np.zeros(3 * n),
                dunode=np.zeros(3 * n))
    ctx, hecMAT, solid = _solid(hip, case, thermal=False)
    solid.set_thermal(d["ref_temp"], None if d["temp_init"] is None else np.full(n, d["temp_init"]))
    I, Rr = default_params(method=1, precond=1, maxit=5000, tol=1e-8)
    hecMAT.Iarray[:] = I
    hecMAT.Rarray[:] = Rr
    nsub = NT.DECK_SUBSTEPS
    got, bak = [], solid.temperature_at_step_start()
    assert np.array_equal(bak, model.th.temperature)
    solid.set_temperature(bak)
    fstr.fstr_UpdateState(solid)                 # fstr_solve_NLGEOM.f90:96 (what fstr.fstr_solve_NLGEOM does at the start of a step)
    for sub in range(1, nsub + 1):
        ok, log = fstr.fstr_Newton(solid, hecMAT, ((sub - 1) / nsub, sub / nsub), bc, None, 50, NT.DECK_CONVERG,
                                   temperature=bak + (target - bak) * (sub / nsub))
        assert ok
        got.append(log.shape[0])
        st = solid.get_state(("unode", "strain", "stress"))
        diffs = f1.compare_step(NT.H.summary(p["etype"], p["conn"], st["unode"], st["strain"].reshape(p["st"]["strain"].shape),
                                             st["stress"].reshape(p["st"]["stress"].shape)), rlog[len(rlog) - nsub + sub - 1])
        print(name, "sub-step", sub, "summary entries beyond 1e-4:", diffs)
        if d["material"] != "mooney":
            assert diffs == [], sub
    print(name, "Newton iterations per sub-step", got, "reference", newton)
    assert got == newton
    ctx.close()


def test_solve_nlgeom_ramps_the_temperature(hip, oracle):
    """fstr_solve_NLGEOM itself on one recorded deck: the same counts through its own ramp from temp_bak"""
    import json
    import os
    from frontistr_amd import fstr
    from oracle.refrun import default_params
    name = "t361_mises_ic"
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nl_thermal_decks.npz"))
    newton = [int(x) for x in g[name + "/newton"]]
    d = NT.THERMAL_DECKS[name]
    model, bc, target = NT.golden_deck(name)
    p = model.parts[0]
    n = model.coord.shape[0]

    class _M:
        coord, n_node = model.coord, n
    case = dict(mesh=_M, groups=[(p["etype"], p["conn"], 2, None)], mats=model.mats, unode=np.zeros(3 * n), dunode=np.zeros(3 * n))
    ctx, hecMAT, solid = _solid(hip, case, thermal=False)
    solid.set_thermal(d["ref_temp"], np.full(n, d["temp_init"]))
    I, Rr = default_params(method=1, precond=1, maxit=5000, tol=1e-8)
    hecMAT.Iarray[:] = I
    hecMAT.Rarray[:] = Rr
    log = fstr.fstr_solve_NLGEOM(solid, hecMAT, bc, None, 3, 50, NT.DECK_CONVERG, commit_unconverged=False, temperature=target)
    assert [int((log[:, 0] == s).sum()) for s in (1, 2, 3)] == newton
    s = solid.get_state(("istat", "last_temp"))
    assert np.array_equal(s["last_temp"], target) and s["istat"].any()
    ctx.close()
