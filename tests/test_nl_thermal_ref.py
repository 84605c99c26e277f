"""The restatement tests/nl_thermal_ref.py on the CPU: the table lookup at its four places, the thermal update routines against the
existing restatements where the temperature causes no strain, the choice of tt0, commit and snapshot of last_temp, and the
conditions under which the GPU comparison at 1e-11 (tests/test_gpu_nl_thermal.py) means something: float64 against np.longdouble
for the thermal terms, and every Mises point of the GPU cases at least 10 tol away from the yield edge.  And the restatement
itself against the unmodified reference program: the recorded cube decks of tests/golden/nl_thermal_decks.npz."""
import numpy as np
import pytest

import c3_nl_ref as CN
import fbar_ref as FB
import hyper_ref as H
import nl_thermal_ref as NT
import yield_ref as Y

TAB = NT.ELASTIC_TAB


def test_table_lookup_below_above_on_and_between_rows():
    assert np.array_equal(NT.table_lookup(TAB, -5.0), TAB[0, :2])          # below the first row: the first row
    assert np.array_equal(NT.table_lookup(TAB, 300.0), TAB[2, :2])         # at the last row: the last row
    assert np.array_equal(NT.table_lookup(TAB, 1.0e4), TAB[2, :2])         # above it
    assert np.array_equal(NT.table_lookup(TAB, 100.0), TAB[1, :2])         # exactly on a row: lambda = 0 in [row 1, row 2)
    assert np.array_equal(NT.table_lookup(TAB, 0.0), TAB[0, :2])           # on the first row
    got = NT.table_lookup(TAB, 150.0)                                      # between rows 1 and 2: the linear blend
    assert np.allclose(got, [187500.0, 0.3075], rtol=1e-15)
    assert np.array_equal(NT.table_lookup(TAB[:1], 77.0), TAB[0, :2])      # one row: that row
    assert NT.table_lookup(NT.ALPHA_TAB, 50.0)[0] == pytest.approx(1.15e-5, rel=1e-15)


def test_table_lookup_float64_against_longdouble():
    rng = np.random.default_rng(1)
    for tab in (NT.ELASTIC_TAB, NT.ALPHA_TAB):
        for a in rng.uniform(-60.0, 380.0, 200):
            d, q = NT.table_lookup(tab, a), NT.table_lookup(tab.astype(np.longdouble), np.longdouble(a))
            assert np.abs(d - q).max() <= 1e-12 * np.abs(tab[:, :-1]).max()


def test_epsth_float64_against_longdouble():
    """EPSTH of every point temperature pair the GPU table cases can meet, in float64 and in np.longdouble from the same inputs:
    within 1e-12 of the largest entry"""
    rng = np.random.default_rng(2)
    m = NT.material("elastic", "361", tables=True)
    tc, t0 = rng.uniform(-60.0, 380.0, 500), rng.uniform(-60.0, 380.0, 500)
    d = np.array([NT.epsth(m, a, b, NT.REF_TEMP)[0] for a, b in zip(tc, t0)])
    L, tab = np.longdouble, NT.ALPHA_TAB.astype(np.longdouble)
    q = np.array([NT.table_lookup(tab, L(a))[0] * (L(a) - L(NT.REF_TEMP)) - NT.table_lookup(tab, L(b))[0] * (L(b) - L(NT.REF_TEMP))
                  for a, b in zip(tc, t0)])
    assert np.abs(d - q).max() <= 1e-12 * np.abs(q).max()


@pytest.mark.parametrize("fam", NT.FAMILIES)
def test_no_thermal_strain_reproduces_the_existing_restatements(fam, oracle):
    """temperature == temp_init == last_temp == ref_temp: the routines restated here give what c3_nl_ref / hyper_ref / fbar_ref give"""
    case = NT.gpu_case(fam, "two")
    et, m = NT.family_type(fam), case["mesh"]
    flat = np.full(m.n_node, case["ref_temp"])
    case.update(temp_init=flat, last_temp=flat, temperature=flat)
    ref = NT.model_of(case)
    qf = ref.element_update()[0]
    u, du = case["unode"].reshape(-1, 3), case["dunode"].reshape(-1, 3)
    for e, nd in enumerate(m.conn - 1):
        mat = case["mats"][case["elem_mats"][0][e] - 1]
        z6, z1 = np.zeros((H.POINTS[et], 6)), np.zeros(H.POINTS[et])
        if fam == "361f":
            want = FB.update_c3d8fbar(m.coord[nd], u[nd], du[nd], mat, z1, z1.astype(np.int32), z1)[:3]
        elif fam == "361" and not mat.plastic:
            want = H.update_c3d8bbar(m.coord[nd], u[nd] + du[nd], mat)
        elif fam == "361":
            continue                    # Mises B-bar has no numpy restatement without temperatures (the C oracle serves it)
        else:
            want = CN.update_c3(et, m.coord[nd], u[nd], du[nd], mat, z6, z6, z1, z1.astype(np.int32), z1)[:3]
        got = (qf[e], ref.parts[0]["st"]["stress"][e], ref.parts[0]["st"]["strain"][e])
        for a, b, name in zip(got, want, ("qf", "stress", "strain")):
            assert np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1e-300), (fam, e, name)


def test_tt0_is_last_temp_for_elastoplastic_elements_only():
    case = NT.gpu_case("341", "two")
    ref = NT.model_of(case)
    nd = case["mesh"].conn[0] - 1
    el, pl = case["mats"]
    assert np.array_equal(NT.elem_tt0(el, nd, ref.th), case["temp_init"][nd])
    assert np.array_equal(NT.elem_tt0(pl, nd, ref.th), case["last_temp"][nd])
    assert not np.array_equal(case["temp_init"][nd], case["last_temp"][nd])


def test_commit_and_snapshot_of_last_temp(oracle):
    ref = NT.model_of(NT.gpu_case("341", "two"))
    before = ref.th.last_temp.copy()
    ref.snapshot(0)
    ref.element_update()
    ref.commit()
    assert np.array_equal(ref.th.last_temp, ref.th.temperature) and not np.array_equal(before, ref.th.temperature)
    ref.snapshot(1)
    assert np.array_equal(ref.th.last_temp, before)


# every gpu_case variant with an elastoplastic material (UPDATELAG: the STF_C3 types, as in the GPU test)
PLASTIC_CASES = [(f, v) for f in NT.FAMILIES for v in ("two", "tables", "infinite", "yield", "mohr", "updatelag")
                 if v != "updatelag" or f not in ("361", "361f")]


@pytest.mark.parametrize("fam,variant", PLASTIC_CASES)
def test_plastic_points_of_the_gpu_cases_keep_off_the_yield_edge(fam, variant, oracle):
    """Every elastoplastic point of the GPU cases -- Mises, Drucker-Prager, Mohr-Coulomb: |f| of the trial stress at least 10 tol
    from the edges of BackwardEuler's branches (|f| = tol, Elastoplastic.f90:378-383), no return through the `dlambda < 0` reset, for
    Mohr-Coulomb |sin 3 theta| <= 0.95 at the trial and the returned stress and separated principal stresses (yield_ref.margins_hold's
    conditions); and a point yields.  No point is left out."""
    check_plastic_points(NT.gpu_case(fam, variant))


def check_plastic_points(case):
    """the conditions of test_plastic_points_of_the_gpu_cases_keep_off_the_yield_edge on one case (tests/test_nl_shapes.py runs them on
    its meshes too)"""
    fam = "361" if case["groups"][0][0] == 361 else str(case["groups"][0][0])
    ref = NT.model_of(case)
    trial = []
    orig = NT._return_map
    NT._return_map = lambda m, s, p, i, f: (trial.append((m, np.array(s), p)) if NT.is_elastoplastic(m) else None, orig(m, s, p, i, f))[1]
    try:
        ref.element_update()
    finally:
        NT._return_map = orig
    em = case["elem_mats"][0] if case["elem_mats"][0] is not None else np.ones(case["mesh"].conn.shape[0], dtype=np.int32)
    n_pl = sum(1 for e in em if case["mats"][e - 1].plastic) * H.POINTS[NT.family_type(fam)]
    assert len(trial) == n_pl and n_pl > 0
    if Y.is_yield(trial[0][0]):
        reps = [Y.point_report(m, [s]) for m, s, p in trial]
        f = np.array([r["f"][0] for r in reps])
        assert not any(r["reset"][0] for r in reps)
        if trial[0][0].kind == Y.MOHR:
            assert max(abs(r["sin3"][0]) for r in reps) <= 0.95 and max(abs(r["sin3_ret"][0]) for r in reps) <= 0.95
            assert min(r["gap"][0] for r in reps) >= 1.0e-6
    else:
        f = np.array([CN.mises(s) - (m.plconst[0] + m.plconst[1] * p) for m, s, p in trial])
    assert np.all(np.abs(np.abs(f) - Y.TOL) >= 10 * Y.TOL), np.abs(np.abs(f) - Y.TOL).min()
    assert (f > 0).any(), "no point yields"


@pytest.mark.parametrize("name", list(NT.THERMAL_DECKS))
def test_restatement_reproduces_the_recorded_decks(name, oracle):
    """The unmodified reference program's runs (tests/golden/nl_thermal_decks.npz, make_nl_thermal_golden.py): the restatement's
    sub-step loop takes the recorded number of Newton iterations in every sub-step and its Global summaries match every printed
    step at the reference harness's 1e-4"""
    import json
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nl_thermal_decks.npz"))
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    oracle.nl_reset_latch()
    model, bc, target = NT.golden_deck(name)
    nsub = NT.DECK_SUBSTEPS
    bak = model.th.temperature.copy()
    model.th.last_temp = bak.copy()
    its = []
    for sub in range(1, nsub + 1):
        ok, it = model.newton_substep((sub - 1) / nsub, sub / nsub, bc, None, 50, NT.DECK_CONVERG, bak + (target - bak) * (sub / nsub))
        assert ok
        its.append(it)
        assert H.within_1e4(NT.deck_summary(model), rlog[len(rlog) - nsub + sub - 1]) == [], (name, sub)
    assert its == newton


def test_restatement_reproduces_thermal_stress_sample1(oracle):
    """The reference's own examples/static/thermal_stress/sample1 (TYPE=361, !ELASTIC and !EXPANSION_COEFF with DEPENDENCIES=1,
    temperatures read from the eight result files): the recorded Newton count exactly, the Global summaries at 1e-4"""
    import json
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nl_thermal_decks.npz"))
    rlog, newton = json.loads(str(g[NT.SAMPLE1 + "/log"])), [int(x) for x in g[NT.SAMPLE1 + "/newton"]]
    model, bc, temp = NT.sample1_deck()
    assert temp.min() > 25.0 and temp.max() < 550.0 and temp.max() > 400.0        # inside both tables, across several rows
    model.th.last_temp = model.th.temperature.copy()
    ok, it = model.newton_substep(0.0, 1.0, bc, None, 50, NT.SAMPLE1_CONVERG, temp)
    assert ok and [it] == newton
    assert H.within_1e4(NT.deck_summary(model), rlog[-1]) == []


WIDE_CASES = [(f, v) for f in NT.FAMILIES for v in ("one", "two", "tables", "infinite", "yield", "mohr")]


@pytest.mark.parametrize("fam,variant", WIDE_CASES)
def test_update_float64_against_longdouble(fam, variant, oracle):
    """The condition under which the GPU comparison at 1e-11 means something, as tests/test_yield_ref.py states it for its return
    mappings: the restated update of the GPU cases -- ELASTIC, Mises, tables, INFINITE, Drucker-Prager with tables; every family
    -- in float64 and in np.longdouble from the same inputs: stress, strain, fstatus and element forces within 1e-12 of the
    largest entry, the plastic flags equal.  (The Mises material of these cases is UPDATELAG at 361 B-bar, where no stress increment
    is rounded to single precision, and TOTALLAG elsewhere.)"""
    case = NT.gpu_case(fam, variant)
    a, b = NT.model_of(case), NT.model_of(case).widen()
    qa, qb = a.element_update()[0], b.element_update()[0]
    assert qb.dtype == np.longdouble and b.parts[0]["st"]["stress"].dtype == np.longdouble
    for k in ("stress", "strain", "fstat"):
        x, y = a.parts[0]["st"][k], b.parts[0]["st"][k]
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1e-3 if k == "fstat" else 1e-300), (fam, variant, k)
    assert np.abs(qa - qb).max() <= 1e-12 * np.abs(qb).max()
    assert np.array_equal(a.parts[0]["st"]["istat"], b.parts[0]["st"]["istat"])
