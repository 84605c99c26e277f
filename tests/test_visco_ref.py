"""The numpy restatement of the viscoelastic material (tests/visco_ref.py) against what Viscoelastic.f90 defines, and the conditions
under which the 1e-11 comparisons of tests/test_gpu_visco.py mean something, for the inputs those tests use.  No GPU."""
import numpy as np
import pytest

import c3_ref as R
import hyper_ref as H
import visco_ref as V

ETYPES = [361, 341, 342, 351, 352, 362]


def test_hvisc_branches_meet_at_the_switch():
    """the series below 1e-4 and (1 - exp(-x)) / x above it: at the switch the series' truncation error is x^5 / 720 ~ 1e-23 and the
    closed form loses log10(1 / x) = 4 digits to cancellation, so the two agree to 1e-11 there"""
    for x in (0.99e-4, 1.0e-4, 1.01e-4):
        series = 1.0 - 0.5 * x * (1.0 - x / 3.0 * (1.0 - 0.25 * x * (1.0 - 0.2 * x)))
        assert abs(series - (1.0 - np.exp(-x)) / x) < 1e-11
    assert V.hvisc(0.5e-4, np.exp(-0.5e-4)) == 1.0 - 0.5 * 0.5e-4 * (1.0 - 0.5e-4 / 3.0 * (1.0 - 0.25 * 0.5e-4 * (1.0 - 0.2 * 0.5e-4)))
    assert V.hvisc(2.0, np.exp(-2.0)) == (1.0 - np.exp(-2.0)) / 2.0


@pytest.mark.parametrize("rows", list(V.PRONY))
def test_zero_increment_is_the_elastic_material(rows):
    mat = V.gpu_material(rows)
    assert np.array_equal(V.cal_viscoelastic_matrix(mat, 0.0), R.elastic_matrix(mat.E, mat.nu))
    eps = H.random_strains(1, 0.05, 3)[0]
    h = np.full(mat.width, 0.01)
    assert np.array_equal(V.point_stress(mat, eps, h, 0.0), R.elastic_matrix(mat.E, mat.nu) @ eps)
    assert (h == 0.01).all()       # no StressUpdate: the history is not touched


@pytest.mark.parametrize("rows", list(V.PRONY))
@pytest.mark.parametrize("dt", [V.TINCR, V.TINCR_SERIES])
def test_tangent_is_the_derivative_of_the_update(rows, dt):
    """UpdateViscoelastic is linear in the strain: its derivative is calViscoelasticMatrix's D, column by column, to rounding"""
    mat = V.gpu_material(rows)
    rng = np.random.default_rng(5)
    h = rng.uniform(-1, 1, mat.width) * 0.01
    D = V.cal_viscoelastic_matrix(mat, dt)
    s0 = V.update_viscoelastic(mat, np.zeros(6), h.copy(), dt)
    for j in range(6):
        e = np.zeros(6)
        e[j] = 1.0
        col = V.update_viscoelastic(mat, e, h.copy(), dt) - s0
        assert np.abs(col - D[:, j]).max() < 1e-12 * np.abs(D).max(), (j, col, D[:, j])
    assert np.array_equal(D, D.T)
    E0 = R.elastic_matrix(mat.E, mat.nu)
    if dt == V.TINCR:          # softer than the instantaneous response by more than the GPU test's 1e-3
        assert np.abs(D - E0).max() > 1e-3 * np.abs(E0).max()


def test_update_is_idempotent_and_the_state_update_shifts():
    mat = V.gpu_material("three")
    rng = np.random.default_rng(7)
    h = rng.uniform(-1, 1, mat.width) * 0.01
    eps = H.random_strains(1, 0.05, 9)[0]
    h1 = h.copy()
    s1 = V.update_viscoelastic(mat, eps, h1, V.TINCR)
    h2 = h1.copy()
    s2 = V.update_viscoelastic(mat, eps, h2, V.TINCR)
    assert np.array_equal(s1, s2) and np.array_equal(h1, h2)
    nrow = mat.prony.shape[0]
    for n in range(nrow):
        assert np.array_equal(h1[12 * n:12 * n + 6], h[12 * n:12 * n + 6])        # old slots are read only
    V.update_viscoelastic_state(mat, h1, eps)
    for n in range(nrow):
        assert np.array_equal(h1[12 * n:12 * n + 6], h2[12 * n + 6:12 * n + 12])
    th = eps[:3].sum() / 3.0
    assert np.array_equal(h1[12 * nrow:], np.concatenate([eps[:3] - th, eps[3:] * 0.5]))


def test_held_strain_relaxes_to_the_long_term_modulus():
    """a strain applied in the first increment and held: every q_n decays by exp(-dt / tau_n) per increment, the deviatoric stress
    goes to 2 G (1 - sum g_n) dev(eps) and the pressure stays K tr(eps)"""
    mat = V.gpu_material("two")
    eps = np.array([0.01, -0.004, 0.002, 0.006, -0.003, 0.001])
    h = np.zeros(mat.width)
    dt = 5.0
    first = None
    for k in range(60):
        sig = V.update_viscoelastic(mat, eps, h, dt)
        first = sig if first is None else first
        V.update_viscoelastic_state(mat, h, eps)
    G, K = mat.E / (2 * (1 + mat.nu)), mat.E / (3 * (1 - 2 * mat.nu))
    th = eps[:3].sum() / 3.0
    dev = np.concatenate([eps[:3] - th, eps[3:] * 0.5])
    want = 2 * G * (1.0 - mat.prony[:, 0].sum()) * dev
    want[:3] += 3 * K * th
    assert np.abs(sig - want).max() < 1e-9 * np.abs(want).max()
    assert np.abs(first - want).max() > 0.05 * np.abs(want).max()        # and it did relax


def _all_cases():
    """every case tests/test_gpu_visco.py runs: id -> (the Model of the case with its time pair set, displacement amplitude)"""
    out = {}
    for cid, (make, tincr) in V.VISCO_CASES.items():
        def f(make=make, tincr=tincr):
            model = make()[1]
            model.tincr = tincr
            return [model], V.GPU_AMP
        out["visco_" + cid] = f
    for cid, make in V.CREEP_CASES.items():
        out["creep_" + cid] = lambda make=make: ([make()[1]], V.CREEP_AMP)
    for order in (1, 2):
        def g(order=order):
            parts = V.group_case(order)[2].parts
            for p in parts:         # the groups share their nodes: each walks through the two updates on a copy of its own
                p.unode, p.dunode = p.unode.copy(), p.dunode.copy()
            return parts, V.CREEP_AMP
        out["groups_%d" % order] = g
    return out


ALL_CASES = _all_cases()


@pytest.mark.parametrize("cid", list(ALL_CASES))
def test_gpu_inputs_are_well_conditioned(cid):
    """The conditions under which the 1e-11 comparisons of tests/test_gpu_visco.py mean something, for every viscoelastic and NORTON
    point of every case it runs and for both of the stress updates a case makes (visco_ref.case_point_inputs; no point is left out):
    float64 and np.longdouble evaluations agree to 1e-12 of the largest entry (stress, new history, dg); the INFINITE branch rounds
    both to the same default real; every dt / tau of every material of the case sits on its side of hvisc's 1e-4 switch by a factor
    of 10; every NORTON point takes the same number of iterations in both precisions, at most a quarter of the device's cap; and in
    each update at least half of the NORTON points have a creep strain increment above 1e-6 of their elastic strain increment."""
    parts, amp = ALL_CASES[cid]()
    check_conditioning(cid, parts, amp)


def check_conditioning(cid, parts, amp):
    """the conditions of test_gpu_inputs_are_well_conditioned on the Models `parts` of one case (tests/test_nl_shapes.py runs them on
    its meshes too)"""
    ld = np.longdouble
    pts = []
    for model in parts:
        want = sum(model.hist.shape[1] for e in range(model.conn.shape[0]) if V.is_visco(model.mat(e)) or V.is_creep(model.mat(e)))
        got = V.case_point_inputs(model, amp)
        assert len(got) == 2 * want
        pts += got
        for mat in model.mats:
            if V.is_visco(mat):
                x = V.hvisc_arguments(mat, model.tincr)
                assert ((x > 10 * 1e-4) | (x < 1e-4 / 10)).all(), (cid, x)
    assert pts
    s64, sld, h64, hld, inf = [], [], [], [], []
    for kind, mat, eps, h, tincr in [p for p in pts if p[0] == "visco"]:
        a, b = h.copy(), h.astype(ld)
        s64.append(V.update_viscoelastic(mat, eps, a, tincr))
        sld.append(V.update_viscoelastic(mat, eps.astype(ld), b, tincr))
        h64.append(np.abs(a - b).max() / max(np.abs(a).max(), 1e-300))
        inf.append(mat.nlgeom == V.INFINITE)
    if s64:
        s64, sld, inf = np.array(s64), np.array(sld), np.array(inf)
        assert np.abs(s64 - sld).max() < 1e-12 * np.abs(s64).max()
        assert max(h64) < 1e-12
        assert np.abs(s64).max() > 1.0        # not a comparison of zeros
        assert np.array_equal(s64[inf].astype(np.float32), sld[inf].astype(np.float32))
    creep = [p for p in pts if p[0] == "creep"]
    if creep:
        a = [V.update_iso_creep(mat, tr, tincr, time) for _, mat, tr, de, time, tincr in creep]
        b = [V.update_iso_creep(mat, tr.astype(ld), tincr, time) for _, mat, tr, de, time, tincr in creep]
        c64, cld = np.array([x[0] for x in a]), np.array([x[0] for x in b])
        assert np.abs(c64 - cld).max() < 1e-12 * np.abs(c64).max()
        dg64, dgld = np.array([x[1] for x in a]), np.array([x[1] for x in b])
        assert np.abs(dg64 - dgld).max() < 1e-12 * np.abs(dg64).max()
        assert [x[3] for x in a] == [x[3] for x in b]
        its = max(x[3] for x in a)
        assert its <= V.CREEP_CAP // 4
        de = np.array([np.abs(p[3]).max() for p in creep])
        times = np.array([p[4] for p in creep])
        for t in np.unique(times):          # the two updates of the case
            big = dg64[times == t] > 1e-6 * de[times == t]
            print(cid, "time %g: largest iteration count %d, %d of %d points with dg above 1e-6 of the strain increment" % (t, its, big.sum(), big.size))
            assert big.sum() >= big.size / 2


def test_model_newton_converges_with_a_time_increment():
    """the sub-step loop of a small cube under a held top-face displacement: Newton converges in every increment with the viscoelastic
    tangent, and the reaction relaxes from increment to increment"""
    m, _, _, bc = H.golden_deck("h341_neohooke")
    model = V.Model(m.etype, m.coord, m.conn, V.gpu_material("two", V.TOTALLAG))
    model.tincr = V.TINCR
    ok, it = model.newton_substep(0.0, 1.0, bc, None, 20, 1e-6)
    assert ok and it <= 6
    q0 = np.abs(model.qforce).max()
    hold = (bc[0], bc[1], np.zeros_like(bc[2]))
    for k in range(3):
        ok, it = model.newton_substep(0.0, 1.0, hold, None, 20, 1e-6)
        assert ok
    assert np.abs(model.qforce).max() < 0.95 * q0


# ---- NORTON ------------------------------------------------------------------------------------------------------------------------------
def test_creep_tangent_softens_the_deviatoric_response():
    """iso_creep at a relaxed state: symmetric, the elastic matrix in the volumetric direction (creep is isochoric: the terms it adds
    annihilate the unit tensor), softer along the stress deviator"""
    mat = V.creep_material()
    D = R.elastic_matrix(mat.E, mat.nu)
    e0 = np.array([1.5e-3, -0.4e-3, 0.2e-3, 0.9e-3, -0.5e-3, 0.3e-3])
    t, dt = V.CREEP_TIME, 50 * V.CREEP_TINCR
    s, dg, eqvs, it = V.update_iso_creep(mat, D @ e0, dt, t)
    assert dg > 1e-3 * np.abs(e0).max()
    Dc = V.iso_creep(mat, s, dg, dt, t)
    assert np.abs(Dc - Dc.T).max() < 1e-12 * np.abs(D).max()
    one = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    assert np.abs((Dc - D) @ one).max() < 1e-10 * np.abs(D).max()
    dev = s - one * s[:3].mean()
    assert dev @ Dc @ dev < 0.9 * (dev @ D @ dev)


def test_creep_zero_increment_and_zero_stress_are_elastic():
    mat = V.creep_material()
    s = np.array([300.0, -20.0, 10.0, 40.0, 5.0, -60.0])
    assert np.array_equal(V.iso_creep(mat, s, 1e-5, 0.0, 1.0), R.elastic_matrix(mat.E, mat.nu))
    assert np.array_equal(V.iso_creep(mat, np.zeros(6), 1e-5, 1.0, 1.0), R.elastic_matrix(mat.E, mat.nu))
    out = V.creep_point(mat, s, 1e-5, 7.0, 0.0, 1.0)
    assert out[0] is s and out[1:] == (1e-5, 7.0)
    z = np.zeros(6)
    assert V.creep_point(mat, z, 1e-5, 7.0, 1.0, 1.0)[0] is z


def test_hydrostatic_stress_does_not_end_the_reference_loop():
    """dstri = 0: eqvs = 0, df = 0 / 0, dg is NaN and neither exit test is ever true -- the reference spins; the restatement raises, the
    device stops the point after its bounded loop with FX_ERROR_RUNTIME"""
    with pytest.raises(V.CreepSpins):
        V.update_iso_creep(V.creep_material(), np.array([100.0, 100.0, 100.0, 0.0, 0.0, 0.0]), 1.0e-6, 0.0)


def test_creep_model_sets_the_latch_and_accumulates():
    m, model = V.creep_case(341)
    model.tincr = 0.0
    model.element_update()
    assert model.latch == 1                 # even at tincr = 0
    m, model = V.creep_case(341)
    acc = model.hist[..., 1].copy()
    model.element_update()
    assert np.array_equal(model.hist[..., 0], model.st["fstat"])
    model.commit()
    assert np.array_equal(model.hist[..., 1], acc + model.st["plstrain"])


# ---- the recorded runs of the unmodified reference program ------------------------------------------------------------------------------
def run_deck(name, model_hook=None):
    """the restatement's sub-step loop over a recorded cube deck -> (Newton counts, summaries per sub-step, model)"""
    m, mats, em, bc, dt, fbar = V.golden_deck(name)
    model = V.Model(m.etype, m.coord, m.conn, mats, em, fbar=fbar)
    counts, sums = [], []
    for share, time, tincr in V.deck_schedule(name):
        model.time, model.tincr = time, tincr
        ok, it = model.newton_substep(0.0, share, bc, None, 50, V.DECK_CONVERG)
        assert ok, (name, time)
        counts.append(it)
        sums.append(V.summary(m.etype, m.conn, model.unode, model.st["strain"], model.st["stress"]))
    return counts, sums, model


@pytest.mark.parametrize("name", list(V.GOLDEN_DECKS))
def test_restatement_reproduces_the_recorded_decks(name):
    """Newton counts of every sub-step exactly, the Global summaries of every printed step at the harness's 1e-4; and the creep
    iteration of every NORTON point of every deck stays within a quarter of the device's cap"""
    import json
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visco_decks.npz"))
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    V.CREEP_ITERATIONS.clear()
    counts, sums, model = run_deck(name)
    print(name, "Newton", counts, "recorded", newton, "largest creep iteration count", max(V.CREEP_ITERATIONS + [0]))
    assert counts == newton
    for k, s in enumerate(sums):
        assert V.within_1e4(s, rlog[len(rlog) - len(sums) + k]) == [], (name, k)
    assert max(V.CREEP_ITERATIONS + [0]) <= V.CREEP_CAP // 4
    if "norton" in name:
        assert model.latch == 1 and V.CREEP_ITERATIONS


@pytest.mark.parametrize("name", list(V.ONE_ELEM_DECKS))
def test_restatement_reproduces_the_reference_one_element_decks(name):
    """examples/static/1elem/{viscoe,viscof,relax,creep}: Newton counts exactly and the summaries of every converged sub-step at 1e-4.
    relax is the only record whose time exponent m is not zero (-0.2): aa = A ((t + dt)**0.8 - t**0.8) / 0.8 with t the time at the START
    of the increment, from 1.0 on -- the end of the increment in its place changes aa by 1.6 % in the first one, the two arguments
    swapped by orders of magnitude.  creep: the unmodified program runs into ITMAX = 20 in the first VISCO increment, and so does
    the restatement; its load stays whole there because the group was active in the STATIC step (fstr_ass_load.f90:69-70)."""
    import json
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visco_decks.npz"))
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    V.CREEP_ITERATIONS.clear()
    counts, sums, finished = V.run_one_elem_deck(name)
    print(name, "Newton", counts, "recorded", newton, "largest creep iteration count", max(V.CREEP_ITERATIONS + [0]))
    assert counts == newton
    assert finished == (name != "1elem_creep")
    assert len(rlog) == len(sums) + 1          # 0.log opens with the summary of the initial state
    for k, s in enumerate(sums):
        assert V.within_1e4(s, rlog[1 + k]) == [], (name, k)
    assert max(V.CREEP_ITERATIONS + [0]) <= V.CREEP_CAP // 4


def test_relax_deck_tells_the_time_readings_apart():
    """what the test above rests on: with the end of the increment for ttime, or with time and increment swapped, the restatement no
    longer reproduces the record of 1elem/relax"""
    import json
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visco_decks.npz"))
    rlog = json.loads(str(g["1elem_relax/log"]))
    keep = V.creep_aa
    try:
        for wrong in (lambda m, t, dt, dtype=np.float64: keep(m, t + dt, dt, dtype), lambda m, t, dt, dtype=np.float64: keep(m, dt, t, dtype)):
            V.creep_aa = wrong
            counts, sums, finished = V.run_one_elem_deck("1elem_relax")
            assert any(V.within_1e4(s, rlog[1 + k]) for k, s in enumerate(sums)) or not finished
    finally:
        V.creep_aa = keep
