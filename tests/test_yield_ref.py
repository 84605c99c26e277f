"""The numpy restatement of the Mohr-Coulomb and Drucker-Prager materials (tests/yield_ref.py) against the unmodified reference
program, and the conditions under which the GPU comparisons at 1e-11 mean something.

(a) Recorded decks.  tests/golden/yield_decks.npz (make_yield_golden.py) holds what fistr1 built from the unmodified reference
    computed on its own examples/static/1elem/{drucker,mohr,mohrshear}, and on cube decks of every solid type and both yield functions:
    the Newton count of every sub-step and the printed Global summaries.  Model reproduces the counts exactly and the summaries at the
    reference harness's 1e-4 (hyper_ref.within_1e4).  This is what pins the places where the reference disagrees with itself.
    tutorial/06_plastic_can is recorded too but not restated: 14 000 nodes and pressure loads are outside a dense numpy loop; the
    GPU test of fistr1 runs it against the record.
(b) Conditioning and margins.  The GPU tests compare stress, fstat and the tangent at the project's nonlinear 1e-11 of the largest
    entry.  That needs the restated values to be determined to better than that by their float64 inputs: evaluated in float64 and
    in np.longdouble from the same trial stresses they agree to 1e-12 of the largest entry.  A point on a branch edge would break
    that whatever the arithmetic (the branch is taken on one side and not on the other), so the inputs were constructed
    (yield_ref.search_gpu_case) to keep every point away from every edge, and this test asserts the margins as conditions:
    | |f| - tol | >= 10 tol, no return through the `dlambda < 0` reset, and for Mohr-Coulomb |sin 3 theta| <= 0.95 (trial and
    returned stress) with principal stresses separated by 1e-6 of the largest; at least a quarter of the points plastic and a tenth
    elastic.  No point is left out.
    (These inputs stay off the edges on purpose.  The edges are run separately, on trial stresses that sit exactly on them, where
    the branch is the same in every arithmetic: tests/point_ref.py holds the cases, tests/test_point_ref.py their conditions.)
"""
import json
import os

import numpy as np
import pytest

import yield_ref as Y

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
TYPES = [361, 341, 342, 351, 352, 362]


def _golden():
    return np.load(os.path.join(HERE, "golden", "yield_decks.npz"))


def test_constants_are_the_cards():
    """fstr_ctrl_get_PLASTICITY :451-469 with its own PI"""
    m = Y.mohr_coulomb(1.0, 0.0, 500.0, 20.0, 7.0)
    assert m.plconst == (500.0, 7.0, 20.0 * 3.14159265358979 / 180.0) and m.plconst4 == 0.0
    d = Y.drucker_prager(1.0, 0.0, 500.0, 20.0, 7.0)
    phi = 20.0 * 3.14159265358979 / 180.0
    assert d.plconst[2] == 2.0 * np.sin(phi) / (np.sqrt(3.0) * (3.0 + np.sin(phi)))
    assert d.plconst4 == 6.0 * np.cos(phi) / (np.sqrt(3.0) * (3.0 + np.sin(phi)))


def test_python_materials_are_the_parsed_ones():
    """tMaterial.mohr_coulomb / drucker_prager compute phi, eta and xi as fstr_ctrl_get_PLASTICITY does: equal to yield_ref's, bit for bit"""
    from frontistr_amd import fstr      # builds the views only: no device, no library call
    a, b = fstr.tMaterial.mohr_coulomb(2.0e4, 0.3, 300.0, 25.0, 400.0), Y.mohr_coulomb(2.0e4, 0.3, 300.0, 25.0, 400.0)
    assert a.kind == fstr.MOHRCOULOMB == 4 and a.plconst == b.plconst and a.plconst4 == 0.0 and a.nlgeom_flag == fstr.UPDATELAG
    a, b = fstr.tMaterial.drucker_prager(2.0e4, 0.3, 300.0, 25.0, 400.0, nlgeom_flag=fstr.TOTALLAG), Y.drucker_prager(2.0e4, 0.3, 300.0, 25.0, 400.0)
    assert a.kind == fstr.DRUCKERPRAGER == 5 and a.plconst == b.plconst and a.plconst4 == b.plconst4 and a.nlgeom_flag == fstr.TOTALLAG
    v = a.view()
    assert v.plastic == 5 and v.harden == 0 and v.plconst4 == b.plconst4 and list(v.plconst) == list(b.plconst)


def test_eigen3_is_an_eigen_decomposition():
    rng = np.random.default_rng(3)
    for _ in range(20):
        t = rng.uniform(-1, 1, 6) * 1.0e3
        ev, pr = Y.eigen3(t)
        A = np.array([[t[0], t[3], t[5]], [t[3], t[1], t[4]], [t[5], t[4], t[2]]])
        assert np.abs(pr @ np.diag(ev) @ pr.T - A).max() <= 1e-12 * np.abs(A).max()
        assert np.abs(pr.T @ pr - np.eye(3)).max() <= 1e-14
        assert np.abs(np.sort(ev) - np.linalg.eigvalsh(A)).max() <= 1e-12 * np.abs(A).max()
    ev, pr = Y.eigen3(np.array([3.0, 1.0, 2.0, 0.0, 0.0, 0.0]))      # diagonal: returned at once, in the given order
    assert ev.tolist() == [3.0, 1.0, 2.0] and np.array_equal(pr, np.eye(3))


@pytest.mark.parametrize("family", ["drucker", "mohr"])
def test_returned_stress_is_on_the_surface_the_return_iterates_on(family):
    """The Drucker-Prager return ends on sqrt(J2) + eta p - xi (c + H pl) = 0 with p the MEAN stress; the Mohr-Coulomb return on the
    principal-stress form -- not on calYieldFunc's surface, which is why a returned point is found `yielded` again."""
    mat = Y.gpu_material(family, Y.INFINITE, Y.GPU_CASES[(361, family)][1])
    rep = Y.point_report(mat, Y.trial_stresses(361, family, Y.INFINITE))
    c, Hd, p3 = mat.plconst
    for s, fs, ist in zip(rep["stress"], rep["fstat"], rep["istat"]):
        if not ist:
            continue
        if family == "drucker":
            p = (s[0] + s[1] + s[2]) / 3.0
            d = np.array([s[0] - p, s[1] - p, s[2] - p, s[3], s[4], s[5]])
            f = np.sqrt(0.5 * d[:3] @ d[:3] + d[3:] @ d[3:]) + p3 * p - mat.plconst4 * (c + Hd * fs)
            assert abs(f) < Y.TOL ** 2 + 1e-9
            assert Y.cal_yield_func(mat, s, fs) > Y.TOL or p <= 0.0
        else:
            pr = np.sort(np.linalg.eigvalsh(np.array([[s[0], s[3], s[5]], [s[3], s[1], s[4]], [s[5], s[4], s[2]]])))
            assert fs > 0.0 and pr[2] - pr[0] > 0.0


@pytest.mark.parametrize("family", ["drucker", "mohr"])
@pytest.mark.parametrize("etype", TYPES)
def test_gpu_inputs_are_well_conditioned(etype, family):
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    for nlgeom in (Y.INFINITE, Y.TOTALLAG, Y.UPDATELAG):
        _, mat, _, _ = Y.gpu_case(etype, family, nlgeom)
        check_points(mat, Y.trial_stresses(etype, family, nlgeom), "%d %s nlgeom %d" % (etype, family, nlgeom))


def check_points(mat, trial, tag):
    """the margins and the float64 / long double agreement of test_gpu_inputs_are_well_conditioned on the trial stresses of one
    material (tests/test_nl_shapes.py runs them on its meshes too)"""
    family = "mohr" if mat.kind == Y.MOHR else "drucker"
    rep = Y.point_report(mat, trial)
    # ---- the margins, as conditions
    assert np.all(np.abs(np.abs(rep["f"]) - Y.TOL) >= 10 * Y.TOL), "a point within 10 tol of the |f| < tol edge"
    assert not rep["reset"].any(), "a return ended through the dlambda < 0 reset"
    if family == "mohr":
        assert np.abs(rep["sin3"]).max() <= 0.95 and np.abs(rep["sin3_ret"]).max() <= 0.95
        assert rep["gap"].min() >= 1.0e-6
    plastic = rep["istat"].mean()
    assert plastic >= 0.25 and 1.0 - plastic >= 0.10, plastic
    assert Y.margins_hold(mat, rep)
    # ---- float64 against long double from the same trial stresses
    smax, dmax = np.abs(rep["stress"]).max(), np.abs(rep["tangent"]).max()
    fmax = np.abs(rep["fstat"]).max()
    worst = [0.0, 0.0, 0.0]
    for k, s in enumerate(trial):
        sl, il, fl = Y.backward_euler(mat, s.astype(np.longdouble), 0.0, 0, np.longdouble(0))
        Dl = Y.elastoplastic_matrix(mat, sl, il, fl)
        assert sl.dtype == np.longdouble and Dl.dtype == np.longdouble and il == rep["istat"][k]
        worst[0] = max(worst[0], float(np.abs(sl - rep["stress"][k]).max()) / smax)
        worst[1] = max(worst[1], abs(float(fl) - rep["fstat"][k]) / fmax)
        worst[2] = max(worst[2], float(np.abs(Dl - rep["tangent"][k]).max()) / dmax)
    print("%s: %d points, %.0f %% plastic, min ||f| - tol| %.3g, float64 vs long double: stress %.1e fstat %.1e tangent %.1e"
          % (tag, len(trial), 100 * plastic, np.abs(np.abs(rep["f"]) - Y.TOL).min(), *worst))
    assert max(worst) <= 1e-12


@pytest.mark.parametrize("etype", [361, 342, 352])
def test_mixed_section_inputs_meet_the_margins(etype):
    """The inputs of the mixed-section GPU comparisons (yield_ref.mixed_case): the Drucker-Prager SUBSET of the deal meets the margins
    and the shares of the single-material cases, and every point of the Mises section is 10 tol away from the |f| < tol edge of its
    own return, with a tenth of them on either side (its return cannot end through `dlambda < 0`: see yield_ref)."""
    mat, rep, fm = Y.mixed_report(etype)
    assert np.all(np.abs(np.abs(rep["f"]) - Y.TOL) >= 10 * Y.TOL) and not rep["reset"].any()
    plastic = rep["istat"].mean()
    assert plastic >= 0.25 and 1.0 - plastic >= 0.10, plastic
    assert np.all(np.abs(np.abs(fm) - Y.TOL) >= 10 * Y.TOL), "a Mises point within 10 tol of the |f| < tol edge"
    assert (fm > 0).mean() >= 0.10 and (fm < 0).mean() >= 0.10
    print("%d: Drucker-Prager subset %d points, %.0f %% plastic, min ||f| - tol| %.3g; Mises subset %d points, %.0f %% plastic, min ||f| - tol| %.3g"
          % (etype, len(rep["f"]), 100 * plastic, np.abs(np.abs(rep["f"]) - Y.TOL).min(), len(fm), 100 * (fm > 0).mean(),
             np.abs(np.abs(fm) - Y.TOL).min()))
    assert Y.mixed_margins_hold(mat, rep, fm)
    # the restated update of the mixed model agrees with these reports point by point
    m, mats, em, unode, dunode = Y.mixed_case(etype, "mises")
    ref = Y.Model(etype, m.coord, m.conn, mats, em)
    ref.unode[:], ref.dunode[:] = unode, dunode
    ref.element_update()
    assert np.array_equal(ref.st["istat"][em == 1].ravel(), rep["istat"]) and np.array_equal(ref.st["istat"][em == 2].ravel() != 0, fm > 0)
    # float64 against long double on the Drucker-Prager subset
    if np.finfo(np.longdouble).eps < EPS:
        trial = Y.trial_stresses(etype, "drucker", Y.UPDATELAG, Y.MIXED_CASES[etype][0], 1.0).reshape(m.n_elem, -1, 6)[em == 1].reshape(-1, 6)
        smax, dmax = np.abs(rep["stress"]).max(), np.abs(rep["tangent"]).max()
        for k, s in enumerate(trial):
            sl, il, fl = Y.backward_euler(mat, s.astype(np.longdouble), 0.0, 0, np.longdouble(0))
            Dl = Y.elastoplastic_matrix(mat, sl, il, fl)
            assert il == rep["istat"][k] and float(np.abs(sl - rep["stress"][k]).max()) <= 1e-12 * smax
            assert float(np.abs(Dl - rep["tangent"][k]).max()) <= 1e-12 * dmax


def test_both_mohr_coulomb_tangent_branches():
    """The two one-element inputs of the GPU test: an exactly uniaxial state takes C1 = 0, C2 = sqrt 3, C3 = 0, a generic one the
    trigonometric branch."""
    for generic, want in ((False, "edge"), (True, "trig")):
        mat, unode = Y.branch_case(generic)
        ref = Y.Model(361, Y.ONE_ELEM_COORD, Y.ONE_ELEM_CONN, mat)
        ref.dunode[:] = unode
        ref.element_update()
        assert ref.st["istat"].all() == generic and ref.st["istat"].any() == generic
        for s, fs in zip(ref.st["stress"][0], ref.st["fstat"][0]):
            info = {}
            Y.elastoplastic_matrix(mat, s, 1, fs, info)
            assert info["branch"] == want, info
            assert generic or abs(abs(info["sin3"]) - 1.0) < 1e-12
            assert not generic or abs(info["sin3"]) <= 0.95


def test_stop_conditions_raise():
    mat = Y.mohr_coulomb(1.0e5, 0.0, 500.0, 20.0)
    with pytest.raises(Y.MathError, match="Mohr-Coulomb"):
        Y.elastoplastic_matrix(mat, Y.STOP_STRESS, 1, 0.0)
    with pytest.raises(Y.MathError, match="Mohr-Coulomb"):
        Y.cal_yield_func(mat, Y.STOP_STRESS, 0.0)


@pytest.mark.parametrize("name", list(Y.ONE_ELEM_DECKS))
def test_recorded_1elem_decks(name):
    g = _golden()
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    mat, bc = Y.one_elem_deck(name)
    ref = Y.Model(361, Y.ONE_ELEM_COORD, Y.ONE_ELEM_CONN, mat)
    ok, it = ref.newton_substep(0.0, 1.0, bc, None, 50, Y.ONE_ELEM_CONVERG)
    assert ok
    got = [it]
    s = Y.summary(361, Y.ONE_ELEM_CONN, ref.unode, ref.st["strain"], ref.st["stress"])
    bad = Y.within_1e4(s, rlog[-1])
    assert bad == [], bad
    assert got == newton, (got, newton)
    assert ref.st["istat"].all(), "the deck does not yield"


@pytest.mark.parametrize("name", list(Y.GOLDEN_DECKS))
def test_recorded_cube_decks(name):
    g = _golden()
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    m, mats, em, bc = Y.golden_deck(name)
    ref = Y.Model(m.etype, m.coord, m.conn, mats, em)
    nsub, got = Y.DECK_SUBSTEPS, []
    for sub in range(1, nsub + 1):
        ok, it = ref.newton_substep((sub - 1) / nsub, sub / nsub, bc, None, 50, Y.DECK_CONVERG)
        assert ok
        got.append(it)
        s = Y.summary(m.etype, m.conn, ref.unode, ref.st["strain"], ref.st["stress"])
        bad = Y.within_1e4(s, rlog[len(rlog) - nsub + sub - 1])
        assert bad == [], (sub, bad)
    assert got == newton, (got, newton)
    assert ref.st["istat"].any()


def test_tutorial_06_is_on_record():
    g = _golden()
    assert [int(x) for x in g["t06_can/newton"]] == [2] * 10 and len(json.loads(str(g["t06_can/log"]))) == 11
    with open(os.path.join(HERE, "golden", "yield_not_converging.json")) as fh:
        assert json.load(fh) == {}, "every reference deck completed in the unmodified program"
