"""The numpy restatement of the F-bar hexahedron (tests/fbar_ref.py) against the reference program's own runs and against what the
formulation has to satisfy; and the conditioning of the inputs that tests/test_gpu_fbar.py compares the device kernels on.  No GPU."""
import json
import os

import numpy as np
import pytest

import fbar_ref as F
import hyper_ref as H
import yield_ref as Y

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps


def _golden():
    return np.load(os.path.join(HERE, "golden", "nl_fbar_decks.npz"))


@pytest.mark.parametrize("name", list(F.GOLDEN_DECKS))
def test_recorded_cube_decks(name):
    """The restatement's dense-solve Newton loop on the cube decks the unmodified reference program ran with FORM361=FBAR
    (tests/golden/nl_fbar_decks.npz): the Newton count of every sub-step and the Global summaries of every printed step at the reference
    harness's 1e-4."""
    from oracle import fistr1_run as f1
    g = _golden()
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    m, mats, em, bc = F.golden_deck(name)
    ref = F.Model(m.coord, m.conn, mats, em)
    nsub, got = F.DECK_SUBSTEPS, []
    for sub in range(1, nsub + 1):
        ok, it = ref.newton_substep((sub - 1) / nsub, sub / nsub, bc, None, 50, F.DECK_CONVERG)
        assert ok
        got.append(it)
        s = F.summary(361, m.conn, ref.unode, ref.st["strain"], ref.st["stress"])
        bad = f1.compare_step(s, rlog[len(rlog) - nsub + sub - 1])
        assert bad == [], (sub, bad)
    assert got == newton, (got, newton)


def test_recorded_decks_differ_from_bbar():
    """The recorded F-bar numbers are not the B-bar ones of the same cube and material (tests/golden/hyper_decks.npz): the decks tell
    the two formulations apart at the harness's 1e-4."""
    from oracle import fistr1_run as f1
    g, b = _golden(), np.load(os.path.join(HERE, "golden", "hyper_decks.npz"))
    for mat in ("neohooke", "mooney", "arruda"):
        fl, bl = json.loads(str(g["f361_%s/log" % mat])), json.loads(str(b["h361_%s/log" % mat]))
        assert f1.compare_step(fl[-1], bl[-1]) != [], mat


def test_t01_beam_hyperelastic():
    """examples/static/FbarElement/T01_BEAM_HYPERELASTIC: the Newton count at CONVERG = 1e-10 (seven: a wrong tangent takes more) and
    the Global summaries against the recorded run and against the deck's own _correct.log."""
    from oracle import fistr1_run as f1
    g = _golden()
    rlog, newton = json.loads(str(g["T01_BEAM_HYPERELASTIC/log"])), [int(x) for x in g["T01_BEAM_HYPERELASTIC/newton"]]
    coord, conn, mat, bc, cload = F.t01_deck()
    ref = F.Model(coord, conn, mat)
    ok, it = ref.newton_substep(0.0, 1.0, bc, cload, F.T01_MAXITER, F.T01_CONVERG)
    assert ok and [it] == newton, (ok, it, newton)
    s = F.summary(361, conn, ref.unode, ref.st["strain"], ref.st["stress"])
    assert f1.compare_step(s, rlog[-1]) == []
    correct = f1.read_log(os.path.join(HERE, "golden", "decks", "static", "FbarElement", "T01_BEAM_HYPERELASTIC_correct.log"))
    assert f1.compare_step(s, correct[-1]) == []


def _one_element(seed=3):
    rng = np.random.default_rng(seed)
    ec = Y.ONE_ELEM_COORD + 0.1 * rng.uniform(-1, 1, (8, 3))
    return ec, rng


MATS = {"elastic_inf": lambda: _elastic(F.INFINITE), "elastic_tl": lambda: _elastic(F.TOTALLAG), "mooney": H.TEST_MATERIALS["mooney"],
        "arruda": H.TEST_MATERIALS["arruda"]}


def _elastic(flag):
    from oracle.refrun import Material
    return Material(2.5, 0.3, nlgeom=flag)


def _plain_totallag(ec, u, mat):
    """Strain, stress and internal force of the plain total-Lagrange hexahedron from F = I + grad u at every point: no averaging"""
    qf, stress, strain = np.zeros(24), np.zeros((8, 6)), np.zeros((8, 6))
    for q in range(8):
        gd, det = H._hex8_gderiv(ec, H.HEX8_POINTS[q])
        Fd = np.eye(3) + u.T @ gd
        C = Fd.T @ Fd
        e = np.array([0.5 * (C[0, 0] - 1), 0.5 * (C[1, 1] - 1), 0.5 * (C[2, 2] - 1), C[0, 1], C[1, 2], C[2, 0]])
        s = H.stress_update(mat, e) if H.kind_of(mat) >= H.MOONEY else F._elastic_matrix(mat, np.dtype(np.float64)) @ e
        S = np.array([[s[0], s[3], s[5]], [s[3], s[1], s[4]], [s[5], s[4], s[2]]])
        qf += (gd @ (Fd @ S).T).ravel() * det          # P = F S, f_a = P grad N_a
        strain[q], stress[q] = e, s
    return qf, stress, strain


@pytest.mark.parametrize("name", ["elastic_tl", "mooney", "arruda"])
def test_affine_field_gives_the_plain_total_lagrange_numbers(name):
    """On an affine displacement field every point has the same jacob, so Jratio = 1 and gderiv1_ave = gderiv1 in the mean: strain,
    stress and internal force are those of F = I + G at every point."""
    ec, rng = _one_element()
    G = 0.1 * rng.uniform(-1, 1, (3, 3))
    u = ec @ G.T
    mat = MATS[name]()
    _, _, jr, _, _ = F.averages(ec, u, F.TOTALLAG)
    assert np.abs(jr - 1.0).max() < 50 * EPS
    z = np.zeros(8)
    qf, stress, strain, _, _ = F.update_c3d8fbar(ec, u, np.zeros_like(u), mat, z, z.astype(np.int32), z)
    pq, ps, pe = _plain_totallag(ec, u, mat)
    assert np.abs(strain - pe).max() <= 1e-13 * max(np.abs(pe).max(), 1.0)
    assert np.abs(stress - ps).max() <= 1e-12 * np.abs(ps).max()
    assert np.abs(qf - pq).max() <= 1e-12 * np.abs(pq).max()


@pytest.mark.parametrize("name", ["elastic_tl", "mooney", "arruda"])
def test_rigid_rotation_gives_zero_strain(name):
    ec, rng = _one_element()
    a = 0.7
    Rm = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ np.array(
        [[1.0, 0.0, 0.0], [0.0, np.cos(0.4), -np.sin(0.4)], [0.0, np.sin(0.4), np.cos(0.4)]])
    u = ec @ Rm.T - ec + np.array([0.3, -0.2, 0.1])
    z = np.zeros(8)
    qf, stress, strain, _, _ = F.update_c3d8fbar(ec, u, np.zeros_like(u), MATS[name](), z, z.astype(np.int32), z)
    assert np.abs(strain).max() < 1e-14
    scale = np.abs(F._material_matrix(MATS[name](), 0, np.zeros(6), np.zeros(6), 0, 0.0, np.dtype(np.float64))).max()
    assert np.abs(stress).max() < 1e-13 * scale and np.abs(qf).max() < 1e-13 * scale


@pytest.mark.parametrize("name", list(MATS))
def test_element_tangent_is_symmetric(name):
    m, mat, unode, dunode = F.elastic_case("mooney")
    mat = MATS[name]()
    ref = F.Model(m.coord, m.conn, mat)
    ref.unode[:], ref.dunode[:] = unode, dunode
    for when in ("before", "after"):
        K = ref.element_tangents()
        assert np.abs(K - K.transpose(0, 2, 1)).max() <= 1e-14 * np.abs(K).max(), when
        ref.element_update()


def test_updatelag_is_not_restated():
    ec, _ = _one_element()
    z = np.zeros(8)
    with pytest.raises(ValueError, match="600-602"):
        F.update_c3d8fbar(ec, np.zeros((8, 3)), np.zeros((8, 3)), _elastic(F.UPDATELAG), z, z.astype(np.int32), z)


def test_too_small_volume_stops():
    ec = Y.ONE_ELEM_COORD * 1.0e-5          # V0 = 1e-15
    z = np.zeros(8)
    with pytest.raises(F.TooSmall, match="too small element volume"):
        F.stf_c3d8fbar(ec, np.zeros((8, 3)), _elastic(F.TOTALLAG), 0, np.zeros((8, 6)), np.zeros((8, 6)), z, z)


# ---- the inputs of tests/test_gpu_fbar.py -------------------------------------------------------------------------------------------------
GPU_ELASTIC = [("elastic", F.INFINITE), ("elastic", F.TOTALLAG), ("neohooke", F.TOTALLAG), ("mooney", F.TOTALLAG), ("arruda", F.TOTALLAG)]


def _longdouble_model(m, mat, unode, dunode, elems=None):
    """mat: one material, or a function of the element index; elems: these elements only (tests/test_nl_shapes.py: a section)"""
    ld = np.longdouble
    coord, u, du = m.coord.astype(ld), unode.astype(ld).reshape(-1, 3), dunode.astype(ld).reshape(-1, 3)
    z = np.zeros(8)
    out = dict(k0=[], qf=[], stress=[], strain=[], k1=[])
    mat_of = mat if callable(mat) else (lambda e: mat)
    for e in (range(m.conn.shape[0]) if elems is None else elems):
        nd, mat = m.conn[e] - 1, mat_of(e)
        out["k0"].append(F.stf_c3d8fbar(coord[nd], u[nd] + du[nd], mat, 0, np.zeros((8, 6), dtype=ld), np.zeros((8, 6), dtype=ld), z, z))
        qf, s, e, _, _ = F.update_c3d8fbar(coord[nd], u[nd], du[nd], mat, z, z.astype(np.int32), z)
        out["k1"].append(F.stf_c3d8fbar(coord[nd], u[nd] + du[nd], mat, 0, e, s, z, z))
        out["qf"].append(qf); out["stress"].append(s); out["strain"].append(e)
    return {k: np.array(v) for k, v in out.items()}


@pytest.mark.parametrize("name,flag", GPU_ELASTIC, ids=["%s_%d" % c for c in GPU_ELASTIC])
def test_gpu_inputs_are_well_conditioned(name, flag):
    """float64 against long double on the elements of the GPU comparisons (hyper_ref.gpu_mesh(361), which holds a collapsed hexahedron,
    random_displacement at hyper_ref.GPU_AMP): tangents before and after the update, stresses and internal forces are determined to
    1e-12 of the largest entry."""
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    m, mat, unode, dunode = F.elastic_case(name, flag)
    ref = F.Model(m.coord, m.conn, mat)
    ref.unode[:], ref.dunode[:] = unode, dunode
    got = dict(k0=ref.element_tangents())
    got["qf"] = ref.element_update()
    got.update(stress=ref.st["stress"], strain=ref.st["strain"], k1=ref.element_tangents())
    want = _longdouble_model(m, mat, unode, dunode)
    assert np.abs(ref.st["strain"]).max() > 0.02, "the inputs do not strain the material"
    check_against_longdouble(got, want, "%s %d" % (name, flag))


def check_against_longdouble(got, want, tag):
    for k, w in want.items():
        assert w.dtype == np.longdouble
        err = float(np.abs(got[k] - w).max() / np.abs(w).max())
        print("%s %s: float64 vs long double %.2e" % (tag, k, err))
        assert err <= 1e-12, (k, err)


@pytest.mark.parametrize("flag", [F.INFINITE, F.TOTALLAG], ids=["infinite", "totallag"])
@pytest.mark.parametrize("family", ["mises", "drucker", "mohr"])
def test_plastic_gpu_inputs_keep_off_the_branch_edges(family, flag):
    """The plastic comparisons: the trial stresses are determined to 1e-12 (float64 against long double), every point keeps the margins
    of yield_ref from the edges of its return mapping, at least a quarter of the points are plastic after the update and a tenth
    stay elastic."""
    seed, c = F.PLASTIC_CASES[family]
    trial = F.trial_stresses(family, flag, seed)
    mat = F.gpu_material(family, flag, c)
    assert F.margins_hold(family, mat, trial)
    m, _, unode, dunode = F.plastic_case(family, flag)
    ref = F.Model(m.coord, m.conn, mat)
    ref.unode[:], ref.dunode[:] = unode, dunode
    ref.element_update()
    share = ref.st["istat"].mean()
    print(family, flag, "plastic share %.2f" % share)
    assert 0.25 <= share <= 0.90
    if np.finfo(np.longdouble).eps < EPS:
        ld = np.longdouble
        far = F.gpu_material(family, flag, 1.0e12)
        z = np.zeros(8)
        u, du = unode.astype(ld).reshape(-1, 3), dunode.astype(ld).reshape(-1, 3)
        wide = np.array([F.update_c3d8fbar(m.coord.astype(ld)[nd], u[nd], du[nd], far, z, z.astype(np.int32), z)[1] for nd in m.conn - 1])
        assert np.abs(trial.reshape(wide.shape) - wide).max() <= 1e-12 * np.abs(wide).max()
