"""The numpy restatement of the hyperelastic materials (tests/hyper_ref.py) against what does not depend on the reference's routines
-- the strain-energy functions -- and the choice of the GPU tolerance.

(a) Finite differences.  The 2nd Piola-Kirchhoff stress is dW/dE and the tangent dS/dE, component by component in the reference's
    strain vector (engineering shears: dW/d(gamma_12) = S_12, and mat_c2d's column of a shear is dS/d(gamma)).  A central difference
    of step h has truncation error h^2 |f'''| / 6 and rounding error eps |f| / h; they balance at h = (3 eps |f| / |f'''|)^(1/3), i.e.
    h of the order eps^(1/3) = 6e-6 for |f| ~ |f'''|, where the error is of the order eps^(2/3) = 3.7e-11 times that scale.  The
    scale |f| + |f'''| of the functions here is not bounded analytically; the test prints the errors it finds instead -- at most
    5.4e-11 of the largest tangent entry for the stress and 7.2e-10 for the tangent on these inputs (strains to 47 %), i.e. 1.5 and
    20 times eps^(2/3) -- and asserts FD_TOL = 100 eps^(2/3) = 3.7e-9 of the largest tangent entry, five times the largest error seen.
    A wrong coefficient or index in the restatement shows at 1e-2 and more.
(c) Sensitivity.  The GPU tests compare at the project's nonlinear tolerance, 1e-11 of the largest entry of the compared array.
    That needs the restated stress and tangent to be determined to better than that by their float64 inputs: evaluated in float64
    and in np.longdouble on the strains the GPU tests store, they must agree to 1e-12 on that scale.  The near-incompressible 1 / D
    term is what could break it (examples/static/1elem/arruda.cnt has D = 1.4e-8), so the GPU tests use the constants of the
    reference's tutorials (hyper_ref.TEST_MATERIALS), and this test puts the margin on record.
"""
import numpy as np
import pytest

import hyper_ref as H

EPS = np.finfo(np.float64).eps
FD_H = EPS ** (1.0 / 3.0)
FD_TOL = 1.0e2 * EPS ** (2.0 / 3.0)
NAMES = list(H.TEST_MATERIALS)


def _strains():
    return np.concatenate([np.zeros((1, 6)), H.random_strains(4, 0.02, 1), H.random_strains(6, 0.3, 2)])


@pytest.mark.parametrize("name", NAMES)
def test_stress_and_tangent_are_derivatives_of_the_energy(name):
    mat = H.TEST_MATERIALS[name]()
    for e in _strains():
        S, D = H.stress_update(mat, e), H.tangent(mat, e)
        scale = np.abs(D).max()
        assert np.abs(D - D.T).max() <= 16 * EPS * scale, "tangent not symmetric"
        fdS, fdD = np.zeros(6), np.zeros((6, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = FD_H
            fdS[k] = (H.energy(mat, e + d) - H.energy(mat, e - d)) / (2 * FD_H)
            fdD[:, k] = (H.stress_update(mat, e + d) - H.stress_update(mat, e - d)) / (2 * FD_H)
        errS, errD = np.abs(fdS - S).max() / scale, np.abs(fdD - D).max() / scale
        print("%s |E| %.2f: stress %.2e tangent %.2e (bound %.1e)" % (name, np.abs(e).max(), errS, errD, FD_TOL))
        assert errS < FD_TOL and errD < FD_TOL


def test_stress_free_reference_state_and_small_strain_limit():
    """At E = 0 the stress vanishes and the tangent is the isotropic elastic matrix of mu = 2 (C10 + C01), K = 2 / D1 (Mooney-Rivlin)."""
    mat = H.TEST_MATERIALS["mooney"]()
    z = np.zeros(6)
    assert np.abs(H.stress_update(mat, z)).max() < 1e-14
    c10, c01, d1 = mat.plconst
    mu, K = 2.0 * (c10 + c01), 2.0 / d1
    D = np.zeros((6, 6))
    D[:3, :3] = K - 2.0 * mu / 3.0
    D[[0, 1, 2], [0, 1, 2]] += 2.0 * mu
    D[[3, 4, 5], [3, 4, 5]] = mu
    assert np.abs(H.tangent(mat, z) - D).max() < 1e-13 * np.abs(D).max()


def test_neohooke_is_mooney_rivlin_without_the_second_constant():
    a, b = H.neohooke(0.3, 0.05), H.mooney_rivlin(0.3, 0.0, 0.05)
    for e in _strains():
        assert np.array_equal(H.stress_update(a, e), H.stress_update(b, e)) and np.array_equal(H.tangent(a, e), H.tangent(b, e))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("etype", [361, 341, 342, 351, 352, 362])
def test_gpu_inputs_are_well_conditioned(etype, name):
    """(c): float64 against long double on every strain the GPU tests store (the two-section cases store the same strains in the
    hyperelastic half: the same mesh and displacement), and on the zero strain of the first tangent."""
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    mat = H.TEST_MATERIALS[name]()
    strains = np.concatenate([H.gpu_strains(etype, name).reshape(-1, 6), np.zeros((1, 6))])
    worst_s = worst_d = 0.0
    smax = max(np.abs(H.stress_update(mat, e)).max() for e in strains)
    for e in strains:
        el = e.astype(np.longdouble)
        S, D = H.stress_update(mat, e), H.tangent(mat, e)
        Sl, Dl = H.stress_update(mat, el), H.tangent(mat, el)
        assert Sl.dtype == np.longdouble and Dl.dtype == np.longdouble
        worst_s = max(worst_s, float(np.abs(S - Sl).max()) / smax)
        worst_d = max(worst_d, float(np.abs(D - Dl).max() / np.abs(Dl).max()))
    print("%d %s: %d points, |E| to %.3f, float64 vs long double: stress %.2e, tangent %.2e" % (etype, name, len(strains), np.abs(strains).max(), worst_s, worst_d))
    assert np.abs(strains).max() > 0.02, "the inputs do not strain the material"
    assert worst_s <= 1e-12 and worst_d <= 1e-12


def test_bbar_restatement_reduces_to_the_elastic_oracle(oracle):
    """stf_c3d8bbar / update_c3d8bbar with an ELASTIC TOTALLAG material against the C oracle of the B-bar element (its own check is
    the reference's recorded output): the kinematics the hyperelastic branch shares."""
    from oracle.refrun import Material
    m = H.gpu_mesh(361)
    mat = Material(206900.0, 0.29, nlgeom=H.TOTALLAG)
    unode, dunode = H.random_displacement(m.coord, 5, 2e-3)
    ref = H.Model(361, m.coord, m.conn, mat)
    ref.unode[:], ref.dunode[:] = unode, dunode
    st = oracle.new_state(m.n_elem)
    ke0, qf, ke1, ost = oracle.nl_elements(mat, m.coord, m.conn, unode, dunode, st)
    k0 = ref.element_tangents()
    assert np.abs(k0 - ke0).max() <= 1e-12 * np.abs(ke0).max()
    rqf = ref.element_update()
    assert np.abs(rqf - qf).max() <= 1e-12 * np.abs(qf).max()
    assert np.abs(ref.st["stress"] - ost["stress"].reshape(ref.st["stress"].shape)).max() <= 1e-12 * np.abs(ost["stress"]).max()
    assert np.abs(ref.element_tangents() - ke1).max() <= 1e-12 * np.abs(ke1).max()


@pytest.mark.parametrize("name", list(H.GOLDEN_DECKS))
def test_recorded_decks(name):
    """(b): the restatement's dense-solve Newton loop on the cube decks the unmodified reference program ran
    (tests/golden/hyper_decks.npz): the Newton count of every sub-step and the Global summaries of every printed step at the reference
    harness's 1e-4.  This is what pins the element semantics -- the tangent from the STORED strain, PK2 from the total strain, the B-bar term inside the Green-Lagrange strain."""
    import json
    import os
    from oracle import fistr1_run as f1
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hyper_decks.npz"))
    rlog, newton = json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]
    m, mats, em, bc = H.golden_deck(name)
    ref = H.Model(m.etype, m.coord, m.conn, mats, em)
    nsub, got = H.DECK_SUBSTEPS, []
    for sub in range(1, nsub + 1):
        ok, it = ref.newton_substep((sub - 1) / nsub, sub / nsub, bc, None, 50, H.DECK_CONVERG)
        assert ok
        got.append(it)
        s = H.summary(m.etype, m.conn, ref.unode, ref.st["strain"], ref.st["stress"])
        bad = f1.compare_step(s, rlog[len(rlog) - nsub + sub - 1])
        assert bad == [], (sub, bad)
    assert got == newton, (got, newton)
