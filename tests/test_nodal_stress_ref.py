"""tests/nodal_stress_ref.py, the numpy restatement of fstr_NodalStress3D, against what the reference program itself wrote
(tests/golden/nodal_stress.npz, nodal_stress_nl.npz; tests/golden/make_nodal_stress_golden.py) and against the helpers the
other test modules hold.  No GPU.

Measured by the recording script on every deck (exB/B341 .. B362, refine/hexpritet, autoinc/C3D8beam at its last sub-step, t05/necking at its last
converged one), relative to each
array's largest magnitude: 0 -- the result files hold 17 significant digits, which round-trip a double, and the restatement
repeats the reference's operations in its order, so every array agrees bit for bit, the principal values and the separated
principal vectors included.  The project's convention asserts ten times the measured value: ten times zero, equality."""
import numpy as np
import pytest

import c3_nl_ref
import nodal_stress_decks as ND
import nodal_stress_ref as NR
import tet_nl_ref

BOUND = NR.BOUND                # ten times the deviation the recording script printed: ten times zero
MEASURED_HELPERS = 1.1e-15      # restatement against the np.linalg.inv helpers on the recorded point arrays (B362's nodal strain)
BOUND_HELPERS = 10.0 * MEASURED_HELPERS
ALL = NR.ALL

_CACHE = {}


def deck(name):
    """(golden arrays, n_node, groups, the restatement's result with every principal array) -- computed once per deck"""
    if name not in _CACHE:
        g = np.load(ND.golden_file(name))
        a = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
        ids, groups, eorder = ND.load(name)
        assert np.array_equal(a["node_ids"], ids) and np.array_equal(a["elem_ids"], eorder)
        _CACHE[name] = (a, ids.size, groups, NR.nodal_stress(ids.size, groups, a["ISTRAIN"].ravel(), a["ISTRESS"].ravel(), principal=ALL))
    return _CACHE[name]


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def separated(vals, tol=1e-6):
    s = tol * np.abs(vals).max()
    return (np.abs(vals[:, 0] - vals[:, 1]) > s) & (np.abs(vals[:, 1] - vals[:, 2]) > s) & (np.abs(vals[:, 0] - vals[:, 2]) > s)


def tensor_matrix(t):
    """the symmetric matrix eigen3 reads from (11, 22, 33, 12, 23, 31), shear components as stored"""
    m = np.zeros((t.shape[0], 3, 3))
    for (i, j), k in {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 2): 4, (0, 2): 5}.items():
        m[:, i, j] = m[:, j, i] = t[:, k]
    return m


def residual_excess(t, vals, vecs):
    """largest ||S c - lambda c|| / (|lambda| (1e-10 + 16 eps max|S|)) over all items and columns c = lambda n.  eigen3 returns
    once the off-diagonal terms sum to less than 1e-10 in ABSOLUTE value, which bounds the residual of a unit vector by 1e-10;
    the rotations of at most a few sweeps add a few roundings of the tensor's magnitude each (16 eps is more than any deck
    needs: the recorded tensors reach 1.0 of the first term alone)."""
    res = np.einsum("nab,njb->nja", tensor_matrix(t), vecs) - vals[:, :, None] * vecs
    allowed = np.abs(vals) * (1.0e-10 + 16.0 * np.finfo(np.float64).eps * np.abs(t).max(axis=1)[:, None])
    return float((np.linalg.norm(res, axis=2) / np.maximum(allowed, 1e-300)).max())


@pytest.mark.parametrize("name", list(ND.RECORDED))
def test_restatement_against_the_recorded_arrays(name):
    a, _, _, r = deck(name)
    dev = {"NSTRAIN": rel(r.strain, a["NSTRAIN"]), "NSTRESS": rel(r.stress, a["NSTRESS"]), "NMISES": rel(r.mises, a["NMISES"]),
           "ESTRAIN": rel(r.estrain, a["ESTRAIN"]), "ESTRESS": rel(r.estress, a["ESTRESS"]), "EMISES": rel(r.emises, a["EMISES"])}
    print(name, dev)
    assert max(dev.values()) <= BOUND, dev
    assert not r.failed


@pytest.mark.parametrize("name", list(ND.RECORDED))
def test_principal_values_against_the_recorded_ones(name):
    a, _, _, r = deck(name)
    dev = {"PRINC_NSTRESS": rel(r.pstress, a["PRINC_NSTRESS"]), "PRINC_NSTRAIN": rel(r.pstrain, a["PRINC_NSTRAIN"]),
           "PRINC_ESTRESS": rel(r.epstress, a["PRINC_ESTRESS"])}
    print(name, dev)
    assert max(dev.values()) <= BOUND, dev
    for v in (r.pstress, r.pstrain, r.epstress, r.epstrain):        # get_principal's order
        assert np.all(v[:, 0] >= v[:, 1]) and np.all(v[:, 1] >= v[:, 2])


@pytest.mark.parametrize("name", list(ND.RECORDED))
def test_principal_vectors_against_the_recorded_ones(name):
    """Compared only where the three values are separated by more than 1e-6 of the largest magnitude, up to the sign of each
    column, columns in get_principal's order (a swapped or wrongly scaled column fails).  At most 5 % of a deck's nodes or
    elements may be left out: asserted for the decks of nodal_stress_decks.NODAL_VECTOR_DECKS / ELEMENT_VECTOR_DECKS, among them
    the nonlinear C3D8beam.  necking's nodes do not meet the share for the reference alone (6.8 %): its separated nodes are
    compared all the same, with no claim on the share.  hexpritet's uniform stress leaves no vector to compare.  The residual
    of every returned column is checked for every node and element of every deck, none left out."""
    a, _, _, r = deck(name)
    for key, vals, got, ruled in (("PRINCV_NSTRESS", a["PRINC_NSTRESS"], r.pstress_vect, name in ND.NODAL_VECTOR_DECKS),
                                  ("PRINCV_ESTRESS", a["PRINC_ESTRESS"], r.epstress_vect, name in ND.ELEMENT_VECTOR_DECKS)):
        ok = separated(vals)
        if ruled:
            assert 1.0 - ok.mean() <= 0.05, (key, 1.0 - ok.mean())
        if not ok.any():
            assert not ruled
            continue
        want = a[key][ok]
        sign = np.sign(np.einsum("njc,njc->nj", got[ok], want))[:, :, None]
        dev = float(np.abs(got[ok] * sign - want).max() / np.abs(a[key]).max())
        print(name, key, "left out %.1f %%" % (100 * (1.0 - ok.mean())), "deviation", dev)
        assert dev <= BOUND, (key, dev)
    for t, vals, vecs in ((r.stress, r.pstress, r.pstress_vect), (r.strain, r.pstrain, r.pstrain_vect),
                          (r.estress, r.epstress, r.epstress_vect), (r.estrain, r.epstrain, r.epstrain_vect)):
        assert residual_excess(t, vals, vecs) <= 1.0


def test_the_decks_of_the_vector_rule():
    """a nonlinear deck with sub-steps is among the decks of the 5 % rule for nodal vectors; what keeps necking's nodes and
    hexpritet out of it is the recorded arrays' own"""
    assert "C3D8beam" in ND.NODAL_VECTOR_DECKS and "C3D8beam" in ND.NONLINEAR and "necking" in ND.ELEMENT_VECTOR_DECKS
    a = deck("necking")[0]
    assert 1.0 - separated(a["PRINC_NSTRESS"]).mean() > 0.05
    assert 1.0 - separated(a["PRINC_ESTRESS"]).mean() <= 0.05
    a = deck("hexpritet")[0]
    assert not separated(a["PRINC_NSTRESS"]).any() and not separated(a["PRINC_ESTRESS"]).any()
    assert len(ND.load("hexpritet")[1]) == 3


@pytest.mark.parametrize("name", ["B341", "B342", "B351", "B352", "B362"])
def test_restatement_against_the_existing_helpers(name):
    """tet_nl_ref / c3_nl_ref.nodal_and_element_values invert with np.linalg.inv and add with np.add.at: equal to rounding
    (measured: 0 at 341 and 351, which invert nothing; 3.9e-16 at 342, 3.5e-16 at 352, 1.1e-15 at 362), and the summaries equal to
    the printed digits.  Neither helper serves 361 (c3_nl_ref holds the five types of STF_C3), so B361 has no case here;
    thermal_ref.summary, which does, is held against the device in tests/test_gpu_nodal_stress.py."""
    a, n_node, groups, r = deck(name)
    etype, conn = groups[0]
    helper = tet_nl_ref if etype in (341, 342) else c3_nl_ref
    ns, nt, est, ess = helper.nodal_and_element_values(etype, conn, n_node, a["ISTRAIN"], a["ISTRESS"])
    dev = max(rel(ns, r.strain), rel(nt, r.stress), rel(est, r.estrain), rel(ess, r.estress))
    print(name, dev)
    assert dev <= BOUND_HELPERS
    s = NR.summary(r)
    want = helper.summary(etype, conn, np.zeros(3 * n_node), a["ISTRAIN"], a["ISTRESS"])
    for part in ("Node", "Element"):
        for k, v in s[part].items():
            assert want[part][k] == v, (part, k)       # the five printed digits


def test_inverse_func_is_not_a_library_inverse():
    """Gauss-Jordan without pivoting as written: an inverse to rounding, and not np.linalg.inv's bits"""
    differs = 0
    for etype in (361, 342, 352, 362):
        func = np.array([NR.vertex_shape(etype, NR.quad_point(etype, q)) for q in NR.SEL[etype]])
        inv = NR.inverse(etype)
        assert np.abs(inv @ func - np.eye(func.shape[0])).max() < 1e-13
        differs += int(not np.array_equal(inv, np.linalg.inv(func)))
    assert differs > 0


def test_get_principal_on_degenerate_tensors():
    """a diagonal tensor (eigen3 returns at once: the off-diagonal sum is below 1e-10), two equal values, the zero tensor"""
    t = np.array([[3.0, 1.0, 2.0, 0.0, 0.0, 0.0],
                  [1.0, 2.0, 3.0, 1e-11, -2e-11, 3e-11],
                  [2.0, 2.0, 5.0, 0.0, 0.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                  [1.0, 1.0, 1.0, 0.5, 0.5, 0.5]])
    ev, vec, failed = NR.get_principal(t)
    assert not failed.any()
    assert np.array_equal(ev[0], [3.0, 2.0, 1.0]) and np.array_equal(vec[0], [[3.0, 0, 0], [0, 0, 2.0], [0, 1.0, 0]])
    assert np.array_equal(ev[1], [3.0, 2.0, 1.0])           # the tiny shear terms are never looked at
    assert np.array_equal(ev[2], [5.0, 2.0, 2.0]) and np.array_equal(vec[2], [[0, 0, 5.0], [0, 2.0, 0], [2.0, 0, 0]])
    assert np.array_equal(ev[3], [0.0, 0.0, 0.0]) and not vec[3].any()
    assert ev[4] == pytest.approx([2.0, 0.5, 0.5], abs=1e-14)
