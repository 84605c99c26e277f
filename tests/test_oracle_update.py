"""The stress update of linear static decks (fstr_UpdateNewton with UpdateST_C3D8IC / Update_C3D8Bbar / UPDATE_C3, ELASTIC,
small strain): the CPU restatement (oracle/fstr_update_linear_oracle.c) against the golden outputs of the reference's own
routines (tests/golden/update_linear.npz, generator make_update_linear_golden.py) -- bit for bit -- and, where oracle/_ref
exists, against the reference itself on another mesh."""
import numpy as np
import pytest

from conftest import load_golden


@pytest.mark.parametrize("elemopt,tag", [(1, "ic"), (2, "bbar"), (3, "fi")])
def test_oracle_update_linear_equals_reference_golden(oracle, elemopt, tag):
    g = load_golden("update_linear")
    s, t, q = oracle.update_linear(elemopt, g["coord"], g["conn"], g["E"], g["nu"], g["unode"] + g["dunode"], elem_mat=g["elem_mat"])
    assert np.array_equal(s, g[tag + "_strain"]) and np.array_equal(t, g[tag + "_stress"]) and np.array_equal(q, g[tag + "_qforce"])


def test_update_linear_consistency_with_the_assembled_matrix(oracle):
    """Independent of any reference output: for a linear element QFORCE = K u with K the assembled (condensed, for IC) stiffness
    matrix of the same formulation -- fstr_UpdateNewton and fstr_StiffMatrix must agree on the element."""
    from frontistr_amd.mesh import CubeMesh
    m = CubeMesh(3, skew=0.15)
    u = 1e-3 * np.sin(0.7 * np.arange(3 * m.n_node) + 0.2)
    for elemopt in (1, 2, 3):
        A = oracle.assemble(elemopt, m.coord, m.conn, 210000.0, 0.3)
        ku = oracle.matvec(A, u)
        _, _, q = oracle.update_linear(elemopt, m.coord, m.conn, 210000.0, 0.3, u)
        assert np.abs(q - ku).max() <= 1e-11 * np.abs(ku).max(), elemopt


def update_case(elemopt):
    from frontistr_amd.mesh import CubeMesh
    m = CubeMesh(4, skew=0.1)
    rng = np.random.default_rng(elemopt)
    u, du = 1e-3 * rng.standard_normal(3 * m.n_node), 1e-4 * rng.standard_normal(3 * m.n_node)
    return m, u, du


@pytest.mark.parametrize("elemopt", [1, 2, 3])
def test_oracle_update_linear_equals_reference_build(oracle, elemopt):
    """The reference build run live where oracle/_ref exists; everywhere else what that run gave
    (tests/golden/live_ref.npz <- tests/golden/make_live_ref_golden.py)."""
    from oracle import refrun
    m, u, du = update_case(elemopt)
    if refrun.have_ref("ref_update"):
        sr, tr, qr = refrun.run_update(elemopt, m.coord, m.conn, 210000.0, 0.3, u, du)
    else:
        g = load_golden("live_ref")
        sr, tr, qr = (g["upd%d_%s" % (elemopt, k)] for k in ("strain", "stress", "qforce"))
    s, t, q = oracle.update_linear(elemopt, m.coord, m.conn, 210000.0, 0.3, u + du)
    assert np.array_equal(s, sr) and np.array_equal(t, tr) and np.array_equal(q, qr)
