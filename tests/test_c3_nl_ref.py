"""The numpy restatement of the nonlinear wedges and 20-node hexahedron (tests/c3_nl_ref.py) against the reference's own output:

- it is tet_nl_ref's restatement where both serve a type (341 / 342: same numbers);
- a numpy Newton loop reproduces every printed summary of examples/static/exI A351 / A352 / A362 (`_correct.log`, all 10 steps)
  at the reference harness's 1e-4;
- it reproduces the summaries and Newton counts of the recorded cube decks (tests/golden/nl_c3_decks.npz, the unmodified
  program's runs);
- UPDATELAG rounds the stress increment to single precision: on the inputs of the GPU test (tests/test_gpu_c3_nonlinear.py: the
  skewed 2^3 meshes, seed 17) two evaluations that sum the element's nodes in different orders differ by more than 1e-11 relative
  in at most 1 % of the stress components -- the cap the GPU test applies, so the restatement alone stays inside it.
"""
import json
import os

import numpy as np
import pytest

import c3_nl_ref as N
import c3_ref as R
import tet_nl_ref as TN
from frontistr_amd.mesh import solid_mesh
from oracle.refrun import Material
from test_tet_nl_ref import read_exI

HERE = os.path.dirname(os.path.abspath(__file__))
# the GPU test's skewed meshes and seed
SKEWED = {351: dict(skew=0.1), 352: dict(skew=0.1, curve=0.03), 362: dict(skew=0.1, curve=0.03)}
SEED = 17


@pytest.mark.parametrize("etype", [341, 342])
@pytest.mark.parametrize("nlgeom", [N.INFINITE, N.TOTALLAG, N.UPDATELAG])
def test_same_numbers_as_the_tet_restatement(etype, nlgeom, oracle):
    m = solid_mesh(1, etype, skew=0.1)
    mat = Material(206900.0, 0.29, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=nlgeom)
    unode, dunode, st = TN.random_case(etype, mat, m, 5)
    out = []
    for mod in (TN.Model(etype, m.coord, m.conn, mat), N.Model(etype, m.coord, m.conn, mat)):
        mod.st = {k: v.copy() for k, v in st.items()}
        mod.unode[:], mod.dunode[:] = unode, dunode
        ke = mod.element_tangents()
        out.append((ke, mod.element_update(), mod.st["stress"].copy(), mod.st["fstat"].copy()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def read_exI_c3(model):
    """read_exI for the wedges and the 20-node hexahedron: the file lists 352's triangle mid-edge nodes as (2,3), (3,1), (1,2) and
    (5,6), (6,4), (4,5); 362 is read as written."""
    coord, conn, fix, cl = read_exI(model)
    if conn.shape[1] == 15:
        conn = conn[:, [0, 1, 2, 3, 4, 5, 8, 6, 7, 11, 9, 10, 12, 13, 14]]
    return coord, conn, fix, cl


@pytest.mark.parametrize("etype", [351, 352, 362])
def test_exI_known_answers(etype):
    """A numpy Newton loop (dense direct solve) over the exI mesh reproduces the summaries of every one of the 10 steps of
    A351_correct.log / A352_correct.log / A362_correct.log at the reference harness's 1e-4 (I300.cnt: `!STATIC, TYPE=NLGEOM`,
    `!ELASTIC 4000, 0.3` (total Lagrange), FIX clamped, -1 in z on CL1, 10 sub-steps, the default convergence bound 1e-3)."""
    from oracle import fistr1_run as f1
    model = "A%d" % etype
    coord, conn, fix, cl = read_exI_c3(model)
    assert conn.shape[1] == R.NN[etype]
    mod = N.Model(etype, coord, conn, Material(4000.0, 0.3, nlgeom=N.TOTALLAG))
    bc = (np.repeat(fix, 3), np.tile([1, 2, 3], len(fix)), np.zeros(3 * len(fix)))
    load = np.zeros(3 * coord.shape[0])
    for nd in cl:
        load[3 * (nd - 1) + 2] = -1.0
    correct = f1.read_log(os.path.join(f1.DECKS, "exI", model + "_correct.log"))
    assert len(correct) == 10
    for sub in range(1, 11):
        ok, it = mod.newton_substep((sub - 1) / 10.0, sub / 10.0, bc, load, 20, 1.0e-3)
        assert ok
        actual = N.summary(etype, conn, mod.unode, mod.st["strain"], mod.st["stress"])
        assert set(actual["Node"]) == set(correct[sub - 1]["Node"]) and set(actual["Element"]) == set(correct[sub - 1]["Element"])
        assert f1.compare_step(actual, correct[sub - 1]) == [], sub


@pytest.mark.parametrize("name", list(N.GOLDEN_DECKS))
def test_recorded_decks(name, oracle):
    """The restatement's Newton loop on the recorded cube decks: the Newton count of every sub-step is the reference's, the
    summaries of every step agree at the reference harness's 1e-4, and the plastic decks have plastic points."""
    from oracle import fistr1_run as f1
    g = np.load(os.path.join(HERE, "golden", "nl_c3_decks.npz"))
    log, newton = json.loads(str(g[name + "/log"])), g[name + "/newton"]
    m, mats, em, bc = N.golden_deck(name)
    oracle.nl_reset_latch()
    mod = N.Model(m.etype, m.coord, m.conn, mats, em)
    counts = []
    for sub in range(1, N.DECK_SUBSTEPS + 1):
        ok, it = mod.newton_substep((sub - 1) / N.DECK_SUBSTEPS, sub / N.DECK_SUBSTEPS, bc, None, 50, N.DECK_CONVERG)
        assert ok
        counts.append(it)
        want = log[len(log) - N.DECK_SUBSTEPS + sub - 1]
        actual = N.summary(m.etype, m.conn, mod.unode, mod.st["strain"], mod.st["stress"])
        assert set(actual["Node"]) == set(want["Node"]) and set(actual["Element"]) == set(want["Element"])
        assert f1.compare_step(actual, want) == [], sub
    print(name, "Newton", counts, "reference", list(newton))
    assert counts == list(newton)
    if "bilinear" in name or "multilinear" in name:
        assert (mod.st["plstrain"] > 0.0).any()


@pytest.mark.parametrize("etype", [351, 352, 362])
def test_updated_lagrange_single_precision_share(etype):
    """The share of stress components that two orders of summation put on different single-precision neighbours."""
    m = solid_mesh(2, etype, **SKEWED[etype])
    mat = Material(206900.0, 0.29, nlgeom=N.UPDATELAG)
    unode, dunode, st = N.random_case(etype, mat, m, SEED)
    res = []
    for order in (None, list(range(R.NN[etype]))[::-1]):
        mod = N.Model(etype, m.coord, m.conn, mat)
        mod.st = {k: v.copy() for k, v in st.items()}
        mod.unode[:], mod.dunode[:] = unode, dunode
        mod.element_update(order)
        res.append((mod.st["stress"].copy(), mod.dstress.copy()))
    scale = np.abs(res[0][1]).max()
    diff = np.abs(res[0][0] - res[1][0]) / scale
    share = (diff > 1.0e-11).mean()
    print("etype %d: %.4f of the components differ by more than 1e-11, max %.3e (2 ulp = %.3e)" % (etype, share, diff.max(), 2.0 * 2.0 ** -23))
    assert diff.max() <= 2.0 * 2.0 ** -23
    assert share <= 0.01
