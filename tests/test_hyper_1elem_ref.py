"""The reference's one-element hyperelastic decks, examples/static/1elem/{rivlin,arruda,neohooke} (committed copies under
tests/golden/decks/hyper1/), against what the unmodified program recorded for them.

rivlin, arruda: the restatement's dense-solve Newton loop (tests/hyper_ref.py) reproduces the Newton count of every sub-step and the
Global summaries of every printed step at the reference harness's 1e-4 (tests/golden/hyper_decks.npz).

arruda is the near-incompressible deck (D = 1.429e-8, bulk term 1 / D = 7e7), a unit cube pulled by a force with free lateral faces.
Its lateral stresses S22 = S33 are physically zero; what the log prints for them is what Newton leaves behind, because the sub-steps
stop on the displacement criterion (the default CONVERG = 1e-3 of m_step.f90:77) after two or three iterations, long before the
volumetric residual is gone.  That remainder is deterministic, the restatement reproduces it to the printed digits -- and in step 4
it is 6.757449984 in float64, 1.6e-8 below the rounding edge 6.75745 of the five digits the log prints.  The recorded log of the
unmodified program shows the same thing by itself: S22 and S33 of its single element, equal by symmetry, print as 6.7575 and 6.7574,
and the nodal S22 has maximum 6.7575 and minimum 6.7574.  A relative perturbation of 1e-10 of the linear solves (the deck asks the
Krylov solver for 1e-12) moves the value by 1.6e-7, ten times its distance from that edge.  So the last printed digit of these two entries is not
reproducible, in the reference either, and two correct runs can print values 1e-4 apart there.  In binary floating point
6.7575 - 6.7574 = 1.0000000000065512e-4 > 1e-4: a comparison of the parsed floats rejects what is exactly the bound.  The harness's
bound is on printed decimal numbers, so hyper_ref.within_1e4 takes the difference of the decimals exactly; it differs from the
float comparison only where the printed numbers are exactly 1e-4 apart (which the float comparison accepts or rejects by the
rounding of the subtraction) and is what
tests/test_gpu_fistr1_hyperelastic.py uses for every deck.

neohooke: the unmodified program does not converge on it (tests/golden/hyper_1elem_neohooke.json, see make_hyper_golden.py), so there
are no summaries to reproduce; the tests put that outcome, and why, on record."""
import json
import os
import re

import numpy as np
import pytest

import hyper_ref as H

HERE = os.path.dirname(os.path.abspath(__file__))
DECKS = os.path.join(HERE, "golden", "decks", "hyper1")
def read_deck(stem):
    """(coord, conn, material, bc, cload, sub-steps) of one of the 1elem decks: node ids in file order, `!BOUNDARY, GRPID = 1` and
    `!CLOAD, GRPID = 1` (what their `!STEP` names), the `!HYPERELASTIC` card."""
    ids, coord, conn, cards, cur = [], [], None, {}, None
    for fn in (stem + ".msh", stem + ".cnt"):
        with open(os.path.join(DECKS, fn)) as fh:
            for line in fh:
                s = line.strip()
                if s.startswith("!"):
                    cur = re.sub(r"\s+", "", s.upper())
                    cards.setdefault(cur, [])
                elif s and cur:
                    cards[cur].append([v.strip() for v in s.split(",")])
    for r in cards["!NODE"]:
        ids.append(int(r[0]))
        coord.append([float(v) for v in r[1:4]])
    local = {n: k + 1 for k, n in enumerate(ids)}
    conn = np.array([[local[int(v)] for v in cards["!ELEMENT,TYPE=361,EGRP=P1"][0][1:9]]])
    node, dof = [], []
    for r in cards["!BOUNDARY,GRPID=1"]:
        for d in range(int(r[1]), int(r[2]) + 1):
            node.append(local[int(r[0])])
            dof.append(d)
    cload = np.zeros(3 * len(ids))
    for r in cards["!CLOAD,GRPID=1"]:
        cload[3 * (local[int(r[0])] - 1) + int(r[1]) - 1] = float(r[2])
    nsub = int([k for k in cards if k.startswith("!STEP")][0].split("SUBSTEPS=")[1])
    kind = [k for k in cards if k.startswith("!HYPERELASTIC")][0].split("TYPE=")[1]
    c = [float(v.lower().replace("d", "e")) for v in cards["!HYPERELASTIC,TYPE=" + kind][0]]
    mat = {"MOONEY-RIVLIN": lambda: H.mooney_rivlin(*c), "ARRUDA-BOYCE": lambda: H.arruda_boyce(*c), "NEOHOOKE": lambda: H.neohooke(*c)}[kind]()
    return np.array(coord), conn, mat, (np.array(node), np.array(dof), np.zeros(len(node))), cload, nsub


def run_restatement(stem, solve=None):
    """-> Newton counts, summaries, element mean stress (n sub-steps, 6) of the restatement's loop on the deck"""
    coord, conn, mat, bc, cload, nsub = read_deck(stem)
    ref = H.Model(361, coord, conn, mat)
    keep = np.linalg.solve
    counts, logs, ess = [], [], []
    try:
        if solve is not None:
            np.linalg.solve = solve
        for sub in range(1, nsub + 1):
            ok, it = ref.newton_substep((sub - 1) / nsub, sub / nsub, bc, cload, 50, 1.0e-3)     # m_step.f90:77: the default CONVERG
            assert ok
            counts.append(it)
            logs.append(H.summary(361, conn, ref.unode, ref.st["strain"], ref.st["stress"]))
            ess.append(ref.st["stress"].mean(axis=1)[0].copy())
    finally:
        np.linalg.solve = keep
    return counts, logs, np.array(ess)


@pytest.fixture(scope="module")
def arruda():
    return run_restatement("arruda")


def _recorded(name):
    g = np.load(os.path.join(HERE, "golden", "hyper_decks.npz"))
    return json.loads(str(g[name + "/log"])), [int(v) for v in g[name + "/newton"]]


def _check(counts, logs, name):
    rlog, newton = _recorded(name)
    assert counts == newton
    for k, s in enumerate(logs):
        assert H.within_1e4(s, rlog[len(rlog) - len(logs) + k]) == [], k + 1


def test_rivlin_deck():
    counts, logs, _ = run_restatement("rivlin")
    _check(counts, logs, "1elem_rivlin")


def test_arruda_deck(arruda):
    _check(arruda[0], arruda[1], "1elem_arruda")


def test_arruda_step_4_sits_on_the_rounding_edge_of_the_log(arruda):
    """The evidence of the module docstring, asserted: the recorded log disagrees with itself in the last digit of S22 / S33 of step
    4, the restatement's value is within 1e-7 of the edge, and a perturbation of the linear solves far below what any Krylov solver
    is asked for moves it by more than its distance from the edge."""
    rlog, _ = _recorded("1elem_arruda")
    rec = rlog[4]
    assert rec["Element"]["S22"] == [6.7575, 6.7575] and rec["Element"]["S33"] == [6.7574, 6.7574]
    assert rec["Node"]["S22"] == [6.7575, 6.7574]
    s22, s33 = arruda[2][3, 1], arruda[2][3, 2]
    print("restated S22 %.10f S33 %.10f of step 4, edge 6.75745" % (s22, s33))
    assert abs(s22 - s33) <= 1e-8 and abs(s22 - 6.75745) < 1e-7
    assert 6.7575 - 6.7574 > 1e-4                                     # the float comparison's verdict on a last-digit difference
    rng = np.random.default_rng(3)
    exact = np.linalg.solve
    noisy = lambda K, b: exact(K, b) * (1.0 + 1.0e-10 * rng.uniform(-1.0, 1.0, b.shape))
    counts, logs, ess = run_restatement("arruda", solve=noisy)
    print("with 1e-10 relative noise in the solves: S22 %.10f" % ess[3, 1])
    assert counts == arruda[0]
    assert abs(ess[3, 1] - s22) > abs(s22 - 6.75745)
    assert abs(ess[3, 1] - s22) < 1e-5                                 # and still far inside the harness's bound
    _check(counts, logs, "1elem_arruda")


def test_neohooke_deck_does_not_converge_in_the_unmodified_program():
    with open(os.path.join(HERE, "golden", "hyper_1elem_neohooke.json")) as fh:
        rec = json.load(fh)["1elem_neohooke"]
    assert rec["sta"] == [[1, 1, "1F", 50, "Failed to converge due to MAXITER."]]
    iters = [l for l in rec["step_lines"] if l.lstrip().startswith("iter:")]
    assert len(iters) == 50 and all(re.search(r"residual:\s+NaN", l) for l in iters)
    assert "Fail to Converge" in rec["step_lines"][-1]
    assert rec["printed_steps"] == 1                                    # step 0 only


def test_why_the_neohooke_deck_fails():
    """The card's `2.1E+5, 0.4995` are read as C10 and D1: shear modulus 2 C10 = 4.2e5, bulk modulus 2 / D1 = 4.  The tangent at rest
    has the volumetric eigenvalue 3 K = 12 beside shear eigenvalues of 4.2e5 and more, and the uniaxial stiffness 9 K mu / (3 K + mu)
    is 36 under a load of 4e5 in one sub-step: the first Newton correction of the restatement is 1e4 edge lengths."""
    coord, conn, mat, bc, cload, nsub = read_deck("neohooke")
    assert nsub == 1 and mat.plconst == (2.1e5, 0.0, 0.4995) and cload.sum() == 4.0e5
    ev = np.linalg.eigvalsh(H.tangent(mat, np.zeros(6)))
    assert abs(ev[0] - 6.0 / 0.4995) < 1e-6 and ev[1] > 4.19e5
    ref = H.Model(361, coord, conn, mat)
    import c3_ref as R
    K, b = R.apply_bc(ref.stiffness(), cload.copy(), bc)
    x = np.linalg.solve(K, b)
    assert 1.0e4 < np.abs(x).max() < 1.2e4
