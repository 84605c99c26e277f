"""The numpy restatement of the nonlinear tetrahedra (tests/tet_nl_ref.py) checked without any reference output:

- elastic TOTALLAG: the tangent is the derivative of the internal force.  Central differences with step h have the truncation
  error h^2 |f'''| / 6; the internal force is a cubic polynomial in u (B linear, S quadratic), f''' ~ E |grad N|^4 V, and the
  rounding error is eps |f| / h.  With unit-size elements, |u| ~ 1e-3, h = 1e-5: truncation ~ 1e-10 |K|, rounding
  ~ 1e-16 * 1e-3 / 1e-5 |K| = 1e-14 |K|.  Bound: 1e-8 relative to the largest entry of K (two orders above the estimate).
- the internal force does not change under a rigid translation (bound: a few rounding errors of the coordinates, 1e-9 relative).
- a one-element uniaxial Mises run ends on the hardening curve within the return mapping's tolerance (BackwardEuler iterates
  to |f| < 1e-6; the check of DESIGN.md section 2 for `1elem`).
- UPDATELAG rounds the stress increment to single precision: two evaluations that sum the element's nodes in different orders
  differ by more than 1e-11 relative in only a small share of the components (the GPU test's 1 % rule needs inputs for which the
  restatement alone stays within it).
"""
import numpy as np
import pytest

import tet_nl_ref as N
import tet_ref as R
from frontistr_amd.mesh import TetMesh
from oracle.refrun import Material


def _elastic(nlgeom):
    return Material(206900.0, 0.29, nlgeom=nlgeom)


@pytest.mark.parametrize("etype", [341, 342])
def test_total_lagrange_tangent_is_the_derivative_of_the_internal_force(etype):
    m = TetMesh(1, etype=etype, skew=0.1)
    mat = _elastic(N.TOTALLAG)
    unode, dunode, _ = N.random_case(etype, mat, m, 3, history=False)
    mod = N.Model(etype, m.coord, m.conn, mat)

    def force(u):
        mod.unode[:] = 0.0
        mod.dunode[:] = u
        return mod.update().copy()

    u0 = unode + dunode
    force(u0)                     # the stress of the state the tangent is taken at
    K = mod.stiffness()
    h = 1.0e-5
    Kfd = np.zeros_like(K)
    for j in range(u0.size):
        e = np.zeros(u0.size)
        e[j] = h
        Kfd[:, j] = (force(u0 + e) - force(u0 - e)) / (2.0 * h)
    err = np.abs(K - Kfd).max() / np.abs(K).max()
    print("tangent vs central differences: %.3e" % err)
    assert err < 1.0e-8
    assert np.abs(K - K.T).max() <= 1e-12 * np.abs(K).max()


@pytest.mark.parametrize("etype", [341, 342])
@pytest.mark.parametrize("nlgeom", [N.INFINITE, N.TOTALLAG, N.UPDATELAG])
def test_internal_force_is_invariant_under_translation(etype, nlgeom, oracle):
    m = TetMesh(1, etype=etype, skew=0.1)
    mat = Material(206900.0, 0.29, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=nlgeom)
    unode, dunode, st = N.random_case(etype, mat, m, 5)
    out = []
    for shift in (np.zeros(3), np.array([3.0, -2.0, 5.0])):
        mod = N.Model(etype, m.coord + shift, m.conn, mat)
        mod.st = {k: v.copy() for k, v in st.items()}
        mod.unode[:], mod.dunode[:] = unode, dunode
        out.append(mod.update().copy())
    err = np.abs(out[0] - out[1]).max() / np.abs(out[0]).max()
    print("translation: %.3e" % err)
    assert err < 1.0e-9


@pytest.mark.parametrize("etype", [341, 342])
def test_uniaxial_mises_ends_on_the_hardening_curve(etype, oracle):
    """One tetrahedron, uniaxial stress in z through displacement control of the top with free lateral contraction (Newton on the
    free dofs): at the end the Mises stress equals the yield stress of the accumulated plastic strain."""
    ec = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    conn = np.array([[1, 2, 3, 4]])
    if etype == 342:
        ec = np.concatenate([ec, [0.5 * (ec[a] + ec[b]) for a, b in R.TET10_EDGES]])
        conn = np.arange(1, 11).reshape(1, 10)
    mat = Material(206900.0, 0.29, plastic=True, harden=0, plconst=(450.0, 5000.0, 0.0), nlgeom=N.INFINITE)
    mod = N.Model(etype, ec, conn, mat)
    # z prescribed everywhere (uz = eps z); x / y free except for the rigid-body modes: uniform uniaxial stress
    node, dof, val = [], [], []
    eps = 0.01
    for i, x in enumerate(ec):
        node.append(i + 1); dof.append(3); val.append(eps * x[2])
    for nd, d in ((1, 1), (1, 2), (2, 2)):
        node.append(nd); dof.append(d); val.append(0.0)
    # node 4 (0,0,1) sits on the axis: keep it there so that the rotation about z and the shear modes are fixed
    for nd, d in ((4, 1), (4, 2)):
        node.append(nd); dof.append(d); val.append(0.0)
    bc = (np.array(node), np.array(dof), np.array(val))
    for sub in range(1, 6):
        ok, it = mod.newton_substep((sub - 1) / 5.0, sub / 5.0, bc, None, 30, 1.0e-8)
        assert ok
    s = mod.st["stress"][0]
    mises = np.sqrt(0.5 * ((s[:, 0] - s[:, 1]) ** 2 + (s[:, 1] - s[:, 2]) ** 2 + (s[:, 2] - s[:, 0]) ** 2) + 3.0 * (s[:, 3:] ** 2).sum(axis=1))
    pl = mod.st["plstrain"][0]
    assert (pl > 1.0e-3).all() and (mod.st["istat"][0] == 1).all()
    want = np.array([oracle.curr_yield(mat, p) for p in pl])
    print("mises", mises, "yield", want)
    assert np.abs(mises - want).max() < 1.0e-3          # BackwardEuler's tolerance on the yield function (tol = 1e-3, squared inside the loop)
    assert np.abs(s[:, 2] - mises).max() < 1.0e-6 * mises.max() and np.abs(s[:, :2]).max() < 1.0e-6 * mises.max()   # uniaxial


@pytest.mark.parametrize("etype", [341, 342])
def test_updated_lagrange_single_precision_share(etype):
    """The share of stress components that two orders of summation put on different single-precision neighbours."""
    m = TetMesh(2, etype=etype, skew=0.1)
    mat = _elastic(N.UPDATELAG)
    unode, dunode, st = N.random_case(etype, mat, m, 7)
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


# ---- the reference's known answers: examples/static/exI, A341 / A342 under I300.cnt ----------------------------------------------
def read_exI(model):
    """Nodes, elements (library node order), the FIX group and the loaded node of tests/golden/decks/exI/<model>.msh."""
    import os
    from oracle import fistr1_run as f1
    ids, xyz, conn, fix, cl, sect = [], [], [], [], [], None
    with open(os.path.join(f1.DECKS, "exI", model + ".msh")) as fh:
        for line in fh:
            t = line.strip()
            if t.startswith("!"):
                u = t.upper().replace(" ", "")
                sect = ("node" if u.startswith("!NODE") else "elem" if u.startswith("!ELEMENT") else
                        "fix" if u.startswith("!NGROUP") and "NGRP=FIX" in u else "cl" if u.startswith("!NGROUP") and "NGRP=CL1" in u else None)
                continue
            if not t or t.startswith("#") or sect is None:
                continue
            a = [x for x in t.replace(",", " ").split()]
            if sect == "node":
                ids.append(int(a[0])); xyz.append([float(x) for x in a[1:4]])
            elif sect == "elem":
                conn.append([int(x) for x in a[1:]])
            elif sect == "fix":                     # GENERATE: first, last, step
                fix += list(range(int(a[0]), int(a[1]) + 1, int(a[2])))
            elif sect == "cl":
                cl += [int(x) for x in a]
    lid = {g: i + 1 for i, g in enumerate(ids)}
    conn = np.array([[lid[g] for g in e] for e in conn], dtype=np.int32)
    used = np.zeros(len(ids) + 1, dtype=bool)      # A341.msh keeps the node list of A342: nodes no element names take no part
    used[conn.ravel()] = True
    new = np.cumsum(used) * used                   # old local id -> new local id (0: dropped)
    xyz = [x for x, u in zip(xyz, used[1:]) if u]
    conn = new[conn].astype(np.int32)
    lid = {g: int(new[i]) for g, i in lid.items() if used[i]}
    if conn.shape[1] == 10:      # the file lists the mid-edge nodes as (2,3), (3,1), (1,2), (1,4), (2,4), (3,4)
        conn = conn[:, [0, 1, 2, 3, 6, 4, 5, 7, 8, 9]]
    return np.array(xyz), conn, [lid[g] for g in fix if g in lid], [lid[g] for g in cl]


@pytest.mark.parametrize("etype", [341, 342])
def test_exI_known_answers(etype):
    """A numpy Newton loop (dense direct solve) over the exI mesh reproduces the summaries (displacements, nodal and element strains, stresses and Mises stress) of every one of the 10 steps
    of A341_correct.log / A342_correct.log at the reference harness's 1e-4 (read_log / compare_step).  I300.cnt: `!STATIC,
    TYPE=NLGEOM`, `!ELASTIC 4000, 0.3` (total Lagrange), FIX clamped, -1 in z on CL1, 10 sub-steps, the default convergence bound 1e-3 (m_step.f90:77)."""
    import os
    from oracle import fistr1_run as f1
    model = "A%d" % etype
    coord, conn, fix, cl = read_exI(model)
    assert conn.shape[1] == R.NN[etype]
    mat = Material(4000.0, 0.3, nlgeom=N.TOTALLAG)
    mod = N.Model(etype, coord, conn, mat)
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
    """The restatement's Newton loop on the recorded cube decks (tests/golden/nl_tet_decks.npz: the unmodified reference program's
    runs): the Newton count of every sub-step is the reference's, the summaries of every step (displacements, nodal and element strains, stresses, Mises stress) agree at the
    reference harness's 1e-4, and the plastic decks have plastic points."""
    import json
    import os
    from oracle import fistr1_run as f1
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nl_tet_decks.npz"))
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
