"""The distributed load inside the restated Newton loop (mixed_nl_ref.Model.newton_substep with `dload`, on top of
dload_ref.assemble), pinned to the unmodified reference program: the c361 / c342 / c352 cantilevers of tests/dload_nl_decks.py, with
and without `FOLLOW=NO`, against tests/golden/dload_nl.npz -- the same Newton count in every sub-step and the Global summaries at the
printed decimals (hyper_ref.within_1e4).  The decks solve with CG to 1e-10, the restatement with a dense direct solve; CONVERG is
1e-6.  All six runs take well under a second each; none is left out.

Beside them: the numbering of an empty group (the `empty_middle` variant), and the values chosen for the follower-load sub-step
loop that tests/test_gpu_mixed_nonlinear.py runs on the device (mixed_nl_ref.FOLLOWER)."""
import json

import numpy as np
import pytest

import dload_nl_decks as D
import dload_ref as DL
import hyper_ref as H
import mixed_nl_ref as M
from oracle.refrun import Material


def deck_model(name):
    """-> (Model, bc, the list, rho) of one recorded deck"""
    etype = D.ETYPE[name]
    coord, conn = D.cantilever(etype)
    if name == "c342":
        mat = Material(D.E, D.NU, plastic=True, harden=0, plconst=(D.YIELD0, D.HARDEN, 0.0), nlgeom=M.UPDATELAG)
    else:
        mat = Material(D.E, D.NU, nlgeom=M.TOTALLAG)
    cards = [(0, [e], 10 * f, (D.PRESSURE[name],)) for e, f in D.top_faces(etype, coord, conn)]
    if name == "c342":
        cards.append((0, np.arange(conn.shape[0]), 4, D.GRAV))
    fix = D.fix_nodes(coord)
    bc = (np.repeat(fix, 3).astype(np.int32), np.tile(np.array([1, 2, 3], dtype=np.int32), fix.size), np.zeros(3 * fix.size))
    return M.Model(coord, [(etype, conn, 2, None)], [mat]), bc, DL.entries(*cards), D.RHO if name == "c342" else None


@pytest.mark.parametrize("follow", [True, False], ids=["follow", "fixed"])
@pytest.mark.parametrize("name", D.NAMES)
def test_the_loop_against_the_unmodified_program(oracle, name, follow):
    g = np.load(D.GOLDEN)
    t = D.tag(name, follow)
    rlog, newton = json.loads(str(g[t + "/log"])), [int(x) for x in g[t + "/newton"]]
    ref, bc, dl, rho = deck_model(name)
    p = ref.parts[0]
    nsub, got = D.SUBSTEPS, []
    for sub in range(1, nsub + 1):
        ok, it = ref.newton_substep((sub - 1) / nsub, sub / nsub, bc, None, D.MAX_ITER, D.CONVERG, dload=(dl, rho, follow))
        assert ok, (sub, ref.newton_log)
        got.append(it)
        summary = H.summary(p["etype"], p["conn"], ref.unode, p["st"]["strain"], p["st"]["stress"])
        want = rlog[len(rlog) - nsub + sub - 1]
        print(t, "sub-step", sub, "U3", summary["Node"]["U3"], "reference", want["Node"]["U3"])
        bad = H.within_1e4(summary, want)
        assert bad == [], (sub, bad)
    print(t, "Newton iterations per sub-step", got, "reference", newton)
    assert got == newton


def test_the_recorded_runs_tell_the_two_configurations_apart():
    """with and without FOLLOW=NO the recorded Newton counts or summaries differ, so the comparison above can see a wrong one"""
    g = np.load(D.GOLDEN)
    for name in D.NAMES:
        a, b = (json.loads(str(g[D.tag(name, f) + "/log"]))[-1] for f in (True, False))
        assert H.within_1e4(a, b) != [], name


def test_an_empty_group_keeps_its_number():
    """`empty_middle`: the entries on the groups after the empty one address the same elements as in the list without it, one
    position earlier; the model hands dload_ref.assemble its groups in the caller's numbering."""
    mats = [Material(1000.0, 0.3, nlgeom=M.TOTALLAG), Material(2000.0, 0.3, nlgeom=M.TOTALLAG)]
    rho = (0.4, 1.1)
    gl = {}
    for variant in ("mesh_order", "empty_middle"):
        m, groups, unode, dunode, _ = M.gpu_case("n3", 2, variant, mats, True, history=False)
        dl = M.top_side_dload(m, groups, 2.0, (9.8, (0.2, 0.0, -1.0)), cent=(3.0, (1.5, 1.5, 0.0), (0.0, 0.1, 1.0)))
        grp = dl.arrays()[0]
        if variant == "empty_middle":
            assert groups[1][1].shape[0] == 0 and 1 not in grp and {0, 2, 3} == set(grp.tolist())
            assert DL.boundary_faces(groups) == [(g + (g > 0), e, f) for g, e, f in DL.boundary_faces(M.group_list(m, "mesh_order"))]
        ref = M.Model(m.coord, groups, mats)
        ref.unode[:] = unode
        gl[variant] = ref.load_vector(None, 0.7, (dl.arrays(), rho, True), ref.unode)
        assert np.array_equal(gl[variant], DL.assemble(m.coord, groups, rho, dl.arrays(), factor=0.7, disp=unode))
    assert np.abs(gl["mesh_order"]).max() > 0 and np.array_equal(gl["mesh_order"], gl["empty_middle"])


@pytest.mark.parametrize("order", [1, 2])
def test_the_follower_loop_converges_and_yields(oracle, order):
    """The values of mixed_nl_ref.FOLLOWER: a pressure of 400 on the top side (the yield stress is 450; the clamped bottom and the
    softer ELASTIC section concentrate the stress) with gravity on densities 2 and 3.5, in three sub-steps.  The restatement alone
    converges in every sub-step within 50 iterations and leaves a plastic point; the loop without the follower rebuild gives
    other norms."""
    F = M.FOLLOWER
    assert (F["pressure"], F["nsub"], F["converg"], F["max_iter"], F["rho"]) == (400.0, 3, 1.0e-3, 50, (2.0, 3.5))
    logs = {}
    for follow in (True, False):
        m, groups, mats, bc, dl = M.follower_case(order)
        ref = M.Model(m.coord, groups, mats)
        logs[follow] = []
        for sub in range(1, F["nsub"] + 1):
            ok, it = ref.newton_substep((sub - 1) / F["nsub"], sub / F["nsub"], bc, None, F["max_iter"], F["converg"],
                                        dload=(dl.arrays(), F["rho"], follow))
            print("order %d follow %s sub-step %d: %s in %d iterations" % (order, follow, sub, ok, it))
            assert ok and it <= F["max_iter"], (follow, sub, it)
            logs[follow].append(np.array(ref.newton_log))
        assert (ref.flat("plstrain") > 0).any(), "no plastic point"
    same = all(a.shape == b.shape and np.allclose(a[:, 1:], b[:, 1:], rtol=1e-6, atol=1e-9) for a, b in zip(logs[True], logs[False]))
    assert not same, "the follower load changes nothing the test could see"
