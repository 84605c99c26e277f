"""The numpy restatement of the thermal load and the thermal update branches (tests/thermal_ref.py) against the reference's output:

- a dense linear analysis with it reproduces the recorded runs of the unmodified program on the --thermal cube decks
  (tests/golden/thermal_decks.npz, make_thermal_golden.py) at the reference harness's 1e-4 on the printed digits: every printed
  summary, nodal and element values (thermal_ref.summary).
  The decks that choose the 361 formulation with `!SECTION, FORM361=` show a property of the reference: its load vector is
  TLOAD_C3D8IC whatever the section says (thermal_ref.solve, load_groups).
- the same analysis on the reference's own thermal decks examples/static/exF F341 ... F362 (F300.cnt: `!REFTEMP 20`,
  `!TEMPERATURE ALL, 120`, FIX clamped; thermal_ref.read_msh) reproduces every printed summary of their `_correct.log`, read with
  the project's log reader and compared on the printed digits (fistr1_run.compare_step, the reference harness's 1e-4);
- scripts/fistr1_cube_deck.py without --thermal writes what the parent's script wrote, byte for byte, for the argument sets of the
  golden generators (make_tet_golden, make_c3_golden, make_mixed_golden, make_nl_tet_golden, make_nl_c3_golden, and
  make_cube_fullsize_golden's `N --linear` at N = 4): sha256 of cube.msh + cube.cnt + hecmw_ctrl.dat recorded from the parent's
  script in tests/golden/cube_deck_digests.json.
"""
import hashlib
import importlib.util
import json
import os
import runpy
import sys

import numpy as np
import pytest

import thermal_ref as TH
from oracle import fistr1_run as f1

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("make_thermal_golden", os.path.join(HERE, "golden", "make_thermal_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
E2, NU2, AL2 = np.array([210000.0, 70000.0]), np.array([0.3, 0.33]), np.array([1.2e-5, 2.3e-5])


@pytest.mark.parametrize("name", list(G.DECKS))
def test_recorded_thermal_decks(name):
    from frontistr_amd.mesh import mesh_groups
    g = np.load(os.path.join(HERE, "golden", "thermal_decks.npz"))
    want = json.loads(str(g[name + "/log"]))
    m, n = G.deck_mesh(name)
    a = G.DECKS[name]
    elemopt = {"IC": 1, "BBAR": 2, "FI": 3}[a[a.index("--form361") + 1]] if "--form361" in a else 1
    two = "--two-sections" in a
    em = np.where(np.arange(m.n_elem) < m.n_elem // 2, 1, 2).astype(np.int32) if two else None
    if not hasattr(m, "etype") and not hasattr(m, "groups_with"):
        m.etype = 361
    groups = mesh_groups(m, elemopt, em)
    th = (G.deck_temperature(m, n), np.full(m.n_node, G.T_INIT), G.T_REF, AL2 if two else 1.2e-5)
    u, st, ss, qf, _ = TH.solve(m.coord, groups, E2 if two else 210000.0, NU2 if two else 0.3, m.dirichlet(), m.load(), th,
                                load_groups=mesh_groups(m, 1, em))      # the decks set FORM361 per section: the load stays IC's
    full = TH.summary(groups, u, st, ss)
    assert set(full["Node"]) == set(want["Node"]) and set(full["Element"]) == set(want["Element"])
    assert f1.compare_step(full, want) == []


@pytest.mark.parametrize("etype", [341, 342, 351, 352, 361, 362])
def test_exF_known_answers(etype):
    model = "F%d" % etype
    et, coord, conn, grp, (E, nu, alpha), init = TH.read_msh(os.path.join(f1.DECKS, "static", "exF", model + ".msh"))
    assert et == etype and conn.shape[1] == TH.NN[etype] and init == 20.0
    n = coord.shape[0]
    fix = grp["FIX"]
    bc = (np.repeat(fix, 3), np.tile([1, 2, 3], fix.size), np.zeros(3 * fix.size))
    th = (np.full(n, 120.0), np.full(n, init), 20.0, alpha)            # F300.cnt
    groups = [(etype, conn, 1, None)]                                  # 361: the program's default, IC
    u, st, ss, qf, _ = TH.solve(coord, groups, E, nu, bc, None, th)
    correct = f1.read_log(os.path.join(f1.DECKS, "static", "exF", model + "_correct.log"))
    assert len(correct) == 1
    got = TH.summary(groups, u, st, ss)
    assert set(got["Node"]) == set(correct[0]["Node"]) and set(got["Element"]) == set(correct[0]["Element"])
    assert f1.compare_step(got, correct[0]) == []


def test_deck_writer_without_thermal_is_unchanged(tmp_path, monkeypatch, capsys):
    with open(os.path.join(HERE, "golden", "cube_deck_digests.json")) as fh:
        want = json.load(fh)
    assert len(want) == 35
    script = os.path.join(ROOT, "scripts", "fistr1_cube_deck.py")
    for k, (args, digest) in enumerate(want.items()):
        d = str(tmp_path / ("d%d" % k))
        monkeypatch.setattr(sys, "argv", [script, d] + args.split())
        runpy.run_path(script, run_name="__main__")
        h = hashlib.sha256()
        for f in ("cube.msh", "cube.cnt", "hecmw_ctrl.dat"):
            with open(os.path.join(d, f), "rb") as fh:
                h.update(fh.read())
        assert h.hexdigest() == digest, args
