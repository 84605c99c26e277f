#!/usr/bin/env python3
"""Record what the UNMODIFIED reference program (oracle/_ref/fistr1_ref, CPU) computes for Mohr-Coulomb and Drucker-Prager decks: the
Global summaries of every printed step of 0.log and the Newton count of every sub-step (FSTR.sta) -> tests/golden/yield_decks.npz.

- the reference's own decks, committed copies under tests/golden/decks/: examples/static/1elem/{drucker,mohr,mohrshear}.cnt (yield1/;
  the tree holds no mohrshear.msh: that deck runs on mohr.msh, the one-element mesh its node numbers fit) and
  tutorial/06_plastic_can (t06/, the fixture the suite already runs: TYPE=342, Drucker-Prager, 10 sub-steps);
- cube decks of scripts/fistr1_cube_deck.py --nl-material drucker|mohr for each of the six solid types (the cube sizes of
  make_hyper_golden.py), 3 sub-steps, the top face pulled by 0.5 %; and one --two-sections deck per element family (361, tetrahedra,
  wedges, 20-node hexahedra) whose second half is Mises BILINEAR.  The tests rebuild these decks from the same script.

For every cube deck the numpy restatement (tests/yield_ref.py) is run beside the program and must end with points at istat = 1: a
deck that stays elastic would pin nothing.  A reference deck on which the unmodified program does not converge is recorded as that
outcome in tests/golden/yield_not_converging.json (as hyper_1elem_neohooke.json is) and run nowhere else.
Run where the reference is built: python tests/golden/make_yield_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import fistr1_run as f1      # noqa: E402
import yield_ref as Y                    # noqa: E402

REFERENCE_DECKS = {name: ("yield1", d[0], d[1]) for name, d in Y.ONE_ELEM_DECKS.items()}
REFERENCE_DECKS["t06_can"] = ("t06", "can.msh", "can.cnt")


def deck_args(name):
    et, n, fam, two = Y.GOLDEN_DECKS[name]
    return ([str(n), str(Y.DECK_SUBSTEPS), "CG", "1", str(Y.DECK_STRAIN)] + (["--etype", str(et)] if et != 361 else [])
            + ["--nl-material", fam] + (["--two-sections"] if two else []))


def write_deck(name, d):
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d] + deck_args(name), check=True,
                   stdout=subprocess.DEVNULL)


def _record(out, name, r):
    out[name + "/log"] = np.array(json.dumps(r["log"]))
    out[name + "/newton"] = np.array([row[3] for row in r["sta"]], dtype=np.int32)
    print(name, "steps", len(r["log"]), "Newton", out[name + "/newton"], "U1 max", r["log"][-1]["Node"]["U1"][0])


def restated_plastic_points(name):
    m, mats, em, bc = Y.golden_deck(name)
    ref = Y.Model(m.etype, m.coord, m.conn, mats, em)
    for sub in range(1, Y.DECK_SUBSTEPS + 1):
        ok, _ = ref.newton_substep((sub - 1) / Y.DECK_SUBSTEPS, sub / Y.DECK_SUBSTEPS, bc, None, 50, Y.DECK_CONVERG)
        assert ok, name
    first = np.array([Y.is_yield(ref.mat(e)) for e in range(m.n_elem)])
    return int(ref.st["istat"][first].sum()), int(ref.st["istat"][first].size)


if __name__ == "__main__":
    out, failed = {}, {}
    for name in Y.GOLDEN_DECKS:
        with tempfile.TemporaryDirectory() as d:
            write_deck(name, d)
            r = f1.run("fistr1_ref", d, threads=2)
            assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], (name, f1.step_lines(r["stdout"])[-8:])
            assert len(r["sta"]) == Y.DECK_SUBSTEPS and len(r["log"]) >= 1
            _record(out, name, r)
        npl, npt = restated_plastic_points(name)
        print("   restated: %d of %d points of the first section at istat = 1" % (npl, npt))
        assert npl > 0, name
    for name, (deck, mesh, cnt) in REFERENCE_DECKS.items():
        r = f1.run_deck("fistr1_ref", deck, mesh, cnt, threads=2)
        if r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"] and r["sta"] and r["log"]:
            _record(out, name, r)
        else:
            failed[name] = {"returncode": r["returncode"], "sta": [list(row) for row in r["sta"]], "step_lines": f1.step_lines(r["stdout"]),
                            "printed_steps": len(r["log"]), "stdout_tail": r["stdout"][-600:].split("\n")}
            print(name, "NOT COMPLETED", failed[name]["sta"], failed[name]["stdout_tail"][-6:])
    np.savez_compressed(os.path.join(HERE, "yield_decks.npz"), **out)
    with open(os.path.join(HERE, "yield_not_converging.json"), "w") as fh:
        json.dump(failed, fh, indent=1)
        fh.write("\n")
