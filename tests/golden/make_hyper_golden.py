#!/usr/bin/env python3
"""Record what the UNMODIFIED reference program (oracle/_ref/fistr1_ref, CPU) computes for hyperelastic decks: the Global summaries
of every printed step of 0.log and the Newton count of every sub-step (FSTR.sta) -> tests/golden/hyper_decks.npz.

- the reference's own decks, committed copies under tests/golden/decks/: examples/static/1elem/{rivlin,arruda} (hyper1/; neohooke: see NOT_CONVERGING) and
  tutorial/03_hyperelastic_cylinder (t03/, TYPE=361, Mooney-Rivlin, 5 sub-steps);
- cube decks of scripts/fistr1_cube_deck.py --nl-material neohooke|mooney|arruda for each of the six solid types (the smallest cubes
  of the other recorded decks: n = 2 at 361 / 341 / 351, one cell at 342 / 352 / 362), 3 sub-steps, the top face pulled by 10 %; and
  one --two-sections deck per element family (361, tetrahedra, wedges, 20-node hexahedra), the second half ELASTIC (total Lagrange).
  The tests rebuild these decks from the same script.
Run where the reference is built: python tests/golden/make_hyper_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import fistr1_run as f1      # noqa: E402

STRETCH, SUBSTEPS = 0.1, 3
SIZES = {361: 2, 341: 2, 342: 1, 351: 2, 352: 1, 362: 1}
# name -> (etype, n, material, two sections)
DECKS = {"h%d_%s" % (et, mat): (et, n, mat, False) for et, n in SIZES.items() for mat in ("neohooke", "mooney", "arruda")}
DECKS.update({"h361_mooney_two": (361, 2, "mooney", True), "h342_arruda_two": (342, 1, "arruda", True),
              "h352_neohooke_two": (352, 1, "neohooke", True), "h362_mooney_two": (362, 2, "mooney", True)})
# the reference's own decks: name -> (directory under tests/golden/decks, mesh, control file)
# (examples/static/1elem/neohooke is recorded apart, see NOT_CONVERGING)
REFERENCE_DECKS = {"1elem_rivlin": ("hyper1", "rivlin.msh", "rivlin.cnt"), "1elem_arruda": ("hyper1", "arruda.msh", "arruda.cnt"),
                   "t03_cylinder": ("t03", "cylinder.msh", "cylinder.cnt")}

# examples/static/1elem/neohooke: the unmodified program does not converge on it, so there are no summaries and no Newton count to
# record.  Its card reads `2.1E+5, 0.4995` -- a Young's modulus and a Poisson's ratio -- but fstr_ctrl_get_HYPERELASTIC takes the two
# numbers as C10 and D1: shear modulus 4.2e5 beside a bulk modulus 2 / D1 = 4, and the whole load of 4e5 in one sub-step.  The residual
# is NaN from the first Newton iteration on and the run stops at the 50th.  What is recorded is that outcome: the rows of FSTR.sta,
# the incrementation lines of the standard output and the number of printed steps -> tests/golden/hyper_1elem_neohooke.json.
NOT_CONVERGING = {"1elem_neohooke": ("hyper1", "neohooke.msh", "neohooke.cnt")}


def record_not_converging():
    out = {}
    for name, (deck, mesh, cnt) in NOT_CONVERGING.items():
        r = f1.run_deck("fistr1_ref", deck, mesh, cnt, threads=2)
        assert "FrontISTR Completed !!" not in r["stdout"]
        out[name] = {"sta": [list(row) for row in r["sta"]], "step_lines": f1.step_lines(r["stdout"]), "printed_steps": len(r["log"])}
        print(name, out[name]["sta"], out[name]["step_lines"][-1])
    with open(os.path.join(HERE, "hyper_1elem_neohooke.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def deck_args(name):
    et, n, mat, two = DECKS[name]
    return ([str(n), str(SUBSTEPS), "CG", "1", str(STRETCH)] + (["--etype", str(et)] if et != 361 else []) + ["--nl-material", mat]
            + (["--two-sections"] if two else []))


def write_deck(name, d):
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d] + deck_args(name), check=True,
                   stdout=subprocess.DEVNULL)


def _record(out, name, r):
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert len(r["sta"]) >= 1 and len(r["log"]) >= 1
    out[name + "/log"] = np.array(json.dumps(r["log"]))
    out[name + "/newton"] = np.array([row[3] for row in r["sta"]], dtype=np.int32)
    print(name, "steps", len(r["log"]), "Newton", out[name + "/newton"], "U3 max", r["log"][-1]["Node"]["U3"][0])


if __name__ == "__main__":
    record_not_converging()
    out = {}
    for name in DECKS:
        with tempfile.TemporaryDirectory() as d:
            write_deck(name, d)
            r = f1.run("fistr1_ref", d, threads=2)
            assert len(r["sta"]) == SUBSTEPS
            _record(out, name, r)
    for name, (deck, mesh, cnt) in REFERENCE_DECKS.items():
        _record(out, name, f1.run_deck("fistr1_ref", deck, mesh, cnt, threads=2))
    np.savez_compressed(os.path.join(HERE, "hyper_decks.npz"), **out)
