#!/usr/bin/env python3
"""Record what the UNMODIFIED reference program (oracle/_ref/fistr1_ref, CPU) computes for small NLSTATIC cube decks with a
`!TEMPERATURE` load: the Global summaries of every printed step of 0.log and the Newton count of every sub-step (FSTR.sta)
-> tests/golden/nl_thermal_decks.npz; and the same for the reference's own
examples/static/thermal_stress/sample1 (tests/golden/decks/thermal_stress1, `!TEMPERATURE, READRESULT=8`).  The decks are those of scripts/fistr1_cube_deck.py, edited the way
tests/test_gpu_fistr1_thermal.py edits its deck: `!TEMPERATURE` on the node group TOP, `!REFTEMP`, `!EXPANSION_COEFF` (and, with
tables, `!ELASTIC, DEPENDENCIES=1` / `!EXPANSION_COEFF, DEPENDENCIES=1`) and, where named, `!INITIAL CONDITION, TYPE=TEMPERATURE`
in the mesh file.  Three sub-steps each, so that last_temp matters from the second on.  tests/nl_thermal_ref.py (THERMAL_DECKS,
golden_deck) restates the same decks.  Run where the reference is built: python tests/golden/make_nl_thermal_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import fistr1_run as f1      # noqa: E402
import nl_thermal_ref as NT              # noqa: E402


def deck_args(name):
    d = NT.THERMAL_DECKS[name]
    return ([str(d["n"]), "3", "CG", "1", str(d["strain"])] + (["--etype", str(d["etype"])] if d["etype"] != 361 else [])
            + (["--nl-material", d["material"]] if d["material"] != "multilinear" or d["etype"] != 361 else [])
            + (["--form361", "FBAR"] if d["fbar"] else []))


def _rows(tab):
    return "".join(" " + ", ".join(repr(float(v)) for v in row) + "\n" for row in tab)


def write_deck(name, d):
    spec = NT.THERMAL_DECKS[name]
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d] + deck_args(name), check=True,
                   stdout=subprocess.DEVNULL)
    p = os.path.join(d, "cube.cnt")
    with open(p) as fh:
        s = fh.read()
    step = "!STEP, SUBSTEPS=3, CONVERG=1.0e-3\n BOUNDARY, 1\n"
    assert s.count(step) == 1
    # (the step must name the load group, or the card's temperature is never applied: fstr_isLoadActive, fstr_ass_load.f90:290)
    s = s.replace(step, "!TEMPERATURE, GRPID=1\n TOP, %r\n!REFTEMP\n %r\n" % (spec["temp_top"], spec["ref_temp"]) + step + " LOAD, 1\n")
    if spec["material"] == "mooney":
        card = "!HYPERELASTIC, TYPE=MOONEY-RIVLIN\n 0.1486, 0.4849, 0.0789\n"
        assert s.count(card) == 1
        s = s.replace(card, card + "!EXPANSION_COEFF\n %r\n" % NT.DECK_ALPHA)
    else:
        card = "!ELASTIC\n 206900.0, 0.29\n"
        assert s.count(card) == 1
        if spec["tables"]:
            s = s.replace(card, "!ELASTIC, DEPENDENCIES=1\n" + _rows(NT.ELASTIC_TAB) + "!EXPANSION_COEFF, DEPENDENCIES=1\n" + _rows(NT.ALPHA_TAB))
        else:
            s = s.replace(card, card + "!EXPANSION_COEFF\n %r\n" % NT.DECK_ALPHA)
    with open(p, "w") as fh:
        fh.write(s)
    if spec["temp_init"] is not None:
        p = os.path.join(d, "cube.msh")
        with open(p) as fh:
            s = fh.read()
        k = s.index("!NGROUP")
        s = s[:k] + "!INITIAL CONDITION, TYPE=TEMPERATURE\n ALL, %r\n" % spec["temp_init"] + s[k:]
        with open(p, "w") as fh:
            fh.write(s)


def run_sample1(d, binary="fistr1_ref", env=None):
    """The reference's examples/static/thermal_stress/sample1 (tests/golden/decks/thermal_stress1: mesh, control file, hecmw_ctrl.dat and
    the eight temperature result files V361.res.0.*) with the harness's usual work-arounds and the fstrTEMP entry its control file needs"""
    import shutil
    f1.prepare(NT.SAMPLE1, d, "A361.msh", "A300.cnt")
    for k in range(1, 9):
        shutil.copy(os.path.join(f1.DECKS, NT.SAMPLE1, "V361.res.0.%d" % k), d)
    with open(os.path.join(d, "hecmw_ctrl.dat"), "a") as fh:
        fh.write("!RESULT,NAME=fstrTEMP,IO=IN\n V361.res\n")
    return f1.run(binary, d, threads=2, env=env)


if __name__ == "__main__":
    out = {}
    for name in NT.THERMAL_DECKS:
        with tempfile.TemporaryDirectory() as d:
            write_deck(name, d)
            r = f1.run("fistr1_ref", d, threads=2)
            assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], (name, r["stdout"][-2000:])
            assert len(r["sta"]) == 3 and len(r["log"]) >= 1, name
            out[name + "/log"] = np.array(json.dumps(r["log"]))
            out[name + "/newton"] = np.array([row[3] for row in r["sta"]], dtype=np.int32)
            print(name, "steps", len(r["log"]), "Newton", out[name + "/newton"], "SMS max (node, element)",
                  r["log"][-1]["Node"]["SMS"][0], r["log"][-1]["Element"]["SMS"][0])
    with tempfile.TemporaryDirectory() as d:
        r = run_sample1(d)
        assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
        assert len(r["sta"]) == 1
        out[NT.SAMPLE1 + "/log"] = np.array(json.dumps(r["log"]))
        out[NT.SAMPLE1 + "/newton"] = np.array([row[3] for row in r["sta"]], dtype=np.int32)
        print(NT.SAMPLE1, "steps", len(r["log"]), "Newton", out[NT.SAMPLE1 + "/newton"], "SMS max", r["log"][-1]["Node"]["SMS"][0])
    np.savez_compressed(os.path.join(HERE, "nl_thermal_decks.npz"), **out)
