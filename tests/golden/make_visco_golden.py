#!/usr/bin/env python3
"""Record what the UNMODIFIED reference program (oracle/_ref/fistr1_ref, CPU) computes for decks with the time-dependent materials,
viscoelastic (!VISCOELASTIC) and NORTON creep (!CREEP): the Global summaries of every printed step of 0.log and the Newton count of
every sub-step (FSTR.sta) -> tests/golden/visco_decks.npz.

- the reference's own one-element decks, committed copies under tests/golden/decks/visco1/: examples/static/1elem/creep, relax
  (NORTON; a STATIC step, then a VISCO step of ten increments), viscoe and viscof (viscoelastic; one VISCO step); all four run on the one mesh the reference ships three copies of;
- cube decks of scripts/fistr1_cube_deck.py --nl-material visco|visco_inf|norton for each of the six solid types (the sizes of the
  other recorded cube decks), SUBSTEPS VISCO increments -- for NORTON behind a STATIC step, so that the stress is not zero when the
  creep starts --, one F-bar viscoelastic deck and one deck with a viscoelastic and a Mises section.  The tests rebuild these decks
  from the same script.
tutorial 07 (viscoelastic) and 08 (creep) are recorded already (tests/golden/decks/t07, t08).
Run where the reference is built: python tests/golden/make_visco_golden.py"""
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

SUBSTEPS = 3
SIZES = {361: 2, 341: 2, 342: 1, 351: 2, 352: 1, 362: 1}
# material -> (top-face stretch, time increment): the viscoelastic decks relax over dt / tau = 0.5 per increment; the NORTON decks
# creep at stresses of 60 to 120 (the VISCO step applies the boundary group a second time) by 5 % to 50 % of their elastic strain per
# increment; the program refuses a time increment below 1e-4 (the default lower bound of the step control)
LOADS = {"visco": (0.005, 0.5), "visco_inf": (0.005, 0.5), "norton": (0.0003, 2.0e-4)}
# name -> (etype, n, material, two sections, FORM361 or None)
DECKS = {"v%d_%s" % (et, mat): (et, n, mat, False, None) for et, n in SIZES.items() for mat in ("visco", "norton")}
DECKS.update({"v361_visco_inf": (361, 2, "visco_inf", False, None), "v342_visco_inf": (342, 1, "visco_inf", False, None),
              "v361_visco_fbar": (361, 2, "visco", False, "FBAR"), "v361_visco_two": (361, 2, "visco", True, None),
              "v342_norton_two": (342, 1, "norton", True, None)})
# (the reference's relax.msh and viscoe.msh are byte for byte its creep.msh, which is the one copy kept)
REFERENCE_DECKS = {"1elem_creep": ("visco1", "creep.msh", "creep.cnt"), "1elem_relax": ("visco1", "creep.msh", "relax.cnt"),
                   "1elem_viscoe": ("visco1", "creep.msh", "viscoe.cnt"), "1elem_viscof": ("visco1", "creep.msh", "viscof.cnt")}


def deck_args(name):
    et, n, mat, two, form = DECKS[name]
    strain, dt = LOADS[mat]
    return ([str(n), str(SUBSTEPS), "CG", "1", repr(strain)] + (["--etype", str(et)] if et != 361 else []) + ["--nl-material", mat, "--visco-dt", repr(dt)]
            + (["--two-sections"] if two else []) + (["--form361", form] if form else []))


def write_deck(name, d):
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d] + deck_args(name), check=True,
                   stdout=subprocess.DEVNULL)


# examples/static/1elem/creep: the unmodified program does not finish it in this build.  Its STATIC step converges in one iteration;
# the first increment of the VISCO step (time_inc 0.1) runs into ITMAX=20 at a residual of 2.6e-2 and the program stops with
# `### Fail to Converge`: the first stress update of the NORTON element has set MatlMatrix's saved flag, every tangent after it is the
# elastic one, and at A q**n dt = 1e-10 * 40**5 * 0.1 the creep strain of an increment is as large as the elastic strain.  What is
# recorded is that outcome: the rows of FSTR.sta and the one printed step.
NOT_CONVERGING = ("1elem_creep",)


def _record(out, name, r):
    if name in NOT_CONVERGING:
        assert "FrontISTR Completed !!" not in r["stdout"] and "Fail to Converge" in r["stdout"], r["stdout"][-2000:]
    else:
        assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert len(r["sta"]) >= 1 and len(r["log"]) >= 1
    out[name + "/log"] = np.array(json.dumps(r["log"]))
    out[name + "/newton"] = np.array([row[3] for row in r["sta"]], dtype=np.int32)
    print(name, "steps", len(r["log"]), "Newton", out[name + "/newton"], "U3 max", r["log"][-1]["Node"]["U3"][0])


if __name__ == "__main__":
    out = {}
    for name in DECKS:
        with tempfile.TemporaryDirectory() as d:
            write_deck(name, d)
            r = f1.run("fistr1_ref", d, threads=2)
            assert len(r["sta"]) == SUBSTEPS + (1 if DECKS[name][2] == "norton" else 0), r["sta"]
            _record(out, name, r)
    for name, (deck, mesh, cnt) in REFERENCE_DECKS.items():
        _record(out, name, f1.run_deck("fistr1_ref", deck, mesh, cnt, threads=2))
    np.savez_compressed(os.path.join(HERE, "visco_decks.npz"), **out)
