#!/usr/bin/env python3
"""Record what the UNMODIFIED reference program (oracle/_ref/fistr1_ref, CPU) computes for F-bar decks (`!SECTION, FORM361=FBAR`): the
Global summaries of every printed step of 0.log and the Newton count of every sub-step (FSTR.sta) -> tests/golden/nl_fbar_decks.npz.

- cube decks of scripts/fistr1_cube_deck.py --form361 FBAR, TYPE=361, n = 2, 3 sub-steps: ELASTIC total Lagrange (the top face pulled
  by 0.5 %), Neo-Hooke, Mooney-Rivlin and Arruda-Boyce (pulled by 10 %), and one --two-sections deck (Mooney-Rivlin beside ELASTIC
  2.5 / 0.3, total Lagrange).  The tests rebuild these decks from the same script.  The script states Mises only with the updated
  Lagrange flag of `!PLASTIC`, which Update_C3D8Fbar does not define (static_LIB_Fbar.f90:600-602), so there is no Mises deck.
- the reference's own examples/static/FbarElement/T01_BEAM_HYPERELASTIC (committed copy: tests/golden/decks/static/FbarElement),
  Mooney-Rivlin, one sub-step under a nodal load.
Run where the reference is built: python tests/golden/make_nl_fbar_golden.py"""
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

SUBSTEPS, N = 3, 2
# name -> (material of --nl-material, stretch, two sections)
DECKS = {"f361_elastic_tl": ("elastic_tl", 0.005, False), "f361_neohooke": ("neohooke", 0.1, False), "f361_mooney": ("mooney", 0.1, False),
         "f361_arruda": ("arruda", 0.1, False), "f361_mooney_two": ("mooney", 0.1, True)}
REFERENCE_DECKS = {"T01_BEAM_HYPERELASTIC": ("static/FbarElement", "T01_BEAM_HYPERELASTIC.msh", "T01_BEAM_HYPERELASTIC.cnt")}


def deck_args(name):
    mat, stretch, two = DECKS[name]
    return [str(N), str(SUBSTEPS), "CG", "1", str(stretch), "--nl-material", mat, "--form361", "FBAR"] + (["--two-sections"] if two else [])


def write_deck(name, d):
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d] + deck_args(name), check=True,
                   stdout=subprocess.DEVNULL)


def _record(out, name, r):
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert len(r["sta"]) >= 1 and len(r["log"]) >= 1
    out[name + "/log"] = np.array(json.dumps(r["log"]))
    out[name + "/newton"] = np.array([row[3] for row in r["sta"]], dtype=np.int32)
    print(name, "steps", len(r["log"]), "Newton", out[name + "/newton"])


if __name__ == "__main__":
    out = {}
    for name in DECKS:
        with tempfile.TemporaryDirectory() as d:
            write_deck(name, d)
            r = f1.run("fistr1_ref", d, threads=2)
            assert len(r["sta"]) == SUBSTEPS
            _record(out, name, r)
    for name, (deck, mesh, cnt) in REFERENCE_DECKS.items():
        _record(out, name, f1.run_deck("fistr1_ref", deck, mesh, cnt, threads=2))
    np.savez_compressed(os.path.join(HERE, "nl_fbar_decks.npz"), **out)
