#!/usr/bin/env python3
"""Record what the UNMODIFIED reference program (oracle/_ref/fistr1_ref, CPU) computes for the small nonlinear cube decks of wedges
and 20-node hexahedra of scripts/fistr1_cube_deck.py --etype 351|352|362 --nl-material ...: the Global summaries of every printed
step of 0.log and the Newton count of every sub-step (FSTR.sta) -> tests/golden/nl_c3_decks.npz.  The GPU tests rebuild the same
decks from the same script.  Decks: elastic total Lagrange, elastic updated Lagrange (`!ELASTIC, CAUCHY`), Mises BILINEAR updated
Lagrange (yields), Mises MULTILINEAR with a second, ELASTIC section -- each at 351 (n = 2), 352 (n = 1) and 362 (n = 1; n = 2 with two sections).
Run where the reference is built: python tests/golden/make_nl_c3_golden.py"""
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

YIELD0 = 450.0
# name -> (etype, n, material, two sections); SUBSTEPS = 3
DECKS = {}
for et, n in ((351, 2), (352, 1), (362, 1)):
    for mat, two in (("elastic_tl", False), ("elastic_ul", False), ("bilinear", False), ("multilinear", True)):
        # (two sections need two elements: the single 362 cell becomes the 2^3 cube there)
        DECKS["c%d_%s%s" % (et, mat, "_two" if two else "")] = (et, 2 if two and et == 362 else n, mat, two)


def deck_args(name):
    et, n, mat, two = DECKS[name]
    return [str(n), "3", "--etype", str(et), "--nl-material", mat] + (["--two-sections"] if two else [])


def write_deck(name, d):
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d] + deck_args(name), check=True,
                   stdout=subprocess.DEVNULL)


if __name__ == "__main__":
    out = {}
    for name, (et, n, mat, two) in DECKS.items():
        with tempfile.TemporaryDirectory() as d:
            write_deck(name, d)
            r = f1.run("fistr1_ref", d, threads=2)
            assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
            assert len(r["sta"]) == 3 and len(r["log"]) >= 1
            if mat in ("bilinear", "multilinear"):       # a stress above the initial yield stress is reached plastically only
                # (the largest Mises stress the program prints, nodal or element: the single-cell 352 / 362 cubes yield at some of an
                # element's 9 / 27 points only, and the Mises stress of the element's MEAN stress stays below the yield stress there)
                sms = max(r["log"][-1][k]["SMS"][0] for k in ("Node", "Element"))
                assert sms > YIELD0, (name, r["log"][-1]["Node"]["SMS"], r["log"][-1]["Element"]["SMS"])
            out[name + "/log"] = np.array(json.dumps(r["log"]))
            out[name + "/newton"] = np.array([row[3] for row in r["sta"]], dtype=np.int32)
            print(name, "steps", len(r["log"]), "Newton", out[name + "/newton"], "SMS max (node, element)",
                  r["log"][-1]["Node"]["SMS"][0], r["log"][-1]["Element"]["SMS"][0])
    np.savez_compressed(os.path.join(HERE, "nl_c3_decks.npz"), **out)
