#!/usr/bin/env python3
"""Record what the UNMODIFIED reference program (oracle/_ref/fistr1_ref, CPU) computes for the small nonlinear decks of the mixed
cube of scripts/fistr1_cube_deck.py --mixed 1|2 --nl-material ... (361 + 351 + 341, or 362 + 352 + 342 with shared mid-edge
nodes): the Global summaries of every printed step of 0.log and the Newton count of every sub-step (FSTR.sta) ->
tests/golden/nl_mixed_decks.npz, in the format of nl_c3_decks.npz.  The GPU tests rebuild the same decks from the same script.
Decks: elastic total Lagrange, elastic updated Lagrange (`!ELASTIC, CAUCHY`), Mises BILINEAR updated Lagrange (yields), Mises
MULTILINEAR with a second, ELASTIC section -- each at order 1 and 2 on the 2^3 cube, 3 sub-steps.
Run where the reference is built: python tests/golden/make_nl_mixed_golden.py"""
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
# name -> (order, n, material, two sections); SUBSTEPS = 3
DECKS = {"m%d_%s%s" % (order, mat, "_two" if two else ""): (order, 2, mat, two)
         for order in (1, 2)
         for mat, two in (("elastic_tl", False), ("elastic_ul", False), ("bilinear", False), ("multilinear", True))}
TYPES = {1: "341+351+361", 2: "342+352+362"}      # hecMESH holds the elements type by type in ascending order: the report line's


def deck_args(name):
    order, n, mat, two = DECKS[name]
    return [str(n), "3", "--mixed", str(order), "--nl-material", mat] + (["--two-sections"] if two else [])


def write_deck(name, d):
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d] + deck_args(name), check=True,
                   stdout=subprocess.DEVNULL)


if __name__ == "__main__":
    out = {}
    for name, (order, n, mat, two) in DECKS.items():
        with tempfile.TemporaryDirectory() as d:
            write_deck(name, d)
            r = f1.run("fistr1_ref", d, threads=2)
            assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
            assert len(r["sta"]) == 3 and len(r["log"]) >= 1
            if mat in ("bilinear", "multilinear"):       # a stress above the initial yield stress is reached plastically only
                sms = max(r["log"][-1][k]["SMS"][0] for k in ("Node", "Element"))
                assert sms > YIELD0, (name, r["log"][-1]["Node"]["SMS"], r["log"][-1]["Element"]["SMS"])
            out[name + "/log"] = np.array(json.dumps(r["log"]))
            out[name + "/newton"] = np.array([row[3] for row in r["sta"]], dtype=np.int32)
            print(name, "steps", len(r["log"]), "Newton", out[name + "/newton"], "SMS max (node, element)",
                  r["log"][-1]["Node"]["SMS"][0], r["log"][-1]["Element"]["SMS"][0])
    np.savez_compressed(os.path.join(HERE, "nl_mixed_decks.npz"), **out)
