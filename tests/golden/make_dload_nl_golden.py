#!/usr/bin/env python3
"""Record what the UNMODIFIED reference program (oracle/_ref/fistr1_ref, CPU) computes for the cantilever decks of
tests/dload_nl_decks.py: each deck with `!DLOAD` as it is (the load follows the deformation) and with `!DLOAD, FOLLOW=NO`; the
Global summaries of every printed step of 0.log and the Newton count of every sub-step (FSTR.sta) -> tests/golden/dload_nl.npz,
the decks themselves -> tests/golden/decks/dload/<deck>_<follow|fixed>/.

The two runs of a deck must differ by more than 1 % in at least one displacement extremum of the last step: otherwise a library
that ignores `follow` would pass, and the pressure of the deck has to be raised.
Run where the reference is built: python tests/golden/make_dload_nl_golden.py"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import fistr1_run as f1      # noqa: E402
import dload_nl_decks as D               # noqa: E402


def run(name, follow):
    keep = os.path.join(D.DECKDIR, D.tag(name, follow))
    D.write_deck(name, follow, keep)
    with tempfile.TemporaryDirectory() as d:
        for f in ("cube.msh", "cube.cnt", "hecmw_ctrl.dat"):
            shutil.copy(os.path.join(keep, f), d)
        r = f1.run("fistr1_ref", d, threads=2)
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-3000:]
    assert len(r["sta"]) == D.SUBSTEPS and len(r["log"]) >= D.SUBSTEPS
    return r


if __name__ == "__main__":
    out = {}
    for name in D.NAMES:
        last = {}
        for follow in (True, False):
            r = run(name, follow)
            t = D.tag(name, follow)
            out[t + "/log"] = np.array(json.dumps(r["log"]))
            out[t + "/newton"] = np.array([row[3] for row in r["sta"]], dtype=np.int32)
            last[follow] = r["log"][-1]["Node"]
            print(t, "Newton", out[t + "/newton"], {k: last[follow][k] for k in ("U1", "U2", "U3")})
        rel = max(abs(last[True][k][j] - last[False][k][j]) / max(abs(last[True][k][j]), 1e-300)
                  for k in ("U1", "U2", "U3") for j in (0, 1) if abs(last[True][k][j]) > 1e-3)
        print(name, "largest relative difference of a displacement extremum between the two runs: %.3f" % rel)
        assert rel > 0.01, "%s: the follower and the fixed load differ by %.4f only: raise the pressure" % (name, rel)
    np.savez_compressed(D.GOLDEN, **out)
    print("wrote", D.GOLDEN)
