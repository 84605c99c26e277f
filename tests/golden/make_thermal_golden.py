#!/usr/bin/env python3
"""Record what the UNMODIFIED reference program (oracle/_ref/fistr1_ref, CPU) computes for the small thermal-stress cube decks of
scripts/fistr1_cube_deck.py --linear --thermal: the Global summaries of 0.log -> tests/golden/thermal_decks.npz.  Per type the
smallest cube that holds what is tested: n = 1 for 342 / 352 / 362, n = 2 for 341 / 351 and for 361 in each of IC, B-bar, FI, a
two-section deck (two expansion coefficients) and one --mixed 1 deck.  The temperature (FIX 35, TOP 120, every other node the
initial condition's 25; reference temperature 20) is asserted not to be uniform inside at least one element of every deck.
Run where the reference is built: python tests/golden/make_thermal_golden.py"""
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

# name -> arguments after DIR
DECKS = {"t342_n1": ["1", "--etype", "342"], "t352_n1": ["1", "--etype", "352"], "t362_n1": ["1", "--etype", "362"],
         "t341_n2": ["2", "--etype", "341"], "t351_n2": ["2", "--etype", "351"],
         "t361_n2_ic": ["2", "--form361", "IC"], "t361_n2_bbar": ["2", "--form361", "BBAR"], "t361_n2_fi": ["2", "--form361", "FI"],
         "t361_n2_two": ["2", "--two-sections"], "tmixed1_n2": ["2", "--mixed", "1"]}
T_FIX, T_TOP, T_REF, T_INIT = 35.0, 120.0, 20.0, 25.0


def deck_mesh(name):
    """(coord, groups without materials, n) of a deck, in the library's node order."""
    from frontistr_amd.mesh import CubeMesh, MixedMesh, solid_mesh
    a = DECKS[name]
    n = int(a[0])
    if "--mixed" in a:
        m = MixedMesh(n, order=1)
    elif "--etype" in a:
        m = solid_mesh(n, int(a[a.index("--etype") + 1]))
    else:
        m = CubeMesh(n)
    return m, n


def deck_temperature(m, n):
    z = m.coord[:, 2]
    t = np.full(m.n_node, T_INIT)      # fstr_solve_NLGEOM.f90:52-60: the initial condition first, then the !TEMPERATURE groups
    t[z == 0.0] = T_FIX
    t[z == float(n)] = T_TOP
    return t


def write_deck(name, d):
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d] + DECKS[name] + ["--linear", "--thermal"],
                   check=True, stdout=subprocess.DEVNULL)


if __name__ == "__main__":
    out = {}
    for name in DECKS:
        m, n = deck_mesh(name)
        t = deck_temperature(m, n)
        conns = m.conns if hasattr(m, "conns") else [m.conn]
        assert any(np.ptp(t[c - 1], axis=1).max() > 0.0 for c in conns), name      # the temperature varies inside an element
        with tempfile.TemporaryDirectory() as d:
            write_deck(name, d)
            r = f1.run("fistr1_ref", d, threads=2)
            assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
            out[name + "/log"] = np.array(json.dumps(r["log"][-1]))
            print(name, "U3", r["log"][-1]["Node"]["U3"], "S33", r["log"][-1]["Element"]["S33"])
    np.savez_compressed(os.path.join(HERE, "thermal_decks.npz"), **out)
