"""tests/golden/tet_decks.npz: what the REFERENCE's own fistr1 (oracle/_ref/fistr1_ref, unmodified) assembles and prints for
small linear static tetrahedral cube decks of scripts/fistr1_cube_deck.py --linear --etype 341|342: `!SOLVER ... DUMPTYPE=BSR`
(hecmw_matrix_dump.f90) gives the assembled K after the boundary conditions and the right-hand side; 0.log gives the extrema
of the run.  Decks: the 2x2x2 cube at 341 with one material and with two sections (--two-sections), the 1x1x1 cube at 342
with one material and with two sections.  Build container only (needs oracle/_ref/fistr1_ref)."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
from frontistr_amd import hecmw_dump                         # noqa: E402
from oracle import fistr1_run as f1                          # noqa: E402

DECKS = [("t341_n2", 341, 2, False), ("t341_n2_two", 341, 2, True), ("t342_n1", 342, 1, False), ("t342_n1_two", 342, 1, True)]


def write_deck(d, etype, n, two):
    args = [sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d, str(n), "--linear", "--etype", str(etype)]
    subprocess.run(args + (["--two-sections"] if two else []), check=True, stdout=subprocess.DEVNULL)


if __name__ == "__main__":
    out = {}
    for name, etype, n, two in DECKS:
        with tempfile.TemporaryDirectory() as td:
            write_deck(td, etype, n, two)
            cnt = os.path.join(td, "cube.cnt")
            s = open(cnt).read()
            s = re.sub(r"^(!SOLVER[^\n]*)", r"\1,DUMPTYPE=BSR", s, count=1, flags=re.M)
            open(cnt, "w").write(s)
            r = f1.run("fistr1_ref", td)
            assert r["returncode"] == 0 and "FrontISTR Completed" in r["stdout"], r["stdout"][-2000:]
            m = hecmw_dump.read_bsr(os.path.join(td, "dump_matrix_1_0.bsr"))
            for k in ("indexL", "itemL", "indexU", "itemU", "D", "AL", "AU"):
                out["%s/%s" % (name, k)] = np.asarray(getattr(m, k))
            out[name + "/B"] = hecmw_dump.read_vector(os.path.join(td, "dump_matrix_1_0.rhs"))
            out[name + "/log"] = np.array(json.dumps(r["log"][-1]))
    path = os.path.join(HERE, "tet_decks.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
