"""tests/golden/c3_decks.npz: what the REFERENCE's own fistr1 (oracle/_ref/fistr1_ref, unmodified) assembles and prints for
small linear static cube decks of wedges and 20-node hexahedra, scripts/fistr1_cube_deck.py --linear --etype 351|352|362:
`!SOLVER ... DUMPTYPE=BSR` (hecmw_matrix_dump.f90) gives the assembled K after the boundary conditions and the right-hand side;
0.log gives the extrema of the run.  Decks: the 2x2x2 cube at each type with one material and with two sections
(--two-sections).  Build container only (needs oracle/_ref/fistr1_ref)."""
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

DECKS = [("c351_n2", 351, 2, False), ("c351_n2_two", 351, 2, True), ("c352_n2", 352, 2, False), ("c352_n2_two", 352, 2, True),
         ("c362_n2", 362, 2, False), ("c362_n2_two", 362, 2, True)]


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
    path = os.path.join(HERE, "c3_decks.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
