"""tests/golden/mixed_decks.npz: what the REFERENCE's own fistr1 (oracle/_ref/fistr1_ref, unmodified) assembles and prints for
small linear static decks of SEVERAL solid element types:

- tests/golden/decks/refine/hexpritet (361 + 351 + 341) and refine/tetpri (341 + 351): sample.msh / sample.cnt of the reference's
  examples/static/refine, run unrefined through oracle/fistr1_run.prepare (its hecmw_ctrl.dat has no REFINE, i.e. 0);
- scripts/fistr1_cube_deck.py --linear --mixed 1|2 at n = 2 (361 + 351 + 341, 362 + 352 + 342), one material and --two-sections.

`!SOLVER ... DUMPTYPE=BSR` (hecmw_matrix_dump.f90) gives the assembled K after the boundary conditions and the right-hand side;
0.log gives the extrema of the run (the two reference decks have no *_correct.log: these recorded extrema are what the fistr1
tests compare with).  Build container only (needs oracle/_ref/fistr1_ref)."""
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

REF_DECKS = [("hexpritet", "refine/hexpritet"), ("tetpri", "refine/tetpri")]
CUBE_DECKS = [("m1_n2", 1, 2, False), ("m1_n2_two", 1, 2, True), ("m2_n2", 2, 2, False), ("m2_n2_two", 2, 2, True)]


def add_dump(cnt):
    s = open(cnt).read()
    s = re.sub(r"^(!SOLVER[^\n]*?),?\s*$", r"\1,DUMPTYPE=BSR", s, count=1, flags=re.M)
    open(cnt, "w").write(s)


def record(out, name, td):
    r = f1.run("fistr1_ref", td)
    assert r["returncode"] == 0 and "FrontISTR Completed" in r["stdout"], r["stdout"][-2000:]
    m = hecmw_dump.read_bsr(os.path.join(td, "dump_matrix_1_0.bsr"))
    for k in ("indexL", "itemL", "indexU", "itemU", "D", "AL", "AU"):
        out["%s/%s" % (name, k)] = np.asarray(getattr(m, k))
    out[name + "/B"] = hecmw_dump.read_vector(os.path.join(td, "dump_matrix_1_0.rhs"))
    out[name + "/log"] = np.array(json.dumps(r["log"][-1]))


if __name__ == "__main__":
    out = {}
    for name, deck in REF_DECKS:
        with tempfile.TemporaryDirectory() as td:
            f1.prepare(deck, td, "sample.msh", "sample.cnt", iterlog="NO")
            add_dump(os.path.join(td, "sample.cnt"))
            record(out, name, td)
    for name, order, n, two in CUBE_DECKS:
        with tempfile.TemporaryDirectory() as td:
            args = [sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), td, str(n), "--linear", "--mixed", str(order)]
            subprocess.run(args + (["--two-sections"] if two else []), check=True, stdout=subprocess.DEVNULL)
            add_dump(os.path.join(td, "cube.cnt"))
            record(out, name, td)
    path = os.path.join(HERE, "mixed_decks.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
