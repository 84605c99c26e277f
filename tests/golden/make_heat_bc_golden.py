#!/usr/bin/env python3
"""Record the reference's heat example decks with surface terms through its own main program: tests/golden/heat_bc_decks.npz.

    python tests/golden/make_heat_bc_golden.py

Runs the unmodified oracle/_ref/fistr1_ref (built by __graft_entry__.build(), CPU only) on the decks of tests/heat_bc_decks.RECORDED
exactly as make_heat_golden.py runs its decks (control copies with `!WRITE,RESULT`, no visualizer block, a !SOLVER tolerance of
1e-12, one thread): exP/P341 .. P362 (!DFLUX on a face), exQ/Q341 .. Q362 (!FILM), exR/R341 .. R362 (!RADIATE; itmax = 100 on the
!HEAT line of R340.cnt and R350.cnt), exS/S341 .. S362 (!DFLUX, BF), and two transient variants written here in full into
tests/golden/decks/heat/golden/: S361T and S352T, the meshes of exS/S361 and exS/S352 with two-row density and specific heat
tables, an initial temperature of 100 on every node, an !AMPLITUDE whose rows (0.003 .. 0.005) lie inside the run, and a control
file with !DFLUX (the XMAX face and BF on HGEN), !FILM (the XMAX face and two more faces of HGEN -- on S352T a triangle and a
quadrilateral -- with the amplitude on the sink) and !RADIATE together, on the fixed steps of N361T (0.002 to 0.007: the
amplitude is taken below its first row, between its rows and twice beyond its last).

Recorded per deck, as heat_decks.npz: the node ids and temperatures of every result file (17 digits), and the `iterALL CHK` lines
of FSTR.msg (7 digits) with the step they belong to."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import heat_bc_decks as BD      # noqa: E402
import make_heat_golden as G    # noqa: E402

AMPLITUDE = "!AMPLITUDE, NAME=SINKAMP\n 1.0, 0.003, 0.5, 0.005\n"
# per variant: the face of the XMAX group (that of the exQ deck of the type) and two faces of the HGEN group
FACES = {"S361T": (4, 1, 3), "S352T": (3, 1, 4)}
CNT = """!SOLUTION,TYPE=HEAT
!HEAT
%(heat)s
!FIXTEMP
 XMIN,   0.0
!DFLUX
 XMAX, S%(f)d, 2500.0
 HGEN, BF, 2500.0
!FILM, AMP2=SINKAMP
 XMAX, F%(f)d, 25.0, 600.0
 HGEN, F%(g)d, 10.0, 300.0
 HGEN, F%(h)d, 10.0, 300.0
!RADIATE
 XMAX, R%(f)d, 1.1164E-8, 600.0
 HGEN, R%(g)d, 1.1164E-8, 600.0
!RESTART, FREQUENCY=100000
!SOLVER,METHOD=1,PRECOND=2,ITERLOG=NO,TIMELOG=NO
 2000,  1, 10, 10
 1.0e-12, 1.0, 0.0
!WRITE,RESULT
!END
"""


def write_inputs():
    os.makedirs(BD.GOLDEN_CNT, exist_ok=True)
    for name, (d, msh, cnt) in BD.RECORDED.items():
        if name in BD.TRANSIENT:
            base = name[:-1]
            s = G.transient_mesh(os.path.join(BD.DECKS, "exS", base + ".msh"))
            s = s.replace("!INITIAL CONDITION", AMPLITUDE + "!INITIAL CONDITION")
            with open(os.path.join(BD.GOLDEN_CNT, msh), "w") as f:
                f.write(s)
            f_, g_, h_ = FACES[name]
            s = CNT % dict(heat=G.HEAT_LINE, f=f_, g=g_, h=h_)
        else:
            s = G.control_copy(os.path.join(BD.DECKS, d, cnt))
        with open(os.path.join(BD.GOLDEN_CNT, name + ".cnt"), "w") as f:
            f.write(s)


def run(name):
    d, msh, _ = BD.RECORDED[name]
    tmp = tempfile.mkdtemp(prefix="heat_bc_golden_")
    try:
        shutil.copy(os.path.join(BD.DECKS, d, msh), os.path.join(tmp, msh))
        shutil.copy(os.path.join(BD.GOLDEN_CNT, name + ".cnt"), os.path.join(tmp, name + ".cnt"))
        with open(os.path.join(tmp, "hecmw_ctrl.dat"), "w") as f:
            f.write("!MESH, NAME=fstrMSH,TYPE=HECMW-ENTIRE\n %s\n!CONTROL,NAME=fstrCNT\n %s\n!RESULT,NAME=fstrRES,IO=OUT\n out.res\n"
                    "!RESTART,NAME=restart_out,IO=OUT\n out.restart\n" % (msh, name + ".cnt"))
        env = dict(os.environ, OMP_NUM_THREADS="1")
        r = subprocess.run([G.EXE], cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("%s: fistr1 ended with %d\n%s" % (name, r.returncode, r.stdout[-2000:]))
        res = sorted((int(f.rsplit(".", 1)[1]), f) for f in os.listdir(tmp) if f.startswith("out.res.0."))
        temps, ids = [], None
        for _, f in res:
            tok = open(os.path.join(tmp, f)).read().split("TEMPERATURE", 1)[1].split()
            ids = np.array([int(x) for x in tok[0::2]])
            temps.append([float(x) for x in tok[1::2]])
        hist, step = [], 1 if name not in BD.TRANSIENT else 0
        for line in open(os.path.join(tmp, "FSTR.msg")):
            if "INCREMENT NO." in line:
                step += 1
            m = re.match(r"^\s+(\d+)\s+([0-9.]+E[-+]\d+)\s*$", line)
            if m:
                hist.append((step, int(m.group(1)), float(m.group(2))))
        return ids, np.array(temps), np.array(hist)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    if not os.path.exists(G.EXE):
        sys.exit("oracle/_ref/fistr1_ref missing: run __graft_entry__.build() where the reference tree is present")
    write_inputs()
    rec = {}
    for name in BD.RECORDED:
        ids, temps, hist = run(name)
        rec[name + "_ids"], rec[name + "_temp"], rec[name + "_hist"] = ids, temps, hist
        print("%-6s %4d nodes, %d result files, iterALL per step %s" % (
            name, ids.size, temps.shape[0], [int((hist[:, 0] == s).sum()) for s in sorted(set(hist[:, 0]))]))
    np.savez_compressed(os.path.join(HERE, "heat_bc_decks.npz"), **rec)


if __name__ == "__main__":
    main()
