#!/usr/bin/env python3
"""Record the reference's heat example decks through its own main program: tests/golden/heat_decks.npz.

    python tests/golden/make_heat_golden.py

Runs the unmodified oracle/_ref/fistr1_ref (built by __graft_entry__.build(), CPU only) on the decks of tests/heat_decks.RECORDED:
exN/N341 .. N362 (conductivity 50 -> 35 over 0 .. 500, !FIXTEMP), exO/O341 .. O362 (!CFLUX), exM/MA361, MB361, MG361, and two
transient variants of N361 and N342.  Every deck runs with a control copy written here into tests/golden/decks/heat/golden/:
the deck's own cards with `!WRITE,RESULT`, no visualizer block and a !SOLVER tolerance of 1e-12, so that the linear solver's
residual does not set the comparison.  The transient variants are written out in full: a !HEAT line of fixed steps
(0.002 to 0.007: three whole steps and a clipped one), and a mesh copy with two-row density and specific heat tables and an
initial temperature of 100 on every node.

Recorded per deck: the node ids and temperatures of every result file (17 digits), and the `iterALL CHK` lines of FSTR.msg
(7 digits) with the step they belong to."""
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
import heat_decks as HD      # noqa: E402

EXE = os.path.join(ROOT, "oracle", "_ref", "fistr1_ref")
HEAT_LINE = " 0.002, 0.007, 0.0, 0.0, 20, 1.0e-6"


def control_copy(src):
    """the deck's control file with !WRITE,RESULT, a solver tolerance of 1e-12 and without the visualizer"""
    out, solver_line = [], 0
    for line in open(src).read().split("\n"):
        u = line.strip().upper().replace(" ", "")
        if u.startswith("!VISUAL") or u.startswith("!END"):
            break
        if u.startswith("!WRITE") or u.startswith("!!") or not u:
            continue
        if solver_line:
            solver_line += 1
            if solver_line == 3:
                a = [x.strip() for x in line.split(",")]
                line = " " + ", ".join(["1.0e-12"] + a[1:])
                solver_line = 0
        if u.startswith("!SOLVER"):
            solver_line = 1
            out.append("!RESTART, FREQUENCY=100000")     # the work-around of oracle/fistr1_run.py: restart_nout = 0 is divided by

            line = re.sub(r",\s*(ITERLOG|TIMELOG)\s*=\s*\w+", "", line, flags=re.I) + ",ITERLOG=NO,TIMELOG=NO"
        out.append(line)
    return "\n".join(out + ["!WRITE,RESULT", "!END", ""])


def transient_mesh(src):
    s = open(src).read()
    s = re.sub(r"^!NODE.*$", "!NODE, NGRP=NALL", s, count=1, flags=re.M)
    s = re.sub(r"!ITEM=1\s*\n.*\n", "!ITEM=1, SUBITEM=1\n 7.64E-6,   0.0\n 7.50E-6, 500.0\n", s, count=1)
    s = re.sub(r"!ITEM=2\s*\n.*\n", "!ITEM=2, SUBITEM=1\n 499.0,   0.0\n 540.0, 500.0\n", s, count=1)
    return s.replace("!END", "!INITIAL CONDITION, TYPE=TEMPERATURE\n NALL, 100.0\n!END")


def write_inputs():
    os.makedirs(HD.GOLDEN_CNT, exist_ok=True)
    for name, (d, msh, cnt) in HD.RECORDED.items():
        if name in HD.TRANSIENT:
            base = name[:-1]
            with open(os.path.join(HD.GOLDEN_CNT, msh), "w") as f:
                f.write(transient_mesh(os.path.join(HD.DECKS, "exN", base + ".msh")))
            s = control_copy(os.path.join(HD.DECKS, "exN", "N.cnt"))
            s = re.sub(r"^!HEAT\s*$", "!HEAT\n" + HEAT_LINE, s, count=1, flags=re.M)
        else:
            s = control_copy(os.path.join(HD.DECKS, d, cnt))
        with open(os.path.join(HD.GOLDEN_CNT, name + ".cnt"), "w") as f:
            f.write(s)


def run(name):
    d, msh, _ = HD.RECORDED[name]
    tmp = tempfile.mkdtemp(prefix="heat_golden_")
    try:
        shutil.copy(os.path.join(HD.DECKS, d, msh), os.path.join(tmp, msh))
        shutil.copy(os.path.join(HD.GOLDEN_CNT, name + ".cnt"), os.path.join(tmp, name + ".cnt"))
        with open(os.path.join(tmp, "hecmw_ctrl.dat"), "w") as f:
            f.write("!MESH, NAME=fstrMSH,TYPE=HECMW-ENTIRE\n %s\n!CONTROL,NAME=fstrCNT\n %s\n!RESULT,NAME=fstrRES,IO=OUT\n out.res\n"
                    "!RESTART,NAME=restart_out,IO=OUT\n out.restart\n" % (msh, name + ".cnt"))
        env = dict(os.environ, OMP_NUM_THREADS="1")
        r = subprocess.run([EXE], cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("%s: fistr1 ended with %d\n%s" % (name, r.returncode, r.stdout[-2000:]))
        res = sorted((int(f.rsplit(".", 1)[1]), f) for f in os.listdir(tmp) if f.startswith("out.res.0."))
        temps, ids = [], None
        for _, f in res:
            tok = open(os.path.join(tmp, f)).read().split("TEMPERATURE", 1)[1].split()
            ids = np.array([int(x) for x in tok[0::2]])
            temps.append([float(x) for x in tok[1::2]])
        hist, step = [], 1 if name not in HD.TRANSIENT else 0
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
    if not os.path.exists(EXE):
        sys.exit("oracle/_ref/fistr1_ref missing: run __graft_entry__.build() where the reference tree is present")
    write_inputs()
    rec = {}
    for name in HD.RECORDED:
        ids, temps, hist = run(name)
        rec[name + "_ids"], rec[name + "_temp"], rec[name + "_hist"] = ids, temps, hist
        print("%-6s %4d nodes, %d result files, iterALL per step %s" % (
            name, ids.size, temps.shape[0], [int((hist[:, 0] == s).sum()) for s in sorted(set(hist[:, 0]))]))
    np.savez_compressed(os.path.join(HERE, "heat_decks.npz"), **rec)


if __name__ == "__main__":
    main()
