#!/usr/bin/env python3
"""Record what fstr_NodalStress3D leaves in fstrSOLID through the reference's own main program: tests/golden/nodal_stress.npz
(the linear decks) and tests/golden/nodal_stress_nl.npz (the nonlinear ones; one file would exceed the size limit of a committed file).

    python tests/golden/make_nodal_stress_golden.py

Runs the unmodified oracle/_ref/fistr1_ref (built by __graft_entry__.build(), CPU only) on the decks of
tests/nodal_stress_decks.RECORDED: exB/B341 .. B362 (linear static, one type each), refine/hexpritet (linear static, TYPE=361, 351 and 341 in one mesh),
autoinc/C3D8beam (NLSTATIC, a TYPE=361 cantilever, ten sub-steps of automatic incrementation, the last one recorded) and t05/necking (NLSTATIC, Mises MULTILINEAR,
TYPE=361; the reference converges eight sub-steps and gives up in the ninth, as tests/golden/decks/t05/necking_fistr1_ref_FSTR.sta
shows: the result file of the last converged sub-step is recorded).  Every deck runs with a control copy written here into
tests/golden/decks/nodal_stress/: the deck's own cards without the visualizer and without its own output blocks, with
`!WRITE,RESULT` and an `!OUTPUT_RES` block that turns on ISTRAIN, ISTRESS (the quadrature-point arrays:
the inputs), NSTRAIN, NSTRESS, NMISES, ESTRAIN, ESTRESS, EMISES, PRINC_NSTRESS, PRINCV_NSTRESS, PRINC_NSTRAIN, PRINC_ESTRESS and
PRINCV_ESTRESS.  ISTRAIN / ISTRESS come out per quadrature point for all six types (GaussSTRAIN1 .. GaussSTRAINnq), so no type's
point arrays are taken from anywhere else.

The result files hold 17 significant digits (`%.16E`, counted here from the file), which round-trip a double exactly; recorded per
deck: node and element ids, the point arrays (n_elem, nq, 6) -- for the mesh of several types flat, the groups one after the other
in hecMESH's order, [elem][point][6] inside a group -- and the result arrays; vectors as (n, vector, component).

The script then holds tests/nodal_stress_ref.py against every recorded array and prints the largest deviation relative to the
array's largest magnitude, and the share of nodes / elements whose principal values are not separated by 1e-6 of the largest:
the figures behind the bounds of tests/test_nodal_stress_ref.py and DESIGN.md section 5."""
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
import nodal_stress_decks as ND      # noqa: E402
import nodal_stress_ref as NR        # noqa: E402

EXE = os.path.join(ROOT, "oracle", "_ref", "fistr1_ref")
OUTPUT_BLOCK = ["!OUTPUT_RES"] + [" %s, ON" % f for f in ND.FIELDS]


def control_copy(src, frequency=None):
    """the deck's control file without visualizer and output blocks, with !WRITE,RESULT and the !OUTPUT_RES block above"""
    out, skip = [], False
    for line in open(src).read().split("\n"):
        u = line.strip().upper().replace(" ", "")
        if u.startswith("!VISUAL") or u.startswith("!END"):
            break
        if u.startswith("!"):
            skip = u.startswith("!OUTPUT_")
        if skip or u.startswith("!WRITE") or u.startswith("!!") or u.startswith("#") or not u:
            continue
        if u.startswith("!SOLVER"):
            out.append("!WRITE,RESULT" + (",FREQUENCY=%d" % frequency if frequency else ""))
            out += OUTPUT_BLOCK
            out.append("!RESTART, FREQUENCY=100000")     # the work-around of oracle/fistr1_run.py: restart_nout = 0 is divided by
            line = re.sub(r",\s*(ITERLOG|TIMELOG)\s*=\s*\w+", "", line, flags=re.I).rstrip(", ") + ",ITERLOG=NO,TIMELOG=NO"
        out.append(line)
    return "\n".join(out + ["!END", ""])


def write_inputs():
    os.makedirs(ND.GOLDEN_CNT, exist_ok=True)
    for name, (d, _, cnt) in ND.RECORDED.items():
        with open(os.path.join(ND.GOLDEN_CNT, name + ".cnt"), "w") as f:
            f.write(control_copy(os.path.join(ND.DECKS, d, cnt)))


def read_result(path):
    """one result file -> (node ids, {label: (n_node, ncomp)}, element ids, {label: (n_elem, ncomp)}, significant digits)"""
    text = open(path).read()
    digits = max(len(m.group(1)) + 1 for m in re.finditer(r"\d\.(\d+)E[-+]\d+", text))
    tok = text.split()
    assert tok[0] == "*fstrresult", tok[0]
    n_node, n_elem, nn_item, ne_item = (int(x) for x in tok[1:5])
    at = 5

    def block(n, n_item):
        nonlocal at
        ncomp = [int(x) for x in tok[at:at + n_item]]
        labels = tok[at + n_item:at + 2 * n_item]
        at += 2 * n_item
        w = 1 + sum(ncomp)
        rows = np.array(tok[at:at + n * w], dtype=object).reshape(n, w)
        at += n * w
        ids = rows[:, 0].astype(np.int64)
        vals = rows[:, 1:].astype(np.float64)
        out, c = {}, 0
        for lab, k in zip(labels, ncomp):
            out[lab] = vals[:, c:c + k]
            c += k
        return ids, out
    nid, nodal = block(n_node, nn_item)
    eid, elem = block(n_elem, ne_item)
    assert at == len(tok), (at, len(tok))
    return nid, nodal, eid, elem, digits


def run(name):
    d, msh, _ = ND.RECORDED[name]
    tmp = tempfile.mkdtemp(prefix="nodal_golden_")
    try:
        shutil.copy(os.path.join(ND.DECKS, d, msh), os.path.join(tmp, msh))
        shutil.copy(os.path.join(ND.GOLDEN_CNT, name + ".cnt"), os.path.join(tmp, name + ".cnt"))
        with open(os.path.join(tmp, "hecmw_ctrl.dat"), "w") as f:
            f.write("!MESH, NAME=fstrMSH,TYPE=HECMW-ENTIRE\n %s\n!CONTROL,NAME=fstrCNT\n %s\n!RESULT,NAME=fstrRES,IO=OUT\n out.res\n"
                    "!RESTART,NAME=restart_out,IO=OUT\n out.restart\n" % (msh, name + ".cnt"))
        env = dict(os.environ, OMP_NUM_THREADS="1")
        r = subprocess.run([EXE], cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
        if r.returncode != 0:
            raise RuntimeError("%s: fistr1 ended with %d\n%s" % (name, r.returncode, r.stdout[-2000:]))
        last = max((int(f.rsplit(".", 1)[1]), f) for f in os.listdir(tmp) if f.startswith("out.res.0."))
        return last[0], read_result(os.path.join(tmp, last[1]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def arrays(name, res):
    """the recorded arrays of one deck under the names of the !OUTPUT_RES block"""
    nid, nodal, eid, elem, _ = res
    ids, groups, eorder = ND.load(name)
    assert np.array_equal(nid, ids) and np.array_equal(eid, eorder), name

    def gauss(stem):
        """GaussSTRAINk holds point k of every element (zeros past an element's own points): -> per group [elem][point][6]"""
        out, e0 = [], 0
        for etype, conn in groups:
            ne = conn.shape[0]
            out.append(np.stack([elem["%s%d" % (stem, k + 1)][e0:e0 + ne] for k in range(NR.NQ[etype])], axis=1))
            e0 += ne
        return out[0] if len(out) == 1 else np.concatenate([x.ravel() for x in out])
    vec = lambda d, stem: np.stack([d[stem + "Vector%d" % (j + 1)] for j in range(3)], axis=1)
    return {"node_ids": nid.astype(np.int32), "elem_ids": eid.astype(np.int32),
            "ISTRAIN": gauss("GaussSTRAIN"), "ISTRESS": gauss("GaussSTRESS"),
            "NSTRAIN": nodal["NodalSTRAIN"], "NSTRESS": nodal["NodalSTRESS"], "NMISES": nodal["NodalMISES"][:, 0],
            "ESTRAIN": elem["ElementalSTRAIN"], "ESTRESS": elem["ElementalSTRESS"], "EMISES": elem["ElementalMISES"][:, 0],
            "PRINC_NSTRESS": nodal["NodalPrincipalSTRESS"], "PRINCV_NSTRESS": vec(nodal, "NodalPrincipalSTRESS"),
            "PRINC_NSTRAIN": nodal["NodalPrincipalSTRAIN"], "PRINC_ESTRESS": elem["ElementalPrincipalSTRESS"],
            "PRINCV_ESTRESS": vec(elem, "ElementalPrincipalSTRESS")}


def separated(vals, tol=1e-6):
    """items whose three principal values are pairwise separated by more than tol of the largest magnitude of the array"""
    s = tol * np.abs(vals).max()
    return (np.abs(vals[:, 0] - vals[:, 1]) > s) & (np.abs(vals[:, 1] - vals[:, 2]) > s) & (np.abs(vals[:, 0] - vals[:, 2]) > s)


def deviations(name, a):
    """restatement against the recorded arrays: {array: max |difference| / max |recorded|}, and the unseparated shares"""
    ids, groups, _ = ND.load(name)
    r = NR.nodal_stress(ids.size, groups, a["ISTRAIN"].ravel(), a["ISTRESS"].ravel(), principal=1 | 2 | 4 | 16 | 32)
    rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())
    dev = {"NSTRAIN": rel(r.strain, a["NSTRAIN"]), "NSTRESS": rel(r.stress, a["NSTRESS"]), "NMISES": rel(r.mises, a["NMISES"]),
           "ESTRAIN": rel(r.estrain, a["ESTRAIN"]), "ESTRESS": rel(r.estress, a["ESTRESS"]), "EMISES": rel(r.emises, a["EMISES"]),
           "PRINC_NSTRESS": rel(r.pstress, a["PRINC_NSTRESS"]), "PRINC_NSTRAIN": rel(r.pstrain, a["PRINC_NSTRAIN"]),
           "PRINC_ESTRESS": rel(r.epstress, a["PRINC_ESTRESS"])}
    share = {}
    for key, vals, got in (("PRINCV_NSTRESS", a["PRINC_NSTRESS"], r.pstress_vect), ("PRINCV_ESTRESS", a["PRINC_ESTRESS"], r.epstress_vect)):
        ok = separated(vals)
        share[key] = 1.0 - float(ok.mean())
        if not ok.any():        # a uniform stress state: no vector to compare
            continue
        want = a[key][ok]
        sign = np.sign(np.einsum("njc,njc->nj", got[ok], want))[:, :, None]
        dev[key] = float(np.abs(got[ok] * sign - want).max() / np.abs(a[key]).max())
    return dev, share


def main():
    if not os.path.exists(EXE):
        sys.exit("oracle/_ref/fistr1_ref missing: run __graft_entry__.build() where the reference tree is present")
    write_inputs()
    rec, worst, worst_vec = {ND.GOLDEN: {}, ND.GOLDEN_NL: {}}, 0.0, 0.0
    for name in ND.RECORDED:
        step, res = run(name)
        a = arrays(name, res)
        for k, v in a.items():
            rec[ND.golden_file(name)]["%s_%s" % (name, k)] = v
        dev, share = deviations(name, a)
        worst = max([worst] + [v for k, v in dev.items() if not k.startswith("PRINCV")])
        worst_vec = max([worst_vec] + [v for k, v in dev.items() if k.startswith("PRINCV")])
        print("%-8s step %3d, %4d nodes, %4d elements, %d digits; restatement - recorded, relative to the array's largest magnitude:"
              % (name, step, a["node_ids"].size, a["elem_ids"].size, res[4]))
        print("         " + ", ".join("%s %.2e" % kv for kv in dev.items()))
        print("         principal values not separated by 1e-6: " + ", ".join("%s %.1f %%" % (k, 100 * v) for k, v in share.items()))
    print("largest deviation of values %.3e, of separated vectors %.3e" % (worst, worst_vec))
    for path, arrs in rec.items():
        np.savez_compressed(path, **arrs)
        print("%s: %d bytes" % (os.path.relpath(path, ROOT), os.path.getsize(path)))


if __name__ == "__main__":
    main()
