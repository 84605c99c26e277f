#!/usr/bin/env python3
"""Per-colour cost of the Eisenstat CG + SSOR sweeps ("Round 5: the tail colours in one dataflow launch").

  layout OUT.json [--elems 149]     (GPU) the bench system's colour layout: slice range and L / U block positions of every colour
  table LAYOUT.json TRACE.csv       a rocprofv3 --kernel-trace CSV of `bench.py` -> the table: median duration of every colour's
                                    launch in each half sweep, its algorithmic bytes, its rate, and the cost of the latency-bound
                                    tail at the big colours' rate per byte

Algorithmic bytes of one colour (rows = 64 x slices, blocks = 64 x block positions, padding included as the kernels stream it):
  backward: 76 U blocks + rows x (72 diagonal factor + 24 dt + 24 ph read + 24 ph write + 24 p write)
  forward : 76 L blocks + rows x (72 diagonal factor + 24 ph + 24 p + 24 v + 24 w + 24 q)
gathered entries are not counted (they come from cache, as in bench.py's form_bytes).  Launch order per iteration: backward colours
ncolor-1 .. 0, then forward 0 .. ncolor-1; a dataflow launch (k_eis_*_df) covers the tail colours of its half sweep in one go.
"""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def layout(out, n):
    import ctypes as C
    import numpy as np
    from frontistr_amd import hecmw as hip
    from frontistr_amd.mesh import CubeMesh
    mesh = CubeMesh(n)
    hm = hip.hecmwST_local_mesh(n_node=mesh.n_node)
    hm.elem_node_item = mesh.conn.ravel()
    m = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext(device=0)
    ctx.upload(m, hm, what=hip.FX_UP_PROFILE)
    ctx.assemble_c3d8(mesh.coord, mesh.conn, 210000.0, 0.3, elemopt=1, load=mesh.load(), bc=mesh.dirichlet())
    m.Iarray[0], m.Iarray[1], m.Iarray[2] = 10, 1, 1
    ctx.precond_setup(m)
    buf = np.zeros(3 * 1024, dtype=np.int64)
    nc = C.c_int32(0)
    f = hip.lib().fx_debug_ssor_colours
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    hip._chk(f(ctx.h, hip._ptr(buf), buf.size, C.byref(nc)))
    k = nc.value + 1
    d = {"elems": n, "N": ctx.stats()["N"], "ncolor": nc.value, "color_slice": buf[:k].tolist(),
         "L_ptr": buf[k:2 * k].tolist(), "U_ptr": buf[2 * k:3 * k].tolist()}
    ctx.close()
    with open(out, "w") as fh:
        json.dump(d, fh)
    print("ncolor %d, slices per colour %s" % (d["ncolor"], [d["color_slice"][i + 1] - d["color_slice"][i] for i in range(d["ncolor"])]))


def colour_bytes(L, c, fwd):
    sl = L["color_slice"][c + 1] - L["color_slice"][c]
    ptr = L["L_ptr"] if fwd else L["U_ptr"]
    blocks = 64 * (ptr[c + 1] - ptr[c])
    return 76 * blocks + 64 * sl * (72 + 5 * 24)


def short(n):
    return re.sub(r"\(.*", "", n).replace("void ", "")


def table(lay_path, trace_path, big_min=None):
    L = json.load(open(lay_path))
    nc = L["ncolor"]
    slices = [L["color_slice"][i + 1] - L["color_slice"][i] for i in range(nc)]
    rows = []
    with open(trace_path) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    # iterations: the sweep launches between two k_eis_update launches of the fused loop
    iters, cur = [], []
    for s, e, n in rows:
        if n.startswith("k_eis_backward") or n.startswith("k_eis_forward"):
            cur.append((s, e, n))
        elif n.startswith("k_eis_update<1>") or n.startswith("k_eis_update<2>"):
            if cur:
                iters.append((cur, s, e))
            cur = []
    full = [it for it in iters if sum(1 for x in it[0] if "backward" in x[2]) >= 1 and sum(1 for x in it[0] if "forward" in x[2]) >= 1]
    if not full:
        raise SystemExit("no Eisenstat iterations in the trace")
    nb = sum(1 for x in full[0][0] if "backward" in x[2])
    nf = sum(1 for x in full[0][0] if "forward" in x[2])
    full = [it for it in full if sum(1 for x in it[0] if "backward" in x[2]) == nb and sum(1 for x in it[0] if "forward" in x[2]) == nf]
    med = lambda v: sorted(v)[len(v) // 2]
    # label the launches: a dataflow launch is the tail of its half sweep, every other launch is one colour
    def labels(seq, fwd):
        n_df = sum(1 for x in seq if "_df" in x[2])
        ntail = nc - (len(seq) - n_df)
        order = list(range(nc)) if fwd else list(range(nc - 1, -1, -1))
        tail = sorted(range(nc - ntail, nc))
        out, k = [], 0
        for x in seq:
            if "_df" in x[2]:
                out.append(tuple(tail))
            else:
                while order[k] in tail:
                    k += 1
                out.append((order[k],))
                k += 1
        return out
    lines = []
    wall = med([it[2] - it[0][0][0] for it in full]) / 1e3
    lines.append("Eisenstat CG + SSOR at %d DOF, %d colours, %d iterations of the trace (medians per launch)" % (3 * L["N"], nc, len(full)))
    lines.append("per iteration: %.1f us from the first sweep launch to the end of k_eis_update" % wall)
    res = {}
    for fwd, name in ((False, "backward"), (True, "forward")):
        seqs = [[x for x in it[0] if name in x[2]] for it in full]
        labs = labels(seqs[0], fwd)
        lines.append("")
        lines.append("%s sweep: %d launches" % (name, len(labs)))
        lines.append("%-14s %8s %10s %10s %9s %8s  %s" % ("colours", "slices", "MB", "us", "TB/s", "gap us", "kernel"))
        tot = {}
        for j, lab in enumerate(labs):
            d = med([(s[j][1] - s[j][0]) / 1e3 for s in seqs])
            g = med([(s[j][0] - s[j - 1][1]) / 1e3 if j > 0 else 0.0 for s in seqs])
            b = sum(colour_bytes(L, c, fwd) for c in lab)
            sl = sum(slices[c] for c in lab)
            tot[lab] = (d, g, b, sl)
            cl = "%d" % lab[0] if len(lab) == 1 else "%d-%d" % (lab[0], lab[-1])
            lines.append("%-14s %8d %10.2f %10.1f %9.2f %8.1f  %s" % (cl, sl, b / 1e6, d, b / d / 1e6, g, seqs[0][j][2]))
        res[name] = tot
    # the tail rule and the tail's cost at the big colours' rate
    thr = big_min if big_min is not None else max(slices) // 2
    big = [c for c in range(nc) if slices[c] > thr]
    tail = []
    for c in range(nc - 1, -1, -1):
        if slices[c] > thr:
            break
        tail.insert(0, c)
    lines.append("")
    lines.append("big colours (more than %d slices): %s; tail (the run of colours at the end of the order with at most %d slices): %s"
                 % (thr, big, thr, tail))
    saved = 0.0
    for name in ("backward", "forward"):
        tot = res[name]
        big_t = sum(v[0] for k, v in tot.items() if len(k) == 1 and k[0] in big)
        big_b = sum(v[2] for k, v in tot.items() if len(k) == 1 and k[0] in big)
        tail_t = sum(v[0] + v[1] for k, v in tot.items() if all(c in tail for c in k))
        tail_b = sum(v[2] for k, v in tot.items() if all(c in tail for c in k))
        at_rate = tail_b / (big_b / big_t) if big_t > 0 else 0.0
        lines.append("%s: big colours %.1f us for %.1f MB (%.2f TB/s); tail %.1f us incl. launch gaps for %.1f MB -> %.1f us at the big colours' rate; "
                     "difference %.1f us" % (name, big_t, big_b / 1e6, big_b / big_t / 1e6 if big_t else 0, tail_t, tail_b / 1e6, at_rate, tail_t - at_rate))
        saved += tail_t - at_rate
    lines.append("tail cost above the big colours' rate, both half sweeps: %.1f us per iteration (%.1f %% of %.1f us)" % (saved, 100 * saved / wall, wall))
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "layout":
        n = int(sys.argv[sys.argv.index("--elems") + 1]) if "--elems" in sys.argv else 149
        layout(sys.argv[2], n)
    elif len(sys.argv) >= 4 and sys.argv[1] == "table":
        table(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else None)
    else:
        raise SystemExit(__doc__)
