#!/usr/bin/env python3
"""HIP-event time of the F-bar 361 kernels (elemopt 4: k_nl_stiffness_fbar / k_nl_update_fbar) beside the B-bar ones (elemopt 2:
k_nl_stiffness / k_nl_update) on the same n^3-cell cube and material, in one process (fx_nl_stiffness_at / fx_nl_update_at, three warm
calls each, in the manner of bench_nl_hyper.py): materials elastic TOTALLAG (group 1) and Mooney-Rivlin (group 3).  F-bar does
strictly more arithmetic than B-bar -- two sets of global derivatives per point, the volume averages, the second initial-stress
matrix -- so there is no target ratio; the B-bar figures are there to be compared with the same script on the parent commit (where
--bbar-only keeps it to what that commit serves).
usage: bench_nl_fbar.py [--bbar-only] [--lib PATH] [N]        (N = 40 as bench_nl_hyper.py)"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from frontistr_amd import fstr, hecmw as hip          # noqa: E402
from frontistr_amd.mesh import CubeMesh               # noqa: E402
from _libarg import take_lib                          # noqa: E402

take_lib()

bbar_only = "--bbar-only" in sys.argv
if bbar_only:
    sys.argv.remove("--bbar-only")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
m = CubeMesh(n)
hm = hip.hecmwST_local_mesh(n_node=m.n_node)
hm.nn_elem = m.conn.shape[1]
hm.elem_node_item = m.conn.ravel()
mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
ctx = hip.SolverContext()
ctx.upload(mat, what=hip.FX_UP_PROFILE)
out = {"etype": 361, "n": n, "elements": int(m.n_elem), "dof": int(3 * m.n_node)}
materials = {"elastic_totallag_G1": fstr.tMaterial(2.5, 0.3, nlgeom_flag=fstr.TOTALLAG),
             "mooney_rivlin_G3": fstr.tMaterial.mooney_rivlin(0.1486, 0.4849, 0.0789)}
u = (1.0e-2 * m.coord[:, ::-1]).ravel().copy()
du = (4.0e-2 * m.coord * np.array([0.2, -0.3, 1.0])).ravel().copy()
for name, material in materials.items():
    for form, elemopt in (("bbar", 2), ("fbar", 4)):
        if bbar_only and elemopt != 2:
            continue
        if elemopt == 2:
            fstr.fstr_solid(ctx, m.coord, m.conn, material, etype=361)
        else:
            fstr.fstr_solid(ctx, m.coord, m.conn, material, etype=361, elemopt=elemopt)
        t = C.c_float(0)
        q = np.zeros(3 * m.n_node)
        ts, tu = [], []
        for _ in range(4):
            hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(du), hip._ptr(q), C.byref(t)))
            tu.append(round(t.value, 3))
            hip._chk(hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(u), hip._ptr(du), C.byref(t)))
            ts.append(round(t.value, 3))
        out["%s_%s" % (name, form)] = {"stiffness_ms": ts[1:], "update_ms": tu[1:]}
print(json.dumps(out))
ctx.close()
