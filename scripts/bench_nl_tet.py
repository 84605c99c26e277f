#!/usr/bin/env python3
"""HIP-event time of the nonlinear tet kernels (fx_nl_stiffness_at / fx_nl_update_at, three warm calls each) beside the linear
fx_assemble_c3 of the same mesh: the n^3-cell tet cube (n = 74: 2.43 M elements, 9.9 M DOF at 342), elastic TOTALLAG and Mises
multilinear UPDATELAG.  Algorithmic bytes: stiffness = the linear count (connectivity, coordinates, the position map, every matrix
block written once) + 8 (6 + 1 + 0.5) nq per element of state read (stress, fstatus, istatus) + two displacement vectors; update =
the state read and written once (8 (6 + 6 + 6 + 6 + 1 + 1 + 1 + 0.5 + 0.5) nq: stress / strain out, stress_bak / strain_bak / plstrain
in, fstatus and istatus both ways) + connectivity, coordinates, two displacement vectors and QFORCE.
usage: bench_nl_tet.py [--etype 341|342] [--lib PATH] N      (--lib: another build of libfistr_hip.so, e.g. the parent commit's)"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from frontistr_amd import fstr, hecmw as hip          # noqa: E402
from frontistr_amd.mesh import TetMesh                # noqa: E402
from _libarg import take_lib                          # noqa: E402

take_lib()

etype = 342
if "--etype" in sys.argv:
    k = sys.argv.index("--etype"); etype = int(sys.argv[k + 1]); del sys.argv[k:k + 2]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 74
m = TetMesh(n, etype=etype)
nn, nq = fstr.fstr_solid.NODES[etype], fstr.fstr_solid.POINTS[etype]
hm = hip.hecmwST_local_mesh(n_node=m.n_node)
hm.nn_elem = nn
hm.elem_node_item = m.conn.ravel()
mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
ctx = hip.SolverContext()
ctx.upload(mat, what=hip.FX_UP_PROFILE)
out = {"etype": etype, "n": n, "elements": int(m.n_elem), "dof": int(3 * m.n_node)}
ms = [ctx.assemble_c3(m.coord, m.conn, etype, 206900.0, 0.29, bc=m.dirichlet()) for _ in range(4)]
out["linear_assemble_ms"] = [round(float(x), 3) for x in ms[1:]] if ms[0] is not None else None
TAB = np.array([[450.0, 0.0], [608.0, 0.05], [679.0, 0.1], [732.0, 0.2]])
cases = {"elastic_totallag": fstr.tMaterial(206900.0, 0.29, nlgeom_flag=fstr.TOTALLAG),
         "mises_updatelag": fstr.tMaterial(206900.0, 0.29, plastic=True, harden=fstr.MULTILINEAR, table=TAB)}
blocks = mat.NP + mat.NPL + mat.NPU
lin_bytes = m.n_elem * (4 * nn + 4 * nn * nn) + 24 * m.n_node + 72 * blocks
u = (1.0e-3 * m.coord[:, ::-1]).ravel().copy()
du = (4.0e-3 * m.coord * np.array([0.2, -0.3, 1.0])).ravel().copy()
for name, material in cases.items():
    solid = fstr.fstr_solid(ctx, m.coord, m.conn, material, etype=etype)
    t = C.c_float(0)
    q = np.zeros(3 * m.n_node)
    ts, tu = [], []
    for _ in range(4):
        hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(du), hip._ptr(q), C.byref(t)))
        tu.append(round(t.value, 3))
        hip._chk(hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(u), hip._ptr(du), C.byref(t)))
        ts.append(round(t.value, 3))
    sb = lin_bytes + m.n_elem * nq * 60 + 48 * m.n_node
    ub = m.n_elem * (nq * 8 * 28.0 + 4 * nn) + 24 * m.n_node * 4
    out[name] = {"stiffness_ms": ts[1:], "update_ms": tu[1:], "stiffness_algorithmic_GB": round(sb / 1e9, 3),
                 "update_algorithmic_GB": round(ub / 1e9, 3), "stiffness_GBps": round(sb / 1e6 / min(ts[1:]), 1),
                 "update_GBps": round(ub / 1e6 / min(tu[1:]), 1), "plastic_points": int((solid.get_state(("istat",))["istat"] != 0).sum())}
print(json.dumps(out))
ctx.close()
