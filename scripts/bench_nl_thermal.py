#!/usr/bin/env python3
"""HIP-event time of the nonlinear tangent and update kernels with and without thermal strain (fx_nl_set_thermal) on an n^3-cell
cube of TYPE=361 (B-bar) and of one STF_C3 type, in one process (fx_nl_stiffness_at / fx_nl_update_at, three warm calls each, in
the manner of bench_nl_fbar.py): an ELASTIC total-Lagrange material
  off        no thermal strain: the instantiations every context launched before (compare with --off-only on the parent commit)
  constants  a constant expansion coefficient: the update kernels' thermal variant, the tangent kernels unchanged
  tables     !ELASTIC and !EXPANSION_COEFF tables: the thermal variant of both
usage: bench_nl_thermal.py [--off-only] [--etype 342] [--lib PATH] [N]        (N = 40; the STF_C3 cube is N // 2 cells a side)"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from frontistr_amd import fstr, hecmw as hip          # noqa: E402
from frontistr_amd.mesh import CubeMesh, solid_mesh   # noqa: E402
from _libarg import take_lib                          # noqa: E402

take_lib()

off_only = "--off-only" in sys.argv
if off_only:
    sys.argv.remove("--off-only")
c3 = 342
if "--etype" in sys.argv:
    i = sys.argv.index("--etype")
    c3 = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
ELASTIC_TAB = np.array([[210000.0, 0.28, 0.0], [200000.0, 0.30, 100.0], [150000.0, 0.33, 300.0]])
ALPHA_TAB = np.array([[1.0e-5, 0.0], [1.3e-5, 100.0], [1.8e-5, 300.0]])
out = {"n": n}
for etype, m in ((361, CubeMesh(n)), (c3, solid_mesh(max(n // 2, 1), c3))):
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    u = (1.0e-3 * m.coord[:, ::-1]).ravel().copy()
    du = (2.0e-3 * m.coord * np.array([0.2, -0.3, 1.0])).ravel().copy()
    temp = 20.0 + 300.0 * m.coord[:, 2] / m.coord[:, 2].max()
    res = {"elements": int(m.n_elem), "dof": int(3 * m.n_node)}
    for mode in ("off", "constants", "tables"):
        if off_only and mode != "off":
            continue
        material = fstr.tMaterial(206900.0, 0.29, nlgeom_flag=fstr.TOTALLAG)
        material.expansion = 1.2e-5
        if mode == "tables":
            material.expansion_table, material.elastic_table = ALPHA_TAB, ELASTIC_TAB
        solid = fstr.fstr_solid(ctx, m.coord, m.conn, material, etype=etype)
        if mode != "off":
            solid.set_thermal(20.0)
            solid.set_temperature(temp)
        t = C.c_float(0)
        q = np.zeros(3 * m.n_node)
        ts, tu = [], []
        for _ in range(4):
            hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(du), hip._ptr(q), C.byref(t)))
            tu.append(round(t.value, 3))
            hip._chk(hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(u), hip._ptr(du), C.byref(t)))
            ts.append(round(t.value, 3))
        res[mode] = {"stiffness_ms": ts[1:], "update_ms": tu[1:]}
    out[str(etype)] = res
    ctx.close()
print(json.dumps(out))
