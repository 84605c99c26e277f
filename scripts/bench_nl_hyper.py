#!/usr/bin/env python3
"""HIP-event time of the hyperelastic group (G = 3) of the nonlinear element kernels beside the elastic TOTALLAG instantiation (G = 1)
of the same mesh (fx_nl_stiffness_at / fx_nl_update_at, three warm calls each, in the manner of bench_nl_c3.py): the n^3-cell cube as
TYPE=361 (CubeMesh) and as TYPE=342 (TetMesh), materials elastic TOTALLAG, Mooney-Rivlin and Arruda-Boyce.  G = 3 does strictly more
arithmetic than G = 1 on the same scatter and reads 48 bytes more per quadrature point (the stored strain), so there is no target
ratio; the G = 1 figures are there to be compared with the same script on the parent commit.
usage: bench_nl_hyper.py [--etype 361|342] [--lib PATH] [N]        (both types when --etype is not given; N = 40 as bench_nl_c3.py)"""
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

etypes = [361, 342]
if "--etype" in sys.argv:
    k = sys.argv.index("--etype"); etypes = [int(sys.argv[k + 1])]; del sys.argv[k:k + 2]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
for etype in etypes:
    m = CubeMesh(n) if etype == 361 else solid_mesh(n, etype)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    out = {"etype": etype, "n": n, "elements": int(m.n_elem), "dof": int(3 * m.n_node)}
    cases = {"elastic_totallag_G1": fstr.tMaterial(2.5, 0.3, nlgeom_flag=fstr.TOTALLAG),
             "mooney_rivlin_G3": fstr.tMaterial.mooney_rivlin(0.1486, 0.4849, 0.0789),
             "arruda_boyce_G3": fstr.tMaterial.arruda_boyce(0.71, 1.7029, 0.1408)}
    u = (1.0e-2 * m.coord[:, ::-1]).ravel().copy()
    du = (4.0e-2 * m.coord * np.array([0.2, -0.3, 1.0])).ravel().copy()
    for name, material in cases.items():
        fstr.fstr_solid(ctx, m.coord, m.conn, material, etype=etype)
        t = C.c_float(0)
        q = np.zeros(3 * m.n_node)
        ts, tu = [], []
        for _ in range(4):
            hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(du), hip._ptr(q), C.byref(t)))
            tu.append(round(t.value, 3))
            hip._chk(hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(u), hip._ptr(du), C.byref(t)))
            ts.append(round(t.value, 3))
        out[name] = {"stiffness_ms": ts[1:], "update_ms": tu[1:]}
    print(json.dumps(out))
    ctx.close()
