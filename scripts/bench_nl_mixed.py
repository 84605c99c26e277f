#!/usr/bin/env python3
"""HIP-event time of the tangent and the stress update of a nonlinear context of several element groups (fx_nl_init_groups) on
MixedMesh(n, order) beside the three single-type contexts that hold the same elements, each on its own profile
(fx_nl_stiffness_at / fx_nl_update_at, three warm calls each, in the manner of bench_nl_hyper.py), all in one process.  The element
kernels are the same; what the figures show is launch and clearing overhead (a group context with a 361 part clears the matrix
once and takes no first-write flags; a single-type STF_C3 context stores its first contributions instead).  No pass / fail bound.
Materials: Mises BILINEAR UPDATELAG, or with --two-sections that beside ELASTIC TOTALLAG in the (arange * 7 // 3) % 2 pattern.
usage: bench_nl_mixed.py [--order 1|2] [--two-sections] [--lib PATH] [N]        (both orders when --order is not given; N = 24)"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from frontistr_amd import fstr, hecmw as hip          # noqa: E402
from frontistr_amd.mesh import MixedMesh              # noqa: E402
from _libarg import take_lib                          # noqa: E402

take_lib()

orders = [1, 2]
if "--order" in sys.argv:
    k = sys.argv.index("--order"); orders = [int(sys.argv[k + 1])]; del sys.argv[k:k + 2]
two = "--two-sections" in sys.argv
if two:
    sys.argv.remove("--two-sections")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 24


def timed(ctx, n_node, u, du):
    t = C.c_float(0)
    q = np.zeros(3 * n_node)
    ts, tu = [], []
    for _ in range(4):
        hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(du), hip._ptr(q), C.byref(t)))
        tu.append(round(t.value, 3))
        hip._chk(hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(u), hip._ptr(du), C.byref(t)))
        ts.append(round(t.value, 3))
    return {"stiffness_ms": ts[1:], "update_ms": tu[1:]}


for order in orders:
    m = MixedMesh(n, order)
    mats = [fstr.tMaterial(206900.0, 0.29, plastic=True, harden=fstr.BILINEAR, plconst=(450.0, 2000.0, 0.0))]
    em = None
    if two:
        mats.append(fstr.tMaterial(70000.0, 0.33, nlgeom_flag=fstr.TOTALLAG))
        em = (1 + (np.arange(m.n_elem) * 7 // 3) % 2).astype(np.int32)
    groups = m.groups_with(2, em)
    u = (1.0e-3 * m.coord[:, ::-1]).ravel().copy()
    du = (4.0e-3 * m.coord * np.array([0.2, -0.3, 1.0])).ravel().copy()
    out = {"order": order, "n": n, "two_sections": two, "elements": int(m.n_elem), "dof": int(3 * m.n_node)}
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    ctx = hip.SolverContext()
    ctx.upload(hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups), what=hip.FX_UP_PROFILE)
    fstr.fstr_solid(ctx, m.coord, None, mats, groups=groups)
    out["groups"] = timed(ctx, m.n_node, u, du)
    ctx.close()
    sums = {"stiffness_ms": 0.0, "update_ms": 0.0}
    for et, conn, _, gem in groups:       # the same elements, one type at a time, on the profile of that type's elements alone
        ctx = hip.SolverContext()
        ctx.upload(hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), [(et, conn)]), what=hip.FX_UP_PROFILE)
        fstr.fstr_solid(ctx, m.coord, conn, mats if two else mats[0], elem_mat=gem, etype=et)
        out[str(et)] = timed(ctx, m.n_node, u, du)
        for k in sums:
            sums[k] += min(out[str(et)][k])
        ctx.close()
    out["sum_of_single_types_min"] = {k: round(v, 3) for k, v in sums.items()}
    print(json.dumps(out))
