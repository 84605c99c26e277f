#!/usr/bin/env python3
"""HIP-event time of the tangent and the stress update of the nonlinear element kernels for the time-dependent materials --
viscoelastic TOTALLAG (group 8, two Prony rows) and NORTON creep UPDATELAG (group 9), csrc/fx_visco.h -- beside ELASTIC TOTALLAG
(group 1) and ELASTIC UPDATELAG (group 2) on the same mesh: the n^3-cell cube as TYPE=361 (CubeMesh) and as TYPE=342 (solid_mesh),
fx_nl_update_at / fx_nl_stiffness_at, three warm calls each after a cold one, one process.

The displacement increment stretches and shears the cube with strains that grow linearly in z (0 at the bottom, 0.2 % / 0.1 % at the
top: stresses of a few hundred on E = 206900).  The time increment is set before the calls (fx_nl_set_time): dt / tau = 2.5 and 0.1
for the viscoelastic rows, and a creep strain increment of the order of the elastic one at the top of the NORTON cube, so that the
local iteration of update_iso_creep runs at every stressed point (its largest count is not read back; tests/test_visco_ref.py
bounds it for such inputs).  A NORTON update sets the context's latch, after which the tangent is the elastic one; the script clears
it (fx_nl_set_state) before each timed tangent, so that what is timed is iso_creep's matrix.

The ELASTIC cases use nothing but what the parent commit's library has, so `--only-elastic --lib <parent build>/libfistr_hip.so`
times the parent with this script.
usage: bench_nl_visco.py [--etype 361|342] [--only-elastic] [--lib PATH] [N]        (both types when --etype is not given; N = 40)"""
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
only_elastic = "--only-elastic" in sys.argv
if only_elastic:
    sys.argv.remove("--only-elastic")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
E, NU = 206900.0, 0.29
for etype in etypes:
    m = CubeMesh(n) if etype == 361 else solid_mesh(n, etype)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    out = {"etype": etype, "n": n, "elements": int(m.n_elem), "dof": int(3 * m.n_node), "lib": os.path.relpath(hip.LIBPATH)}
    # name -> (material, (time, tincr) or None)
    cases = {"elastic_G1": (fstr.tMaterial(E, NU, nlgeom_flag=fstr.TOTALLAG), None),
             "elastic_G2": (fstr.tMaterial(E, NU, nlgeom_flag=fstr.UPDATELAG), None)}
    if not only_elastic:
        cases["viscoelastic_G8"] = (fstr.tMaterial.viscoelastic(E, NU, [[0.3, 0.2], [0.25, 5.0]]), (0.0, 0.5))
        cases["norton_G9"] = (fstr.tMaterial.norton(E, NU, 1.0e-10, 5.0, 0.0), (1.0, 2.0e-6))
    z = m.coord[:, 2]
    du = np.zeros_like(m.coord)
    du[:, 2] = 0.002 * z * z / (2.0 * n)
    du[:, 0] = 0.001 * z * z / (2.0 * n)
    du = du.ravel().copy()
    u = np.zeros_like(du)
    for name, (material, time) in cases.items():
        solid = fstr.fstr_solid(ctx, m.coord, m.conn, material, etype=etype)
        if time is not None:
            solid.set_time(*time)
        t = C.c_float(0)
        q = np.zeros(3 * m.n_node)
        ts, tu = [], []
        for _ in range(4):
            hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(du), hip._ptr(q), C.byref(t)))
            tu.append(round(t.value, 3))
            solid.set_state({}, latch=0)
            hip._chk(hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(u), hip._ptr(du), C.byref(t)))
            ts.append(round(t.value, 3))
        out[name] = {"stiffness_ms": ts[1:], "update_ms": tu[1:]}
        if name == "norton_G9":
            dg = solid.get_state(("plstrain",))["plstrain"]
            out[name]["creep_share"] = round(float((dg > 0).mean()), 3)      # points that ran the local iteration
    print(json.dumps(out))
    ctx.close()
