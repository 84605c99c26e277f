#!/usr/bin/env python3
"""HIP-event time of the elastoplastic tangent and stress update of the nonlinear element kernels for the three yield functions --
Mises (groups 0..2), Drucker-Prager and Mohr-Coulomb (groups 4..6, csrc/fx_yield.h) -- on the n^3-cell cube as TYPE=361 (CubeMesh) and
as TYPE=342 (solid_mesh), updated Lagrange, fx_nl_update_at / fx_nl_stiffness_at, three warm calls each after a cold one.

The displacement increment stretches and shears the cube with strains that grow linearly in z (0 at the bottom, 2 % / 1 % at the
top), and the yield constants put the surface at mid height, so that about half of the points yield; the share that did is read
back from istat and printed with the times ("plastic_share").  Every stress update sets the context's latch, after which the tangent
is the elastic one; the script clears it (fx_nl_set_state) before each timed tangent, so that what is timed is the elastoplastic
matrix of the yielded points.

The Mises case uses nothing but what the parent commit's library has, so `--only-mises --lib <parent build>/libfistr_hip.so` times
the parent with this script.  Start the script twice, as two processes: the difference between the two is the spread against which
a difference between two builds is to be read.
usage: bench_nl_yield.py [--etype 361|342] [--only-mises] [--lib PATH] [N]        (both types when --etype is not given; N = 40)"""
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
only_mises = "--only-mises" in sys.argv
if only_mises:
    sys.argv.remove("--only-mises")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
E, NU, PHI, H = 20000.0, 0.3, 25.0, 400.0
for etype in etypes:
    m = CubeMesh(n) if etype == 361 else solid_mesh(n, etype)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    out = {"etype": etype, "n": n, "elements": int(m.n_elem), "dof": int(3 * m.n_node), "lib": os.path.relpath(hip.LIBPATH)}
    # yield constants that put the surface near z = n / 2 (the share that yields is measured, not assumed)
    cases = {"mises_G2": fstr.tMaterial(E, NU, plastic=True, harden=fstr.BILINEAR, plconst=(160.0, H, 0.0))}
    if not only_mises:
        cases["drucker_prager_G6"] = fstr.tMaterial.drucker_prager(E, NU, 180.0, PHI, H)
        cases["mohr_coulomb_G6"] = fstr.tMaterial.mohr_coulomb(E, NU, 180.0, PHI, H)
    z = m.coord[:, 2]
    du = np.zeros_like(m.coord)
    du[:, 2] = 0.02 * z * z / (2.0 * n)
    du[:, 0] = 0.01 * z * z / (2.0 * n)
    du = du.ravel().copy()
    u = np.zeros_like(du)
    for name, material in cases.items():
        solid = fstr.fstr_solid(ctx, m.coord, m.conn, material, etype=etype)
        t = C.c_float(0)
        q = np.zeros(3 * m.n_node)
        ts, tu = [], []
        for _ in range(4):
            hip._chk(hip.lib().fx_nl_update_at(ctx.h, hip._ptr(du), hip._ptr(q), C.byref(t)))
            tu.append(round(t.value, 3))
            solid.set_state({}, latch=0)
            hip._chk(hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(u), hip._ptr(du), C.byref(t)))
            ts.append(round(t.value, 3))
        share = float(solid.get_state(("istat",))["istat"].mean())
        out[name] = {"plastic_share": round(share, 3), "stiffness_ms": ts[1:], "update_ms": tu[1:]}
    print(json.dumps(out))
    ctx.close()
