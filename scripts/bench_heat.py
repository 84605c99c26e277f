#!/usr/bin/env python3
"""Heat conduction assembly on the device, measured: a TYPE=361 cube of n^3 nodes and a TYPE=342 mesh of about as many.

    python scripts/bench_heat.py [--n 150] [--repeats 5] [--no-solve]

Per mesh one JSON line with
  kernel_ms_cond / kernel_ms_cap   device events around clear + element kernels of one fx_heat_assemble_groups call (steady:
                                   conductivity alone; transient: with capacity), median and min over the repeats after one
                                   warm-up call (which also colours the mesh and builds the position map: setup_s)
  copy_back_ms                     the copy of D, AL, AU, B to the caller's arrays (host clock inside the call)
  compulsory_MB, requested_MB      bytes the assembly cannot avoid (profile values and B written once; connectivity, coordinates
                                   and temperatures read once) and bytes the kernels request, both from the shapes (position
                                   map, gathers per element, read-modify-write of nn^2 values); traffic_ratio is their quotient
  solve_s, solve_iterations        CG + SSOR to 1e-8 on the same system with the bottom and top faces fixed -- the comparison the
                                   assembly is to be read against
No CPU fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COND = [(50.0, 0.0), (42.0, 200.0), (35.0, 500.0)]
CP, RHO = [(0.46, 0.0), (0.52, 400.0)], [(7.85, 0.0), (7.70, 400.0)]


def scalar_matrix(hip, m, nn):
    mesh = hip.hecmwST_local_mesh(n_node=m.n_node)
    mesh.elem_node_item, mesh.nn_elem = m.conn.ravel(), nn
    M = hip.hecmw_mat_con(mesh, hip.hecmwST_matrix())
    M.NDOF = 1
    M.D, M.AL, M.AU = np.zeros(M.NP), np.zeros(M.NPL), np.zeros(M.NPU)
    M.B, M.X = np.zeros(M.NP), np.zeros(M.NP)
    return mesh, M


def run(hip, etype, m, repeats, solve):
    from frontistr_amd.heat import tHeatMaterial
    nn = m.conn.shape[1]
    ne = m.conn.shape[0]
    mesh, M = scalar_matrix(hip, m, nn)
    groups = [(etype, m.conn, None, None)]
    mat = [tHeatMaterial(COND, cp=CP, rho=RHO)]
    z = m.coord[:, 2] / m.coord[:, 2].max()
    temp, temp0 = 500.0 * z, 480.0 * z + 10.0
    fix = (np.concatenate([m.bottom_nodes, m.top_nodes]).astype(np.int32),
           np.concatenate([np.zeros(m.bottom_nodes.size), np.full(m.top_nodes.size, 500.0)]))
    ctx = hip.SolverContext(device=0)
    t = time.perf_counter()
    ctx.heat_assemble_groups(m.coord, groups, mat, M, temp, temp0, beta=1.0, dtime=0.0)
    setup = time.perf_counter() - t
    ctx.heat_assemble_groups(m.coord, groups, mat, M, temp, temp0, beta=0.5, dtime=0.1)      # warm-up of the capacity path
    out = {"etype": etype, "n_node": int(m.n_node), "n_elem": int(ne), "NPL": int(M.NPL), "NPU": int(M.NPU), "setup_s": round(setup, 3)}
    for key, beta, dtime in (("cond", 1.0, 0.0), ("cap", 0.5, 0.1)):
        ks, cs, ws = [], [], []
        for _ in range(repeats):
            t = time.perf_counter()
            ks.append(ctx.heat_assemble_groups(m.coord, groups, mat, M, temp, temp0, beta=beta, dtime=dtime))
            ws.append(1e3 * (time.perf_counter() - t))
            cs.append(ctx.heat_stats()["copy_us"] / 1e3)
        out["kernel_ms_" + key] = {"median": round(float(np.median(ks)), 3), "min": round(float(np.min(ks)), 3)}
        out["copy_back_ms_" + key] = {"median": round(float(np.median(cs)), 3), "min": round(float(np.min(cs)), 3)}
        out["call_ms_" + key] = {"median": round(float(np.median(ws)), 1), "min": round(float(np.min(ws)), 1)}
    st = ctx.heat_stats()
    assert st["colourings"] == 1 and st["maps"] == 1 and st["profiles"] == 1, st
    nval = M.NP + M.NPL + M.NPU
    compulsory = 8 * (nval + M.NP) + 4 * nn * ne + 24 * M.NP + 8 * M.NP
    requested = 8 * (nval + M.NP) + ne * (4 * nn + 32 * nn + 4 * nn * nn + 16 * nn * nn + 16 * nn)
    out["compulsory_MB"], out["requested_MB"] = round(compulsory / 1e6, 1), round(requested / 1e6, 1)
    out["traffic_ratio"] = round(requested / compulsory, 2)
    out["compulsory_GBps_cond"] = round(compulsory / 1e6 / out["kernel_ms_cond"]["median"], 1)
    if solve:
        ctx.heat_assemble_groups(m.coord, groups, mat, M, temp, temp0, beta=1.0, dtime=0.0, fix=fix)
        M.Iarray[0], M.Iarray[1], M.Iarray[2] = 20000, 1, 1
        M.Rarray[0] = 1.0e-8
        M.X[:] = 0.0
        t = time.perf_counter()
        hip.hecmw_solve(mesh, M, ctx=ctx, want_history=False)
        out["solve_s"], out["solve_iterations"] = round(time.perf_counter() - t, 3), int(ctx.info.iterations)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=150, help="nodes per edge of the TYPE=361 cube")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-solve", action="store_true")
    a = ap.parse_args()
    from frontistr_amd import hecmw as hip
    from frontistr_amd.mesh import CubeMesh, TetMesh
    for etype, m in ((361, CubeMesh(a.n - 1, skew=0.05)), (342, TetMesh(max(1, (a.n - 1) // 2), etype=342, skew=0.05))):
        print(json.dumps(run(hip, etype, m, a.repeats, not a.no_solve)), flush=True)


if __name__ == "__main__":
    from _libarg import take_lib
    take_lib()      # --lib PATH: another build of the library (the parent commit's, say)
    main()
