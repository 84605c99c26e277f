#!/usr/bin/env python3
"""fstr_NodalStress3D on the device (csrc/fx_nodal_stress.h), measured one case per invocation so that a job script can give
every GPU step a time limit of its own:

    python scripts/bench_nodal_stress.py --case hex361      [--n 150] [--repeats 5] [--principal 0]
    python scripts/bench_nodal_stress.py --case tet342      [--n 150]
    python scripts/bench_nodal_stress.py --case resident361 [--n 150]
    python scripts/bench_nodal_stress.py --case baseline361 [--n 150]

  hex361       the TYPE=361 cube of n^3 nodes through fx_nodal_stress_groups: host point arrays up, results back
  tet342       a TYPE=342 mesh of about the same node count (the cube of ((n - 1) / 2)^3 cells, six tetrahedra each)
  resident361  the same cube as the resident state of a nonlinear context through fx_nl_nodal_stress: only the results cross the bus
  baseline361  what a user of fstr_solid paid before this pass existed, same context and size: get_state of stress and strain
               (2 x 48 bytes per point over PCIe into numpy arrays) plus the numpy helper of the tests (thermal_ref.summary, which
               is c3_nl_ref / tet_nl_ref underneath and serves 361)

One JSON line per case with
  kernel_ms            device events around all launches of the pass (element kernels, node kernel, element Mises), median and min
  call_ms              the whole call on the host clock (uploads, list look-up, launches, copy of the results)
  first_call_ms        the first call, which builds the node -> element list
  bytes                algorithmic traffic of the launches: points read + vertex records written and read (a mid-edge node reads
                       two) + results written
  bytes_all            the same plus what that count leaves out: the list entries (read by both halves of the node kernel) and
                       ESTRESS read again for EMISES
  GBs, GBs_all         bytes / kernel_ms and bytes_all / kernel_ms (median); GBs is the figure to hold against the 6.6-6.8 TB/s the
                       SpMV streams on this card
No CPU fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NQ = {341: 1, 342: 4, 351: 2, 352: 9, 361: 8, 362: 27}
NV = {341: 1, 342: 4, 351: 1, 352: 6, 361: 8, 362: 8}      # vertex records per element


def stat(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3)}


def traffic(n_node, etype, conn, principal):
    """(bytes of every array the launches touch, bytes as the issue counts them: points read + vertex records written and read +
    results written).  The first adds what the second leaves out: the list entries (8 bytes each, read by both halves of the node
    kernel) and ESTRESS read again by the launch that takes EMISES."""
    ne, nn = conn.shape
    mid = nn - NV[etype] if NV[etype] > 1 else 0
    reads = ne * (NV[etype] + 2 * mid if NV[etype] > 1 else nn)     # records read by the node kernel
    extra = sum(w for k, w in enumerate((3, 9, 3, 9)) if principal >> k & 1) * n_node + \
        sum(w for k, w in enumerate((3, 9, 3, 9)) if principal >> (k + 4) & 1) * ne
    narrow = 12 * NQ[etype] * ne + 12 * NV[etype] * ne + 12 * reads + 13 * n_node + 13 * ne + extra
    return 8 * (narrow + 2 * ne * nn + 6 * ne), 8 * narrow


def points(conn, etype, seed=1):
    rng = np.random.default_rng(seed)
    shape = (conn.shape[0], NQ[etype], 6)
    return rng.uniform(-1.0, 1.0, shape), rng.uniform(-3.0, 3.0, shape)


def report(out, n_node, etype, conn, principal, kernel, call):
    out["kernel_ms"], out["call_ms"] = stat(kernel), stat(call)
    out["bytes_all"], out["bytes"] = (int(b) for b in traffic(n_node, etype, conn, principal))
    out["GBs"] = round(out["bytes"] / (1e-3 * out["kernel_ms"]["median"]) / 1e9, 1)
    out["GBs_all"] = round(out["bytes_all"] / (1e-3 * out["kernel_ms"]["median"]) / 1e9, 1)
    print(json.dumps(out), flush=True)


def linear(a, etype, hip, m):
    groups = [(etype, m.conn)]
    st, ss = points(m.conn, etype)
    ctx = hip.SolverContext(device=0)
    out = {"case": a.case, "n_node": int(m.n_node), "n_elem": int(m.conn.shape[0]), "principal": a.principal}
    t = time.perf_counter()
    ctx.nodal_stress_groups(m.n_node, groups, st, ss, principal=a.principal)
    out["first_call_ms"] = round(1e3 * (time.perf_counter() - t), 1)
    kernel, call = [], []
    for _ in range(a.repeats):
        t = time.perf_counter()
        r = ctx.nodal_stress_groups(m.n_node, groups, st, ss, principal=a.principal)
        call.append(1e3 * (time.perf_counter() - t))
        kernel.append(r.ms)
    assert ctx.nodal_stats()["lists"] == 1
    ctx.close()
    report(out, m.n_node, etype, m.conn, a.principal, kernel, call)


def resident(a, hip, m, baseline):
    from frontistr_amd import fstr
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.elem_node_item = m.conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext(device=0)
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    solid = fstr.fstr_solid(ctx, m.coord, m.conn, fstr.tMaterial(206900.0, 0.29, nlgeom_flag=fstr.TOTALLAG))
    st, ss = points(m.conn, 361)
    solid.set_state({"strain": st, "stress": ss})
    out = {"case": a.case, "n_node": int(m.n_node), "n_elem": int(m.conn.shape[0]), "principal": a.principal}
    if baseline:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import thermal_ref
        t = time.perf_counter()
        s = solid.get_state(("stress", "strain"))
        out["get_state_ms"] = round(1e3 * (time.perf_counter() - t), 1)
        t = time.perf_counter()
        thermal_ref.summary([(361, m.conn)], np.zeros(3 * m.n_node), [s["strain"]], [s["stress"]])
        out["numpy_helper_ms"] = round(1e3 * (time.perf_counter() - t), 1)
        out["total_ms"] = round(out["get_state_ms"] + out["numpy_helper_ms"], 1)
        ctx.close()
        print(json.dumps(out), flush=True)
        return
    t = time.perf_counter()
    solid.nodal_stress(principal=a.principal)
    out["first_call_ms"] = round(1e3 * (time.perf_counter() - t), 1)
    kernel, call = [], []
    for _ in range(a.repeats):
        t = time.perf_counter()
        r = solid.nodal_stress(principal=a.principal)
        call.append(1e3 * (time.perf_counter() - t))
        kernel.append(r.ms)
    t = time.perf_counter()
    r.summary()
    out["summary_ms"] = round(1e3 * (time.perf_counter() - t), 1)
    ctx.close()
    report(out, m.n_node, 361, m.conn, a.principal, kernel, call)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", required=True, choices=("hex361", "tet342", "resident361", "baseline361"))
    ap.add_argument("--n", type=int, default=150, help="nodes per edge of the cube")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--principal", type=int, default=0, help="make_principal's bit mask")
    a = ap.parse_args()
    from frontistr_amd import hecmw as hip
    from frontistr_amd.mesh import CubeMesh, TetMesh
    if a.case == "tet342":
        linear(a, 342, hip, TetMesh((a.n - 1) // 2, etype=342))
    elif a.case == "hex361":
        linear(a, 361, hip, CubeMesh(a.n - 1))
    else:
        resident(a, hip, CubeMesh(a.n - 1), a.case == "baseline361")


if __name__ == "__main__":
    from _libarg import take_lib
    take_lib()      # --lib PATH: another build of the library (the parent commit's, say)
    main()
