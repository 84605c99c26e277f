#!/usr/bin/env python3
"""The surface terms of a heat analysis on the device, measured beside the element loops of the same call: a TYPE=361 cube of n^3
nodes with !FILM on three of its sides, !RADIATE on two, !DFLUX on one and the body flux on every element.

    python scripts/bench_heat_bc.py [--n 150] [--repeats 5]

One JSON line with
  faces, bf_elements               entries of the three face lists together, and of the body flux
  first_call_ms, first_*           the first fx_heat_assemble_groups_bc call: whole call (host clock) and its device events; it
                                   colours the groups AND the face lists and builds their position maps (face_colourings, face_maps)
  elem_ms, surf_ms                 later calls (transient: conductivity and capacity): device events around clear + element kernels,
                                   and around the surface kernels (DFLUX with BF, FILM, RADIATE) of the same call; median and
                                   min over the repeats
  surf_faces_ms, surf_bf_ms        the same with the face lists alone and with the body flux alone
  call_ms, call_ms_without         the whole call with and without the surface terms (host clock)
No CPU fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# the face node tables of heat_FILM_361 (1-based): a side of the cube is the elements whose face lies in it
NOD361 = {1: [1, 2, 3, 4], 2: [8, 7, 6, 5], 3: [5, 6, 2, 1], 4: [6, 7, 3, 2], 5: [7, 8, 4, 3], 6: [8, 5, 1, 4]}


def side_faces(m, axis, high):
    """(element, face) of the faces of the cube's TYPE=361 elements on the side x_axis = 0 or its maximum (CubeMesh moves interior
    nodes only)"""
    x = m.coord[:, axis]
    side = np.concatenate([[False], x == (x.max() if high else 0.0)])
    elems, faces = [], []
    for f, nod in NOD361.items():
        on = side[m.conn[:, np.array(nod) - 1]].all(axis=1)
        e = np.nonzero(on)[0]
        elems.append(e)
        faces.append(np.full(e.size, f))
    return np.concatenate(elems).astype(np.int32), np.concatenate(faces).astype(np.int32)


def stat(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=150, help="nodes per edge of the TYPE=361 cube")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from bench_heat import COND, CP, RHO, scalar_matrix
    from frontistr_amd import hecmw as hip
    from frontistr_amd.heat import tHeatMaterial
    from frontistr_amd.mesh import CubeMesh
    m = CubeMesh(a.n - 1, skew=0.05)
    mesh, M = scalar_matrix(hip, m, 8)
    groups = [(361, m.conn, None, None)]
    mat = [tHeatMaterial(COND, cp=CP, rho=RHO)]
    z = m.coord[:, 2] / m.coord[:, 2].max()
    temp, temp0 = 500.0 * z, 480.0 * z + 10.0
    sides = [side_faces(m, ax, hi) for ax in range(3) for hi in (False, True)]

    def lst(which, *vals):
        e = np.concatenate([sides[k][0] for k in which])
        f = np.concatenate([sides[k][1] for k in which])
        return (np.zeros(e.size, dtype=np.int32), e, f) + vals

    film = lst((0, 2, 4), 25.0, 600.0)
    radiate = lst((1, 3), 1.1164e-8, 600.0)
    faces_q = lst((5,), 2500.0)
    ne = m.conn.shape[0]
    bf = (np.zeros(ne, dtype=np.int32), np.arange(ne, dtype=np.int32), np.zeros(ne, dtype=np.int32), np.full(ne, 900.0))
    dflux = tuple(np.concatenate([x, y]) for x, y in zip(faces_q[:3] + (np.full(faces_q[0].size, 2500.0),), bf))
    out = {"n_node": int(m.n_node), "n_elem": int(ne), "faces": int(film[0].size + radiate[0].size + faces_q[0].size), "bf_elements": int(ne)}
    ctx = hip.SolverContext(device=0)
    kw = dict(beta=0.5, dtime=0.1, tzero=-273.15)
    t = time.perf_counter()
    ctx.heat_assemble_groups(m.coord, groups, mat, M, temp, temp0, dflux=dflux, film=film, radiate=radiate, **kw)
    out["first_call_ms"] = round(1e3 * (time.perf_counter() - t), 1)
    b = ctx.heat_bc_stats()
    out["first_elem_ms"], out["first_surf_ms"] = b["elem_us"] / 1e3, b["surf_us"] / 1e3
    out["face_colourings"], out["face_maps"] = b["face_colourings"], b["face_maps"]

    def measure(**lists):
        es, ss, ws = [], [], []
        ctx.heat_assemble_groups(m.coord, groups, mat, M, temp, temp0, **lists, **kw)      # (a changed list is coloured here)
        for _ in range(a.repeats):
            t = time.perf_counter()
            ctx.heat_assemble_groups(m.coord, groups, mat, M, temp, temp0, **lists, **kw)
            ws.append(1e3 * (time.perf_counter() - t))
            s = ctx.heat_bc_stats()
            es.append(s["elem_us"] / 1e3)
            ss.append(s["surf_us"] / 1e3)
        return stat(es), stat(ss), stat(ws)

    out["elem_ms"], out["surf_ms"], out["call_ms"] = measure(dflux=dflux, film=film, radiate=radiate)
    after = ctx.heat_bc_stats()
    assert (after["face_colourings"], after["face_maps"]) == (b["face_colourings"], b["face_maps"]), after
    _, out["surf_faces_ms"], _ = measure(dflux=faces_q, film=film, radiate=radiate)
    _, out["surf_bf_ms"], _ = measure(dflux=bf)
    ws = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        ctx.heat_assemble_groups(m.coord, groups, mat, M, temp, temp0, beta=0.5, dtime=0.1)
        ws.append(1e3 * (time.perf_counter() - t))
    out["call_ms_without"] = stat(ws)
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    from _libarg import take_lib
    take_lib()      # --lib PATH: another build of the library (the parent commit's, say)
    main()
