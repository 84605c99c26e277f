#!/usr/bin/env python3
"""The distributed load on the device (fx_dload_groups), measured for each of the six solid types on a cube: gravity on all
elements and pressure on every face of the top side.

    python scripts/bench_dload.py [--n 150] [--repeats 5] [--types 361,341,...]

--n: nodes per edge of the cube.  The first-order types (341, 351, 361) take n - 1 cells per edge, the second-order types (342,
352, 362) (n - 1) // 2, so that every mesh has about n^3 nodes; 341 / 342 hold 6 tetrahedra per cell, 351 / 352 2 wedges.
One JSON line per type with
  n_node, n_elem, faces          the mesh and the faces under pressure
  grav_ms, face_ms               device events around the volume kernel (GRAV on all elements) and around the face kernel
                                 (fx_dload_get_stats), median and min over the repeats
  grav_gbs                       algorithmic bytes of the volume kernel over grav_ms: per element its node ids (4 nn), parameters
                                 (69), the gathered coordinates (24 nn) and the values added (24 nn; an atomic add counted once)
  thermal_ms                     fx_thermal_load_groups on the same mesh: the same gather and the same atomic scatter, the
                                 in-project yardstick
  follower_ms                    the kernels again with a displacement vector (coord + disp): what rebuilding GL adds to a
                                 Newton iteration, beside
  copies_ms                      one 3 * n_node vector of doubles to the device and one back through pageable host memory
                                 (hipMemcpy), the two bus crossings a follower load computed on the host would cost
  call_ms                        the whole fx_dload_groups call (host clock: list resolution, uploads, kernels, download)
No CPU fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NODES = {341: 4, 342: 10, 351: 6, 352: 15, 361: 8, 362: 20}


def stat(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3)}


def bus_copies_ms(n3, repeats):
    """one vector of n3 doubles to the device and back through pageable host memory (hipMemcpy of the HIP runtime)"""
    import ctypes as C
    rt = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    host = np.zeros(n3)
    dev = C.c_void_p()
    if rt.hipMalloc(C.byref(dev), C.c_size_t(8 * n3)) != 0:
        raise RuntimeError("hipMalloc failed")
    out = []
    for _ in range(repeats + 1):
        t = time.perf_counter()
        e1 = rt.hipMemcpy(dev, host.ctypes.data_as(C.c_void_p), C.c_size_t(8 * n3), 1)      # hipMemcpyHostToDevice
        e2 = rt.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, C.c_size_t(8 * n3), 2)      # hipMemcpyDeviceToHost
        out.append(1e3 * (time.perf_counter() - t))
        if e1 or e2:
            raise RuntimeError("hipMemcpy failed")
    rt.hipFree(dev)
    return stat(out[1:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=150, help="nodes per edge of the cube")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--types", default="361,341,351,362,342,352")
    a = ap.parse_args()
    from frontistr_amd import hecmw as hip
    from frontistr_amd.fstr import dload_faces, tDload
    from frontistr_amd.mesh import CubeMesh, mesh_groups, solid_mesh
    ctx = hip.SolverContext(device=0)
    for etype in [int(t) for t in a.types.split(",")]:
        cells = a.n - 1 if etype in (341, 351, 361) else (a.n - 1) // 2
        m = CubeMesh(cells, skew=0.05) if etype == 361 else solid_mesh(cells, etype, skew=0.05)
        groups = mesh_groups(m)
        ne, nn = int(m.conn.shape[0]), NODES[etype]
        top = m.coord[:, 2] == m.coord[:, 2].max()
        faces = dload_faces(m.coord, groups, top)
        el = np.arange(ne, dtype=np.int32)
        par = np.zeros((ne, 7))
        par[:, 0], par[:, 3] = 9.8, -1.0
        grav = (np.zeros(ne, dtype=np.int32), el, np.full(ne, 4, dtype=np.int32), par, None)
        press = tDload()
        for g, e, f in faces:
            press.pressure(g, [e], f, 1.0)
        out = {"etype": etype, "n_node": int(m.n_node), "n_elem": ne, "faces": len(faces)}

        def measure(dl, key, **kw):
            ks, ws = [], []
            for _ in range(a.repeats + 1):
                t = time.perf_counter()
                ctx.dload_groups(m.coord, groups, 7.8e-9, dl, **kw)
                ws.append(1e3 * (time.perf_counter() - t))
                ks.append(ctx.dload_stats()[key] / 1e3)
            return stat(ks[1:]), stat(ws[1:])

        out["grav_ms"], out["call_ms"] = measure(grav, "vol_us")
        out["grav_gbs"] = round(ne * (4 * nn + 69 + 48 * nn) / (out["grav_ms"]["median"] * 1e-3) / 1e9, 1)
        out["face_ms"], _ = measure(press, "face_us")
        disp = 0.01 * np.sin(np.arange(3 * m.n_node) * 0.37)
        gk, _ = measure(grav, "vol_us", disp=disp)
        fk, _ = measure(press, "face_us", disp=disp)
        out["follower_ms"] = {k: round(gk[k] + fk[k], 3) for k in gk}
        temp = 20.0 + 100.0 * m.coord[:, 2] / m.coord[:, 2].max()
        ts = [ctx.thermal_load_groups(m.coord, groups, 210000.0, 0.3, (temp, np.full(m.n_node, 20.0), 20.0, 1.2e-5))[1]
              for _ in range(a.repeats + 1)]
        out["thermal_ms"] = stat(ts[1:])
        out["copies_ms"] = bus_copies_ms(3 * int(m.n_node), a.repeats)
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    from _libarg import take_lib
    take_lib()      # --lib PATH: another build of the library (the parent commit's, say)
    main()
