"""Device assembly (fstr_StiffMatrix + fstr_AddBC) on the n^3-element cube: ms per call for ELEMOPT361 = IC / B-bar / FI.
FX_ASM_ATOMIC=1 selects the single-launch atomic scatter instead of the coloured one.  Usage: python scripts/bench_assembly.py [n]

--etype 341|342: the same cube split into tetrahedra (TetMesh; 6 per hexahedron, at 342 with mid-edge nodes): ms per call of
fx_assemble_c3 (three warm calls), the algorithmic bytes of one call (matrix values written once, position map, connectivity
and coordinates read once) and the bandwidth they imply.  Usage: python scripts/bench_assembly.py --etype 342 [n]
--etype 351|352|362: the cube split into wedges (WedgeMesh, 2 per hexahedron) or as 20-node hexahedra (Hex20Mesh), the same
figures; n defaults to the smallest cube with a million elements.  --update adds ms per fx_update_c3_linear kernel (three
calls, displacement = a smooth field) and the bytes it must move (strain and stress written, connectivity, coordinates and
displacement read).
--mixed 1|2: the cube as a mesh of three types (MixedMesh: 361 + 351 + 341, or 362 + 352 + 342), n defaults to 72 (1.03 M
elements): ms per fx_assemble_groups call (three warm calls after the first, which colours and maps) and, beside it, the three
single-type assemblies of the same element sets through fx_assemble_c3d8 / fx_assemble_c3, each into the profile of its own
elements, and their sum; the colour launches of the mixed call.
Beside every list of event milliseconds ("ms", "update_ms", ...) stands the wall time of the same calls as the caller sees
them ("wall_ms", "update_wall_ms", ...): the events time the kernels only, the wall time also the host work of the call
(argument checks, colouring checksum, uploads, downloads).  FX_LIBPATH selects another build of the library."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from frontistr_amd import hecmw as hip          # noqa: E402
if os.environ.get("FX_LIBPATH"):
    hip.LIBPATH = os.environ["FX_LIBPATH"]      # timing experiments: another build of the library
from frontistr_amd.mesh import CubeMesh          # noqa: E402

from frontistr_amd.mesh import solid_mesh        # noqa: E402



def timed(calls):
    """([result of each call], [wall milliseconds of each call])"""
    res, wall = [], []
    for call in calls:
        t = time.perf_counter()
        res.append(call())
        wall.append(round(1e3 * (time.perf_counter() - t), 2))
    return res, wall


args = sys.argv[1:]
with_update = "--update" in args
if with_update:
    args.remove("--update")
etype = None
if "--etype" in args:
    k = args.index("--etype")
    etype = int(args[k + 1])
    del args[k:k + 2]
mixed = 0
if "--mixed" in args:
    k = args.index("--mixed")
    mixed = int(args[k + 1])
    del args[k:k + 2]
if mixed:
    import numpy as np
    from frontistr_amd.mesh import MixedMesh
    n = int(args[0]) if args else 72
    mesh = MixedMesh(n, order=mixed)
    groups = mesh.groups
    hm = hip.hecmwST_local_mesh(n_node=mesh.n_node)
    m = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)
    ctx = hip.SolverContext()
    ctx.upload(m, hm, what=hip.FX_UP_PROFILE)
    load, bc = mesh.load(), mesh.dirichlet()
    (first, *ms), (first_wall, *wall) = timed([lambda: ctx.assemble_groups(mesh.coord, groups, 210000.0, 0.3, load=load, bc=bc)] * 4)
    ctx.close()
    out = {"mixed": mixed, "n": n, "types": list(mesh.etypes), "n_elem": [int(c.shape[0]) for c in mesh.conns], "dof": 3 * mesh.n_node,
           "blocks": int(m.NP + m.NPL + m.NPU), "colouring": "per group, groups one after another",
           "scatter": "atomic" if os.environ.get("FX_ASM_ATOMIC", "0") not in ("", "0") else "coloured",
           "first_call_ms": round(first, 2), "ms": [round(v, 2) for v in ms], "spread_ms": round(max(ms) - min(ms), 2),
           "first_call_wall_ms": first_wall, "wall_ms": wall}
    single, single_wall = {}, {}
    for et, conn, _, _ in groups:              # the same elements alone, through the single-type entry point, in their own profile
        hs = hip.hecmwST_local_mesh(n_node=mesh.n_node)
        hs.nn_elem = conn.shape[1]
        hs.elem_node_item = conn.ravel()
        ms1 = hip.hecmw_mat_con(hs, hip.hecmwST_matrix())
        c1 = hip.SolverContext()
        c1.upload(ms1, hs, what=hip.FX_UP_PROFILE)
        if et == 361:
            t, w = timed([lambda: c1.assemble_c3d8(mesh.coord, conn, 210000.0, 0.3, elemopt=1, load=load, bc=bc)] * 4)
        else:
            t, w = timed([lambda: c1.assemble_c3(mesh.coord, conn, et, 210000.0, 0.3, load=load, bc=bc)] * 4)
        c1.close()
        single[str(et)], single_wall[str(et)] = [round(v, 2) for v in t[1:]], w[1:]
    out["single_type_ms"] = single
    out["single_type_wall_ms"] = single_wall
    out["single_type_sum_ms"] = [round(sum(single[k][i] for k in single), 2) for i in range(3)]
    print(json.dumps(out))
    sys.exit(0)
if etype is not None:
    n = int(args[0]) if args else {341: 74, 342: 74, 351: 80, 352: 80, 362: 100}[etype]
    mesh = solid_mesh(n, etype)
    nn = mesh.conn.shape[1]
    hm = hip.hecmwST_local_mesh(n_node=mesh.n_node)
    hm.nn_elem = nn
    hm.elem_node_item = mesh.conn.ravel()
    m = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(m, hm, what=hip.FX_UP_PROFILE)
    load, bc = mesh.load(), mesh.dirichlet()
    ms, wall = timed([lambda: ctx.assemble_c3(mesh.coord, mesh.conn, etype, 210000.0, 0.3, load=load, bc=bc)] * 3)
    nbytes = (72 * (m.NP + m.NPL + m.NPU)                  # D / AL / AU written once
              + 4 * nn * nn * mesh.n_elem                  # position map
              + 4 * nn * mesh.n_elem + 24 * mesh.n_node)   # connectivity, coordinates
    out = {"etype": etype, "n_elem": int(mesh.n_elem), "dof": 3 * mesh.n_node,
           "scatter": "atomic" if os.environ.get("FX_ASM_ATOMIC", "0") not in ("", "0") else "coloured",
           "ms": [round(v, 2) for v in ms], "wall_ms": wall, "algorithmic_GB": round(nbytes / 1e9, 3),
           "GBps": round(nbytes / 1e6 / min(ms), 1), "fraction_of_8TBps": round(nbytes / 1e6 / min(ms) / 8000.0, 3)}
    if with_update:
        import numpy as np
        from frontistr_amd.mesh import C3_POINTS
        u = 1e-3 * np.sin(mesh.coord @ np.array([[0.3, 0.1, 0.2], [0.2, 0.4, 0.1], [0.1, 0.2, 0.5]])).ravel()
        ums, uwall = timed([lambda: ctx.update_c3_linear(mesh.coord, mesh.conn, etype, 210000.0, 0.3, u)[3]] * 3)
        ub = 2 * 48 * C3_POINTS[etype] * mesh.n_elem + 4 * nn * mesh.n_elem + 2 * 24 * mesh.n_node + 24 * mesh.n_node
        out.update({"update_ms": [round(v, 2) for v in ums], "update_wall_ms": uwall, "update_algorithmic_GB": round(ub / 1e9, 3),
                    "update_GBps": round(ub / 1e6 / min(ums), 1)})
    print(json.dumps(out))
    sys.exit(0)
n = int(args[0]) if args else 149
mesh = CubeMesh(n)
hm = hip.hecmwST_local_mesh(n_node=mesh.n_node)
hm.elem_node_item = mesh.conn.ravel()
m = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
ctx = hip.SolverContext()
ctx.upload(m, hm, what=hip.FX_UP_PROFILE)
out = {"n_elem": int(mesh.conn.shape[0]), "dof": 3 * mesh.n_node, "scatter": "atomic" if os.environ.get("FX_ASM_ATOMIC", "0") not in ("", "0") else "coloured"}
load, bc = mesh.load(), mesh.dirichlet()
for eo, name in ((1, "ic"), (2, "bbar"), (3, "fi")):
    ms, wall = timed([lambda: ctx.assemble_c3d8(mesh.coord, mesh.conn, 210000.0, 0.3, elemopt=eo, load=load, bc=bc)] * 3)
    out[name + "_ms"], out[name + "_wall_ms"] = [round(v, 2) for v in ms], wall
print(json.dumps(out))
