"""The three small NLSTATIC cantilever decks under a follower pressure that tests/golden/make_dload_nl_golden.py records through the
unmodified fistr1 (tests/golden/dload_nl.npz; committed copies of the decks under tests/golden/decks/dload/), as arrays and as
files: 3 x 1 x 1 cells along x, the x = 0 side clamped, pressure on every face of the top side (z = 1) given as a surface group,
two sub-steps.

    c361  TYPE=361 B-bar, ELASTIC (total Lagrange)
    c342  TYPE=342, Mises BILINEAR (updated Lagrange), gravity on all elements as well
    c352  TYPE=352, ELASTIC (total Lagrange)

Each deck is run twice: `!DLOAD` as it is (DLOAD_follow = 1, the default) and `!DLOAD, FOLLOW=NO`.  The pressure bends the beam by
about a third of its length, so the two runs differ by far more than 1 % in the displacement extrema (the generator asserts it)."""
import os

import numpy as np

from frontistr_amd.mesh import _KUHN, _PRISMS, PRISM15_EDGES, TET10_EDGES, _add_midedge_nodes

HERE = os.path.dirname(os.path.abspath(__file__))
DECKDIR = os.path.join(HERE, "golden", "decks", "dload")
GOLDEN = os.path.join(HERE, "golden", "dload_nl.npz")
NAMES = ("c361", "c342", "c352")
ETYPE = {"c361": 361, "c342": 342, "c352": 352}
SUBSTEPS, CONVERG, MAX_ITER = 2, 1.0e-6, 50
E, NU = 1000.0, 0.3
YIELD0, HARDEN = 60.0, 200.0            # c342: Mises BILINEAR
PRESSURE = {"c361": 4.0, "c342": 3.0, "c352": 4.0}
RHO, GRAV = 0.1, (9.8, 0.0, 0.0, -1.0)  # c342
FILE_ORDER = {342: [0, 1, 2, 3, 5, 6, 4, 7, 8, 9], 352: [0, 1, 2, 3, 4, 5, 7, 8, 6, 10, 11, 9, 12, 13, 14]}   # the mesh file's node order
SUBFACE_VERTICES = {361: ((1, 2, 3, 4), (8, 7, 6, 5), (5, 6, 2, 1), (6, 7, 3, 2), (7, 8, 4, 3), (8, 5, 1, 4)),
                    342: ((1, 2, 3), (4, 2, 1), (4, 3, 2), (4, 1, 3)),
                    352: ((1, 2, 3), (6, 5, 4), (4, 5, 2, 1), (5, 6, 3, 2), (6, 4, 1, 3))}


def cantilever(etype):
    """-> (coord, conn in FrontISTR's node order, 1-based)"""
    nx, ny, nz = 3, 1, 1
    k, j, i = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    coord = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float64)
    mx, my = nx + 1, ny + 1
    n0 = 1 + np.arange(nx)
    hexes = np.stack([n0, n0 + 1, n0 + 1 + mx, n0 + mx, n0 + mx * my, n0 + 1 + mx * my, n0 + 1 + mx + mx * my, n0 + mx + mx * my], axis=1)
    if etype == 361:
        return coord, np.ascontiguousarray(hexes.astype(np.int32))
    if etype == 342:
        conn = np.concatenate([hexes[:, list(t)] for t in _KUHN], axis=1).reshape(-1, 4)
        edges = TET10_EDGES
    else:
        conn = np.concatenate([hexes[:, list(p)] for p in _PRISMS], axis=1).reshape(-1, 6)
        edges = PRISM15_EDGES
    coord, conn = _add_midedge_nodes(coord, conn, edges, 0.0, 0.0, 1.0, 1.0)
    return np.ascontiguousarray(coord), np.ascontiguousarray(conn.astype(np.int32))


def top_faces(etype, coord, conn):
    """(element 0-based, face 1-based) of the faces whose vertices all lie on z = 1"""
    out = []
    for f, nod in enumerate(SUBFACE_VERTICES[etype]):
        hit = (coord[conn[:, np.array(nod) - 1] - 1, 2] == 1.0).all(axis=1)
        out += [(int(e), f + 1) for e in np.nonzero(hit)[0]]
    return sorted(out)


def fix_nodes(coord):
    return (1 + np.flatnonzero(coord[:, 0] == 0.0)).astype(np.int32)


def material_card(name):
    if name == "c342":
        return "!ELASTIC\n %r, %r\n!PLASTIC, YIELD=MISES, HARDEN=BILINEAR\n %r, %r\n!DENSITY\n %r\n" % (E, NU, YIELD0, HARDEN, RHO)
    return "!ELASTIC\n %r, %r\n" % (E, NU)


def write_deck(name, follow, d):
    """cube.msh, cube.cnt, hecmw_ctrl.dat of deck ``name`` into directory d"""
    etype = ETYPE[name]
    coord, conn = cantilever(etype)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "cube.msh"), "w") as fh:
        fh.write("!HEADER\n cantilever under pressure, tests/dload_nl_decks.py\n!NODE\n")
        np.savetxt(fh, np.column_stack([np.arange(1, coord.shape[0] + 1), coord]), fmt="%d,%.2f,%.2f,%.2f")
        fh.write("!ELEMENT,TYPE=%d,EGRP=E1\n" % etype)
        fc = conn[:, FILE_ORDER[etype]] if etype in FILE_ORDER else conn
        np.savetxt(fh, np.column_stack([np.arange(1, conn.shape[0] + 1), fc]), fmt="%d", delimiter=",")
        fh.write("!MATERIAL,NAME=MAT1,ITEM=1\n!ITEM=1,SUBITEM=2\n %r,%r\n!SECTION,TYPE=SOLID,EGRP=E1,MATERIAL=MAT1\n" % (E, NU))
        fh.write("!NGROUP, NGRP=FIX\n")
        np.savetxt(fh, fix_nodes(coord).reshape(-1, 1), fmt=" %d")
        fh.write("!SGROUP, SGRP=TOPS\n")
        for e, f in top_faces(etype, coord, conn):
            fh.write(" %d, %d\n" % (e + 1, f))
        fh.write("!END\n")
    with open(os.path.join(d, "cube.cnt"), "w") as fh:
        fh.write("!VERSION\n 3\n!SOLUTION, TYPE=NLSTATIC\n!WRITE,RESULT,FREQUENCY=100000\n!BOUNDARY, GRPID=1\n FIX, 1, 3, 0.0\n")
        fh.write("!DLOAD, GRPID=1%s\n TOPS, S, %r\n" % ("" if follow else ", FOLLOW=NO", PRESSURE[name]))
        if name == "c342":
            fh.write(" ALL, GRAV, %r, %r, %r, %r\n" % GRAV)
        fh.write("!STEP, SUBSTEPS=%d, CONVERG=%r\n BOUNDARY, 1\n LOAD, 1\n" % (SUBSTEPS, CONVERG))
        fh.write("!MATERIAL, NAME=MAT1\n" + material_card(name))
        fh.write("!RESTART, FREQUENCY=100000\n!SOLVER,METHOD=CG,PRECOND=1,ITERLOG=NO,TIMELOG=YES\n 5000, 1\n 1.0e-10, 1.0, 0.0\n!END\n")
    with open(os.path.join(d, "hecmw_ctrl.dat"), "w") as fh:
        fh.write("!MESH, NAME=fstrMSH,TYPE=HECMW-ENTIRE\n cube.msh\n!CONTROL,NAME=fstrCNT\n cube.cnt\n"
                 "!RESULT,NAME=fstrRES,IO=OUT\n out.res\n!RESTART,NAME=restart_out,IO=OUT\n out.restart\n")


def tag(name, follow):
    return "%s_%s" % (name, "follow" if follow else "fixed")
