#!/usr/bin/env python3
"""A synthetic NLSTATIC deck for fistr1 at any size: unit-spacing cube of n^3 C3D8 (TYPE=361) elements, z = 0 clamped, the top
face pulled by 0.5 % in z with a little shear, multilinear Mises plasticity of tutorial/05_plastic_cylinder (necking.cnt), updated
Lagrange (NLSTATIC default), SUBSTEPS sub-steps, CG + SSOR (or what --solver says) with TIMELOG.  Writes <dir>/cube.msh, cube.cnt,
hecmw_ctrl.dat (with the restart work-around of oracle/fistr1_run.py).  Used to time fistr1_hip end to end: device assembly
(default) against HECMW_GPU_ASSEMBLY=0 (scripts/r3/fistr1_big.sh).  usage: fistr1_cube_deck.py DIR N [SUBSTEPS] [METHOD] [PRECOND] [STRAIN]
--etype 341|342 (with or without --linear): the same cube split into tetrahedra (frontistr_amd.mesh.TetMesh, 6 per hexahedron; 342 with
mid-edge nodes), the node groups FIX / TOP listed by coordinate.  --etype 351|352|362 (with or without --linear): the cube split into wedges
(WedgeMesh, 2 per hexahedron; 352 with mid-edge nodes) or as 20-node hexahedra (Hex20Mesh).  --two-sections (with --linear): the second half of the elements
forms EGRP=E2 with its own section and material MAT2 (ELASTIC 70000, 0.33).  --mixed 1|2 (with or without --linear; without it an
NLSTATIC deck with the materials, steps and --two-sections variant of the other nonlinear cube decks): the cube as a mesh of
three element types (frontistr_amd.mesh.MixedMesh: 361 + 351 + 341, or 362 + 352 + 342 with shared mid-edge nodes), one !ELEMENT
card per type in mesh order; with --two-sections the second half of the elements in that order is EGRP=E2.
NLSTATIC decks of the STF_C3 types and of the mixed cube (--etype 341|342|351|352|362 or --mixed 1|2, without --linear) take two more options:
  --nl-material multilinear|bilinear|elastic_tl|elastic_ul   MAT1: Mises MULTILINEAR (default) or BILINEAR, both updated Lagrange;
                                                             ELASTIC total Lagrange; `!ELASTIC, CAUCHY`, updated Lagrange.
  --two-sections                                             the second half of the elements is MAT2, ELASTIC 70000 / 0.33, TOTAL
                                                             Lagrange: next to an updated-Lagrange MAT1 the deck mixes the two flags.
  --nl-material neohooke|mooney|arruda                       MAT1: `!HYPERELASTIC` NEOHOOKE (0.1486, 0.0789), MOONEY-RIVLIN (0.1486, 0.4849,
                                                             0.0789) or ARRUDA-BOYCE (0.71, 1.7029, 0.1408), the constants of the reference's
                                                             tutorials; total Lagrange.  Also for the plain TYPE=361 cube, also with
                                                             --two-sections: MAT2 is then ELASTIC 2.5 / 0.3, a material as soft as MAT1.
                                                             The fourth positional argument after DIR N, STRAIN, is the stretch to ask for
                                                             (rubber takes 0.1 where the steel decks take 0.005).
  --nl-material drucker|mohr                                 MAT1: `!PLASTIC, YIELD=DRUCKER-PRAGER` or `YIELD=MOHR-COULOMB` on ELASTIC 206900 / 0.29
                                                             with the data line c, phi, H = 300, 20 degrees, 2000 (Drucker-Prager) or
                                                             300, 5 degrees, 20000 (Mohr-Coulomb: at 20 degrees and H = 2000 the reference
                                                             program itself stops converging in the second sub-step); updated Lagrange.  Also for
                                                             the plain TYPE=361 cube, also with --two-sections: MAT2 is then Mises BILINEAR
                                                             (206900 / 0.29, 450, 2000), so that two yield functions share the mesh.
                                                             These decks ask the linear solver for 1e-12 where the others ask for 1e-8: after
                                                             the first plastic update every tangent is the elastic one, the sub-steps take 10
                                                             to 40 Newton iterations to CONVERG = 1e-3, and what the linear solves leave
                                                             unconverged stays in the printed stresses (2e-4 of 1.5 at 1e-8).
  --nl-material visco|visco_inf|norton [--visco-dt DT]       time-dependent MAT1 on ELASTIC 206900 / 0.29 and a `!STEP, TYPE=VISCO` step of
                                                             SUBSTEPS increments of DT (default 0.5; data line `DT, SUBSTEPS * DT`).
                                                             visco: `!VISCOELASTIC` with the Prony row 0.5, 1.0 of tutorial 07, total
                                                             Lagrange; visco_inf: the same with the card's INFINITE parameter.  norton:
                                                             `!CREEP, TYPE=NORTON` 1e-10, 5, 0 of tutorial 08, updated Lagrange, with a
                                                             `!STEP, TYPE=STATIC` step of one increment in front (time 0 to 1), so that the
                                                             VISCO step starts from a stressed state; its boundary group is applied a second
                                                             time by the VISCO step.  --two-sections: MAT2 is Mises BILINEAR, as for drucker / mohr.
--form361 FI|BBAR|IC|FBAR (TYPE=361 cubes, linear or NLSTATIC): `!SECTION, SECNUM=1, FORM361=...` (fstr_ctrl_common.f90:303-320), and the
same for SECNUM=2 with --two-sections; without it the program's default (IC in a linear analysis, B-bar under NLSTATIC).
--thermal (with --linear): a thermal-stress deck.  `!REFTEMP 20`, `!INITIAL CONDITION, TYPE=TEMPERATURE` (ALL, 25) in the mesh file,
`!TEMPERATURE` on the node groups FIX (35) and TOP (120) -- every other node keeps the initial condition's, so the temperature
varies inside the elements -- and `!EXPANSION_COEFF` 1.2e-5 for MAT1, 2.3e-5 for MAT2."""
import os
import sys

import numpy as np

linear = "--linear" in sys.argv      # !SOLUTION, TYPE=STATIC: bench.py's workload (z = 0 clamped, unit load in x on every top node, E = 210000, nu = 0.3)
if linear:
    sys.argv.remove("--linear")
form361 = None                       # --form361 FI|BBAR|IC|FBAR: `!SECTION, SECNUM=1, FORM361=...` (fstr_ctrl_common.f90:303-320); default: the program's
if "--form361" in sys.argv:
    k = sys.argv.index("--form361"); form361 = sys.argv[k + 1]; del sys.argv[k:k + 2]
    if form361 not in ("FI", "BBAR", "IC", "FBAR"):
        sys.exit("--form361 takes FI, BBAR, IC or FBAR")
etype = 361                          # --etype 341|342|351|352|362: tetrahedra, wedges, 20-node hexahedra
if "--etype" in sys.argv:
    k = sys.argv.index("--etype"); etype = int(sys.argv[k + 1]); del sys.argv[k:k + 2]
    if etype not in (341, 342, 351, 352, 362):
        sys.exit("--etype takes 341, 342, 351, 352 or 362")
mixed = 0                            # --mixed 1|2: hexahedra + wedges + tetrahedra of that order (linear or NLSTATIC decks)
if "--mixed" in sys.argv:
    k = sys.argv.index("--mixed"); mixed = int(sys.argv[k + 1]); del sys.argv[k:k + 2]
    if mixed not in (1, 2) or etype != 361:
        sys.exit("--mixed takes 1 or 2, without --etype")
nlmat = "multilinear"                # --nl-material (NLSTATIC decks): MAT1 = multilinear (default) | bilinear | elastic_tl | elastic_ul
if "--nl-material" in sys.argv:
    k = sys.argv.index("--nl-material"); nlmat = sys.argv[k + 1]; del sys.argv[k:k + 2]
    if linear or nlmat not in ("multilinear", "bilinear", "elastic_tl", "elastic_ul", "neohooke", "mooney", "arruda", "drucker", "mohr",
                               "visco", "visco_inf", "norton"):
        sys.exit("--nl-material takes multilinear, bilinear, elastic_tl, elastic_ul, neohooke, mooney, arruda, drucker, mohr, visco, "
                 "visco_inf or norton, without --linear")
hyper = nlmat in ("neohooke", "mooney", "arruda")
yieldf = nlmat in ("drucker", "mohr")
timed = nlmat in ("visco", "visco_inf", "norton")   # a `!STEP, TYPE=VISCO` step
visco_dt = 0.5
if "--visco-dt" in sys.argv:
    k = sys.argv.index("--visco-dt"); visco_dt = float(sys.argv[k + 1]); del sys.argv[k:k + 2]
    if not timed:
        sys.exit("--visco-dt needs --nl-material visco, visco_inf or norton")
two = "--two-sections" in sys.argv
if two:
    sys.argv.remove("--two-sections")
    if not linear and etype == 361 and not mixed and not hyper and not yieldf and not timed:
        sys.exit("--two-sections needs --linear, or --etype 341|342|351|352|362, or --mixed, or a hyperelastic or drucker / mohr --nl-material")
thermal = "--thermal" in sys.argv
if thermal:
    sys.argv.remove("--thermal")
    if not linear:
        sys.exit("--thermal needs --linear")
d, n = sys.argv[1], int(sys.argv[2])
nsub = int(sys.argv[3]) if len(sys.argv) > 3 else 2
method = sys.argv[4] if len(sys.argv) > 4 else "CG"
precond = sys.argv[5] if len(sys.argv) > 5 else "1"
strain = float(sys.argv[6]) if len(sys.argv) > 6 else 0.005      # top-face stretch (yield strain of the table: 0.0022)
os.makedirs(d, exist_ok=True)
m = n + 1
k, j, i = np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij")
nid = (1 + i + m * (j + m * k)).ravel()
xyz = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(float)
ek, ej, ei = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
n0 = (1 + ei + m * (ej + m * ek)).ravel()
conn = np.stack([n0, n0 + 1, n0 + 1 + m, n0 + m, n0 + m * m, n0 + 1 + m * m, n0 + 1 + m + m * m, n0 + m + m * m], axis=1)
if etype != 361:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from frontistr_amd.mesh import solid_mesh
    tm = solid_mesh(n, etype)
    nid, xyz, conn = np.arange(1, tm.n_node + 1), tm.coord, tm.conn
    if etype == 342:   # the mesh file lists the mid-edge nodes as (2,3), (3,1), (1,2), (1,4), (2,4), (3,4); fistr1 reorders them on input
        conn = conn[:, [0, 1, 2, 3, 5, 6, 4, 7, 8, 9]]
    if etype == 352:   # likewise: the file's triangle mid-edge nodes are (2,3), (3,1), (1,2) and (5,6), (6,4), (4,5); 362 is read as written
        conn = conn[:, [0, 1, 2, 3, 4, 5, 7, 8, 6, 10, 11, 9, 12, 13, 14]]
FILE_ORDER = {342: [0, 1, 2, 3, 5, 6, 4, 7, 8, 9], 352: [0, 1, 2, 3, 4, 5, 7, 8, 6, 10, 11, 9, 12, 13, 14]}   # as above
blocks = [(etype, conn)]             # (type, connectivity in the file's node order) per !ELEMENT type, in mesh order
if mixed:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from frontistr_amd.mesh import MixedMesh
    tm = MixedMesh(n, order=mixed)
    nid, xyz = np.arange(1, tm.n_node + 1), tm.coord
    blocks = [(et, c[:, FILE_ORDER[et]] if et in FILE_ORDER else c) for et, c in zip(tm.etypes, tm.conns)]
n_elem_all = sum(c.shape[0] for _, c in blocks)
with open(os.path.join(d, "cube.msh"), "w") as fh:
    fh.write("!HEADER\n synthetic cube, frontistr_amd scripts/fistr1_cube_deck.py\n!NODE\n")
    np.savetxt(fh, np.column_stack([nid, xyz]), fmt="%d,%.1f,%.1f,%.1f" if etype == 361 and not mixed else "%d,%.2f,%.2f,%.2f")
    half = n_elem_all // 2 if two else n_elem_all
    first = 0                        # elements before this block
    for btype, bconn in blocks:
        eid = np.arange(first + 1, first + bconn.shape[0] + 1)
        cut = min(max(half - first, 0), bconn.shape[0])
        if cut > 0:
            fh.write("!ELEMENT,TYPE=%d,EGRP=E1\n" % btype)
            np.savetxt(fh, np.column_stack([eid[:cut], bconn[:cut]]), fmt="%d", delimiter=",")
        if cut < bconn.shape[0]:
            fh.write("!ELEMENT,TYPE=%d,EGRP=E2\n" % btype)
            np.savetxt(fh, np.column_stack([eid[cut:], bconn[cut:]]), fmt="%d", delimiter=",")
        first += bconn.shape[0]
    fh.write("!MATERIAL,NAME=MAT1,ITEM=1\n!ITEM=1,SUBITEM=2\n 206900.0,0.29\n!SECTION,TYPE=SOLID,EGRP=E1,MATERIAL=MAT1\n")
    if two:
        fh.write("!MATERIAL,NAME=MAT2,ITEM=1\n!ITEM=1,SUBITEM=2\n 70000.0,0.33\n!SECTION,TYPE=SOLID,EGRP=E2,MATERIAL=MAT2\n")
    if thermal:
        fh.write("!INITIAL CONDITION, TYPE=TEMPERATURE\n ALL, 25.0\n")
    if etype == 361 and not mixed:
        fh.write("!NGROUP, NGRP=FIX, GENERATE\n 1,%d,1\n" % (m * m))
        fh.write("!NGROUP, NGRP=TOP, GENERATE\n %d,%d,1\n!END\n" % (m * m * n + 1, m * m * m))
    else:
        for name, ids in (("FIX", tm.bottom_nodes), ("TOP", tm.top_nodes)):
            fh.write("!NGROUP, NGRP=%s\n" % name)
            np.savetxt(fh, ids.reshape(-1, 1), fmt=" %d")
        fh.write("!END\n")
SECTIONS = "".join("!SECTION, SECNUM=%d, FORM361=%s\n" % (s, form361) for s in ((1, 2) if two else (1,))) if form361 else ""
if linear:
    with open(os.path.join(d, "cube.cnt"), "w") as fh:
        fh.write("""!VERSION
 3
!SOLUTION, TYPE=STATIC
!WRITE,RESULT,FREQUENCY=100000
%s!BOUNDARY
 FIX, 1, 3, 0.0
!CLOAD
 TOP, 1, 1.0
%s!MATERIAL, NAME=MAT1
!ELASTIC
 210000.0, 0.3
%s%s%s!RESTART, FREQUENCY=100000
!SOLVER,METHOD=%s,PRECOND=%s,ITERLOG=NO,TIMELOG=YES
 10000, 1
 1.0e-8, 1.0, 0.0
!END
""" % ("!REFTEMP\n 20.0\n" if thermal else "", "!TEMPERATURE\n FIX, 35.0\n TOP, 120.0\n" if thermal else "",
       "!EXPANSION_COEFF\n 1.2e-5\n" if thermal else "",
       ("!MATERIAL, NAME=MAT2\n!ELASTIC\n 70000.0, 0.33\n" + ("!EXPANSION_COEFF\n 2.3e-5\n" if thermal else "")) if two else "",
       SECTIONS, method, precond))
# MAT1 of the NLSTATIC deck.  multilinear / bilinear: Mises, updated Lagrange (the default of !PLASTIC); elastic_tl: total Lagrange
# (the default of !ELASTIC under NLSTATIC); elastic_ul: `!ELASTIC, CAUCHY`, updated Lagrange.  --two-sections: MAT2 is ELASTIC (total Lagrange).
NL_MATERIALS = {
    "multilinear": """!ELASTIC
 206900.0, 0.29
!PLASTIC, YIELD=MISES, HARDEN=MULTILINEAR
 450.0, 0.0
 608.0, 0.05
 679.0, 0.1
 732.0, 0.2
 752.0, 0.3
 766.0, 0.4
 780.0, 0.5
""",
    "bilinear": "!ELASTIC\n 206900.0, 0.29\n!PLASTIC, YIELD=MISES, HARDEN=BILINEAR\n 450.0, 2000.0\n",
    "elastic_tl": "!ELASTIC\n 206900.0, 0.29\n",
    "elastic_ul": "!ELASTIC, CAUCHY\n 206900.0, 0.29\n",
    "neohooke": "!HYPERELASTIC, TYPE=NEOHOOKE\n 0.1486, 0.0789\n",
    "mooney": "!HYPERELASTIC, TYPE=MOONEY-RIVLIN\n 0.1486, 0.4849, 0.0789\n",
    "arruda": "!HYPERELASTIC, TYPE=ARRUDA-BOYCE\n 0.71, 1.7029, 0.1408\n",
    "drucker": "!ELASTIC\n 206900.0, 0.29\n!PLASTIC, YIELD=DRUCKER-PRAGER\n 300.0, 20.0, 2000.0\n",
    "mohr": "!ELASTIC\n 206900.0, 0.29\n!PLASTIC, YIELD=MOHR-COULOMB\n 300.0, 5.0, 20000.0\n",
    "visco": "!ELASTIC\n 206900.0, 0.29\n!VISCOELASTIC\n 0.5, 1.0\n",
    "visco_inf": "!ELASTIC\n 206900.0, 0.29\n!VISCOELASTIC, INFINITE\n 0.5, 1.0\n",
    "norton": "!ELASTIC\n 206900.0, 0.29\n!CREEP, TYPE=NORTON\n 1.0e-10, 5.0, 0.0\n",
}
MAT2 = "!MATERIAL, NAME=MAT2\n!ELASTIC\n 70000.0, 0.33\n"
if hyper:
    MAT2 = "!MATERIAL, NAME=MAT2\n!ELASTIC\n 2.5, 0.3\n"
if yieldf or timed:
    MAT2 = "!MATERIAL, NAME=MAT2\n!ELASTIC\n 206900.0, 0.29\n!PLASTIC, YIELD=MISES, HARDEN=BILINEAR\n 450.0, 2000.0\n"
STEPS = "!STEP, SUBSTEPS=%d, CONVERG=1.0e-3\n BOUNDARY, 1\n" % nsub
if timed:
    STEPS = "!STEP, TYPE=VISCO, SUBSTEPS=%d, CONVERG=1.0e-3\n %r, %r\n BOUNDARY, 1\n" % (nsub, visco_dt, nsub * visco_dt)
    if nlmat == "norton":
        STEPS = "!STEP, TYPE=STATIC, SUBSTEPS=1, CONVERG=1.0e-3\n BOUNDARY, 1\n" + STEPS
with open(os.path.join(d, "cube.cnt"), "a" if linear else "w") as fh:
    if not linear:
      fh.write("""!VERSION
 3
!SOLUTION, TYPE=NLSTATIC
!WRITE,RESULT,FREQUENCY=100000
!BOUNDARY, GRPID=1
 FIX, 1, 3, 0.0
 TOP, 3, 3, %g
 TOP, 1, 1, %g
%s!MATERIAL, NAME=MAT1
%s%s%s!RESTART, FREQUENCY=100000
!SOLVER,METHOD=%s,PRECOND=%s,ITERLOG=NO,TIMELOG=YES
 5000, 1
 %s, 1.0, 0.0
!END
""" % (strain * n, 0.2 * strain * n, STEPS, NL_MATERIALS[nlmat],
       MAT2 if two else "", SECTIONS, method, precond, "1.0e-12" if yieldf or timed else "1.0e-8"))
with open(os.path.join(d, "hecmw_ctrl.dat"), "w") as fh:
    fh.write("!MESH, NAME=fstrMSH,TYPE=HECMW-ENTIRE\n cube.msh\n!CONTROL,NAME=fstrCNT\n cube.cnt\n"
             "!RESULT,NAME=fstrRES,IO=OUT\n out.res\n!RESTART,NAME=restart_out,IO=OUT\n out.restart\n")
print("wrote", d, "nodes", nid.size, "dof", 3 * nid.size, "elements", n_elem_all)
