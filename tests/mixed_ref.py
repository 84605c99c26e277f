"""Numpy / oracle restatement of the reference's assembly and linear stress update for a mesh of SEVERAL solid element types:
fstr_StiffMatrix.f90:43-212's and fstr_Update.f90:73-264's loops over hecMESH%elem_type_item, each type through the restatement
the single-type tests already pin to the reference -- tests/tet_ref.py (341, 342), tests/c3_ref.py (351, 352, 362) and
oracle.pyoracle.stf_c3d8 / update_linear (361: STF_C3D8IC, STF_C3D8Bbar, STF_C3 by elemopt).  ``groups`` is what
SolverContext.assemble_groups takes: [(etype, conn, elemopt, elem_mat)] (conn (n_elem, nn) 1-based; elem_mat 1-based or None)."""
import os

import numpy as np

import c3_ref as C3
import tet_ref as T
from tet_ref import apply_bc, dense_of, to_blocks  # noqa: F401

NN = {361: 8, 341: 4, 342: 10, 351: 6, 352: 15, 362: 20}
NQ = {361: 8, 341: 1, 342: 4, 351: 2, 352: 9, 362: 27}
DECK_E, DECK_NU = T.DECK_E, T.DECK_NU
HERE = os.path.dirname(os.path.abspath(__file__))


def _module(etype):
    return T if etype in (341, 342) else C3


def element_stiffness(etype, ec, E, nu, elemopt=1):
    if etype == 361:
        from oracle import pyoracle as po
        return po.stf_c3d8(int(elemopt), ec, float(E), float(nu))
    return _module(etype).element_stiffness(etype, ec, E, nu)


def element_dets(etype, ec):
    """Jacobian determinants at the quadrature points (361: the 2 x 2 x 2 Gauss points, through the trilinear derivatives)."""
    if etype == 361:
        g = 0.577350269189626
        out = []
        for lc in [(x, y, z) for z in (-g, g) for y in (-g, g) for x in (-g, g)]:
            dN = np.array([[sx * (1 + sy * lc[1]) * (1 + sz * lc[2]), sy * (1 + sx * lc[0]) * (1 + sz * lc[2]),
                            sz * (1 + sx * lc[0]) * (1 + sy * lc[1])] for sx, sy, sz in C3.HEX_VERTS]) / 8.0
            out.append(np.linalg.det(np.asarray(ec).T @ dN))
        return np.array(out)
    return _module(etype).element_dets(etype, ec)


def global_matrix(coord, groups, E, nu):
    """Dense global stiffness, the groups in order, element matrices added in element order.  E, nu scalars or per-material
    arrays (a group without elem_mat takes the first)."""
    Es, nus = np.atleast_1d(np.asarray(E, dtype=np.float64)), np.atleast_1d(np.asarray(nu, dtype=np.float64))
    n = coord.shape[0]
    K = np.zeros((3 * n, 3 * n))
    for grp in groups:
        etype, conn = int(grp[0]), np.asarray(grp[1])
        elemopt = grp[2] if len(grp) > 2 and grp[2] is not None else 1
        em = grp[3] if len(grp) > 3 else None
        for e in range(conn.shape[0]):
            m = 0 if em is None else em[e] - 1
            dofs = (3 * (conn[e][:, None] - 1) + np.arange(3)).ravel()
            # every (ie, je) block is added (hecmw_mat_ass_elem): np.add.at also where a collapsed hexahedron names a node twice
            np.add.at(K, (dofs[:, None], dofs[None, :]), element_stiffness(etype, coord[conn[e] - 1], Es[m], nus[m], elemopt))
    return K


def assemble(coord, groups, E, nu, bc=None, load=None):
    """Dense K and right-hand side after the boundary conditions (applied once, after the last group)."""
    K = global_matrix(coord, groups, E, nu)
    f = np.zeros(3 * coord.shape[0]) if load is None else np.asarray(load, dtype=np.float64).copy()
    return apply_bc(K, f, bc)


def update(coord, groups, E, nu, disp):
    """([strain per group], [stress per group], qforce summed over the groups)."""
    from oracle import pyoracle as po
    Es, nus = np.atleast_1d(np.asarray(E, dtype=np.float64)), np.atleast_1d(np.asarray(nu, dtype=np.float64))
    strain, stress, qf = [], [], np.zeros(3 * coord.shape[0])
    for grp in groups:
        etype, conn = int(grp[0]), np.asarray(grp[1])
        elemopt = grp[2] if len(grp) > 2 and grp[2] is not None else 1
        em = grp[3] if len(grp) > 3 else None
        if etype == 361:
            if em is None:
                s, t, q = po.update_linear(int(elemopt), coord, conn, float(Es[0]), float(nus[0]), disp)[:3]
            else:
                s, t, q = po.update_linear(int(elemopt), coord, conn, Es, nus, disp, elem_mat=em)[:3]
        elif em is None:
            s, t, q = _module(etype).update(etype, coord, conn, Es[0], nus[0], disp)
        else:
            s, t, q = _module(etype).update(etype, coord, conn, Es, nus, disp, elem_mat=em)
        strain.append(s); stress.append(t)
        qf += q
    return strain, stress, qf


def profile(hip, n_node, groups):
    """hecmwST_matrix with the block profile of the union of the groups."""
    hm = hip.hecmwST_local_mesh(n_node=n_node)
    return hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)


def faces_of(etype, nodes):
    """The faces of a first-order element (or of the vertices of a second-order one) as sorted vertex tuples."""
    v = list(nodes)
    if etype in (361, 362):
        f = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7))
    elif etype in (351, 352):
        f = ((0, 1, 2), (3, 4, 5), (0, 1, 4, 3), (1, 2, 5, 4), (2, 0, 3, 5))
    else:
        f = ((0, 1, 2), (0, 1, 3), (1, 2, 3), (2, 0, 3))
    return [tuple(sorted(int(v[i]) for i in face)) for face in f]


# ---- the reference's own assembly: tests/golden/mixed_decks.npz (make_mixed_golden.py) -----------------------------------
REF_DECKS = ("hexpritet", "tetpri")                       # tests/golden/decks/refine/<name>/sample.msh, sample.cnt
CUBE_DECKS = (("m1_n2", 1, 2, False), ("m1_n2_two", 1, 2, True), ("m2_n2", 2, 2, False), ("m2_n2_two", 2, 2, True))


def dense_of_dump(g, name):
    iL, jL, iU, jU = (g[name + "/" + k] for k in ("indexL", "itemL", "indexU", "itemU"))
    D, AL, AU = g[name + "/D"], g[name + "/AL"], g[name + "/AU"]
    nr = iL.size - 1
    K = np.zeros((3 * nr, 3 * nr))
    for i in range(nr):
        K[3 * i:3 * i + 3, 3 * i:3 * i + 3] = D[9 * i:9 * i + 9].reshape(3, 3)
        for k in range(iL[i], iL[i + 1]):
            K[3 * i:3 * i + 3, 3 * (jL[k] - 1):3 * jL[k]] = AL[9 * k:9 * k + 9].reshape(3, 3)
        for k in range(iU[i], iU[i + 1]):
            K[3 * i:3 * i + 3, 3 * (jU[k] - 1):3 * jU[k]] = AU[9 * k:9 * k + 9].reshape(3, 3)
    return K


def cube_deck(order, n, two):
    """(mesh, groups, E, nu) of a recorded --mixed cube deck: MixedMesh(n, order) in the library's node order; with two
    sections the first half of the elements (mesh order) is MAT1, the second MAT2."""
    from frontistr_amd.mesh import MixedMesh
    m = MixedMesh(n, order=order)
    if not two:
        return m, m.groups, DECK_E[0], DECK_NU[0]
    em = np.where(np.arange(m.n_elem) < m.n_elem // 2, 1, 2).astype(np.int32)
    return m, m.groups_with(elem_mat=em), DECK_E, DECK_NU


def read_ref_deck(name):
    """(coord, groups, E, nu, bc) of tests/golden/decks/refine/<name>: sample.msh's nodes, elements (one group per !ELEMENT card),
    material and node groups, and the !BOUNDARY card of sample.cnt.  Local node ids are the positions in the !NODE card (tetpri
    numbers its nodes from 1001; HEC-MW keeps the file's order)."""
    d = os.path.join(HERE, "golden", "decks", "refine", name)
    coord, groups, ngroups, E, nu, local = [], [], {}, None, None, {}
    card, arg = None, None
    for line in open(os.path.join(d, "sample.msh")):
        s = line.strip()
        if not s or s.startswith("#") or s.startswith("!!"):
            continue
        if s.startswith("!"):
            p = [x.strip() for x in s[1:].split(",")]
            card, arg = p[0].upper(), {k.strip().upper(): v.strip() for k, v in (x.split("=") for x in p[1:] if "=" in x)}
            arg["_FLAGS"] = [x.upper() for x in p[1:] if "=" not in x]
            if card == "ELEMENT":
                groups.append([int(arg["TYPE"]), []])
            if card == "NGROUP":
                ngroups.setdefault(arg["NGRP"], [])
            continue
        v = [x for x in s.replace(",", " ").split()]
        if card == "NODE":
            local[int(v[0])] = len(coord) + 1
            coord.append([float(x) for x in v[1:4]])
        elif card == "ELEMENT":
            groups[-1][1].append([local[int(x)] for x in v[1:]])
        elif card == "ITEM=1" or (card == "MATERIAL" and E is None and len(v) == 2):
            E, nu = float(v[0]), float(v[1])
        elif card == "NGROUP":
            ids = [int(x) for x in v]
            ids = list(range(ids[0], ids[1] + 1)) if "GENERATE" in arg["_FLAGS"] else ids
            ngroups[arg["NGRP"]] += [local[i] for i in ids]
    bn, bd, bv = [], [], []
    card = None
    for line in open(os.path.join(d, "sample.cnt")):
        s = line.strip()
        if not s or s.startswith("#") or s.startswith("!!"):
            continue
        if s.startswith("!"):
            card = s[1:].split(",")[0].strip().upper()
            continue
        if card == "BOUNDARY":
            v = [x.strip() for x in s.split(",")]
            for node in ngroups[v[0]]:
                for dof in range(int(v[1]), int(v[2]) + 1):
                    bn.append(node); bd.append(dof); bv.append(float(v[3]))
    out = [(et, np.array(c, dtype=np.int32), 1, None) for et, c in groups]
    return np.array(coord), out, E, nu, (np.array(bn, dtype=np.int32), np.array(bd, dtype=np.int32), np.array(bv))
