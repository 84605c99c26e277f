"""Numpy restatement of the reference's thermal load vector and of the thermal branches of its linear stress update, for the six
solid types of the device path (isotropic ELASTIC, one constant expansion coefficient per material, small strain):

  TLOAD_C3        static_LIB_3d.f90:381-511      341 / 342 / 351 / 352 / 362, and 361 with full integration (elemopt 3)
  TLOAD_C3D8Bbar  static_LIB_C3D8.f90:556-705    361 elemopt 2 -- the thermal strain of EVERY point from the CENTROID's temperatures
  TLOAD_C3D8IC    static_LIB_3dIC.f90:460-625    361 elemopt 1 -- 8 + 3 modes, condensed with the element's own [Kaa]^-1
  UPDATE_C3 :516-837, Update_C3D8Bbar :203-552 (INFINITE branches), UpdateST_C3D8IC :220-455

  EPSTH(1:3) = alp (TEMPC - ref_temp) - alp0 (TEMP0 - ref_temp), TEMPC = H . TT, TEMP0 = H . T0; stress = D (strain - EPSTH), the
  stored strain is the total one; qf = sum_g wg B^T stress; IC: qf = [Kdd Kda][u; alpha] - TLOAD_C3D8IC (its alpha has no thermal part).

Element data (shape-function derivatives, quadrature) come from c3_ref / tet_ref; the shape functions themselves (the update
needed only derivatives) of the tetrahedra and of the 8-node hexahedron are added here.  ``order``: a permutation of the element's
nodes in which the sums over nodes run (the spread between two orders is the rounding the GPU tolerance has to allow).
``thermal`` = (temp, temp0, ref_temp, alpha) with node arrays and one alpha per material.
"""
import numpy as np

import c3_ref as R
import tet_ref as T

GP = 0.577350269189626
NN = dict(R.NN)
NN[361] = 8
HEX8_PTS = np.array([[sx * GP, sy * GP, sz * GP] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)])   # xi fastest (quadrature.f90)


def quad(etype):
    return (HEX8_PTS, np.ones(8)) if etype == 361 else R.QUAD[etype]


def nq(etype):
    return quad(etype)[0].shape[0]


def shape_func(etype, lc):
    xi, et, ze = lc
    if etype == 361:
        return np.array([0.125 * (1 + sx * xi) * (1 + sy * et) * (1 + sz * ze) for sx, sy, sz in R.HEX_VERTS])
    if etype == 341:
        return np.array([1.0 - xi - et - ze, xi, et, ze])
    if etype == 342:
        a = 1.0 - xi - et - ze
        return np.array([(2 * a - 1) * a, xi * (2 * xi - 1), et * (2 * et - 1), ze * (2 * ze - 1), 4 * xi * a, 4 * xi * et, 4 * et * a,
                         4 * ze * a, 4 * xi * ze, 4 * et * ze])
    return R.shape_func(etype, lc)


def shape_deriv(etype, lc):
    if etype == 361:
        xi, et, ze = lc
        return np.array([[sx * 0.125 * (1 + sy * et) * (1 + sz * ze), sy * 0.125 * (1 + sx * xi) * (1 + sz * ze),
                          sz * 0.125 * (1 + sx * xi) * (1 + sy * et)] for sx, sy, sz in R.HEX_VERTS])
    return R.shape_deriv(etype, lc)


def _gderiv(etype, ec, lc):
    dN = shape_deriv(etype, lc)
    det, inv = T.jacobian(ec, dN)
    return dN @ inv, det


def _bbar_matrix(gd, bbar):
    B = T.b_matrix(gd)
    h = (bbar - gd) / 3.0
    for r in range(3):
        B[r, 0::3] += h[:, 0]; B[r, 1::3] += h[:, 1]; B[r, 2::3] += h[:, 2]
    return B


def _dot(h, t, order):
    s = 0.0
    for a in order:
        s += h[a] * t[a]
    return s


def _epsth(alp, tc, t0, ref):
    e = np.zeros(6)
    e[:3] = alp * (tc - ref) - alp * (t0 - ref)
    return e


def _ic_parts(ec, E, nu):
    """The 33 x 33 matrix [Kdd Kda; Kad Kaa] of the IC element, and per point (B (6, 33), wg, natural coordinates)."""
    D = T.elastic_matrix(E, nu)
    det0, inv0 = T.jacobian(ec, shape_deriv(361, (0.0, 0.0, 0.0)))
    inv0 = inv0 * det0
    K = np.zeros((33, 33))
    pts = []
    for lc in HEX8_PTS:
        gd, det = _gderiv(361, ec, lc)
        gm = np.array([-2.0 * lc[m] * inv0[m] / det for m in range(3)])
        B = T.b_matrix(np.concatenate([gd, gm]))
        K += (B.T @ (D @ B)) * det
        pts.append((B, det, lc))
    return D, K, pts


def tload(etype, elemopt, ec, tt, t0, ref, alp, E, nu, order=None):
    """One element's thermal load vector (3 nn)."""
    nn = NN[etype]
    order = range(nn) if order is None else order
    D = T.elastic_matrix(E, nu)
    if etype == 361 and elemopt == 1:
        D, K, pts = _ic_parts(ec, E, nu)
        tmp = np.zeros(33)
        for B, wg, lc in pts:
            h = shape_func(361, lc)
            tmp += ((D @ _epsth(alp, _dot(h, tt, order), _dot(h, t0, order), ref)) @ B) * wg
        return tmp[:24] - K[:24, 24:] @ (np.linalg.inv(K[24:, 24:]) @ tmp[24:])
    pts, w = quad(etype)
    vect = np.zeros(3 * nn)
    if etype == 361 and elemopt == 2:
        bbar, _ = _gderiv(361, ec, (0.0, 0.0, 0.0))
        h0 = shape_func(361, (0.0, 0.0, 0.0))
        e = _epsth(alp, _dot(h0, tt, order), _dot(h0, t0, order), ref)
    for q in range(pts.shape[0]):
        gd, det = _gderiv(etype, ec, pts[q])
        if etype == 361 and elemopt == 2:
            B = _bbar_matrix(gd, bbar)
        else:
            B = T.b_matrix(gd)
            h = shape_func(etype, pts[q])
            e = _epsth(alp, _dot(h, tt, order), _dot(h, t0, order), ref)
        vect += ((D @ e) @ B) * (w[q] * det)
    return vect


def update_element(etype, elemopt, ec, ue, tt, t0, ref, alp, E, nu, order=None):
    """(strain (nq, 6), stress (nq, 6), qf (3 nn)) of one element; tt None: no temperature."""
    nn = NN[etype]
    order = range(nn) if order is None else order
    th = tt is not None
    D = T.elastic_matrix(E, nu)
    pts, w = quad(etype)
    strain, stress = np.zeros((pts.shape[0], 6)), np.zeros((pts.shape[0], 6))

    def eth(lc):
        if not th:
            return np.zeros(6)
        h = shape_func(etype, lc)
        return _epsth(alp, _dot(h, tt, order), _dot(h, t0, order), ref)
    if etype == 361 and elemopt == 1:
        D, K, ipts = _ic_parts(ec, E, nu)
        cd = np.concatenate([ue, -np.linalg.inv(K[24:, 24:]) @ (K[24:, :24] @ ue)])
        qf = K[:24] @ cd
        if th:
            qf = qf - tload(361, 1, ec, tt, t0, ref, alp, E, nu, order)
        for g, (B, wg, lc) in enumerate(ipts):
            strain[g] = B @ cd
            stress[g] = D @ (strain[g] - eth(lc))
        return strain, stress, qf
    qf = np.zeros(3 * nn)
    if etype == 361 and elemopt == 2:
        bbar, _ = _gderiv(361, ec, (0.0, 0.0, 0.0))
    for g in range(pts.shape[0]):
        gd, det = _gderiv(etype, ec, pts[g])
        B = _bbar_matrix(gd, bbar) if etype == 361 and elemopt == 2 else T.b_matrix(gd)
        e = eth(pts[g])
        d = B @ ue - e
        strain[g] = d + e
        stress[g] = D @ d
        qf += (stress[g] @ B) * (w[g] * det)
    return strain, stress, qf


def _mat(E, nu, alpha, em, e):
    m = 0 if em is None else em[e] - 1
    Es, nus = np.atleast_1d(E), np.atleast_1d(nu)
    return Es[m], nus[m], (0.0 if alpha is None else np.atleast_1d(alpha)[m])


def thermal_load(coord, groups, E, nu, thermal, order_of=None):
    """fstr_ass_load's thermal part over ``groups`` = [(etype, conn, elemopt, elem_mat)]: the 3 n_node vector."""
    temp, temp0, ref, alpha = thermal
    f = np.zeros(3 * coord.shape[0])
    for grp in groups:
        etype, conn = grp[0], grp[1]
        elemopt = grp[2] if len(grp) > 2 and grp[2] is not None else 1
        em = grp[3] if len(grp) > 3 else None
        for e in range(conn.shape[0]):
            nodes = conn[e] - 1
            Ee, ne, al = _mat(E, nu, alpha, em, e)
            v = tload(etype, elemopt, coord[nodes], temp[nodes], temp0[nodes], ref, al, Ee, ne, None if order_of is None else order_of(NN[etype]))
            np.add.at(f, (3 * nodes[:, None] + np.arange(3)).ravel(), v)
    return f


def update(coord, groups, E, nu, disp, thermal=None, order_of=None):
    """([strain per group], [stress per group], qforce) of the linear update over the groups, with the thermal branches when
    ``thermal`` is given."""
    temp, temp0, ref, alpha = thermal if thermal is not None else (None, None, 0.0, None)
    u = np.asarray(disp).reshape(-1, 3)
    qf = np.zeros(3 * coord.shape[0])
    strains, stresses = [], []
    for grp in groups:
        etype, conn = grp[0], grp[1]
        elemopt = grp[2] if len(grp) > 2 and grp[2] is not None else 1
        em = grp[3] if len(grp) > 3 else None
        st, ss = np.zeros((conn.shape[0], nq(etype), 6)), np.zeros((conn.shape[0], nq(etype), 6))
        for e in range(conn.shape[0]):
            nodes = conn[e] - 1
            Ee, ne, al = _mat(E, nu, alpha, em, e)
            st[e], ss[e], v = update_element(etype, elemopt, coord[nodes], u[nodes].ravel(), None if temp is None else temp[nodes],
                                             None if temp is None else temp0[nodes], ref, al, Ee, ne,
                                             None if order_of is None else order_of(NN[etype]))
            np.add.at(qf, (3 * nodes[:, None] + np.arange(3)).ravel(), v)
        strains.append(st); stresses.append(ss)
    return strains, stresses, qf


def element_stiffness(etype, elemopt, ec, E, nu):
    """The element matrix the load vector belongs to (STF_C3, STF_C3D8Bbar, STF_C3D8IC condensed)."""
    D = T.elastic_matrix(E, nu)
    if etype == 361 and elemopt == 1:
        _, K, _ = _ic_parts(ec, E, nu)
        return K[:24, :24] - K[:24, 24:] @ np.linalg.inv(K[24:, 24:]) @ K[24:, :24]
    pts, w = quad(etype)
    K = np.zeros((3 * NN[etype], 3 * NN[etype]))
    if etype == 361 and elemopt == 2:
        bbar, _ = _gderiv(361, ec, (0.0, 0.0, 0.0))
    for q in range(pts.shape[0]):
        gd, det = _gderiv(etype, ec, pts[q])
        B = _bbar_matrix(gd, bbar) if etype == 361 and elemopt == 2 else T.b_matrix(gd)
        K += (B.T @ (D @ B)) * (w[q] * det)
    return K


def solve(coord, groups, E, nu, bc, load, thermal=None, load_groups=None):
    """The linear static analysis, dense: K u = load + thermal load with the boundary conditions, then the update.
    load_groups: the groups the thermal load is computed with, where they differ from those of the stiffness and the update --
    fstr_ass_load.f90:380-390 picks TLOAD_C3D8Bbar / TLOAD_C3D8IC by the analysis-wide fstrSOLID%elemopt361, not by the section's
    FORM361, so a deck that selects FI or B-bar per section still gets the IC load vector.
    Returns (u, strains, stresses, qforce, the right-hand side before the boundary conditions)."""
    n = coord.shape[0]
    K = np.zeros((3 * n, 3 * n))
    for grp in groups:
        etype, conn = grp[0], grp[1]
        elemopt = grp[2] if len(grp) > 2 and grp[2] is not None else 1
        em = grp[3] if len(grp) > 3 else None
        for e in range(conn.shape[0]):
            Ee, ne, _ = _mat(E, nu, None, em, e)
            dofs = (3 * (conn[e][:, None] - 1) + np.arange(3)).ravel()
            K[np.ix_(dofs, dofs)] += element_stiffness(etype, elemopt, coord[conn[e] - 1], Ee, ne)
    f = np.zeros(3 * n) if load is None else np.asarray(load, dtype=np.float64).copy()
    if thermal is not None:
        f = f + thermal_load(coord, groups if load_groups is None else load_groups, E, nu, thermal)
    Kb, fb = T.apply_bc(K, f, bc)
    u = np.linalg.solve(Kb, fb)
    st, ss, qf = update(coord, groups, E, nu, u, thermal)
    return u, st, ss, qf, f


# ---- summaries and the reference's own thermal decks --------------------------------------------------------------------
def summary(groups, unode, strains, stresses):
    """The Global summaries of 0.log with the printed digits, for a mesh of any of the six types (c3_nl_ref.summary serves the
    five of STF_C3): nodal values by fstr_NodalStress3D -- 361 through NodalStress_INV3 with the inverse of the 8 shape functions
    at the 8 quadrature points (fstr_NodalStress.f90:75-80, :350-359) --, averaged over the elements that hold the node."""
    import c3_nl_ref as N
    U = np.asarray(unode).reshape(-1, 3)
    n_node = U.shape[0]
    cnt, ns, nt, est, ess = np.zeros(n_node), np.zeros((n_node, 6)), np.zeros((n_node, 6)), [], []
    inv8 = np.linalg.inv(np.array([shape_func(361, p) for p in HEX8_PTS]))
    for grp, st, ss in zip(groups, strains, stresses):
        etype, conn = grp[0], np.asarray(grp[1])
        if etype == 361:
            nde, nds = np.einsum("ij,ejk->eik", inv8, st), np.einsum("ij,ejk->eik", inv8, ss)
            idx = (conn - 1).ravel()
            np.add.at(cnt, idx, 1.0); np.add.at(ns, idx, nde.reshape(-1, 6)); np.add.at(nt, idx, nds.reshape(-1, 6))
        else:       # c3_nl_ref returns the means over the holding elements of this group: weight them back into sums
            a, b, _, _ = N.nodal_and_element_values(etype, conn, n_node, st, ss)
            c = np.zeros(n_node)
            np.add.at(c, (conn - 1).ravel(), 1.0)
            cnt += c; ns += a * c[:, None]; nt += b * c[:, None]
        est.append(st.mean(axis=1)); ess.append(ss.mean(axis=1))
    held = cnt > 0
    ns[held] /= cnt[held, None]; nt[held] /= cnt[held, None]
    est, ess = np.concatenate(est), np.concatenate(ess)
    ext = lambda v: (float("%.4E" % v.max()), float("%.4E" % v.min()))
    node = {"U%d" % (c + 1): ext(U[:, c]) for c in range(3)}
    elem = {}
    for k, c in enumerate(N.COMPONENTS):
        node["E" + c], node["S" + c] = ext(ns[held][:, k]), ext(nt[held][:, k])
        elem["E" + c], elem["S" + c] = ext(est[:, k]), ext(ess[:, k])
    node["SMS"], elem["SMS"] = ext(N.mises(nt[held])), ext(N.mises(ess))
    return {"Node": node, "Element": elem}


# the mesh file lists the mid-edge nodes of 342 as (2,3), (3,1), (1,2), (1,4), (2,4), (3,4) and the triangle mid-edge nodes of 352 as
# (2,3), (3,1), (1,2) and (5,6), (6,4), (4,5): file column -> library column (fistr1 reorders on input)
FILE_TO_LIB = {342: [0, 1, 2, 3, 6, 4, 5, 7, 8, 9], 352: [0, 1, 2, 3, 4, 5, 8, 6, 7, 11, 9, 10, 12, 13, 14]}


def read_msh(path):
    """A HEC-MW mesh file of one solid element type with one material, as the exF decks are: (etype, coord, conn in the library's
    node order, {node group: local ids}, (E, nu, alpha), initial temperature or None).  Nodes that no element names are dropped
    (F341.msh keeps the node list of F342); `ALL` is every remaining node."""
    ids, xyz, conn, groups, items, etype, init = [], [], [], {}, {}, None, None
    sect, name, gen, item = None, None, False, None
    with open(path) as fh:
        for line in fh:
            t = line.strip()
            if not t or t.startswith("!!") or t.startswith("#"):
                continue
            if t.startswith("!"):
                u = t.upper().replace(" ", "")
                key = u.split(",")[0]
                par = dict(kv.split("=", 1) for kv in u.split(",")[1:] if "=" in kv)
                sect = {"!NODE": "node", "!ELEMENT": "elem", "!NGROUP": "ngrp", "!INITIALCONDITION": "init"}.get(key)
                if key == "!ELEMENT":
                    etype = int(par["TYPE"])
                if key == "!NGROUP":
                    name, gen = par["NGRP"], "GENERATE" in u.split(",")
                    groups.setdefault(name, [])
                if key.startswith("!ITEM"):
                    sect, item = "item", int(key.split("=")[1])
                continue
            a = t.replace(",", " ").split()
            if sect == "node":
                ids.append(int(a[0])); xyz.append([float(x) for x in a[1:4]])
            elif sect == "elem":
                conn.append([int(x) for x in a[1:]])
            elif sect == "ngrp":
                groups[name] += list(range(int(a[0]), int(a[1]) + 1, int(a[2]))) if gen else [int(x) for x in a]
            elif sect == "item":
                items[item] = [float(x) for x in a]
            elif sect == "init":
                assert a[0].upper() == "ALL"
                init = float(a[1])
    lid = {g: i for i, g in enumerate(ids)}
    conn = np.array([[lid[g] for g in e] for e in conn])
    used = np.zeros(len(ids), dtype=bool)
    used[conn.ravel()] = True
    new = np.cumsum(used) - 1
    conn = (new[conn] + 1).astype(np.int32)
    if etype in FILE_TO_LIB:
        conn = conn[:, FILE_TO_LIB[etype]]
    out = {k: np.array([new[lid[g]] + 1 for g in v if used[lid[g]]], dtype=np.int32) for k, v in groups.items()}
    out["ALL"] = np.arange(1, int(used.sum()) + 1, dtype=np.int32)
    return etype, np.array(xyz)[used], np.ascontiguousarray(conn), out, (items[1][0], items[1][1], items[3][0]), init
