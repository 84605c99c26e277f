"""fstr_NodalStress3D restated in numpy float64, the whole routine (fistr1/src/analysis/static/fstr_NodalStress.f90:13-272):
NodalStress_INV3 (:337-481) with inverse_func's own Gauss-Jordan (:714-748), NodalStress_C3 / ElementStress_C3
(static_LIB_3d.f90:840-913), get_mises (:483-499), make_principal (:889-980) over get_principal (utilities.f90:362-406) and eigen3
(:107-201) as they are written, with the reference's order of addition: elements in ascending position through the groups, the
nodes of an element in their local order.  The reference of tests/test_gpu_nodal_stress.py; tests/test_nodal_stress_ref.py holds
it against the arrays the reference program itself wrote (tests/golden/nodal_stress.npz).

Products and sums are separate numpy operations (no fused multiply-add), sums run in the reference's order."""
import numpy as np

NN = {341: 4, 342: 10, 351: 6, 352: 15, 361: 8, 362: 20}
NQ = {341: 1, 342: 4, 351: 2, 352: 9, 361: 8, 362: 27}
G2, G3 = 0.577350269189626, 0.774596669241483       # quadrature.f90, as printed there
# 0-based quadrature points NodalStress_INV3 extrapolates from (:84, :95)
SEL = {361: tuple(range(8)), 342: (0, 1, 2, 3), 352: (0, 1, 2, 6, 7, 8), 362: (0, 2, 6, 8, 18, 20, 24, 26)}
# vertex pairs (0-based) of the mid-edge nodes, in node order (:370-387, :402-428, :444-479)
PAIRS = {342: ((0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3)),
         352: ((0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (0, 3), (1, 4), (2, 5)),
         362: ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))}
HEX_SIGNS = ((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1))

PRINC_NSTRESS, PRINCV_NSTRESS, PRINC_NSTRAIN, PRINCV_NSTRAIN = 1, 2, 4, 8
PRINC_ESTRESS, PRINCV_ESTRESS, PRINC_ESTRAIN, PRINCV_ESTRAIN = 16, 32, 64, 128
ALL = 255

# Largest deviation of this restatement from the arrays the reference program wrote, relative to each array's largest magnitude,
# as tests/golden/make_nodal_stress_golden.py printed it for every recorded deck -- values, principal values and separated
# principal vectors alike: 0 (the result files hold 17 significant digits, which round-trip a double, and the operations and
# their order are the reference's).  The project's convention asserts ten times the measured value: ten times zero, equality.
MEASURED = 0.0
BOUND = 10.0 * MEASURED


def quad_point(etype, q):
    """getQuadPoint: natural coordinates of 0-based point q (gauss3d2, gauss3d5, gauss3d8, gauss3d3)"""
    if etype == 361:
        return np.array([G2 if q & 1 else -G2, G2 if q & 2 else -G2, G2 if q & 4 else -G2])
    if etype == 342:
        A, B = 0.138196601125011, 0.585410196624968
        return np.array([B if q == 1 else A, B if q == 2 else A, B if q == 3 else A])
    if etype == 352:
        A, B = 0.166666666666667, 0.666666666666667
        t, h = q % 3, q // 3
        return np.array([B if t == 1 else A, B if t == 2 else A, (-G3, 0.0, G3)[h]])
    if etype == 362:
        v = (-G3, 0.0, G3)
        return np.array([v[q % 3], v[q // 3 % 3], v[q // 9]])
    raise ValueError(etype)


def vertex_shape(etype, lc):
    """getShapeFunc of the vertex element: hex8n (361, 362), tet4n (342), prism6n (352)"""
    xi, et, ze = lc
    if etype in (361, 362):
        return np.array([0.125 * (1.0 + sx * xi) * (1.0 + sy * et) * (1.0 + sz * ze) for sx, sy, sz in HEX_SIGNS])
    if etype == 342:
        return np.array([1.0 - xi - et - ze, xi, et, ze])
    a = 1.0 - xi - et
    return np.array([0.5 * a * (1.0 - ze), 0.5 * xi * (1.0 - ze), 0.5 * et * (1.0 - ze),
                     0.5 * a * (1.0 + ze), 0.5 * xi * (1.0 + ze), 0.5 * et * (1.0 + ze)])


def inverse_func(a):
    """inverse_func (:714-748): Gauss-Jordan without pivoting, divide the row, then eliminate it from every other"""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    inv = np.eye(n)
    for i in range(n):
        buf = 1.0 / a[i, i]
        for j in range(n):
            a[i, j] = a[i, j] * buf
            inv[i, j] = inv[i, j] * buf
        for j in range(n):
            if i != j:
                buf = a[j, i]
                for k in range(n):
                    a[j, k] = a[j, k] - a[i, k] * buf
                    inv[j, k] = inv[j, k] - inv[i, k] * buf
    return inv


_INV = {}


def inverse(etype):
    """inv_func of fstr_NodalStress3D (:68-104) for 361, 342, 352, 362"""
    if etype not in _INV:
        _INV[etype] = inverse_func(np.array([vertex_shape(etype, quad_point(etype, q)) for q in SEL[etype]]))
    return _INV[etype]


def element_values(etype, pts):
    """(element mean (n_elem, 6), nodal values of the element (n_elem, nn, 6)) of one array of point values (n_elem, nq, 6)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, NQ[etype], 6)
    mean = np.zeros((pts.shape[0], 6))
    for q in range(NQ[etype]):
        mean = mean + pts[:, q]
    mean = mean / NQ[etype]
    nn = NN[etype]
    if etype in (341, 351):
        return mean, np.repeat(mean[:, None, :], nn, axis=1)
    inv, sel = inverse(etype), SEL[etype]
    nodal = np.zeros((pts.shape[0], nn, 6))
    for i in range(len(sel)):
        acc = np.zeros((pts.shape[0], 6))
        for j in range(len(sel)):
            acc = acc + inv[i, j] * pts[:, sel[j]]
        nodal[:, i] = acc
    for k, (a, b) in enumerate(PAIRS.get(etype, ())):
        nodal[:, len(sel) + k] = (nodal[:, a] + nodal[:, b]) / 2.0
    return mean, nodal


def get_mises(s):
    s = np.asarray(s, dtype=np.float64)
    ps = (s[..., 0] + s[..., 1] + s[..., 2]) / 3.0
    a, b, c = s[..., 0] - ps, s[..., 1] - ps, s[..., 2] - ps
    sm = 0.5 * (a * a + b * b + c * c) + s[..., 3] * s[..., 3] + s[..., 4] * s[..., 4] + s[..., 5] * s[..., 5]
    return np.sqrt(3.0 * sm)


def eigen3(tensor):
    """eigen3 (utilities.f90:107-201) of tensors (n, 6) in the order 11, 22, 33, 12, 23, 31, every tensor following its own
    branches -> (eigval (n, 3), princ (n, 3, 3) with the vectors as columns, failed (n,): the reference would stop)"""
    t = np.asarray(tensor, dtype=np.float64).reshape(-1, 6)
    n = t.shape[0]
    ev = t[:, :3].copy()
    pr = np.tile(np.eye(3), (n, 1, 1))
    b = {(0, 1): t[:, 3].copy(), (1, 2): t[:, 4].copy(), (0, 2): t[:, 5].copy()}
    key = lambda i, j: (min(i, j), max(i, j))
    active = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(50):
            fsum = np.abs(b[(0, 1)]) + np.abs(b[(0, 2)]) + np.abs(b[(1, 2)])
            active &= ~(fsum < 1.0e-10)
            if not active.any():
                break
            for ip, iq in ((0, 1), (0, 2), (1, 2)):
                bpq = b[(ip, iq)]
                od = 100.0 * np.abs(bpq)
                rot = active & (od + np.abs(ev[:, ip]) != np.abs(ev[:, ip])) & (od + np.abs(ev[:, iq]) != np.abs(ev[:, iq]))
                hd = ev[:, iq] - ev[:, ip]
                small = np.abs(hd) + od == np.abs(hd)
                theta = 0.5 * hd / bpq
                tt = 1.0 / (np.abs(theta) + np.sqrt(1.0 + theta * theta))
                tt = np.where(theta < 0.0, -tt, tt)
                tt = np.where(small, bpq / hd, tt)
                c = 1.0 / np.sqrt(1.0 + tt * tt)
                s = tt * c
                tau = s / (1.0 + c)
                h = tt * bpq
                ev[:, ip] = np.where(rot, ev[:, ip] - h, ev[:, ip])
                ev[:, iq] = np.where(rot, ev[:, iq] + h, ev[:, iq])
                ir = 3 - ip - iq
                g, h = b[key(ir, ip)].copy(), b[key(ir, iq)].copy()
                b[key(ir, ip)] = np.where(rot, g - s * (h + g * tau), g)
                b[key(ir, iq)] = np.where(rot, h + s * (g - h * tau), h)
                for r in range(3):
                    g, h = pr[:, r, ip].copy(), pr[:, r, iq].copy()
                    pr[:, r, ip] = np.where(rot, g - s * (h + g * tau), g)
                    pr[:, r, iq] = np.where(rot, h + s * (g - h * tau), h)
                b[(ip, iq)] = np.where(active, 0.0, bpq)
    return ev, pr, active       # still active after 50 sweeps: the reference's `stop`


def get_principal(tensor):
    """get_principal (utilities.f90:362-406) of tensors (n, 6) -> (values (n, 3) descending, princmatrix (n, 3, 3) as
    [item, vector j, component i] = princnormal(i, j) * eigval(j), failed (n,))"""
    ev, pr, failed = eigen3(tensor)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        sw = ev[:, a] < ev[:, b]
        ev[sw, a], ev[sw, b] = ev[sw, b].copy(), ev[sw, a].copy()
        ca, cb = pr[sw, :, a].copy(), pr[sw, :, b].copy()
        pr[sw, :, a], pr[sw, :, b] = cb, ca
    mat = pr * ev[:, None, :]                   # (n, i, j)
    return ev, np.ascontiguousarray(mat.transpose(0, 2, 1)), failed


class Result:
    pass


def nodal_stress(n_node, groups, strain, stress, principal=0):
    """groups: [(etype, conn (n_elem, nn) 1-based, ...)]; strain, stress: per-group lists of (n_elem, nq, 6), or one flat array,
    the groups one after the other.  -> Result with strain, stress, mises, estrain, estress, emises, count (elements per node,
    a node named twice by one element counted twice) and the eight principal arrays (None where the flag is off)."""
    def split(v):
        if isinstance(v, (list, tuple)):
            return [np.asarray(a, dtype=np.float64) for a in v]
        v, out, at = np.asarray(v, dtype=np.float64).ravel(), [], 0
        for g in groups:
            n = np.asarray(g[1]).shape[0] * NQ[g[0]] * 6
            out.append(v[at:at + n])
            at += n
        return out
    r = Result()
    ns, nt, cnt = np.zeros((n_node, 6)), np.zeros((n_node, 6)), np.zeros(n_node, dtype=np.int64)
    est, ess = [], []
    for g, st, ss in zip(groups, split(strain), split(stress)):
        etype, conn = int(g[0]), np.asarray(g[1])
        idx = (conn.reshape(-1, NN[etype]) - 1).ravel()
        if idx.size and (idx.min() < 0 or idx.max() >= n_node):
            raise ValueError("node id out of range")
        m, nd = element_values(etype, st)
        est.append(m)
        np.add.at(ns, idx, nd.reshape(-1, 6))       # unbuffered, in the order given: element by element, local node by node
        m, nd = element_values(etype, ss)
        ess.append(m)
        np.add.at(nt, idx, nd.reshape(-1, 6))
        np.add.at(cnt, idx, 1)
    held = cnt > 0
    ns[held] = ns[held] / cnt[held, None].astype(np.float64)
    nt[held] = nt[held] / cnt[held, None].astype(np.float64)
    r.strain, r.stress, r.count = ns, nt, cnt
    r.estrain, r.estress = np.concatenate(est), np.concatenate(ess)
    r.mises, r.emises = get_mises(nt), get_mises(r.estress)
    r.failed = False
    for vals, vecs, src, bv, bw in (("pstress", "pstress_vect", nt, 1, 2), ("pstrain", "pstrain_vect", ns, 4, 8),
                                    ("epstress", "epstress_vect", r.estress, 16, 32), ("epstrain", "epstrain_vect", r.estrain, 64, 128)):
        setattr(r, vals, None)
        setattr(r, vecs, None)
        if principal & (bv | bw):
            ev, mat, failed = get_principal(src)
            r.failed |= bool(failed.any())
            if principal & bv:
                setattr(r, vals, ev)
            if principal & bw:
                setattr(r, vecs, mat)
    return r


COMPONENTS = ("11", "22", "33", "12", "23", "31")


def summary(r, unode=None):
    """the Global Summary dictionary (oracle/fistr1_run.read_log's shape) with the five printed digits"""
    ext = lambda v: (float("%.4E" % v.max()), float("%.4E" % v.min()))
    node, elem = {}, {}
    if unode is not None:
        U = np.asarray(unode).reshape(-1, 3)
        node.update({"U%d" % (c + 1): ext(U[:, c]) for c in range(3)})
    for k, c in enumerate(COMPONENTS):
        node["E" + c], node["S" + c] = ext(r.strain[:, k]), ext(r.stress[:, k])
        elem["E" + c], elem["S" + c] = ext(r.estrain[:, k]), ext(r.estress[:, k])
    node["SMS"], elem["SMS"] = ext(r.mises), ext(r.emises)
    return {"Node": node, "Element": elem}
