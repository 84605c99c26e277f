"""DL_C3 (fistr1/src/lib/static_LIB_3d.f90:210-377) restated in numpy for TYPE=341, 342, 351, 352, 361, 362, with what it calls:
getSubFace (element.f90:181-315), the face rules gauss2d4 / gauss2d5 / gauss2d2 / gauss2d3 and the volume rules gauss3d4 /
gauss3d5 / gauss3d7 / gauss3d8 / gauss3d2 / gauss3d3 with their weights as quadrature.f90 prints them, the shape functions and
derivatives of the element files, and SurfaceNormal (element.f90:822-854).  The sums run in the reference's order; the products
keep its association.  ``assemble`` is the DLOAD block of fstr_ass_load (fstr_ass_load.f90:138-257) over a list of entries."""
import numpy as np

NODES = {341: 4, 342: 10, 351: 6, 352: 15, 361: 8, 362: 20}
SUBFACE = {
    341: ((1, 2, 3), (4, 2, 1), (4, 3, 2), (4, 1, 3)),
    342: ((1, 2, 3, 5, 6, 7), (4, 2, 1, 9, 5, 8), (4, 3, 2, 10, 6, 9), (4, 1, 3, 8, 7, 10)),
    351: ((1, 2, 3), (6, 5, 4), (4, 5, 2, 1), (5, 6, 3, 2), (6, 4, 1, 3)),
    352: ((1, 2, 3, 7, 8, 9), (6, 5, 4, 11, 10, 12), (4, 5, 2, 1, 10, 14, 7, 13), (5, 6, 3, 2, 11, 15, 8, 14),
          (6, 4, 1, 3, 12, 13, 9, 15)),
    361: ((1, 2, 3, 4), (8, 7, 6, 5), (5, 6, 2, 1), (6, 7, 3, 2), (7, 8, 4, 3), (8, 5, 1, 4)),
    362: ((1, 2, 3, 4, 9, 10, 11, 12), (8, 7, 6, 5, 15, 14, 13, 16), (5, 6, 2, 1, 13, 18, 9, 17), (6, 7, 3, 2, 14, 19, 10, 18),
          (7, 8, 4, 3, 15, 20, 11, 19), (8, 5, 1, 4, 16, 17, 12, 20)),
}
G2, G3 = 0.577350269189626, 0.774596669241483


def get_sub_face(etype, face):
    """-> 1-based positions of the face's nodes in the element (getSubFace's `nodes`)"""
    return SUBFACE[etype][face - 1]


# ---- faces: rule, shape functions, derivatives by number of nodes
def face_rule(mm):
    if mm == 3:
        return [((0.333333333333333, 0.333333333333333), 0.5)]
    if mm == 6:
        A, B, w = 0.166666666666667, 0.666666666666667, 0.166666666666666
        return [((A, A), w), ((B, A), w), ((A, B), w)]
    if mm == 4:
        return [((r, s), 1.0) for s in (-G2, G2) for r in (-G2, G2)]
    w1 = (0.308641975308642, 0.493827160493827, 0.790123456790123)
    pts = (-G3, 0.0, G3)
    return [((pts[i], pts[j]), w1[(i == 1) + (j == 1)]) for j in range(3) for i in range(3)]


def face_func(mm, r, s):
    if mm == 3:
        return np.array([r, s, 1.0 - r - s])
    if mm == 6:
        st = 1.0 - r - s
        return np.array([st * (2.0 * st - 1.0), r * (2.0 * r - 1.0), s * (2.0 * s - 1.0), 4.0 * r * st, 4.0 * r * s, 4.0 * s * st])
    if mm == 4:
        return np.array([0.25 * (1.0 - r) * (1.0 - s), 0.25 * (1.0 + r) * (1.0 - s), 0.25 * (1.0 + r) * (1.0 + s),
                         0.25 * (1.0 - r) * (1.0 + s)])
    RP, SP, RM, SM = 1.0 + r, 1.0 + s, 1.0 - r, 1.0 - s
    return np.array([0.25 * RM * SM * (-1.0 - r - s), 0.25 * RP * SM * (-1.0 + r - s), 0.25 * RP * SP * (-1.0 + r + s),
                     0.25 * RM * SP * (-1.0 - r + s), 0.5 * (1.0 - r * r) * (1.0 - s), 0.5 * (1.0 - s * s) * (1.0 + r),
                     0.5 * (1.0 - r * r) * (1.0 + s), 0.5 * (1.0 - s * s) * (1.0 - r)])


def face_deriv(mm, r, s):
    """-> (mm, 2)"""
    if mm == 3:
        return np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, -1.0]])
    if mm == 6:
        st = 1.0 - r - s
        return np.array([[1.0 - 4.0 * st, 1.0 - 4.0 * st], [4.0 * r - 1.0, 0.0], [0.0, 4.0 * s - 1.0], [4.0 * (st - r), -4.0 * r],
                         [4.0 * s, 4.0 * r], [-4.0 * s, 4.0 * (st - s)]])
    if mm == 4:
        return np.array([[-0.25 * (1.0 - s), -0.25 * (1.0 - r)], [0.25 * (1.0 - s), -0.25 * (1.0 + r)],
                         [0.25 * (1.0 + s), 0.25 * (1.0 + r)], [-0.25 * (1.0 + s), 0.25 * (1.0 - r)]])
    return np.array([[.25 * (1.0 - s) * (2.0 * r + s), .25 * (1.0 - r) * (r + 2.0 * s)],
                     [.25 * (1.0 - s) * (2.0 * r - s), -.25 * (1.0 + r) * (r - 2.0 * s)],
                     [.25 * (1.0 + s) * (2.0 * r + s), .25 * (1.0 + r) * (r + 2.0 * s)],
                     [.25 * (1.0 + s) * (2.0 * r - s), -.25 * (1.0 - r) * (r - 2.0 * s)],
                     [-r * (1.0 - s), -0.5 * (1.0 - r * r)], [0.5 * (1.0 - s * s), -s * (1.0 + r)],
                     [-r * (1.0 + s), 0.5 * (1.0 - r * r)], [-0.5 * (1.0 - s * s), -s * (1.0 - r)]])


def _matmul(a, b):
    """Fortran's matmul as gfortran inlines it: the sum over the inner index in ascending order"""
    out = np.zeros((a.shape[0], b.shape[1]))
    for k in range(a.shape[1]):
        out = out + np.outer(a[:, k], b[k, :])
    return out


def surface_normal(mm, r, s, elecoord):
    """elecoord (3, mm) -> the un-normalised normal"""
    g = _matmul(elecoord, face_deriv(mm, r, s))
    return np.array([g[1, 0] * g[2, 1] - g[2, 0] * g[1, 1], g[2, 0] * g[0, 1] - g[0, 0] * g[2, 1], g[0, 0] * g[1, 1] - g[1, 0] * g[0, 1]])


# ---- volumes
def volume_rule(etype):
    if etype == 341:
        return [((0.25, 0.25, 0.25), 0.166666666666667)]
    if etype == 342:
        A, B, w = 0.138196601125011, 0.585410196624968, 0.041666666666667
        return [((A, A, A), w), ((B, A, A), w), ((A, B, A), w), ((A, A, B), w)]
    if etype == 351:
        t = 0.333333333333333
        return [((t, t, -G2), 0.5), ((t, t, G2), 0.5)]
    if etype == 352:
        A, B = 0.166666666666667, 0.666666666666667
        tri = ((A, A), (B, A), (A, B))
        return [((x, y, z), w) for z, w in ((-G3, 0.092592592592593), (0.0, 0.148148148148148), (G3, 0.092592592592593)) for x, y in tri]
    if etype == 361:
        return [((x, y, z), 1.0) for z in (-G2, G2) for y in (-G2, G2) for x in (-G2, G2)]
    w3 = (0.171467764060357, 0.274348422496571, 0.438957475994513, 0.702331961591221)
    p = (-G3, 0.0, G3)
    return [((p[i], p[j], p[k]), w3[(i == 1) + (j == 1) + (k == 1)]) for k in range(3) for j in range(3) for i in range(3)]


_HEX_S = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=np.float64)


def shape_func(etype, xi, et, ze):
    if etype == 341:
        return np.array([1.0 - xi - et - ze, xi, et, ze])
    if etype == 342:
        a = 1.0 - xi - et - ze
        return np.array([(2.0 * a - 1.0) * a, xi * (2.0 * xi - 1.0), et * (2.0 * et - 1.0), ze * (2.0 * ze - 1.0), 4.0 * xi * a,
                         4.0 * xi * et, 4.0 * et * a, 4.0 * ze * a, 4.0 * xi * ze, 4.0 * et * ze])
    if etype == 351:
        a = 1.0 - xi - et
        return np.array([0.5 * a * (1.0 - ze), 0.5 * xi * (1.0 - ze), 0.5 * et * (1.0 - ze), 0.5 * a * (1.0 + ze), 0.5 * xi * (1.0 + ze),
                         0.5 * et * (1.0 + ze)])
    if etype == 352:
        a = 1.0 - xi - et
        return np.array([0.5 * a * (1.0 - ze) * (2.0 * a - 2.0 - ze), 0.5 * xi * (1.0 - ze) * (2.0 * xi - 2.0 - ze),
                         0.5 * et * (1.0 - ze) * (2.0 * et - 2.0 - ze), 0.5 * a * (1.0 + ze) * (2.0 * a - 2.0 + ze),
                         0.5 * xi * (1.0 + ze) * (2.0 * xi - 2.0 + ze), 0.5 * et * (1.0 + ze) * (2.0 * et - 2.0 + ze),
                         2.0 * xi * a * (1.0 - ze), 2.0 * xi * et * (1.0 - ze), 2.0 * et * a * (1.0 - ze),
                         2.0 * xi * a * (1.0 + ze), 2.0 * xi * et * (1.0 + ze), 2.0 * et * a * (1.0 + ze),
                         a * (1.0 - ze * ze), xi * (1.0 - ze * ze), et * (1.0 - ze * ze)])
    if etype == 361:
        return np.array([0.125 * (1.0 + s[0] * xi) * (1.0 + s[1] * et) * (1.0 + s[2] * ze) for s in _HEX_S])
    f = np.zeros(20)
    for n, s in enumerate(_HEX_S):
        f[n] = -0.125 * (1.0 + s[0] * xi) * (1.0 + s[1] * et) * (1.0 + s[2] * ze) * (2.0 - s[0] * xi - s[1] * et - s[2] * ze)
    for c, (sy, sz) in enumerate(((-1, -1), (1, -1))):      # 9, 11 along xi at the bottom; 13, 15 at the top
        for top in (0, 1):
            f[8 + 2 * c + 4 * top] = 0.25 * (1.0 - xi * xi) * (1.0 + sy * et) * (1.0 + (1 if top else -1) * ze)
    for c, sx in ((1, 1), (3, -1)):                         # 10, 12 along eta; 14, 16
        for top in (0, 1):
            f[8 + c + 4 * top] = 0.25 * (1.0 + sx * xi) * (1.0 - et * et) * (1.0 + (1 if top else -1) * ze)
    for c in range(4):
        f[16 + c] = 0.25 * (1.0 + _HEX_S[c, 0] * xi) * (1.0 + _HEX_S[c, 1] * et) * (1.0 - ze * ze)
    return f


def shape_deriv(etype, xi, et, ze):
    """-> (nn, 3): the element files' ShapeDeriv_*"""
    if etype == 341:
        return np.array([[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    if etype == 342:
        a = 1.0 - xi - et - ze
        return np.array([[1.0 - 4.0 * a] * 3, [4.0 * xi - 1.0, 0.0, 0.0], [0.0, 4.0 * et - 1.0, 0.0], [0.0, 0.0, 4.0 * ze - 1.0],
                         [4.0 * (1.0 - 2.0 * xi - et - ze), -4.0 * xi, -4.0 * xi], [4.0 * et, 4.0 * xi, 0.0],
                         [-4.0 * et, 4.0 * (1.0 - xi - 2.0 * et - ze), -4.0 * et], [-4.0 * ze, -4.0 * ze, 4.0 * (1.0 - xi - et - 2.0 * ze)],
                         [4.0 * ze, 0.0, 4.0 * xi], [0.0, 4.0 * ze, 4.0 * et]])
    if etype == 351:
        a = 1.0 - xi - et
        m, p = 0.5 * (1.0 - ze), 0.5 * (1.0 + ze)
        return np.array([[-m, -m, -0.5 * a], [m, 0.0, -0.5 * xi], [0.0, m, -0.5 * et], [-p, -p, 0.5 * a], [p, 0.0, 0.5 * xi],
                         [0.0, p, 0.5 * et]])
    if etype == 352:
        a = 1.0 - xi - et
        zm, zp, zz = 1.0 - ze, 1.0 + ze, 1.0 - ze * ze
        d0 = -0.5 * zm * (4.0 * a - ze - 2.0)
        d3 = -0.5 * zp * (4.0 * a + ze - 2.0)
        return np.array([[d0, d0, a * (xi + et + ze - 0.5)], [0.5 * zm * (4.0 * xi - ze - 2.0), 0.0, xi * (-xi + ze + 0.5)],
                         [0.0, 0.5 * zm * (4.0 * et - ze - 2.0), et * (-et + ze + 0.5)], [d3, d3, a * (-xi - et + ze + 0.5)],
                         [0.5 * zp * (4.0 * xi + ze - 2.0), 0.0, xi * (xi + ze - 0.5)],
                         [0.0, 0.5 * zp * (4.0 * et + ze - 2.0), et * (et + ze - 0.5)],
                         [2.0 * zm * (1.0 - 2.0 * xi - et), -2.0 * xi * zm, -2.0 * xi * a], [2.0 * et * zm, 2.0 * xi * zm, -2.0 * xi * et],
                         [-2.0 * et * zm, 2.0 * zm * (1.0 - xi - 2.0 * et), -2.0 * et * a],
                         [2.0 * zp * (1.0 - 2.0 * xi - et), -2.0 * xi * zp, 2.0 * xi * a], [2.0 * et * zp, 2.0 * xi * zp, 2.0 * xi * et],
                         [-2.0 * et * zp, 2.0 * zp * (1.0 - xi - 2.0 * et), 2.0 * et * a],
                         [-zz, -zz, -2.0 * a * ze], [zz, 0.0, -2.0 * xi * ze], [0.0, zz, -2.0 * et * ze]])
    if etype == 361:
        d = np.zeros((8, 3))
        for n, s in enumerate(_HEX_S):
            fx, fy, fz = 1.0 + s[0] * xi, 1.0 + s[1] * et, 1.0 + s[2] * ze
            d[n] = (s[0] * 0.125 * fy * fz, s[1] * 0.125 * fx * fz, s[2] * 0.125 * fx * fy)
        return d
    # ShapeDeriv_hex20n (hex20n.f90), the vertices by their signs, the mid-edge nodes as written
    RI, SI, TI = xi, et, ze
    RP, SP, TP, RM, SM, TM = 1.0 + RI, 1.0 + SI, 1.0 + TI, 1.0 - RI, 1.0 - SI, 1.0 - TI
    d = np.zeros((20, 3))
    for n, s in enumerate(_HEX_S):
        Xf, Yf, Zf = 1.0 + s[0] * RI, 1.0 + s[1] * SI, 1.0 + s[2] * TI
        Pf = 2.0 - s[0] * RI - s[1] * SI - s[2] * TI
        d[n] = (s[0] * (0.125 * Xf * Yf * Zf) - s[0] * (0.125 * Yf * Zf * Pf), s[1] * (0.125 * Xf * Yf * Zf) - s[1] * (0.125 * Xf * Zf * Pf),
                s[2] * (0.125 * Xf * Yf * Zf) - s[2] * (0.125 * Xf * Yf * Pf))
    d[8:] = [[-0.50 * RI * SM * TM, -0.25 * (1.0 - RI ** 2) * TM, -0.25 * (1.0 - RI ** 2) * SM],
             [+0.25 * (1.0 - SI ** 2) * TM, -0.50 * RP * SI * TM, -0.25 * RP * (1.0 - SI ** 2)],
             [-0.50 * RI * SP * TM, +0.25 * (1.0 - RI ** 2) * TM, -0.25 * (1.0 - RI ** 2) * SP],
             [-0.25 * (1.0 - SI ** 2) * TM, -0.50 * RM * SI * TM, -0.25 * RM * (1.0 - SI ** 2)],
             [-0.50 * RI * SM * TP, -0.25 * (1.0 - RI ** 2) * TP, 0.25 * (1.0 - RI ** 2) * SM],
             [+0.25 * (1.0 - SI ** 2) * TP, -0.50 * RP * SI * TP, 0.25 * RP * (1.0 - SI ** 2)],
             [-0.50 * RI * SP * TP, +0.25 * (1.0 - RI ** 2) * TP, 0.25 * (1.0 - RI ** 2) * SP],
             [-0.25 * (1.0 - SI ** 2) * TP, -0.50 * RM * SI * TP, 0.25 * RM * (1.0 - SI ** 2)],
             [-0.25 * SM * (1.0 - TI ** 2), -0.25 * RM * (1.0 - TI ** 2), -0.5 * RM * SM * TI],
             [+0.25 * SM * (1.0 - TI ** 2), -0.25 * RP * (1.0 - TI ** 2), -0.5 * RP * SM * TI],
             [+0.25 * SP * (1.0 - TI ** 2), +0.25 * RP * (1.0 - TI ** 2), -0.5 * RP * SP * TI],
             [-0.25 * SP * (1.0 - TI ** 2), +0.25 * RM * (1.0 - TI ** 2), -0.5 * RM * SP * TI]]
    return d


def dl_c3(etype, ecoord, rho, ltype, params):
    """DL_C3: ecoord (nn, 3), PARAMS(0:6) -> VECT (3 nn)"""
    nn = NODES[etype]
    X = np.asarray(ecoord, dtype=np.float64).reshape(nn, 3)
    P = np.asarray(params, dtype=np.float64)
    val = P[0]
    vect = np.zeros(3 * nn)
    if ltype >= 10:
        nod = np.array(get_sub_face(etype, ltype // 10)) - 1
        mm = len(nod)
        ele = X[nod].T.copy()
        for (r, s), WG in face_rule(mm):
            H = face_func(mm, r, s)
            normal = surface_normal(mm, r, s, ele)
            for i in range(mm):
                for k in range(3):
                    vect[3 * nod[i] + k] = vect[3 * nod[i] + k] + val * WG * H[i] * normal[k]
        return vect
    PL = np.zeros((nn, 3))
    for (xi, et, ze), w in volume_rule(etype):
        H = shape_func(etype, xi, et, ze)
        XJ = _matmul(X.T, shape_deriv(etype, xi, et, ze))
        DET = (XJ[0, 0] * XJ[1, 1] * XJ[2, 2] + XJ[1, 0] * XJ[2, 1] * XJ[0, 2] + XJ[2, 0] * XJ[0, 1] * XJ[1, 2]
               - XJ[2, 0] * XJ[1, 1] * XJ[0, 2] - XJ[1, 0] * XJ[0, 1] * XJ[2, 2] - XJ[0, 0] * XJ[2, 1] * XJ[1, 2])
        coef = np.array([1.0, 1.0, 1.0])
        if ltype == 5:
            A, R = P[1:4], P[4:7]
            cod = np.zeros(3)
            for n in range(nn):
                cod = cod + H[n] * X[n]
            t = ((cod[0] - A[0]) * R[0] + (cod[1] - A[1]) * R[1] + (cod[2] - A[2]) * R[2]) / (R[0] ** 2 + R[1] ** 2 + R[2] ** 2)
            foot = A + t * R
            coef = rho * val * val * (cod - foot)
        WG = w * DET
        for k in range(3):
            PL[:, k] = PL[:, k] + H * WG * coef[k]
    if ltype in (1, 2, 3):
        vect[ltype - 1::3] = val * PL[:, ltype - 1]
    elif ltype == 4:
        ln = np.sqrt(P[1] ** 2 + P[2] ** 2 + P[3] ** 2)
        for k in range(3):
            vect[k::3] = val * PL[:, k] * rho * (P[1 + k] / ln)
    elif ltype == 5:
        vect[:] = PL.ravel()
    else:
        raise ValueError("LTYPE %d" % ltype)
    return vect


def assemble(coord, groups, rho, dload, factor=1.0, disp=None, elem_mat=None):
    """The DLOAD block of fstr_ass_load: sum of factor * VECT (1 * VECT for a held entry) over the entries, entry after entry.
    groups [(etype, conn, ...)]; dload = (group, elem, ltype, params (n, 7), held or None); rho a scalar or one per material
    (picked by the group's elem_mat, groups[g][3], 1-based)."""
    X = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
    if disp is not None:
        X = X + np.asarray(disp, dtype=np.float64).reshape(-1, 3)
    rho = np.atleast_1d(np.asarray(0.0 if rho is None else rho, dtype=np.float64))
    grp, elem, ltype, params = dload[:4]
    held = dload[4] if len(dload) > 4 and dload[4] is not None else np.zeros(len(grp), dtype=np.uint8)
    params = np.asarray(params, dtype=np.float64).reshape(-1, 7)
    GL = np.zeros(X.size)
    for k in range(len(grp)):
        G = groups[int(grp[k])]
        etype = int(G[0])
        nod = np.asarray(G[1]).reshape(-1, NODES[etype])[int(elem[k])] - 1
        em = G[3] if len(G) > 3 and G[3] is not None else None
        r = rho[int(em[int(elem[k])]) - 1] if em is not None and rho.size > 1 else rho[0]
        v = dl_c3(etype, X[nod], r, int(ltype[k]), params[k])
        f = 1.0 if held[k] else factor
        idx = (3 * nod[:, None] + np.arange(3)).ravel()
        np.add.at(GL, idx, f * v)
    return GL


def boundary_faces(groups):
    """(group, element, face) -- 0-based, 0-based, 1-based -- of every face that only one element of the mesh holds"""
    seen = {}
    for g, G in enumerate(groups):
        etype = int(G[0])
        conn = np.asarray(G[1]).reshape(-1, NODES[etype])
        for f, nod in enumerate(SUBFACE[etype]):
            nv = 3 if len(nod) in (3, 6) else 4
            for e, key in enumerate(map(tuple, np.sort(conn[:, np.array(nod[:nv]) - 1], axis=1))):
                seen.setdefault(key, []).append((g, e, f + 1))
    return sorted(v[0] for v in seen.values() if len(v) == 1)


def entries(*cards):
    """cards of (group, elems, ltype, params[, held]) -> the dload tuple of ``assemble``"""
    g, e, lt, par, held = [], [], [], [], []
    for c in cards:
        for el in np.atleast_1d(c[1]):
            g.append(int(c[0])); e.append(int(el)); lt.append(int(c[2])); par.append(list(c[3]) + [0.0] * (7 - len(c[3])))
            held.append(1 if len(c) > 4 and c[4] else 0)
    return (np.array(g, dtype=np.int32), np.array(e, dtype=np.int32), np.array(lt, dtype=np.int32),
            np.array(par, dtype=np.float64).reshape(-1, 7), np.array(held, dtype=np.uint8))
