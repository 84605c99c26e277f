"""A numpy restatement of the reference's surface terms of a heat analysis, on top of heat_ref.py, for the tests of
frontistr_amd/csrc/fx_heat_bc.h and frontistr_amd/heat.py (TYPE=341, 342, 351, 352, 361, 362).

    heat_FILM_3xx                                      fistr1/src/lib/heat_LIB_FILM.f90
    heat_RADIATE_3xx                                   fistr1/src/lib/heat_LIB_RADIATE.f90
    heat_DFLUX_3xx, faces S1.. and the body flux BF    fistr1/src/lib/heat_LIB_DFLUX.f90
    heat_mat_ass_bc_DFLUX, _FILM, _RADIATE             the list loops, entry after entry (without the weld line)
    heat_init_amplitude, heat_get_amplitude            heat_init.f90:30-86, heat_get_amplitude.f90
    heat_solve_SS, heat_solve_TRAN                     heat_ref's loops with heat_mat_ass_boundary complete

The routines share four face shapes: the 3-node triangle (a closed form), the 6-node triangle (3 x 3 collapsed points, the
normal divided by its length and a determinant taken of the result), the 4-node quadrilateral (2 x 2 points) and the 8-node
quadrilateral (3 x 3 points); heat_DFLUX_352 alone integrates its triangles with a 6-node set collapsed from the 8-node
quadrilateral.  They differ in the order of their products, which is kept routine by routine, and every literal without `d0`
(all Gauss constants of these three files) is the nearest float32, as in heat_ref (SINGLE).  Faces are vectorised over the first
axis; nothing else is reordered."""
import numpy as np

import heat_ref as R

NOD = {
    341: {1: [1, 2, 3], 2: [4, 2, 1], 3: [4, 3, 2], 4: [4, 1, 3]},
    342: {1: [1, 2, 3, 5, 6, 7], 2: [4, 2, 1, 9, 5, 8], 3: [4, 3, 2, 10, 6, 9], 4: [4, 1, 3, 8, 7, 10]},
    351: {1: [1, 2, 3], 2: [6, 5, 4], 3: [4, 5, 2, 1], 4: [5, 6, 3, 2], 5: [6, 4, 1, 3]},
    352: {1: [1, 2, 3, 7, 8, 9], 2: [6, 5, 4, 11, 10, 12], 3: [4, 5, 2, 1, 10, 14, 7, 13], 4: [5, 6, 3, 2, 11, 15, 8, 14],
          5: [6, 4, 1, 3, 12, 13, 9, 15]},
    361: {1: [1, 2, 3, 4], 2: [8, 7, 6, 5], 3: [5, 6, 2, 1], 4: [6, 7, 3, 2], 5: [7, 8, 4, 3], 6: [8, 5, 1, 4]},
    362: {1: [1, 2, 3, 4, 9, 10, 11, 12], 2: [8, 7, 6, 5, 15, 14, 13, 16], 3: [5, 6, 2, 1, 13, 18, 9, 17],
          4: [6, 7, 3, 2, 14, 19, 10, 18], 5: [7, 8, 4, 3, 15, 20, 11, 19], 6: [8, 5, 1, 4, 16, 17, 12, 20]},
}
NFACE = {et: len(f) for et, f in NOD.items()}


def face_nodes(etype, face):
    """NOD of the routines, 0-based positions in the element"""
    return np.array(NOD[etype][face]) - 1


# ---- the face point sets ------------------------------------------------------------------------------------------------------------
def _q4():
    g = R._r(0.5773502691896)                  # `data XG/-0.5773502691896, 0.5773502691896/`: default-real literals
    XG, WGT = (-g, g), (1.0, 1.0)
    pts = []
    for IG2 in range(2):
        SI = XG[IG2]
        for IG1 in range(2):
            RI = XG[IG1]
            H = [0.25 * (1.0 - RI) * (1.0 - SI), 0.25 * (1.0 + RI) * (1.0 - SI), 0.25 * (1.0 + RI) * (1.0 + SI), 0.25 * (1.0 - RI) * (1.0 + SI)]
            HR = [-.25 * (1.0 - SI), .25 * (1.0 - SI), .25 * (1.0 + SI), -.25 * (1.0 + SI)]
            HS = [-.25 * (1.0 - RI), -.25 * (1.0 + RI), .25 * (1.0 + RI), .25 * (1.0 - RI)]
            pts.append((H, HR, HS, WGT[IG1], WGT[IG2], 1.0))
    return pts


def _q8(collapsed=False):
    XG, WGT = R._gauss3()
    pts = []
    for IG2 in range(3):
        SI = XG[IG2]
        for IG1 in range(3):
            RI = XG[IG1]
            RP, SP, RM, SM = 1.0 + RI, 1.0 + SI, 1.0 - RI, 1.0 - SI
            if not collapsed:
                H = [0.25 * RM * SM * (-1.0 - RI - SI), 0.25 * RP * SM * (-1.0 + RI - SI), 0.25 * RP * SP * (-1.0 + RI + SI),
                     0.25 * RM * SP * (-1.0 - RI + SI), 0.5 * (1.0 - RI * RI) * (1.0 - SI), 0.5 * (1.0 - SI * SI) * (1.0 + RI),
                     0.5 * (1.0 - RI * RI) * (1.0 + SI), 0.5 * (1.0 - SI * SI) * (1.0 - RI)]
                HR = [-.25 * SM * (-1.0 - RI - SI) - 0.25 * RM * SM, .25 * SM * (-1.0 + RI - SI) + 0.25 * RP * SM,
                      .25 * SP * (-1.0 + RI + SI) + 0.25 * RP * SP, -.25 * SP * (-1.0 - RI + SI) - 0.25 * RM * SP,
                      -RI * (1.0 - SI), .5 * (1.0 - SI * SI), -RI * (1.0 + SI), -.5 * (1.0 - SI * SI)]
                HS = [-.25 * RM * (-1.0 - RI - SI) - 0.25 * RM * SM, -.25 * RP * (-1.0 + RI - SI) - 0.25 * RP * SM,
                      .25 * RP * (-1.0 + RI + SI) + 0.25 * RP * SP, .25 * RM * (-1.0 - RI + SI) + 0.25 * RM * SP,
                      -.5 * (1.0 - RI * RI), -SI * (1.0 + RI), .5 * (1.0 - RI * RI), -SI * (1.0 - RI)]
            else:                               # heat_DFLUX_352, ISUF = 2 (heat_LIB_DFLUX.f90:1296-1351)
                H = [0.25 * RM * SM * (-1.0 - RI - SI), 0.25 * RP * SM * (-1.0 + RI - SI), 0.5 * SP * SI,
                     0.5 * (1.0 - RI * RI) * (1.0 - SI), 0.5 * (1.0 - SI * SI) * (1.0 + RI), 0.5 * (1.0 - SI * SI) * (1.0 - RI)]
                HR = [-.25 * SM * (-1.0 - RI - SI) - 0.25 * RM * SM, .25 * SM * (-1.0 + RI - SI) + 0.25 * RP * SM, 0.0,
                      -RI * (1.0 - SI), 0.5 * (1.0 - SI * SI), -0.5 * (1.0 - SI * SI)]
                HS = [-.25 * RM * (-1.0 - RI - SI) - 0.25 * RM * SM, -.25 * RP * (-1.0 + RI - SI) - 0.25 * RP * SM,
                      0.5 * (1.0 + 2.0 * SI), -0.5 * (1.0 - RI * RI), -SI * (1.0 + RI), -SI * (1.0 - RI)]
            pts.append((H, HR, HS, WGT[IG1], WGT[IG2], 1.0))
    return pts


def _t6():
    XG, WGT = R._gauss3()
    pts = []
    for L2 in range(3):
        XL2 = XG[L2]
        X2 = (XL2 + 1.0) * 0.5
        for L1 in range(3):
            XL1 = XG[L1]
            X1 = 0.5 * (1.0 - X2) * (XL1 + 1.0)
            X3 = 1.0 - X1 - X2
            H = [X1 * (2.0 * X1 - 1.), X2 * (2.0 * X2 - 1.), X3 * (2.0 * X3 - 1.), 4.0 * X1 * X2, 4.0 * X2 * X3, 4.0 * X1 * X3]
            HL1 = [4.0 * X1 - 1.0, 0.0, 0.0, 4.0 * X2, 0.0, 4.0 * X3]
            HL2 = [0.0, 4.0 * X2 - 1.0, 0.0, 4.0 * X1, 4.0 * X3, 0.0]
            HL3 = [0.0, 0.0, 4.0 * X3 - 1.0, 0.0, 4.0 * X2, 4.0 * X1]
            pts.append((H, [a - b for a, b in zip(HL1, HL3)], [a - b for a, b in zip(HL2, HL3)], WGT[L1], WGT[L2], (1.0 - X2)))
    return pts


def face_points(shape):
    """[(H, d1, d2, w1, w2, g)] of 'Q4', 'Q8', 'T6' or 'C6' (the collapsed set of heat_DFLUX_352)"""
    return {"Q4": _q4, "Q8": _q8, "T6": _t6, "C6": lambda: _q8(True)}[shape]()


def _geometry(pt, XF, unit):
    """XSUM of a point, and with unit the determinant the 6-node triangle takes of (G1, G2, G3 / XSUM); XF (nf, mm, 3)"""
    _, d1, d2 = pt[:3]
    G = []
    for d in (d1, d2):
        for c in range(3):
            s = np.zeros(XF.shape[0])
            for i in range(len(d)):
                s = s + d[i] * XF[:, i, c]
            G.append(s)
    G1X, G1Y, G1Z, G2X, G2Y, G2Z = G
    G3X = G1Y * G2Z - G1Z * G2Y
    G3Y = G1Z * G2X - G1X * G2Z
    G3Z = G1X * G2Y - G1Y * G2X
    XSUM = np.sqrt(G3X * G3X + G3Y * G3Y + G3Z * G3Z)
    if not unit:
        return XSUM
    G3X, G3Y, G3Z = G3X / XSUM, G3Y / XSUM, G3Z / XSUM
    XJ11, XJ12, XJ13, XJ21, XJ22, XJ23, XJ31, XJ32, XJ33 = G1X, G1Y, G1Z, G2X, G2Y, G2Z, G3X, G3Y, G3Z
    return XJ11 * XJ22 * XJ33 + XJ12 * XJ23 * XJ31 + XJ13 * XJ21 * XJ32 - XJ13 * XJ22 * XJ31 - XJ12 * XJ21 * XJ33 - XJ11 * XJ23 * XJ32


def _cross3(XF):
    A, B = XF[:, 1] - XF[:, 0], XF[:, 2] - XF[:, 0]
    AX, AY, AZ, BX, BY, BZ = A[:, 0], A[:, 1], A[:, 2], B[:, 0], B[:, 1], B[:, 2]
    return AY * BZ - AZ * BY, AZ * BX - AX * BZ, AX * BY - AY * BX


def _face_input(etype, face, X, *vals):
    X = np.asarray(X, dtype=np.float64).reshape(-1, R.NODES[etype], 3)
    nod = face_nodes(etype, face)
    return (X[:, nod], nod) + tuple(np.broadcast_to(np.asarray(v, dtype=np.float64), (X.shape[0],)) for v in vals)


def _film_like(etype, XF, CFfun, SINK, split):
    """TERM1, TERM2 of one face shape.  CFfun(H) is HH, or RRR at the point; split: heat_FILM_351 / _361 / _362 multiply
    XSUM WGT WGT H(IP) H(JP) HH in that order instead of forming WG first"""
    nf, mm = XF.shape[:2]
    T1, T2 = np.zeros((nf, mm, mm)), np.zeros((nf, mm))
    if mm == 3:
        a, b, c = _cross3(XF)
        AA = np.sqrt(a * a + b * b + c * c) / 6.0
        CF = CFfun(None)
        for IP in range(3):
            T2[:, IP] = -(AA * CF * SINK)
            for JP in range(3):
                T1[:, IP, JP] = -(AA * CF / 3.0)
        return T1, T2
    for pt in face_points({4: "Q4", 8: "Q8", 6: "T6"}[mm]):
        H, _, _, W1, W2, g = pt
        CF = CFfun(H)
        if mm == 6:
            DET = _geometry(pt, XF, True)
            WG = W1 * W2 * DET * g * 0.25 * CF
        else:
            XSUM = _geometry(pt, XF, False)
            WG = None if split else XSUM * W1 * W2 * CF
        for IP in range(mm):
            for JP in range(mm):
                if WG is None:
                    T1[:, IP, JP] = T1[:, IP, JP] - XSUM * W1 * W2 * H[IP] * H[JP] * CF
                else:
                    T1[:, IP, JP] = T1[:, IP, JP] - WG * H[IP] * H[JP]
            if WG is None:
                T2[:, IP] = T2[:, IP] - XSUM * W1 * W2 * H[IP] * CF * SINK
            else:
                T2[:, IP] = T2[:, IP] - WG * H[IP] * SINK
    return T1, T2


def film(etype, face, X, HH, SINK):
    """heat_FILM_<etype>(LTYPE = face) for nf elements X (nf, nn, 3) -> TERM1 (nf, mm, mm), TERM2 (nf, mm), NOD (0-based)"""
    XF, nod, HH, SINK = _face_input(etype, face, X, HH, SINK)
    split = etype in (351, 361, 362) and XF.shape[1] in (4, 8)
    T1, T2 = _film_like(etype, XF, lambda H: HH, SINK, split)
    return T1, T2, nod


def radiate(etype, face, X, TEMP, RR, SINK, TZERO):
    """heat_RADIATE_<etype>: TEMP (nf, nn) the element's node temperatures"""
    XF, nod, RR, SINK = _face_input(etype, face, X, RR, SINK)
    TF = np.asarray(TEMP, dtype=np.float64).reshape(-1, R.NODES[etype])[:, nod]

    def RRR(H):
        if H is None:
            TT = (TF[:, 0] + TF[:, 1] + TF[:, 2]) / 3.0
        else:
            TT = H[0] * TF[:, 0]
            for i in range(1, len(H)):
                TT = TT + H[i] * TF[:, i]
        T1 = TT - TZERO
        T2 = SINK - TZERO
        return (T1 + T2) * (T1 * T1 + T2 * T2) * RR

    T1, T2 = _film_like(etype, XF, RRR, SINK, False)
    return T1, T2, nod


def _rule_351_bf():
    c = R._r                                   # heat_DFLUX_351's DATA statements carry no D0
    g = c(0.5773502691896)
    XG, WGT = (-g, g), (1.0, 1.0)
    XG1 = (c(0.6666666667), c(0.16666666667), c(0.16666666667))
    XG2 = (c(0.1666666667), c(0.66666666667), c(0.16666666667))
    WGT1 = (c(0.1666666667), c(0.16666666667), c(0.16666666667))
    r = R.Rule(6, 1.0)
    for LZ in range(2):
        ZI = XG[LZ]
        for L12 in range(3):
            X1, X2 = XG1[L12], XG2[L12]
            H = [X1 * (1.0 - ZI) * 0.5, X2 * (1.0 - ZI) * 0.5, (1.0 - X1 - X2) * (1.0 - ZI) * 0.5,
                 X1 * (1.0 + ZI) * 0.5, X2 * (1.0 + ZI) * 0.5, (1.0 - X1 - X2) * (1.0 + ZI) * 0.5]
            HR = [(1.0 - ZI) * 0.5, 0.0, -(1.0 - ZI) * 0.5, (1.0 + ZI) * 0.5, 0.0, -(1.0 + ZI) * 0.5]
            HS = [0.0, (1.0 - ZI) * 0.5, -(1.0 - ZI) * 0.5, 0.0, (1.0 + ZI) * 0.5, -(1.0 + ZI) * 0.5]
            HT = [-0.5 * X1, -0.5 * X2, -0.5 * (1.0 - X1 - X2), 0.5 * X1, 0.5 * X2, 0.5 * (1.0 - X1 - X2)]
            r.push(H, HR, HS, HT, [WGT1[L12], WGT[LZ], 1.0, 1.0, 1.0, 1.0])
    return r


def _rule_352_bf():
    """the 15-node set of heat_DFLUX_352's volume load (heat_LIB_DFLUX.f90:1356-1468): collapsed from the 20-node hexahedron"""
    XG, WGT = R._gauss3()
    r = R.Rule(15, 1.0)
    for LX in range(3):
        RI = XG[LX]
        for LY in range(3):
            SI = XG[LY]
            for LZ in range(3):
                TI = XG[LZ]
                RP, SP, TP, RM, SM, TM = 1.0 + RI, 1.0 + SI, 1.0 + TI, 1.0 - RI, 1.0 - SI, 1.0 - TI
                H = [-0.125 * RM * SM * TM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM * (2.0 - RI + SI + TI), -0.25 * SP * TM * (1.0 - SI + TI),
                     -0.125 * RM * SM * TP * (2.0 + RI + SI - TI), -0.125 * RP * SM * TP * (2.0 - RI + SI - TI), 0.25 * SP * TP * (SI + TI - 1.0),
                     0.25 * (1.0 - RI * RI) * SM * TM, 0.25 * RP * (1.0 - SI * SI) * TM, 0.25 * RM * (1.0 - SI * SI) * TM,
                     0.25 * (1.0 - RI * RI) * SM * TP, 0.25 * RP * (1.0 - SI * SI) * TP, 0.25 * RM * (1.0 - SI * SI) * TP,
                     0.25 * RM * SM * (1.0 - TI * TI), 0.25 * RP * SM * (1.0 - TI * TI), 0.5 * SP * (1.0 - TI * TI)]
                HR = [-0.125 * RM * SM * TM + 0.125 * SM * TM * (2.0 + RI + SI + TI), +0.125 * RP * SM * TM - 0.125 * SM * TM * (2.0 - RI + SI + TI), 0.0,
                      -0.125 * RM * SM * TP + 0.125 * SM * TP * (2.0 + RI + SI - TI), +0.125 * RP * SM * TP - 0.125 * SM * TP * (2.0 - RI + SI - TI), 0.0,
                      -0.50 * RI * SM * TM, +0.25 * (1.0 - SI * SI) * TM, -0.25 * (1.0 - SI * SI) * TM,
                      -0.50 * RI * SM * TP, +0.25 * (1.0 - SI * SI) * TP, -0.25 * (1.0 - SI * SI) * TP,
                      -0.25 * SM * (1.0 - TI * TI), +0.25 * SM * (1.0 - TI * TI), 0.0]
                HS = [-0.125 * RM * SM * TM + 0.125 * RM * TM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM + 0.125 * RP * TM * (2.0 - RI + SI + TI),
                      +0.25 * TM * (2.0 * SI - TI),
                      -0.125 * RM * SM * TP + 0.125 * RM * TP * (2.0 + RI + SI - TI), -0.125 * RP * SM * TP + 0.125 * RP * TP * (2.0 - RI + SI - TI),
                      +0.25 * TP * (2.0 * SI + TI),
                      -0.25 * (1.0 - RI * RI) * TM, -0.50 * RP * SI * TM, -0.50 * RM * SI * TM,
                      -0.25 * (1.0 - RI * RI) * TP, -0.50 * RP * SI * TP, -0.50 * RM * SI * TP,
                      -0.25 * RM * (1.0 - TI * TI), -0.25 * RP * (1.0 - TI * TI), +0.50 * (1.0 - TI * TI)]
                HT = [-0.125 * RM * SM * TM + 0.125 * RM * SM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM + 0.125 * RP * SM * (2.0 - RI + SI + TI),
                      +0.25 * SP * (2.0 * TI - SI),
                      +0.125 * RM * SM * TP - 0.125 * RM * SM * (2.0 + RI + SI - TI), +0.125 * RP * SM * TP - 0.125 * RP * SM * (2.0 - RI + SI - TI),
                      +0.25 * SP * (SI + 2.0 * TI),
                      -0.25 * (1.0 - RI * RI) * SM, -0.25 * RP * (1.0 - SI * SI), -0.25 * RM * (1.0 - SI * SI),
                      0.25 * (1.0 - RI * RI) * SM, 0.25 * RP * (1.0 - SI * SI), 0.25 * RM * (1.0 - SI * SI),
                      -0.5 * RM * SM * TI, -0.5 * RP * SM * TI, -SP * TI]
                r.push(H, HR, HS, HT, [WGT[LX], WGT[LY], WGT[LZ], 1.0, 1.0, 1.0])
    return r


def bf_rule(etype):
    """the volume points of heat_DFLUX_<etype>; 341, 342, 361, 362 share theirs with heat_CAPACITY_<etype>"""
    if etype == 351:
        return _rule_351_bf()
    if etype == 352:
        return _rule_352_bf()
    return R.rule(etype, True)


def body_flux(etype, X, val):
    """heat_DFLUX_<etype>(LTYPE = 0) -> VECT (nf, nn)"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, R.NODES[etype], 3)
    val = np.broadcast_to(np.asarray(val, dtype=np.float64), (X.shape[0],))
    r = bf_rule(etype)
    V = np.zeros(X.shape[:2])
    for q in range(r.nq):
        _, DET = R._jacobian(r, q, X)
        H, w = r.H[q], r.W[q]
        for i in range(r.nn):
            if etype == 341:
                V[:, i] = V[:, i] + val * H[i] * DET * w[4] * w[3] * 0.125      # (1 - X3), (1 - X2 - X3)
            elif etype == 342:
                WG = (-DET) * w[0] * w[1] * w[2] * w[3] * w[4] * 0.125
                V[:, i] = V[:, i] - val * WG * H[i]
            elif etype == 351:
                WG = w[0] * w[1] * DET
                V[:, i] = V[:, i] - val * H[i] * WG
            elif etype == 352:
                WG = DET * w[0] * w[1] * w[2]
                V[:, i] = V[:, i] - val * WG * H[i]
            else:
                WG = w[0] * w[1] * w[2] * DET
                V[:, i] = V[:, i] - H[i] * WG * val
    return V


def dflux(etype, face, X, val):
    """heat_DFLUX_<etype>(LTYPE = face; 0: BF) -> VECT (nf, nn) on the element's nodes"""
    if face == 0:
        return body_flux(etype, X, val)
    XF, nod, val = _face_input(etype, face, X, val)
    nf, mm = XF.shape[:2]
    VF = np.zeros((nf, mm))
    if mm == 3:
        a, b, c = _cross3(XF)
        AA = 0.5 * np.sqrt(a * a + b * b + c * c)
        for i in range(3):
            VF[:, i] = -val * AA / 3.0
    else:
        shape = {4: "Q4", 8: "Q8", 6: "T6" if etype == 342 else "C6"}[mm]
        for pt in face_points(shape):
            H, _, _, W1, W2, g = pt
            if shape == "T6":
                WG = W1 * W2 * _geometry(pt, XF, True) * g * 0.25
                for i in range(mm):
                    VF[:, i] = VF[:, i] - val * WG * H[i]
            else:
                XSUM = _geometry(pt, XF, False)
                for i in range(mm):
                    VF[:, i] = VF[:, i] - XSUM * val * W1 * W2 * H[i]
    V = np.zeros((nf, R.NODES[etype]))
    V[:, nod] = VF
    return V


# ---- amplitudes -------------------------------------------------------------------------------------------------------------------------
class Amplitude:
    """heat_init_amplitude's tables of one !AMPLITUDE, rows = [(value, time), ...], and heat_get_amplitude as __call__"""

    def __init__(self, rows):
        self.val = [float(v) for v, _ in rows]
        self.time = [float(t) for _, t in rows]
        nn = self.n = len(rows)
        self.fA, self.fB = np.zeros(nn + 1), np.zeros(nn + 1)
        self.fB[0] = self.val[0]
        for k in range(1, nn):
            x1, y1, x2, y2 = self.time[k - 1], self.val[k - 1], self.time[k], self.val[k]
            self.fA[k] = (y2 - y1) / (x2 - x1)
            self.fB[k] = -(y2 - y1) / (x2 - x1) * x1 + y1
        self.fB[nn] = self.val[nn - 1]

    def __call__(self, TT):
        nn = self.n
        if TT < self.time[0]:
            ii = 0
        elif TT >= self.time[nn - 1]:
            ii = nn
        else:
            ii = 1
            for k in range(nn - 1):
                if self.time[k] <= TT < self.time[k + 1]:
                    ii = k + 1
                    break
        return self.fA[ii] * TT + self.fB[ii]


def amp(a, t):
    """QQ of heat_get_amplitude: 1 without an amplitude"""
    return 1.0 if a is None else a(t)


# ---- the list loops ---------------------------------------------------------------------------------------------------------------------
def _entries(lst):
    g, e, f = (np.asarray(lst[k], dtype=np.int64) for k in range(3))
    vals = [np.broadcast_to(np.asarray(v, dtype=np.float64), g.shape) for v in lst[3:]]
    return g, e, f, vals


def surface_terms(A, coord, groups, temp, dflux_list=None, film_list=None, radiate_list=None, tzero=0.0):
    """heat_mat_ass_bc_DFLUX, _FILM, _RADIATE into A, entry after entry.  A list is (group, elem, face, val[, sink]) with 0-based
    group and element positions and the values already multiplied by their amplitudes"""
    coord = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
    temp = np.asarray(temp, dtype=np.float64)
    if dflux_list is not None:
        g, e, f, (val,) = _entries(dflux_list)
        for k in range(g.size):
            et, conn = int(groups[g[k]][0]), np.asarray(groups[g[k]][1], dtype=np.int64)[e[k]] - 1
            V = dflux(et, int(f[k]), coord[conn][None], val[k])[0]
            for j in range(conn.size):
                A.B[conn[j]] = A.B[conn[j]] - V[j]
    for lst, kind in ((film_list, 1), (radiate_list, 2)):
        if lst is None:
            continue
        g, e, f, (val, sink) = _entries(lst)
        for k in range(g.size):
            et, conn = int(groups[g[k]][0]), np.asarray(groups[g[k]][1], dtype=np.int64)[e[k]] - 1
            if kind == 1:
                T1, T2, nod = film(et, int(f[k]), coord[conn][None], val[k], sink[k])
            else:
                T1, T2, nod = radiate(et, int(f[k]), coord[conn][None], temp[conn][None], val[k], sink[k], tzero)
            n = conn[nod]
            for ip in range(n.size):
                for jp in range(n.size):
                    if n[jp] > n[ip]:
                        p = A.positions(n[ip:ip + 1], n[jp:jp + 1], False)[0]
                        A.AU[p] = A.AU[p] - T1[0, ip, jp]
                    elif n[jp] < n[ip]:
                        p = A.positions(n[ip:ip + 1], n[jp:jp + 1], True)[0]
                        A.AL[p] = A.AL[p] - T1[0, ip, jp]
                    else:
                        A.D[n[ip]] = A.D[n[ip]] - T1[0, ip, jp]
                        A.B[n[jp]] = A.B[n[jp]] - T2[0, jp]
    return A


def assemble(A, coord, groups, mats, temp, temp0, beta, dtime, flux=None, fix=None, dflux_list=None, film_list=None, radiate_list=None,
             tzero=0.0):
    """the whole assembly of one iteration in the reference's order: elements, !CFLUX, !DFLUX, !FILM, !RADIATE, !FIXTEMP"""
    R.assemble(A, coord, groups, mats, temp, temp0, beta, dtime)
    R.boundary(A, flux, None)
    surface_terms(A, coord, groups, temp, dflux_list, film_list, radiate_list, tzero)
    R.boundary(A, None, fix)
    return A


def split_list(lst, nval, t):
    """(group, elem, face, nval values, up to nval amplitudes or None) at time t"""
    if lst is None:
        return None
    amps = list(lst[3 + nval:]) + [None] * nval
    return tuple(lst[:3]) + tuple(np.asarray(v, dtype=np.float64) * amp(a, t) for v, a in zip(lst[3:3 + nval], amps))


def _bc_at(t, fix, flux, fix_amp, flux_amp):
    f = None if fix is None else (fix[0], np.asarray(fix[1], dtype=np.float64) * amp(fix_amp, t))
    q = None if flux is None else np.asarray(flux, dtype=np.float64) * amp(flux_amp, t)
    return f, q


def solve_SS(coord, groups, mats, temp, flux=None, fix=None, dflux=None, film=None, radiate=None, tzero=0.0,
             fix_amp=None, flux_amp=None, eps=1.0e-6, itmax=20):
    """heat_solve_SS with the surface terms; the lists carry amplitudes as heat.heat_solve_SS takes them (evaluated at CTIME = 0)"""
    coord = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
    A = R.profile_of(coord.shape[0], groups)
    TEMP = np.array(temp, dtype=np.float64)
    hist, iterALL = [], 0
    fx, fl = _bc_at(0.0, fix, flux, fix_amp, flux_amp)
    lists = [split_list(l, n, 0.0) for l, n in zip((dflux, film, radiate), (1, 2, 2))]
    while True:
        iterALL += 1
        assemble(A, coord, groups, mats, TEMP, TEMP, 1.0, 0.0, fl, fx, lists[0], lists[1], lists[2], tzero)
        X = np.linalg.solve(A.dense(), A.B)
        TEMPC, TEMP = TEMP, X
        CHK = float(np.sqrt(np.sum((TEMP - TEMPC) ** 2)))
        hist.append((iterALL, CHK))
        if CHK < eps:
            return TEMP, hist
        if iterALL >= itmax:
            raise RuntimeError("ITERATION COUNT OVER : MAX = %d" % itmax)


def solve_TRAN(coord, groups, mats, temp0, dtime, eetime, flux=None, fix=None, dflux=None, film=None, radiate=None, tzero=0.0,
               fix_amp=None, flux_amp=None, eps=1.0e-6, itmax=20, keep=None):
    """heat_solve_TRAN with fixed steps and the surface terms at CTIME = TT (ST = 0: the first step of the analysis)"""
    coord = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
    A = R.profile_of(coord.shape[0], groups)
    TEMP0 = np.array(temp0, dtype=np.float64)
    TEMP = TEMP0.copy()
    TT, DTIME, BETA = 0.0, float(dtime), 0.5
    steps, times = [], []
    while True:
        if TT + DTIME * 1.0000001 >= eetime:
            DTIME = eetime - TT
            TT = eetime
            iend = 1
        else:
            TT = TT + DTIME
            iend = 0
        fx, fl = _bc_at(TT, fix, flux, fix_amp, flux_amp)
        lists = [split_list(l, n, TT) for l, n in zip((dflux, film, radiate), (1, 2, 2))]
        iterALL, hist = 0, []
        while True:
            iterALL += 1
            assemble(A, coord, groups, mats, TEMP, TEMP0, BETA, DTIME, fl, fx, lists[0], lists[1], lists[2], tzero)
            X = np.linalg.solve(A.dense(), A.B)
            TEMPC, TEMP = TEMP, X
            CHK = float(np.sqrt(np.sum((TEMP - TEMPC) ** 2)))
            hist.append((iterALL, CHK))
            if CHK < eps:
                break
            if iterALL > itmax:
                raise RuntimeError("ITERATION COUNT OVER : MAX = %d" % itmax)
        TEMP0 = TEMP.copy()
        steps.append(hist)
        times.append(TT)
        if keep is not None:
            keep.append(TEMP.copy())
        if iend:
            return TEMP, steps, times
