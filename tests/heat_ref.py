"""A numpy restatement of the reference's heat conduction assembly and of its two solution loops, for the tests of
frontistr_amd/csrc/fx_heat.h and frontistr_amd/heat.py (TYPE=341, 342, 351, 352, 361, 362).

    heat_THERMAL_3xx, heat_GET_CONDUCTIVITY           fistr1/src/lib/heat_LIB_THERMAL.f90 (module m_heat_lib_thermal, the one
                                                      heat_mat_ass_conductivity uses; heat_LIB_CONDUCTIVITY.f90 is not called)
    heat_CAPACITY_3xx, heat_GET_CP, heat_GET_DENSITY  fistr1/src/lib/heat_LIB_CAPACITY.f90
    heat_init_material                                fistr1/src/analysis/heat/heat_init.f90:197-231
    heat_mat_ass_conductivity, heat_mat_ass_capacity  the element loops, in element order
    heat_mat_ass_bc_CFLUX, heat_mat_ass_bc_FIXT       with hecmw_mat_ass_bc at NDOF = 1 (hecmw_mat_ass.f90:292-429)
    heat_solve_SS, heat_solve_TRAN                    with a dense solve in place of solve_LINEQ

The order of every sum is the routine's; every literal the routines write without `d0` is taken as the nearest float32
(SINGLE = True; False takes the double value instead, which is what a restatement that overlooks this would compute).
Elements are vectorised over the first axis; nothing else is reordered."""
import numpy as np

SINGLE = True
NODES = {341: 4, 342: 10, 351: 6, 352: 15, 361: 8, 362: 20}


def _r(x):
    """a default-real literal as it reaches double arithmetic"""
    return float(np.float32(x)) if SINGLE else float(x)


# ---- the routines' points -----------------------------------------------------------------------------------------------------------
class Rule:
    def __init__(self, nn, sign):
        self.nn, self.sign = nn, sign
        self.H, self.dR, self.dS, self.dT, self.W = [], [], [], [], []

    def push(self, H, dR, dS, dT, W):
        assert len(H) == len(dR) == len(dS) == len(dT) == self.nn and len(W) == 6
        self.H.append(H); self.dR.append(dR); self.dS.append(dS); self.dT.append(dT); self.W.append(W)

    @property
    def nq(self):
        return len(self.H)


def _rule_341(cap):
    g = _r(0.5773502691896) if cap else 0.5773502691896          # heat_THERMAL_341 writes D0, heat_CAPACITY_341 does not
    XG, WGT = (-g, g), (1.0, 1.0)
    r = Rule(4, -1.0)
    for L3 in range(2):
        XL3 = XG[L3]
        X3 = (XL3 + 1.0) * 0.5
        for L2 in range(2):
            XL2 = XG[L2]
            X2 = (1.0 - X3) * (XL2 + 1.0) * 0.5
            for L1 in range(2):
                XL1 = XG[L1]
                X1 = (1.0 - X2 - X3) * (XL1 + 1.0) * 0.5
                H = [X1, X2, X3, 1.0 - X1 - X2 - X3]
                geo = [(1.0 - X2 - X3), (1.0 - X3), 0.125] if cap else [(1.0 - X3), (1.0 - X2 - X3), 0.125]
                r.push(H, [1.0, 0.0, 0.0, -1.0], [0.0, 1.0, 0.0, -1.0], [0.0, 0.0, 1.0, -1.0], [WGT[L1], WGT[L2], WGT[L3]] + geo)
    return r


def _rule_351(cap):
    c = float                           # both 351 routines write their truncated decimals with D0
    g = c(0.5773502691896)
    XG, WGT = (-g, g), (1.0, 1.0)
    XG1 = (c(0.6666666667), c(0.16666666667), c(0.16666666667))
    XG2 = (c(0.1666666667), c(0.66666666667), c(0.16666666667))
    WGT1 = (c(0.1666666667), c(0.16666666667), c(0.16666666667))
    r = Rule(6, 1.0)
    for LZ in range(2):
        ZI = XG[LZ]
        for L12 in range(3):
            X1, X2 = XG1[L12], XG2[L12]
            H = [X1 * (1.0 - ZI) * 0.5, X2 * (1.0 - ZI) * 0.5, (1.0 - X1 - X2) * (1.0 - ZI) * 0.5,
                 X1 * (1.0 + ZI) * 0.5, X2 * (1.0 + ZI) * 0.5, (1.0 - X1 - X2) * (1.0 + ZI) * 0.5]
            HR = [(1.0 - ZI) * 0.5, 0.0, -(1.0 - ZI) * 0.5, (1.0 + ZI) * 0.5, 0.0, -(1.0 + ZI) * 0.5]
            HS = [0.0, (1.0 - ZI) * 0.5, -(1.0 - ZI) * 0.5, 0.0, (1.0 + ZI) * 0.5, -(1.0 + ZI) * 0.5]
            HT = [-0.5 * X1, -0.5 * X2, -0.5 * (1.0 - X1 - X2), 0.5 * X1, 0.5 * X2, 0.5 * (1.0 - X1 - X2)]
            W = [WGT[LZ], WGT1[L12]] if cap else [WGT1[L12], WGT[LZ]]
            r.push(H, HR, HS, HT, W + [1.0, 1.0, 1.0, 1.0])
    return r


def _rule_361(cap):
    g = _r(0.5773502691896258) if cap else 0.5773502691896      # heat_THERMAL_361 writes D0
    XG, WGT = (-g, g), (1.0, 1.0)
    r = Rule(8, 1.0)
    for LX in range(2):
        RI = XG[LX]
        for LY in range(2):
            SI = XG[LY]
            for LZ in range(2):
                TI = XG[LZ]
                RP, SP, TP, RM, SM, TM = 1.0 + RI, 1.0 + SI, 1.0 + TI, 1.0 - RI, 1.0 - SI, 1.0 - TI
                H = [0.125 * RM * SM * TM, 0.125 * RP * SM * TM, 0.125 * RP * SP * TM, 0.125 * RM * SP * TM,
                     0.125 * RM * SM * TP, 0.125 * RP * SM * TP, 0.125 * RP * SP * TP, 0.125 * RM * SP * TP]
                HR = [-.125 * SM * TM, .125 * SM * TM, .125 * SP * TM, -.125 * SP * TM,
                      -.125 * SM * TP, .125 * SM * TP, .125 * SP * TP, -.125 * SP * TP]
                HS = [-.125 * RM * TM, -.125 * RP * TM, .125 * RP * TM, .125 * RM * TM,
                      -.125 * RM * TP, -.125 * RP * TP, .125 * RP * TP, .125 * RM * TP]
                HT = [-.125 * RM * SM, -.125 * RP * SM, -.125 * RP * SP, -.125 * RM * SP,
                      .125 * RM * SM, .125 * RP * SM, .125 * RP * SP, .125 * RM * SP]
                r.push(H, HR, HS, HT, [WGT[LX], WGT[LY], WGT[LZ], 1.0, 1.0, 1.0])
    return r


def _gauss3():
    g = _r(0.7745966692)
    return (-g, 0.0, g), (_r(0.5555555555), _r(0.8888888888), _r(0.5555555555))


def _rule_342(cap):
    XG, WGT = _gauss3()
    r = Rule(10, -1.0)
    for L3 in range(3):
        XL3 = XG[L3]
        X3 = (XL3 + 1.0) * 0.5
        for L2 in range(3):
            XL2 = XG[L2]
            X2 = (1.0 - X3) * (XL2 + 1.0) * 0.5
            for L1 in range(3):
                XL1 = XG[L1]
                X1 = (1.0 - X2 - X3) * (XL1 + 1.0) * 0.5
                X4 = 1.0 - X1 - X2 - X3
                H = [X1 * (2.0 * X1 - 1.0), X2 * (2.0 * X2 - 1.0), X3 * (2.0 * X3 - 1.0), X4 * (2.0 * X4 - 1.0), 4.0 * X1 * X2,
                     4.0 * X2 * X3, 4.0 * X1 * X3, 4.0 * X1 * X4, 4.0 * X2 * X4, 4.0 * X3 * X4]
                HL1 = [4.0 * X1 - 1.0, 0.0, 0.0, 0.0, 4.0 * X2, 0.0, 4.0 * X3, 4.0 * X4, 0.0, 0.0]
                HL2 = [0.0, 4.0 * X2 - 1.0, 0.0, 0.0, 4.0 * X1, 4.0 * X3, 0.0, 0.0, 4.0 * X4, 0.0]
                HL3 = [0.0, 0.0, 4.0 * X3 - 1.0, 0.0, 0.0, 4.0 * X2, 4.0 * X1, 0.0, 0.0, 4.0 * X4]
                HL4 = [0.0, 0.0, 0.0, 4.0 * X4 - 1.0, 0.0, 0.0, 0.0, 4.0 * X1, 4.0 * X2, 4.0 * X3]
                r.push(H, [a - b for a, b in zip(HL1, HL4)], [a - b for a, b in zip(HL2, HL4)], [a - b for a, b in zip(HL3, HL4)],
                       [WGT[L1], WGT[L2], WGT[L3], (1.0 - X3), (1.0 - X2 - X3), 0.125])
    return r


def _rule_352(cap):
    XG, WGT = _gauss3()
    r = Rule(15, 1.0)
    for LZ in range(3):
        ZI = XG[LZ]
        for L2 in range(3):
            XL2 = XG[L2]
            X2 = (XL2 + 1.0) * 0.5
            for L1 in range(3):
                XL1 = XG[L1]
                X1 = 0.5 * (1.0 - X2) * (XL1 + 1.0)
                X3 = 1.0 - X1 - X2
                H = [0.5 * X1 * (2.0 * X1 - 2. - ZI) * (1.0 - ZI), 0.5 * X2 * (2.0 * X2 - 2. - ZI) * (1.0 - ZI),
                     0.5 * X3 * (2.0 * X3 - 2. - ZI) * (1.0 - ZI), 0.5 * X1 * (2.0 * X1 - 2. + ZI) * (1.0 + ZI),
                     0.5 * X2 * (2.0 * X2 - 2. + ZI) * (1.0 + ZI), 0.5 * X3 * (2.0 * X3 - 2. + ZI) * (1.0 + ZI),
                     2.0 * X1 * X2 * (1.0 - ZI), 2.0 * X2 * X3 * (1.0 - ZI), 2.0 * X1 * X3 * (1.0 - ZI),
                     2.0 * X1 * X2 * (1.0 + ZI), 2.0 * X2 * X3 * (1.0 + ZI), 2.0 * X1 * X3 * (1.0 + ZI),
                     X1 * (1.0 - ZI * ZI), X2 * (1.0 - ZI * ZI), X3 * (1.0 - ZI * ZI)]
                HL1 = [0.5 * (4.0 * X1 - 2. - ZI) * (1.0 - ZI), 0.0, 0.0, 0.5 * (4.0 * X1 - 2. + ZI) * (1.0 + ZI), 0.0, 0.0,
                       2.0 * X2 * (1.0 - ZI), 0.0, 2.0 * X3 * (1.0 - ZI), 2.0 * X2 * (1.0 + ZI), 0.0, 2.0 * X3 * (1.0 + ZI),
                       1.0 - ZI * ZI, 0.0, 0.0]
                HL2 = [0.0, 0.5 * (4.0 * X2 - 2. - ZI) * (1.0 - ZI), 0.0, 0.0, 0.5 * (4.0 * X2 - 2. + ZI) * (1.0 + ZI), 0.0,
                       2.0 * X1 * (1.0 - ZI), 2.0 * X3 * (1.0 - ZI), 0.0, 2.0 * X1 * (1.0 + ZI), 2.0 * X3 * (1.0 + ZI), 0.0,
                       0.0, 1.0 - ZI * ZI, 0.0]
                HL3 = [0.0, 0.0, 0.5 * (4.0 * X3 - 2. - ZI) * (1.0 - ZI), 0.0, 0.0, 0.5 * (4.0 * X3 - 2. + ZI) * (1.0 + ZI),
                       0.0, 2.0 * X2 * (1.0 - ZI), 2.0 * X1 * (1.0 - ZI), 0.0, 2.0 * X2 * (1.0 + ZI), 2.0 * X1 * (1.0 + ZI),
                       0.0, 0.0, 1.0 - ZI * ZI]
                HZ = [0.5 * X1 * (-2.0 * X1 + 1.0 + 2.0 * ZI), 0.5 * X2 * (-2.0 * X2 + 1.0 + 2.0 * ZI),
                      0.5 * X3 * (-2.0 * X3 + 1.0 + 2.0 * ZI), 0.5 * X1 * (2.0 * X1 - 1.0 + 2.0 * ZI),
                      0.5 * X2 * (2.0 * X2 - 1.0 + 2.0 * ZI), 0.5 * X3 * (2.0 * X3 - 1.0 + 2.0 * ZI),
                      -2.0 * X1 * X2, -2.0 * X2 * X3, -2.0 * X1 * X3, 2.0 * X1 * X2, 2.0 * X2 * X3, 2.0 * X1 * X3,
                      -2.0 * X1 * ZI, -2.0 * X2 * ZI, -2.0 * X3 * ZI]
                r.push(H, [a - b for a, b in zip(HL1, HL3)], [a - b for a, b in zip(HL2, HL3)], HZ,
                       [WGT[L1], WGT[L2], WGT[LZ], (1.0 - X2), 0.25, 1.0])
    return r


def _rule_362(cap):
    XG, WGT = _gauss3()
    r = Rule(20, 1.0)
    for LX in range(3):
        RI = XG[LX]
        for LY in range(3):
            SI = XG[LY]
            for LZ in range(3):
                TI = XG[LZ]
                RP, SP, TP, RM, SM, TM = 1.0 + RI, 1.0 + SI, 1.0 + TI, 1.0 - RI, 1.0 - SI, 1.0 - TI
                H = [-0.125 * RM * SM * TM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM * (2.0 - RI + SI + TI),
                     -0.125 * RP * SP * TM * (2.0 - RI - SI + TI), -0.125 * RM * SP * TM * (2.0 + RI - SI + TI),
                     -0.125 * RM * SM * TP * (2.0 + RI + SI - TI), -0.125 * RP * SM * TP * (2.0 - RI + SI - TI),
                     -0.125 * RP * SP * TP * (2.0 - RI - SI - TI), -0.125 * RM * SP * TP * (2.0 + RI - SI - TI),
                     0.25 * (1.0 - RI * RI) * SM * TM, 0.25 * RP * (1.0 - SI * SI) * TM, 0.25 * (1.0 - RI * RI) * SP * TM,
                     0.25 * RM * (1.0 - SI * SI) * TM, 0.25 * (1.0 - RI * RI) * SM * TP, 0.25 * RP * (1.0 - SI * SI) * TP,
                     0.25 * (1.0 - RI * RI) * SP * TP, 0.25 * RM * (1.0 - SI * SI) * TP, 0.25 * RM * SM * (1.0 - TI * TI),
                     0.25 * RP * SM * (1.0 - TI * TI), 0.25 * RP * SP * (1.0 - TI * TI), 0.25 * RM * SP * (1.0 - TI * TI)]
                HR = [-0.125 * RM * SM * TM + 0.125 * SM * TM * (2.0 + RI + SI + TI), +0.125 * RP * SM * TM - 0.125 * SM * TM * (2.0 - RI + SI + TI),
                      +0.125 * RP * SP * TM - 0.125 * SP * TM * (2.0 - RI - SI + TI), -0.125 * RM * SP * TM + 0.125 * SP * TM * (2.0 + RI - SI + TI),
                      -0.125 * RM * SM * TP + 0.125 * SM * TP * (2.0 + RI + SI - TI), +0.125 * RP * SM * TP - 0.125 * SM * TP * (2.0 - RI + SI - TI),
                      +0.125 * RP * SP * TP - 0.125 * SP * TP * (2.0 - RI - SI - TI), -0.125 * RM * SP * TP + 0.125 * SP * TP * (2.0 + RI - SI - TI),
                      -0.50 * RI * SM * TM, +0.25 * (1.0 - SI * SI) * TM, -0.50 * RI * SP * TM, -0.25 * (1.0 - SI * SI) * TM,
                      -0.50 * RI * SM * TP, +0.25 * (1.0 - SI * SI) * TP, -0.50 * RI * SP * TP, -0.25 * (1.0 - SI * SI) * TP,
                      -0.25 * SM * (1.0 - TI * TI), +0.25 * SM * (1.0 - TI * TI), +0.25 * SP * (1.0 - TI * TI), -0.25 * SP * (1.0 - TI * TI)]
                HS = [-0.125 * RM * SM * TM + 0.125 * RM * TM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM + 0.125 * RP * TM * (2.0 - RI + SI + TI),
                      +0.125 * RP * SP * TM - 0.125 * RP * TM * (2.0 - RI - SI + TI), +0.125 * RM * SP * TM - 0.125 * RM * TM * (2.0 + RI - SI + TI),
                      -0.125 * RM * SM * TP + 0.125 * RM * TP * (2.0 + RI + SI - TI), -0.125 * RP * SM * TP + 0.125 * RP * TP * (2.0 - RI + SI - TI),
                      +0.125 * RP * SP * TP - 0.125 * RP * TP * (2.0 - RI - SI - TI), +0.125 * RM * SP * TP - 0.125 * RM * TP * (2.0 + RI - SI - TI),
                      -0.25 * (1.0 - RI * RI) * TM, -0.50 * RP * SI * TM, +0.25 * (1.0 - RI * RI) * TM, -0.50 * RM * SI * TM,
                      -0.25 * (1.0 - RI * RI) * TP, -0.50 * RP * SI * TP, +0.25 * (1.0 - RI * RI) * TP, -0.50 * RM * SI * TP,
                      -0.25 * RM * (1.0 - TI * TI), -0.25 * RP * (1.0 - TI * TI), +0.25 * RP * (1.0 - TI * TI), +0.25 * RM * (1.0 - TI * TI)]
                HT = [-0.125 * RM * SM * TM + 0.125 * RM * SM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM + 0.125 * RP * SM * (2.0 - RI + SI + TI),
                      -0.125 * RP * SP * TM + 0.125 * RP * SP * (2.0 - RI - SI + TI), -0.125 * RM * SP * TM + 0.125 * RM * SP * (2.0 + RI - SI + TI),
                      +0.125 * RM * SM * TP - 0.125 * RM * SM * (2.0 + RI + SI - TI), +0.125 * RP * SM * TP - 0.125 * RP * SM * (2.0 - RI + SI - TI),
                      +0.125 * RP * SP * TP - 0.125 * RP * SP * (2.0 - RI - SI - TI), +0.125 * RM * SP * TP - 0.125 * RM * SP * (2.0 + RI - SI - TI),
                      -0.25 * (1.0 - RI * RI) * SM, -0.25 * RP * (1.0 - SI * SI), -0.25 * (1.0 - RI * RI) * SP, -0.25 * RM * (1.0 - SI * SI),
                      0.25 * (1.0 - RI * RI) * SM, 0.25 * RP * (1.0 - SI * SI), 0.25 * (1.0 - RI * RI) * SP, 0.25 * RM * (1.0 - SI * SI),
                      -0.5 * RM * SM * TI, -0.5 * RP * SM * TI, -0.5 * RP * SP * TI, -0.5 * RM * SP * TI]
                r.push(H, HR, HS, HT, [WGT[LX], WGT[LY], WGT[LZ], 1.0, 1.0, 1.0])
    return r


_RULES = {341: _rule_341, 342: _rule_342, 351: _rule_351, 352: _rule_352, 361: _rule_361, 362: _rule_362}


def rule(etype, cap=False):
    return _RULES[etype](cap)


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def make_table(rows):
    """heat_init_material: rows = [(value, temperature), ...] -> (ntab, temp[ntab], funcA[ntab + 1], funcB[ntab + 1])"""
    val = [float(v) for v, _ in rows]
    tmp = [float(t) for _, t in rows]
    n = len(rows)
    fA, fB = np.zeros(n + 1), np.zeros(n + 1)
    fB[0] = val[0]
    for k in range(1, n):
        bb = val[k] - val[k - 1]
        aa = tmp[k] - tmp[k - 1]
        fA[k] = bb / aa
        fB[k] = -(bb / aa) * tmp[k - 1] + val[k - 1]
    fB[n] = val[n - 1]
    return n, np.array(tmp), fA, fB


class Material:
    def __init__(self, cond, cp=None, rho=None):
        self.cond = make_table(cond)
        self.cp = None if cp is None else make_table(cp)
        self.rho = None if rho is None else make_table(rho)


def get_conductivity(T, tab):
    ntab, temp, fA, fB = tab
    T = np.asarray(T, dtype=np.float64)
    if ntab == 1:
        return np.full(T.shape, fB[0])
    itab = np.full(T.shape, ntab, dtype=np.int64)
    for k in range(ntab - 2, -1, -1):
        itab[(T > temp[k]) & (T <= temp[k + 1])] = k + 1
    itab[T <= temp[0]] = 0
    return fA[itab] * T + fB[itab]


def get_cp(T, tab):
    """heat_GET_CP and heat_GET_DENSITY"""
    ntab, temp, fA, fB = tab
    T = np.asarray(T, dtype=np.float64)
    itab = np.full(T.shape, ntab, dtype=np.int64)
    for k in range(ntab - 2, -1, -1):
        itab[(T >= temp[k]) & (T < temp[k + 1])] = k + 1
    itab[T >= temp[ntab - 1]] = ntab
    itab[T < temp[0]] = 0
    return fA[itab] * T + fB[itab]


# ---- the element routines ---------------------------------------------------------------------------------------------------------------
def _jacobian(r, q, X):
    """XJ[a][b] (a: derivative, b: coordinate) and DET of point q; X (ne, nn, 3)"""
    XJ = [[None] * 3 for _ in range(3)]
    for a, d in enumerate((r.dR[q], r.dS[q], r.dT[q])):
        for b in range(3):
            s = np.zeros(X.shape[0])
            for i in range(r.nn):
                s = s + d[i] * X[:, i, b]
            XJ[a][b] = s
    (XJ11, XJ12, XJ13), (XJ21, XJ22, XJ23), (XJ31, XJ32, XJ33) = XJ
    DET = XJ11 * XJ22 * XJ33 + XJ12 * XJ23 * XJ31 + XJ13 * XJ21 * XJ32 - XJ13 * XJ22 * XJ31 - XJ12 * XJ21 * XJ33 - XJ11 * XJ23 * XJ32
    return XJ, DET


def thermal(etype, X, TT, cond):
    """heat_THERMAL_<etype> for ne elements: X (ne, nn, 3), TT (ne, nn) -> SS (ne, nn, nn)"""
    r = rule(etype, False)
    X, TT = np.asarray(X, dtype=np.float64), np.asarray(TT, dtype=np.float64)
    ne, nn = TT.shape
    SS = np.zeros((ne, nn, nn))
    for q in range(r.nq):
        XJ, DET = _jacobian(r, q, X)
        (XJ11, XJ12, XJ13), (XJ21, XJ22, XJ23), (XJ31, XJ32, XJ33) = XJ
        CTEMP = np.zeros(ne)
        for i in range(nn):
            CTEMP = CTEMP + r.H[q][i] * TT[:, i]
        CC = get_conductivity(CTEMP, cond)
        w = r.W[q]
        WG = r.sign * (CC * w[0] * w[1] * w[2] * DET * w[3] * w[4] * w[5])
        DUM = 1.0 / DET
        XJI11 = DUM * (XJ22 * XJ33 - XJ23 * XJ32); XJI21 = DUM * (-XJ21 * XJ33 + XJ23 * XJ31); XJI31 = DUM * (XJ21 * XJ32 - XJ22 * XJ31)
        XJI12 = DUM * (-XJ12 * XJ33 + XJ13 * XJ32); XJI22 = DUM * (XJ11 * XJ33 - XJ13 * XJ31); XJI32 = DUM * (-XJ11 * XJ32 + XJ12 * XJ31)
        XJI13 = DUM * (XJ12 * XJ23 - XJ13 * XJ22); XJI23 = DUM * (-XJ11 * XJ23 + XJ13 * XJ21); XJI33 = DUM * (XJ11 * XJ22 - XJ12 * XJ21)
        BX, BY, BZ = np.zeros((ne, nn)), np.zeros((ne, nn)), np.zeros((ne, nn))
        for j in range(nn):
            hr, hs, ht = r.dR[q][j], r.dS[q][j], r.dT[q][j]
            BX[:, j] = XJI11 * hr + XJI12 * hs + XJI13 * ht
            BY[:, j] = XJI21 * hr + XJI22 * hs + XJI23 * ht
            BZ[:, j] = XJI31 * hr + XJI32 * hs + XJI33 * ht
        g = WG[:, None, None]
        SS = SS + BX[:, :, None] * BX[:, None, :] * g + BY[:, :, None] * BY[:, None, :] * g + BZ[:, :, None] * BZ[:, None, :] * g
    return SS


def capacity(etype, X, TT, cp, rho):
    """heat_CAPACITY_<etype> for ne elements at the temperatures TT (the caller passes TEMP0) -> S0 (ne, nn)"""
    r = rule(etype, True)
    X, TT = np.asarray(X, dtype=np.float64), np.asarray(TT, dtype=np.float64)
    ne, nn = TT.shape
    hrz = etype in (342, 352, 362)
    S = np.zeros((ne, nn))
    TOTD, TOTM = np.zeros(ne), np.zeros(ne)
    for q in range(r.nq):
        _, DET = _jacobian(r, q, X)
        H = r.H[q]
        if etype == 341:
            T = TT[:, nn - 1]                # `do I = 1, NN: TEMP = TT(I)`
        else:
            T = np.zeros(ne)
            for i in range(nn):
                T = T + TT[:, i] * H[i]
        SPE, DEN = get_cp(T, cp), get_cp(T, rho)
        w = r.W[q]
        WG = r.sign * (w[0] * w[1] * w[2] * DET * w[3] * w[4] * w[5])
        if not hrz:
            for i in range(nn):
                S[:, i] = S[:, i] + WG * SPE * DEN * H[i]
            continue
        for j in range(nn):
            for j2 in range(j + 1):
                t = H[j] * H[j2] * WG * SPE * DEN
                if j == j2:
                    S[:, j] = S[:, j] + t
                    TOTD = TOTD + t
                TOTM = TOTM + t
    if hrz:
        S = S * (2. * TOTM - TOTD)[:, None] / TOTD[:, None]
    return S


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------
class Matrix:
    """scalar CRS of hecmwST_matrix with NDOF = 1: indexL/U (0:NP), itemL/U 1-based"""

    def __init__(self, NP, indexL, itemL, indexU, itemU):
        self.NP = NP
        self.indexL, self.itemL, self.indexU, self.itemU = (np.asarray(a, dtype=np.int64) for a in (indexL, itemL, indexU, itemU))
        self.D, self.AL, self.AU, self.B = np.zeros(NP), np.zeros(self.itemL.size), np.zeros(self.itemU.size), np.zeros(NP)
        rowL = np.repeat(np.arange(NP), np.diff(self.indexL))
        rowU = np.repeat(np.arange(NP), np.diff(self.indexU))
        self._keyL = rowL * NP + (self.itemL - 1)      # sorted: rows ascend, items ascend inside a row
        self._keyU = rowU * NP + (self.itemU - 1)

    def positions(self, row, col, lower):
        """0-based positions in AL (lower) or AU of the entries (row, col), 0-based node ids; every one must exist"""
        key, keys = row * self.NP + col, self._keyL if lower else self._keyU
        p = np.searchsorted(keys, key)
        assert np.all(p < keys.size) and np.all(keys[np.minimum(p, keys.size - 1)] == key), "entry absent from the profile"
        return p

    def dense(self):
        A = np.diag(self.D)
        for i in range(self.NP):
            A[i, self.itemL[self.indexL[i]:self.indexL[i + 1]] - 1] = self.AL[self.indexL[i]:self.indexL[i + 1]]
            A[i, self.itemU[self.indexU[i]:self.indexU[i + 1]] - 1] = self.AU[self.indexU[i]:self.indexU[i + 1]]
        return A


def profile_of(n_node, groups):
    """hecmw_mat_con of the union of the groups: -> Matrix"""
    keys = []
    for etype, conn in ((g[0], g[1]) for g in groups):
        c = np.asarray(conn, dtype=np.int64) - 1
        keys.append((c[:, :, None] * n_node + c[:, None, :]).ravel())
    keys = np.unique(np.concatenate(keys))
    row, col = keys // n_node, keys % n_node
    lo, up = col < row, col > row
    indexL, indexU = np.zeros(n_node + 1, dtype=np.int64), np.zeros(n_node + 1, dtype=np.int64)
    indexL[1:] = np.cumsum(np.bincount(row[lo], minlength=n_node))
    indexU[1:] = np.cumsum(np.bincount(row[up], minlength=n_node))
    return Matrix(n_node, indexL, col[lo] + 1, indexU, col[up] + 1)


def _area_4(X):
    """heat_get_area (heat_LIB_THERMAL.f90:1010-1067): X (ne, 4, 3)"""
    g = 0.5773502691896258
    XG = (-g, g)
    AA = np.zeros(X.shape[0])
    for LX in range(2):
        RI = XG[LX]
        for LY in range(2):
            SI = XG[LY]
            RP, SP, RM, SM = 1.0 + RI, 1.0 + SI, 1.0 - RI, 1.0 - SI
            HR = [.25 * SP, -.25 * SP, -.25 * SM, .25 * SM]
            HS = [.25 * RP, .25 * RM, -.25 * RM, -.25 * RP]
            d = []
            for h in (HR, HS):
                for c in range(3):
                    d.append(h[0] * X[:, 0, c] + h[1] * X[:, 1, c] + h[2] * X[:, 2, c] + h[3] * X[:, 3, c])
            XR, YR, ZR, XS, YS, ZS = d
            AA = AA + np.sqrt((YR * ZS - ZR * YS) ** 2 + (ZR * XS - XR * ZS) ** 2 + (XR * YS - YR * XS) ** 2)
    return AA


def thermal_541(X, TEMP, TZERO, THICK, HH, RR1, RR2):
    """heat_THERMAL_541 (heat_LIB_THERMAL.f90:902-1007), the 8-node interface element of the exM/MG361 deck; host only: the device
    assembly does not take interface elements.  X (ne, 8, 3), TEMP (ne, 8) -> SS (ne, 8, 8)"""
    ne = X.shape[0]
    SA, SB = _area_4(X[:, 0:4]), _area_4(X[:, 4:8])
    TZ = TEMP - TZERO
    RRR1, RRR2 = RR1 ** 0.25, RR2 ** 0.25
    SS = np.zeros((ne, 8, 8))
    HHH = HH / THICK
    SM = (SA + SB) * 0.5
    for i in range(4):
        a, b = RRR1 * TZ[:, i], RRR2 * TZ[:, i + 4]
        HA = (a ** 2 + b ** 2) * (a + b) * RRR1
        HB = (a ** 2 + b ** 2) * (a + b) * RRR2
        SS[:, i, i] = (HHH + HA) * SA * 0.25
        SS[:, i + 4, i + 4] = (HHH + HB) * SB * 0.25
        HHi = (HA + HB) * 0.5
        SS[:, i + 4, i] = -(HHH + HHi) * SM * 0.25
        SS[:, i, i + 4] = SS[:, i + 4, i]
    return SS


def element_arrays(coord, groups, mats, temp, temp0, dtime):
    """per group (SS (ne, nn, nn) at temp, S0 (ne, nn) at temp0 or None): computed once, shared by the tests that need them"""
    coord = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
    out = []
    for grp in groups:
        etype, conn = int(grp[0]), np.asarray(grp[1], dtype=np.int64) - 1
        if etype == 541:                      # (541, conn, (TZERO, THICK, HH, RR1, RR2)); heat_mat_ass_capacity adds nothing for it
            out.append((thermal_541(coord[conn], temp[conn], *grp[2]), np.zeros(conn.shape) if dtime > 0 else None))
            continue
        em = np.zeros(conn.shape[0], dtype=np.int64) if len(grp) < 4 or grp[3] is None else np.asarray(grp[3], dtype=np.int64) - 1
        SS = np.zeros((conn.shape[0], conn.shape[1], conn.shape[1]))
        S0 = np.zeros(conn.shape) if dtime > 0 else None
        for m in np.unique(em):
            sel = em == m
            SS[sel] = thermal(etype, coord[conn[sel]], temp[conn[sel]], mats[m].cond)
            if dtime > 0:
                S0[sel] = capacity(etype, coord[conn[sel]], temp0[conn[sel]], mats[m].cp, mats[m].rho)
        out.append((SS, S0))
    return out


def assemble(A, coord, groups, mats, temp, temp0, beta, dtime, elems=None):
    """heat_mat_ass_conductivity (BETA) and, with dtime > 0, heat_mat_ass_capacity into A (cleared first): every entry receives its
    contributions in the reference's order (group after group, element after element, ip, jp)"""
    temp = np.asarray(temp, dtype=np.float64)
    temp0 = temp if temp0 is None else np.asarray(temp0, dtype=np.float64)
    ALFA = 1.0 - beta
    A.D[:] = 0.0; A.AL[:] = 0.0; A.AU[:] = 0.0; A.B[:] = 0.0
    elems = element_arrays(coord, groups, mats, temp, temp0, dtime) if elems is None else elems
    for grp, (SS, _) in zip(groups, elems):
        conn = np.asarray(grp[1], dtype=np.int64) - 1
        ne, nn = conn.shape
        inod = np.broadcast_to(conn[:, :, None], (ne, nn, nn)).ravel()
        jnod = np.broadcast_to(conn[:, None, :], (ne, nn, nn)).ravel()
        v = (SS * beta).ravel()
        up, lo, di = jnod > inod, jnod < inod, jnod == inod
        np.add.at(A.AU, A.positions(inod[up], jnod[up], False), v[up])
        np.add.at(A.AL, A.positions(inod[lo], jnod[lo], True), v[lo])
        np.add.at(A.D, inod[di], v[di])
        T0 = np.broadcast_to(temp0[conn][:, None, :], (ne, nn, nn))
        np.subtract.at(A.B, inod, (SS * T0 * ALFA).ravel())
    if dtime > 0:
        for grp, (_, S0) in zip(groups, elems):
            conn = np.asarray(grp[1], dtype=np.int64) - 1
            np.add.at(A.D, conn.ravel(), (S0 / dtime).ravel())
            np.add.at(A.B, conn.ravel(), (S0 * temp0[conn] / dtime).ravel())
    return A


def mat_ass_bc(A, inode, RHS):
    """hecmw_mat_ass_bc(hecMAT, inode, 1, RHS) with NDOF = 1; inode 1-based"""
    i = inode - 1
    A.B[i] = RHS
    A.D[i] = 1.0
    for k in range(A.indexL[i], A.indexL[i + 1]):
        A.AL[k] = 0.0
        n = A.itemL[k] - 1
        for ik in range(A.indexU[n], A.indexU[n + 1]):
            if A.itemU[ik] == inode:
                A.B[n] = A.B[n] - A.AU[ik] * RHS
                A.AU[ik] = 0.0
                break
    for k in range(A.indexU[i], A.indexU[i + 1]):
        A.AU[k] = 0.0
        n = A.itemU[k] - 1
        for ik in range(A.indexL[n], A.indexL[n + 1]):
            if A.itemL[ik] == inode:
                A.B[n] = A.B[n] - A.AL[ik] * RHS
                A.AL[ik] = 0.0
                break


def boundary(A, flux=None, fix=None):
    """heat_mat_ass_boundary with !CFLUX and !FIXTEMP at constant amplitude: flux (n_node) or None, fix = (nodes 1-based, values)"""
    if flux is not None:
        A.B += np.asarray(flux, dtype=np.float64)
    if fix is not None:
        for n, v in zip(*fix):
            mat_ass_bc(A, int(n), float(v))


# ---- the two loops ------------------------------------------------------------------------------------------------------------------------
def solve_SS(coord, groups, mats, temp, flux=None, fix=None, eps=1.0e-6, itmax=20, A=None):
    """heat_solve_SS -> (TEMP, [(iterALL, CHK)]); raises where the reference aborts (ITERATION COUNT OVER)"""
    coord = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
    A = profile_of(coord.shape[0], groups) if A is None else A
    TEMP = np.array(temp, dtype=np.float64)
    hist, iterALL = [], 0
    while True:
        iterALL += 1
        assemble(A, coord, groups, mats, TEMP, TEMP, 1.0, 0.0)
        boundary(A, flux, fix)
        X = np.linalg.solve(A.dense(), A.B)
        TEMPC, TEMP = TEMP, X
        CHK = float(np.sqrt(np.sum((TEMP - TEMPC) ** 2)))
        hist.append((iterALL, CHK))
        if CHK < eps:
            return TEMP, hist
        if iterALL >= itmax:
            raise RuntimeError("ITERATION COUNT OVER : MAX = %d" % itmax)


def solve_TRAN(coord, groups, mats, temp0, dtime, eetime, flux=None, fix=None, eps=1.0e-6, itmax=20, delmin=0.0, A=None, keep=None):
    """heat_solve_TRAN with fixed steps (DELMIN = 0) -> (TEMP, [[(iterALL, CHK), ...] per step], [time per step])"""
    if delmin > 0.0:
        raise NotImplementedError("automatic time step")
    coord = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
    A = profile_of(coord.shape[0], groups) if A is None else A
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
        iterALL, hist = 0, []
        while True:
            iterALL += 1
            assemble(A, coord, groups, mats, TEMP, TEMP0, BETA, DTIME)
            boundary(A, flux, fix)
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
            keep.append(TEMP.copy())        # what the result file of this step holds
        if iend:
            return TEMP, steps, times
