// Heat conduction (!SOLUTION, TYPE=HEAT): heat_mat_ass_conductivity.f90 and heat_mat_ass_capacity.f90 on the device for
// TYPE=341, 342, 351, 352, 361, 362 (included by fistr_hip.hip after fx_assemble_groups.h); the surface terms of
// heat_mat_ass_boundary are fx_heat_bc.h, included below.
//
// What is restated, routine by routine: heat_THERMAL_3xx and heat_GET_CONDUCTIVITY of module m_heat_lib_thermal
// (heat_LIB_THERMAL.f90: the module heat_mat_ass_conductivity uses through m_heat_lib; heat_LIB_CONDUCTIVITY.f90 holds older
// copies whose 341 / 351 / 361 constants lack the D0 and which fistr1 does not call), heat_CAPACITY_3xx, heat_GET_CP and
// heat_GET_DENSITY (heat_LIB_CAPACITY.f90).  These routines have their own point sets, loop order, shape functions
// and weights (none is the STF_C3 table of fx_c3_element.h), and several of their constants (the 3-point rule of the quadratic
// types, heat_CAPACITY_341 / _361) are default-real literals: they reach the arithmetic as the nearest float32, widened to
// double.  Everything of a routine that depends only on the quadrature point -- H, the derivatives, the weight factors -- is evaluated once on the host with the routine's own
// expressions in the routine's own order (fxh::rule_3xx) and kept as a table on the device; everything that depends on the
// element -- Jacobian, determinant, inverse, B, the table lookups, the sums over the points -- is k_heat, in the routine's order.
//
// Lane mapping: HEAT_LPE = 16 lanes per element, 4 elements per workgroup of one wave.  Per quadrature point: lanes 0..8 each
// sum one entry of the Jacobian over the nodes, lane 9 the temperature and its table value; every lane then inverts the 3x3
// (registers), lanes < NN make BX, BY, BZ of their node (LDS), and every lane adds the point's term to its own entries of the
// upper triangle of SS (entry e of NN (NN + 1) / 2 belongs to lane e % 16: 14 accumulators at TYPE=362, so nothing spills).
// Scatter: colour by colour through the cached position map, plain read-modify-write into a cleared matrix, no atomics.
#pragma once

namespace fxh {
struct Rule {  // one routine's points: [nq][nn] tables and [nq][6] weight factors (w1, w2, w3, g1, g2, g3)
  int nn = 0, nq = 0;
  double sign = 1.0;  // the routine's DET = -DET and leading minus signs, together
  std::vector<double> H, dR, dS, dT, W;
  void push(const double *h, const double *r, const double *s, const double *t, double w1, double w2, double w3, double g1, double g2,
            double g3) {
    H.insert(H.end(), h, h + nn); dR.insert(dR.end(), r, r + nn); dS.insert(dS.end(), s, s + nn); dT.insert(dT.end(), t, t + nn);
    const double w[6] = {w1, w2, w3, g1, g2, g3};
    W.insert(W.end(), w, w + 6);
    nq++;
  }
};

// heat_THERMAL_341 (heat_LIB_THERMAL.f90:260-401, constants with D0) / heat_CAPACITY_341 (heat_LIB_CAPACITY.f90:222-318,
// default-real constants): 2 x 2 x 2 collapsed points, DET = -DET
static void rule_341(Rule &r, bool cap) {
#pragma clang fp contract(off)
  const double g = cap ? (double)0.5773502691896f : 0.5773502691896;
  const double XG[2] = {-g, g}, WGT[2] = {1.0, 1.0};
  r.nn = 4; r.sign = -1.0;
  for (int L3 = 0; L3 < 2; L3++) {
    const double XL3 = XG[L3], X3 = (XL3 + 1.0) * 0.5;
    for (int L2 = 0; L2 < 2; L2++) {
      const double XL2 = XG[L2], X2 = (1.0 - X3) * (XL2 + 1.0) * 0.5;
      for (int L1 = 0; L1 < 2; L1++) {
        const double XL1 = XG[L1], X1 = (1.0 - X2 - X3) * (XL1 + 1.0) * 0.5;
        const double H[4] = {X1, X2, X3, 1.0 - X1 - X2 - X3};
        const double HR[4] = {1.0, 0.0, 0.0, -1.0}, HS[4] = {0.0, 1.0, 0.0, -1.0}, HT[4] = {0.0, 0.0, 1.0, -1.0};
        if (!cap) r.push(H, HR, HS, HT, WGT[L1], WGT[L2], WGT[L3], (1.0 - X3), (1.0 - X2 - X3), 0.125);
        else r.push(H, HR, HS, HT, WGT[L1], WGT[L2], WGT[L3], (1.0 - X2 - X3), (1.0 - X3), 0.125);
      }
    }
  }
}
// heat_THERMAL_351 (heat_LIB_THERMAL.f90:404-608) and heat_CAPACITY_351 (heat_LIB_CAPACITY.f90:321-422): truncated decimals, all with D0
static void rule_351(Rule &r, bool cap) {
#pragma clang fp contract(off)
  const double XG[2] = {-0.5773502691896, 0.5773502691896};
  const double XG1[3] = {0.6666666667, 0.16666666667, 0.16666666667}, XG2[3] = {0.1666666667, 0.66666666667, 0.16666666667};
  const double WGT1[3] = {0.1666666667, 0.16666666667, 0.16666666667};
  const double WGT[2] = {1.0, 1.0};
  r.nn = 6; r.sign = 1.0;
  for (int LZ = 0; LZ < 2; LZ++) {
    const double ZI = XG[LZ];
    for (int L12 = 0; L12 < 3; L12++) {
      const double X1 = XG1[L12], X2 = XG2[L12];
      const double H[6] = {X1 * (1.0 - ZI) * 0.5, X2 * (1.0 - ZI) * 0.5, (1.0 - X1 - X2) * (1.0 - ZI) * 0.5,
                           X1 * (1.0 + ZI) * 0.5, X2 * (1.0 + ZI) * 0.5, (1.0 - X1 - X2) * (1.0 + ZI) * 0.5};
      const double HR[6] = {(1.0 - ZI) * 0.5, 0.0, -(1.0 - ZI) * 0.5, (1.0 + ZI) * 0.5, 0.0, -(1.0 + ZI) * 0.5};
      const double HS[6] = {0.0, (1.0 - ZI) * 0.5, -(1.0 - ZI) * 0.5, 0.0, (1.0 + ZI) * 0.5, -(1.0 + ZI) * 0.5};
      const double HT[6] = {-0.5 * X1, -0.5 * X2, -0.5 * (1.0 - X1 - X2), 0.5 * X1, 0.5 * X2, 0.5 * (1.0 - X1 - X2)};
      if (!cap) r.push(H, HR, HS, HT, WGT1[L12], WGT[LZ], 1.0, 1.0, 1.0, 1.0);
      else r.push(H, HR, HS, HT, WGT[LZ], WGT1[L12], 1.0, 1.0, 1.0, 1.0);
    }
  }
}
// heat_THERMAL_361 (heat_LIB_THERMAL.f90:611-885, XG with D0): DET = -DET, then -CC * ... * DET; heat_CAPACITY_361
// (heat_LIB_CAPACITY.f90:425-542): XG(1) = -0.5773502691896258, a default-real literal
static void rule_361(Rule &r, bool cap) {
#pragma clang fp contract(off)
  const double g = cap ? (double)0.5773502691896258f : 0.5773502691896;
  const double XG[2] = {-g, g}, WGT[2] = {1.0, 1.0};
  r.nn = 8; r.sign = 1.0;
  for (int LX = 0; LX < 2; LX++) {
    const double RI = XG[LX];
    for (int LY = 0; LY < 2; LY++) {
      const double SI = XG[LY];
      for (int LZ = 0; LZ < 2; LZ++) {
        const double TI = XG[LZ];
        const double RP = 1.0 + RI, SP = 1.0 + SI, TP = 1.0 + TI, RM = 1.0 - RI, SM = 1.0 - SI, TM = 1.0 - TI;
        const double H[8] = {0.125 * RM * SM * TM, 0.125 * RP * SM * TM, 0.125 * RP * SP * TM, 0.125 * RM * SP * TM,
                             0.125 * RM * SM * TP, 0.125 * RP * SM * TP, 0.125 * RP * SP * TP, 0.125 * RM * SP * TP};
        const double HR[8] = {-.125 * SM * TM, .125 * SM * TM, .125 * SP * TM, -.125 * SP * TM,
                              -.125 * SM * TP, .125 * SM * TP, .125 * SP * TP, -.125 * SP * TP};
        const double HS[8] = {-.125 * RM * TM, -.125 * RP * TM, .125 * RP * TM, .125 * RM * TM,
                              -.125 * RM * TP, -.125 * RP * TP, .125 * RP * TP, .125 * RM * TP};
        const double HT[8] = {-.125 * RM * SM, -.125 * RP * SM, -.125 * RP * SP, -.125 * RM * SP,
                              .125 * RM * SM, .125 * RP * SM, .125 * RP * SP, .125 * RM * SP};
        r.push(H, HR, HS, HT, WGT[LX], WGT[LY], WGT[LZ], 1.0, 1.0, 1.0);
      }
    }
  }
}
static const double XG3[3] = {-(double)0.7745966692f, 0.0, (double)0.7745966692f};
static const double WGT3[3] = {(double)0.5555555555f, (double)0.8888888888f, (double)0.5555555555f};
// heat_THERMAL_342 (heat_LIB_THERMAL.f90:1853-2021, default-real constants) / heat_CAPACITY_342 (:881-1042): 3 x 3 x 3 collapsed points, derivatives HL1 - HL4, ...; DET = -DET
static void rule_342(Rule &r, bool) {
#pragma clang fp contract(off)
  const double *XG = XG3, *WGT = WGT3;
  r.nn = 10; r.sign = -1.0;
  for (int L3 = 0; L3 < 3; L3++) {
    const double XL3 = XG[L3], X3 = (XL3 + 1.0) * 0.5;
    for (int L2 = 0; L2 < 3; L2++) {
      const double XL2 = XG[L2], X2 = (1.0 - X3) * (XL2 + 1.0) * 0.5;
      for (int L1 = 0; L1 < 3; L1++) {
        const double XL1 = XG[L1], X1 = (1.0 - X2 - X3) * (XL1 + 1.0) * 0.5;
        const double X4 = 1.0 - X1 - X2 - X3;
        const double H[10] = {X1 * (2.0 * X1 - 1.0), X2 * (2.0 * X2 - 1.0), X3 * (2.0 * X3 - 1.0), X4 * (2.0 * X4 - 1.0), 4.0 * X1 * X2,
                              4.0 * X2 * X3, 4.0 * X1 * X3, 4.0 * X1 * X4, 4.0 * X2 * X4, 4.0 * X3 * X4};
        const double HL1[10] = {4.0 * X1 - 1.0, 0.0, 0.0, 0.0, 4.0 * X2, 0.0, 4.0 * X3, 4.0 * X4, 0.0, 0.0};
        const double HL2[10] = {0.0, 4.0 * X2 - 1.0, 0.0, 0.0, 4.0 * X1, 4.0 * X3, 0.0, 0.0, 4.0 * X4, 0.0};
        const double HL3[10] = {0.0, 0.0, 4.0 * X3 - 1.0, 0.0, 0.0, 4.0 * X2, 4.0 * X1, 0.0, 0.0, 4.0 * X4};
        const double HL4[10] = {0.0, 0.0, 0.0, 4.0 * X4 - 1.0, 0.0, 0.0, 0.0, 4.0 * X1, 4.0 * X2, 4.0 * X3};
        double d1[10], d2[10], d3[10];
        for (int i = 0; i < 10; i++) { d1[i] = HL1[i] - HL4[i]; d2[i] = HL2[i] - HL4[i]; d3[i] = HL3[i] - HL4[i]; }
        r.push(H, d1, d2, d3, WGT[L1], WGT[L2], WGT[L3], (1.0 - X3), (1.0 - X2 - X3), 0.125);
      }
    }
  }
}
// heat_THERMAL_352 (heat_LIB_THERMAL.f90:2024-2211) / heat_CAPACITY_352 (:1045-1227): LZ, L2, L1; derivatives HL1 - HL3, HL2 - HL3, HZ
static void rule_352(Rule &r, bool) {
#pragma clang fp contract(off)
  const double *XG = XG3, *WGT = WGT3;
  r.nn = 15; r.sign = 1.0;
  for (int LZ = 0; LZ < 3; LZ++) {
    const double ZI = XG[LZ];
    for (int L2 = 0; L2 < 3; L2++) {
      const double XL2 = XG[L2], X2 = (XL2 + 1.0) * 0.5;
      for (int L1 = 0; L1 < 3; L1++) {
        const double XL1 = XG[L1], X1 = 0.5 * (1.0 - X2) * (XL1 + 1.0);
        const double X3 = 1.0 - X1 - X2;
        const double H[15] = {0.5 * X1 * (2.0 * X1 - 2. - ZI) * (1.0 - ZI), 0.5 * X2 * (2.0 * X2 - 2. - ZI) * (1.0 - ZI),
                              0.5 * X3 * (2.0 * X3 - 2. - ZI) * (1.0 - ZI), 0.5 * X1 * (2.0 * X1 - 2. + ZI) * (1.0 + ZI),
                              0.5 * X2 * (2.0 * X2 - 2. + ZI) * (1.0 + ZI), 0.5 * X3 * (2.0 * X3 - 2. + ZI) * (1.0 + ZI),
                              2.0 * X1 * X2 * (1.0 - ZI), 2.0 * X2 * X3 * (1.0 - ZI), 2.0 * X1 * X3 * (1.0 - ZI),
                              2.0 * X1 * X2 * (1.0 + ZI), 2.0 * X2 * X3 * (1.0 + ZI), 2.0 * X1 * X3 * (1.0 + ZI),
                              X1 * (1.0 - ZI * ZI), X2 * (1.0 - ZI * ZI), X3 * (1.0 - ZI * ZI)};
        const double HL1[15] = {0.5 * (4.0 * X1 - 2. - ZI) * (1.0 - ZI), 0.0, 0.0, 0.5 * (4.0 * X1 - 2. + ZI) * (1.0 + ZI), 0.0, 0.0,
                                2.0 * X2 * (1.0 - ZI), 0.0, 2.0 * X3 * (1.0 - ZI), 2.0 * X2 * (1.0 + ZI), 0.0, 2.0 * X3 * (1.0 + ZI),
                                1.0 - ZI * ZI, 0.0, 0.0};
        const double HL2[15] = {0.0, 0.5 * (4.0 * X2 - 2. - ZI) * (1.0 - ZI), 0.0, 0.0, 0.5 * (4.0 * X2 - 2. + ZI) * (1.0 + ZI), 0.0,
                                2.0 * X1 * (1.0 - ZI), 2.0 * X3 * (1.0 - ZI), 0.0, 2.0 * X1 * (1.0 + ZI), 2.0 * X3 * (1.0 + ZI), 0.0,
                                0.0, 1.0 - ZI * ZI, 0.0};
        const double HL3[15] = {0.0, 0.0, 0.5 * (4.0 * X3 - 2. - ZI) * (1.0 - ZI), 0.0, 0.0, 0.5 * (4.0 * X3 - 2. + ZI) * (1.0 + ZI),
                                0.0, 2.0 * X2 * (1.0 - ZI), 2.0 * X1 * (1.0 - ZI), 0.0, 2.0 * X2 * (1.0 + ZI), 2.0 * X1 * (1.0 + ZI),
                                0.0, 0.0, 1.0 - ZI * ZI};
        const double HZ[15] = {0.5 * X1 * (-2.0 * X1 + 1.0 + 2.0 * ZI), 0.5 * X2 * (-2.0 * X2 + 1.0 + 2.0 * ZI),
                               0.5 * X3 * (-2.0 * X3 + 1.0 + 2.0 * ZI), 0.5 * X1 * (2.0 * X1 - 1.0 + 2.0 * ZI),
                               0.5 * X2 * (2.0 * X2 - 1.0 + 2.0 * ZI), 0.5 * X3 * (2.0 * X3 - 1.0 + 2.0 * ZI),
                               -2.0 * X1 * X2, -2.0 * X2 * X3, -2.0 * X1 * X3, 2.0 * X1 * X2, 2.0 * X2 * X3, 2.0 * X1 * X3,
                               -2.0 * X1 * ZI, -2.0 * X2 * ZI, -2.0 * X3 * ZI};
        double d1[15], d2[15];
        for (int i = 0; i < 15; i++) { d1[i] = HL1[i] - HL3[i]; d2[i] = HL2[i] - HL3[i]; }
        r.push(H, d1, d2, HZ, WGT[L1], WGT[L2], WGT[LZ], (1.0 - X2), 0.25, 1.0);
      }
    }
  }
}
// heat_THERMAL_362 (heat_LIB_THERMAL.f90:2214-): DET = -DET, then -CC * ... * DET; heat_CAPACITY_362 (:1230-1420): WG = ... * DET
static void rule_362(Rule &r, bool) {
#pragma clang fp contract(off)
  const double *XG = XG3, *WGT = WGT3;
  r.nn = 20; r.sign = 1.0;
  for (int LX = 0; LX < 3; LX++) {
    const double RI = XG[LX];
    for (int LY = 0; LY < 3; LY++) {
      const double SI = XG[LY];
      for (int LZ = 0; LZ < 3; LZ++) {
        const double TI = XG[LZ];
        const double RP = 1.0 + RI, SP = 1.0 + SI, TP = 1.0 + TI, RM = 1.0 - RI, SM = 1.0 - SI, TM = 1.0 - TI;
        const double H[20] = {
            -0.125 * RM * SM * TM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM * (2.0 - RI + SI + TI),
            -0.125 * RP * SP * TM * (2.0 - RI - SI + TI), -0.125 * RM * SP * TM * (2.0 + RI - SI + TI),
            -0.125 * RM * SM * TP * (2.0 + RI + SI - TI), -0.125 * RP * SM * TP * (2.0 - RI + SI - TI),
            -0.125 * RP * SP * TP * (2.0 - RI - SI - TI), -0.125 * RM * SP * TP * (2.0 + RI - SI - TI),
            0.25 * (1.0 - RI * RI) * SM * TM, 0.25 * RP * (1.0 - SI * SI) * TM, 0.25 * (1.0 - RI * RI) * SP * TM, 0.25 * RM * (1.0 - SI * SI) * TM,
            0.25 * (1.0 - RI * RI) * SM * TP, 0.25 * RP * (1.0 - SI * SI) * TP, 0.25 * (1.0 - RI * RI) * SP * TP, 0.25 * RM * (1.0 - SI * SI) * TP,
            0.25 * RM * SM * (1.0 - TI * TI), 0.25 * RP * SM * (1.0 - TI * TI), 0.25 * RP * SP * (1.0 - TI * TI), 0.25 * RM * SP * (1.0 - TI * TI)};
        const double HR[20] = {
            -0.125 * RM * SM * TM + 0.125 * SM * TM * (2.0 + RI + SI + TI), +0.125 * RP * SM * TM - 0.125 * SM * TM * (2.0 - RI + SI + TI),
            +0.125 * RP * SP * TM - 0.125 * SP * TM * (2.0 - RI - SI + TI), -0.125 * RM * SP * TM + 0.125 * SP * TM * (2.0 + RI - SI + TI),
            -0.125 * RM * SM * TP + 0.125 * SM * TP * (2.0 + RI + SI - TI), +0.125 * RP * SM * TP - 0.125 * SM * TP * (2.0 - RI + SI - TI),
            +0.125 * RP * SP * TP - 0.125 * SP * TP * (2.0 - RI - SI - TI), -0.125 * RM * SP * TP + 0.125 * SP * TP * (2.0 + RI - SI - TI),
            -0.50 * RI * SM * TM, +0.25 * (1.0 - SI * SI) * TM, -0.50 * RI * SP * TM, -0.25 * (1.0 - SI * SI) * TM,
            -0.50 * RI * SM * TP, +0.25 * (1.0 - SI * SI) * TP, -0.50 * RI * SP * TP, -0.25 * (1.0 - SI * SI) * TP,
            -0.25 * SM * (1.0 - TI * TI), +0.25 * SM * (1.0 - TI * TI), +0.25 * SP * (1.0 - TI * TI), -0.25 * SP * (1.0 - TI * TI)};
        const double HS[20] = {
            -0.125 * RM * SM * TM + 0.125 * RM * TM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM + 0.125 * RP * TM * (2.0 - RI + SI + TI),
            +0.125 * RP * SP * TM - 0.125 * RP * TM * (2.0 - RI - SI + TI), +0.125 * RM * SP * TM - 0.125 * RM * TM * (2.0 + RI - SI + TI),
            -0.125 * RM * SM * TP + 0.125 * RM * TP * (2.0 + RI + SI - TI), -0.125 * RP * SM * TP + 0.125 * RP * TP * (2.0 - RI + SI - TI),
            +0.125 * RP * SP * TP - 0.125 * RP * TP * (2.0 - RI - SI - TI), +0.125 * RM * SP * TP - 0.125 * RM * TP * (2.0 + RI - SI - TI),
            -0.25 * (1.0 - RI * RI) * TM, -0.50 * RP * SI * TM, +0.25 * (1.0 - RI * RI) * TM, -0.50 * RM * SI * TM,
            -0.25 * (1.0 - RI * RI) * TP, -0.50 * RP * SI * TP, +0.25 * (1.0 - RI * RI) * TP, -0.50 * RM * SI * TP,
            -0.25 * RM * (1.0 - TI * TI), -0.25 * RP * (1.0 - TI * TI), +0.25 * RP * (1.0 - TI * TI), +0.25 * RM * (1.0 - TI * TI)};
        const double HT[20] = {
            -0.125 * RM * SM * TM + 0.125 * RM * SM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM + 0.125 * RP * SM * (2.0 - RI + SI + TI),
            -0.125 * RP * SP * TM + 0.125 * RP * SP * (2.0 - RI - SI + TI), -0.125 * RM * SP * TM + 0.125 * RM * SP * (2.0 + RI - SI + TI),
            +0.125 * RM * SM * TP - 0.125 * RM * SM * (2.0 + RI + SI - TI), +0.125 * RP * SM * TP - 0.125 * RP * SM * (2.0 - RI + SI - TI),
            +0.125 * RP * SP * TP - 0.125 * RP * SP * (2.0 - RI - SI - TI), +0.125 * RM * SP * TP - 0.125 * RM * SP * (2.0 + RI - SI - TI),
            -0.25 * (1.0 - RI * RI) * SM, -0.25 * RP * (1.0 - SI * SI), -0.25 * (1.0 - RI * RI) * SP, -0.25 * RM * (1.0 - SI * SI),
            0.25 * (1.0 - RI * RI) * SM, 0.25 * RP * (1.0 - SI * SI), 0.25 * (1.0 - RI * RI) * SP, 0.25 * RM * (1.0 - SI * SI),
            -0.5 * RM * SM * TI, -0.5 * RP * SM * TI, -0.5 * RP * SP * TI, -0.5 * RM * SP * TI};
        r.push(H, HR, HS, HT, WGT[LX], WGT[LY], WGT[LZ], 1.0, 1.0, 1.0);
      }
    }
  }
}
static bool make_rule(int32_t etype, bool cap, Rule &r) {
  switch (etype) {
    case 341: rule_341(r, cap); return true;
    case 342: rule_342(r, cap); return true;
    case 351: rule_351(r, cap); return true;
    case 352: rule_352(r, cap); return true;
    case 361: rule_361(r, cap); return true;
    case 362: rule_362(r, cap); return true;
    default: return false;
  }
}
}  // namespace fxh

// ---- device ---------------------------------------------------------------------------------------------------------------------
#define HEAT_LPE 16  // lanes per element
#define HEAT_BS 64   // lanes per workgroup (one wave)
#define HEAT_EPB (HEAT_BS / HEAT_LPE)

struct HeatRuleDev {  // a Rule on the device
  const double *H, *dR, *dS, *dT, *W;
  double sign;
};
// A material's tables on the device: mblk + moff[3 m + p] is {temp[ntab], funcA[ntab + 1], funcB[ntab + 1]} of property p
// (0 conductivity, 1 specific heat, 2 density), mntab[3 m + p] its ntab.
struct HeatArgs {
  int32_t e0, e1;
  const int32_t *list;  // element ids of the positions [e0, e1) (a colour), or null: the position is the id
  const double *coord;
  const int32_t *conn, *emat;
  const double *temp, *temp0;
  double beta, alfa, dtime;
  int32_t with_cap;
  HeatRuleDev rc, rk;  // conductivity, capacity
  const int32_t *moff, *mntab;
  const double *mblk;
  const int32_t *pos;
  double *D, *AL, *AU, *B;
  double *ss_out, *s0_out;  // element matrices out (fx_heat_element): nothing is scattered
  int32_t *err;
};

// heat_GET_CONDUCTIVITY (heat_LIB_THERMAL.f90:12-40)
__device__ __forceinline__ double heat_get_conductivity(double T, int ntab, const double *__restrict__ blk) {
  const double *temp = blk, *fA = blk + ntab, *fB = fA + ntab + 1;
  double c = fB[0];
  if (ntab > 1) {
    int itab;
    if (T <= temp[0]) itab = 0;
    else {
      itab = ntab;
      for (int k = 0; k < ntab - 1; k++)
        if (T > temp[k] && T <= temp[k + 1]) { itab = k + 1; break; }
    }
    c = fA[itab] * T + fB[itab];
  }
  return c;
}
// heat_GET_CP / heat_GET_DENSITY (heat_LIB_CAPACITY.f90:1424-1477): the intervals are closed on the other side, and ntab == 1 reads
// funcA too.  (A T that no branch takes -- a NaN -- leaves itab unset there; here it takes the last interval.)
__device__ __forceinline__ double heat_get_cp(double T, int ntab, const double *__restrict__ blk) {
  const double *temp = blk, *fA = blk + ntab, *fB = fA + ntab + 1;
  int itab = ntab;
  if (T < temp[0]) itab = 0;
  else if (T >= temp[ntab - 1]) itab = ntab;
  else
    for (int k = 0; k < ntab - 1; k++)
      if (T >= temp[k] && T < temp[k + 1]) { itab = k + 1; break; }
  return fA[itab] * T + fB[itab];
}

// lanes 0..8: XJ(r + 1, c + 1) = sum_i d_r(i) * X_c(i) of point q into J[0..8] (XJ11, XJ12, XJ13, XJ21, ...)
template <int NN>
__device__ __forceinline__ void heat_jacobian_entry(const HeatRuleDev &R, int q, int lane, const double (*X)[NN], double *J) {
  const int r = lane / 3, c = lane % 3;
  const double *d = (r == 0 ? R.dR : (r == 1 ? R.dS : R.dT)) + (size_t)q * NN;
  double s = 0.0;
  for (int i = 0; i < NN; i++) s = s + d[i] * X[c][i];
  J[lane] = s;
}
__device__ __forceinline__ double heat_det(const double *J) {
  return J[0] * J[4] * J[8] + J[1] * J[5] * J[6] + J[2] * J[3] * J[7] - J[2] * J[4] * J[6] - J[1] * J[3] * J[8] - J[0] * J[5] * J[7];
}

// HRZ: the quadratic types' capacity (the diagonal of the consistent matrix scaled to the total: SS(num) * (2 TOTM - TOTD) / TOTD);
// LASTT: heat_CAPACITY_341 evaluates the tables at the LAST node's temperature (its `do I: TEMP = TT(I)`), not at the point's.
template <int NN, int NQ, bool HRZ, bool LASTT>
__global__ __launch_bounds__(HEAT_BS) void k_heat(const HeatArgs a) {
  constexpr int NE = NN * (NN + 1) / 2, NACC = (NE + HEAT_LPE - 1) / HEAT_LPE, NPL = (NN + HEAT_LPE - 1) / HEAT_LPE;
  __shared__ double sX[HEAT_EPB][3][NN], sT[HEAT_EPB][NN], sT0[HEAT_EPB][NN], sJ[HEAT_EPB][12], sB[HEAT_EPB][3][NN], sSS[HEAT_EPB][NE],
      sS0[HEAT_EPB][NN];
  __shared__ int32_t sNode[HEAT_EPB][NN];
  const int le = threadIdx.x / HEAT_LPE, lane = threadIdx.x % HEAT_LPE;
  const int64_t p = (int64_t)a.e0 + (int64_t)blockIdx.x * HEAT_EPB + le;
  const bool valid = p < a.e1;
  const int32_t elem = valid ? (a.list ? a.list[p] : (int32_t)p) : 0;
  int mat = 0;
  if (valid) {
    for (int i = lane; i < NN; i += HEAT_LPE) {
      const int32_t node = a.conn[(size_t)NN * elem + i];
      sNode[le][i] = node;
      for (int k = 0; k < 3; k++) sX[le][k][i] = a.coord[(size_t)3 * (node - 1) + k];
      sT[le][i] = a.temp[node - 1];
      sT0[le][i] = a.temp0 ? a.temp0[node - 1] : 0.0;
    }
    if (a.emat) mat = a.emat[elem] - 1;
  }
  // this lane's entries (i <= j) of the upper triangle, row by row
  int ei[NACC], ej[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) {
    int e = lane + HEAT_LPE * k, i = 0;
    ei[k] = -1; ej[k] = 0;
    if (e < NE) {
      while (e >= NN - i) { e -= NN - i; i++; }
      ei[k] = i; ej[k] = i + e;
    }
  }
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) acc[k] = 0.0;
  __syncthreads();

  // ---- heat_THERMAL_3xx at TEMP ----
  {
    const int ntab = a.mntab[3 * mat];
    const double *blk = a.mblk + a.moff[3 * mat];
    for (int q = 0; q < NQ; q++) {
      if (valid && lane < 9) heat_jacobian_entry<NN>(a.rc, q, lane, sX[le], sJ[le]);
      else if (valid && lane == 9) {
        const double *h = a.rc.H + (size_t)q * NN;
        double t = 0.0;
        for (int i = 0; i < NN; i++) t = t + h[i] * sT[le][i];
        sJ[le][9] = heat_get_conductivity(t, ntab, blk);
      }
      __syncthreads();
      double WG = 0.0;
      if (valid) {
        const double *J = sJ[le];
        const double DET = heat_det(J), CC = J[9];
        const double *w = a.rc.W + (size_t)6 * q;
        WG = a.rc.sign * (CC * w[0] * w[1] * w[2] * DET * w[3] * w[4] * w[5]);
        const double DUM = 1.0 / DET;  // the sign of DET (341, 361, 362 invert -DET) changes the sign of every B, not a product of two
        const double XJI11 = DUM * (J[4] * J[8] - J[5] * J[7]), XJI21 = DUM * (-J[3] * J[8] + J[5] * J[6]),
                     XJI31 = DUM * (J[3] * J[7] - J[4] * J[6]), XJI12 = DUM * (-J[1] * J[8] + J[2] * J[7]),
                     XJI22 = DUM * (J[0] * J[8] - J[2] * J[6]), XJI32 = DUM * (-J[0] * J[7] + J[1] * J[6]),
                     XJI13 = DUM * (J[1] * J[5] - J[2] * J[4]), XJI23 = DUM * (-J[0] * J[5] + J[2] * J[3]),
                     XJI33 = DUM * (J[0] * J[4] - J[1] * J[3]);
        for (int i = lane; i < NN; i += HEAT_LPE) {
          const double hr = a.rc.dR[(size_t)q * NN + i], hs = a.rc.dS[(size_t)q * NN + i], ht = a.rc.dT[(size_t)q * NN + i];
          sB[le][0][i] = XJI11 * hr + XJI12 * hs + XJI13 * ht;
          sB[le][1][i] = XJI21 * hr + XJI22 * hs + XJI23 * ht;
          sB[le][2][i] = XJI31 * hr + XJI32 * hs + XJI33 * ht;
        }
      }
      __syncthreads();
      if (valid) {
#pragma unroll
        for (int k = 0; k < NACC; k++)
          if (ei[k] >= 0) {
            const int i = ei[k], j = ej[k];
            acc[k] = acc[k] + sB[le][0][i] * sB[le][0][j] * WG + sB[le][1][i] * sB[le][1][j] * WG + sB[le][2][i] * sB[le][2][j] * WG;
          }
      }
    }
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < NACC; k++)
      if (ei[k] >= 0) sSS[le][lane + HEAT_LPE * k] = acc[k];
  }

  // ---- heat_CAPACITY_3xx at TEMP0 ----
  if (a.with_cap) {
    const int ntcp = a.mntab[3 * mat + 1], ntrho = a.mntab[3 * mat + 2];
    const double *bcp = a.mblk + a.moff[3 * mat + 1], *brho = a.mblk + a.moff[3 * mat + 2];
    double s0[NPL], TOTD = 0.0, TOTM = 0.0;
#pragma unroll
    for (int k = 0; k < NPL; k++) s0[k] = 0.0;
    for (int q = 0; q < NQ; q++) {
      __syncthreads();  // sJ of the point before (and of the conductivity loop) has been read
      if (valid && lane < 9) heat_jacobian_entry<NN>(a.rk, q, lane, sX[le], sJ[le]);
      else if (valid && lane == 9) {
        const double *h = a.rk.H + (size_t)q * NN;
        double t = 0.0;
        if (LASTT) t = sT0[le][NN - 1];
        else
          for (int i = 0; i < NN; i++) t = t + sT0[le][i] * h[i];
        sJ[le][9] = heat_get_cp(t, ntcp, bcp);
        sJ[le][10] = heat_get_cp(t, ntrho, brho);
      }
      __syncthreads();
      if (valid) {
        const double *J = sJ[le], *w = a.rk.W + (size_t)6 * q, *h = a.rk.H + (size_t)q * NN;
        const double DET = heat_det(J), SPE = J[9], DEN = J[10];
        const double WG = a.rk.sign * (w[0] * w[1] * w[2] * DET * w[3] * w[4] * w[5]);
#pragma unroll
        for (int k = 0; k < NPL; k++) {
          const int i = lane + HEAT_LPE * k;
          if (i < NN) s0[k] = HRZ ? s0[k] + h[i] * h[i] * WG * SPE * DEN : s0[k] + WG * SPE * DEN * h[i];
        }
        if (HRZ && lane == 10) {  // TOTD, TOTM in the routine's order
          for (int j = 0; j < NN; j++)
            for (int j2 = 0; j2 <= j; j2++) {
              const double t = h[j] * h[j2] * WG * SPE * DEN;
              if (j == j2) TOTD = TOTD + t;
              TOTM = TOTM + t;
            }
        }
      }
    }
    __syncthreads();
    if (HRZ && valid && lane == 10) { sJ[le][0] = TOTD; sJ[le][1] = TOTM; }
    __syncthreads();
    if (valid) {
#pragma unroll
      for (int k = 0; k < NPL; k++) {
        const int i = lane + HEAT_LPE * k;
        if (i < NN) sS0[le][i] = HRZ ? s0[k] * (2. * sJ[le][1] - sJ[le][0]) / sJ[le][0] : s0[k];
      }
    }
  }
  __syncthreads();
  if (!valid) return;

  if (a.ss_out) {  // fx_heat_element
    for (int t = lane; t < NN * NN; t += HEAT_LPE) {
      const int i = t / NN, j = t % NN, lo = i < j ? i : j, hi = i < j ? j : i;
      a.ss_out[(size_t)NN * NN * elem + t] = sSS[le][lo * NN - lo * (lo - 1) / 2 + (hi - lo)];
    }
    if (a.with_cap && a.s0_out)
      for (int i = lane; i < NN; i += HEAT_LPE) a.s0_out[(size_t)NN * elem + i] = sS0[le][i];
    return;
  }
  // ---- heat_mat_ass_conductivity.f90:152-177, heat_mat_ass_capacity.f90:148-152 ----
  const int32_t *pos = a.pos + (size_t)NN * NN * elem;
#pragma unroll
  for (int k = 0; k < NACC; k++) {
    if (ei[k] < 0) continue;
    const int i = ei[k], j = ej[k];
    const int32_t ni = sNode[le][i], nj = sNode[le][j];
    const double v = acc[k] * a.beta;
    if (i == j) {
      double d = a.D[ni - 1] + v;
      if (a.with_cap) d = d + sS0[le][i] / a.dtime;
      a.D[ni - 1] = d;
    } else {
      const int32_t p1 = pos[NN * i + j], p2 = pos[NN * j + i];
      if (p1 < 0 || p2 < 0) { atomicExch(a.err, 2); continue; }
      double *x1 = (nj < ni ? a.AL : a.AU) + p1, *x2 = (ni < nj ? a.AL : a.AU) + p2;
      *x1 = *x1 + v;
      *x2 = *x2 + v;
    }
  }
  for (int i = lane; i < NN; i += HEAT_LPE) {
    const int32_t ni = sNode[le][i];
    double r = a.B[ni - 1];
    if (a.alfa != 0.0)
      for (int j = 0; j < NN; j++) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        r = r - sSS[le][lo * NN - lo * (lo - 1) / 2 + (hi - lo)] * sT0[le][j] * a.alfa;
      }
    if (a.with_cap) r = r + sS0[le][i] * sT0[le][i] / a.dtime;
    a.B[ni - 1] = r;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static void heat_bc_free(HeatAsm &h);  // fx_heat_bc.h
static void heat_free(fx_context *c) {
  HeatAsm &h = c->heat;
  heat_bc_free(h);
  for (ElemColors &ec : h.ec) elem_colors_free(ec);
  h.ec.clear();
  dev_free(h.indexL); dev_free(h.itemL); dev_free(h.indexU); dev_free(h.itemU);
  dev_free(h.D); dev_free(h.AL); dev_free(h.AU); dev_free(h.B);
  for (int t = 0; t < 6; t++)
    for (int k = 0; k < 2; k++) dev_free(h.rule[t][k]);
  h.prof_key = 0;
}

// A rule's tables back to back in one device block, uploaded when the slot is still empty (a type's or a face shape's first use);
// the caller slices the block in the order given.
static int upload_tables_once(double **slot, std::initializer_list<const std::vector<double> *> tables) {
  if (*slot) return 0;
  std::vector<double> all;
  for (const std::vector<double> *t : tables) all.insert(all.end(), t->begin(), t->end());
  if (dev_alloc(slot, all.size())) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpy(*slot, all.data(), all.size() * 8, hipMemcpyHostToDevice));
  return 0;
}
static int heat_rule_dev(double **slot, const fxh::Rule &r, HeatRuleDev &d) {
  if (upload_tables_once(slot, {&r.H, &r.dR, &r.dS, &r.dT, &r.W})) return FX_ERROR_RUNTIME;
  const size_t n = (size_t)r.nn * r.nq;
  const double *b = *slot;
  d = HeatRuleDev{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, r.sign};
  return 0;
}
// the two rules of a type on the device, made at the type's first use
static int heat_rules(fx_context *c, int32_t etype, HeatRuleDev &rc, HeatRuleDev &rk) {
  for (int k = 0; k < 2; k++) {
    fxh::Rule r;
    fxh::make_rule(etype, k == 1, r);
    if (heat_rule_dev(&c->heat.rule[c3_type_index(etype)][k], r, k ? rk : rc)) return FX_ERROR_RUNTIME;
  }
  return 0;
}

// k_heat's template arguments by type: the points of heat_THERMAL_3xx / heat_CAPACITY_3xx, HRZ and LASTT as the kernel explains them
template <int ETYPE>
struct HeatEl {
  static constexpr int NN = c3_facts(ETYPE).nn, NQ = NN > 8 ? 27 : (ETYPE == 351 ? 6 : 8);
  static constexpr bool HRZ = NN > 8, LASTT = ETYPE == 341;
};
static void heat_launch(fx_context *c, int32_t etype, dim3 grid, const HeatArgs &a) {  // grid: HEAT_EPB elements per workgroup
  with_solid_type(etype, [&](auto t) {
    using El = HeatEl<decltype(t)::value>;
    hipLaunchKernelGGL((k_heat<El::NN, El::NQ, El::HRZ, El::LASTT>), grid, dim3(HEAT_BS), 0, c->stream, a);
  });
}

// fx_heat_material_view[] as one device block (HeatArgs); need_cap: the capacity tables are read
struct HeatMatsDev {
  int32_t *moff = nullptr, *mntab = nullptr;
  double *mblk = nullptr;
};
static int heat_check_mats(const char *who, int32_t n_mat, const fx_heat_material_view *mats, bool need_cap) {
  if (n_mat < 1 || !mats) return fx_fail(who, FX_ERROR_RUNTIME, "materials missing");
  for (int32_t m = 0; m < n_mat; m++) {
    const fx_heat_table *t[3] = {&mats[m].cond, &mats[m].cp, &mats[m].rho};
    for (int p = 0; p < (need_cap ? 3 : 1); p++) {
      if (t[p]->ntab < 1) return fx_fail(who, FX_ERROR_RUNTIME, "material %d: ntab must be >= 1", (int)m + 1);
      if (!t[p]->temp || !t[p]->funcA || !t[p]->funcB) return fx_fail(who, FX_ERROR_RUNTIME, "material %d: table arrays missing", (int)m + 1);
    }
  }
  return 0;
}
static int heat_upload_mats(fx_context *c, DevScratch &tmp, int32_t n_mat, const fx_heat_material_view *mats, bool need_cap, HeatMatsDev &d) {
  std::vector<int32_t> off((size_t)3 * n_mat, 0), nt((size_t)3 * n_mat, 1);
  std::vector<double> blk;
  for (int32_t m = 0; m < n_mat; m++) {
    const fx_heat_table *t[3] = {&mats[m].cond, &mats[m].cp, &mats[m].rho};
    for (int p = 0; p < 3; p++) {
      off[3 * m + p] = (int32_t)blk.size();
      if (p > 0 && !need_cap) { blk.insert(blk.end(), 5, 0.0); continue; }
      const int n = t[p]->ntab;
      nt[3 * m + p] = n;
      blk.insert(blk.end(), t[p]->temp, t[p]->temp + n);
      blk.insert(blk.end(), t[p]->funcA, t[p]->funcA + n + 1);
      blk.insert(blk.end(), t[p]->funcB, t[p]->funcB + n + 1);
    }
  }
  if (tmp.alloc(&d.moff, off.size()) || tmp.alloc(&d.mntab, nt.size()) || tmp.alloc(&d.mblk, blk.size())) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpy(d.moff, off.data(), off.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.mntab, nt.data(), nt.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.mblk, blk.data(), blk.size() * 8, hipMemcpyHostToDevice));
  return 0;
}

static uint64_t heat_hash_i32(const int32_t *v, int64_t n) {
  constexpr int NCH = 64;
  uint64_t part[NCH];
  parallel_for(NCH, [&](int64_t a, int64_t b) {
    for (int64_t q = a; q < b; q++) {
      uint64_t h = 1469598103934665603ull;
      for (int64_t i = n * q / NCH; i < n * (q + 1) / NCH; i++) h = (h ^ (uint32_t)v[i]) * 1099511628211ull;
      part[q] = h;
    }
  });
  uint64_t key = 1469598103934665603ull;
  for (int q = 0; q < NCH; q++) key = fnv_mix(key, part[q]);
  return key;
}

// The caller's scalar profile on the device, with room for its values: kept while the profile stays the same (checksum).
static int heat_ensure_profile(fx_context *c, const fx_matrix_view *m) {
  HeatAsm &h = c->heat;
  uint64_t key = fnv_mix(fnv_mix(fnv_mix(1469598103934665603ull, (uint64_t)m->NP), (uint64_t)m->NPL), (uint64_t)m->NPU);
  key = fnv_mix(key, heat_hash_i32(m->indexL, (int64_t)m->NP + 1));
  key = fnv_mix(key, heat_hash_i32(m->indexU, (int64_t)m->NP + 1));
  if (m->NPL > 0) key = fnv_mix(key, heat_hash_i32(m->itemL, m->NPL));
  if (m->NPU > 0) key = fnv_mix(key, heat_hash_i32(m->itemU, m->NPU));
  key |= 1;
  if (h.prof_key == key) return 0;
  for (ElemColors &ec : h.ec) dev_free(ec.pos);  // the maps belong to the profile
  dev_free(h.indexL); dev_free(h.itemL); dev_free(h.indexU); dev_free(h.itemU);
  dev_free(h.D); dev_free(h.AL); dev_free(h.AU); dev_free(h.B);
  h.prof_key = 0;
  const size_t np = (size_t)m->NP, npl = (size_t)std::max(m->NPL, 1), npu = (size_t)std::max(m->NPU, 1);
  if (dev_alloc(&h.indexL, np + 1) || dev_alloc(&h.indexU, np + 1) || dev_alloc(&h.itemL, npl) || dev_alloc(&h.itemU, npu) ||
      dev_alloc(&h.D, np) || dev_alloc(&h.AL, npl) || dev_alloc(&h.AU, npu) || dev_alloc(&h.B, np))
    return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpy(h.indexL, m->indexL, (np + 1) * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h.indexU, m->indexU, (np + 1) * 4, hipMemcpyHostToDevice));
  if (m->NPL > 0) HIP_TRY(hipMemcpy(h.itemL, m->itemL, (size_t)m->NPL * 4, hipMemcpyHostToDevice));
  if (m->NPU > 0) HIP_TRY(hipMemcpy(h.itemU, m->itemU, (size_t)m->NPU * 4, hipMemcpyHostToDevice));
  h.NP = m->NP; h.NPL = m->NPL; h.NPU = m->NPU;
  h.prof_key = key;
  h.n_profile++;
  return 0;
}

#include "fx_heat_bc.h"  // the surface terms: kernels, their lists, fx_heat_face

// hecmw_mat_ass_bc (hecmw_mat_ass.f90:292-429) with NDOF = 1 on the caller's arrays, node after node as heat_mat_ass_bc_FIXT calls it
static void heat_ass_bc(const fx_matrix_view *m, double *D, double *AL, double *AU, double *B, int32_t inode, double RHS) {
  B[inode - 1] = RHS;
  D[inode - 1] = 1.0;
  for (int32_t k = m->indexL[inode - 1]; k < m->indexL[inode]; k++) {
    AL[k] = 0.0;
    const int32_t in = m->itemL[k];
    for (int32_t ik = m->indexU[in - 1]; ik < m->indexU[in]; ik++)
      if (m->itemU[ik] == inode) { B[in - 1] = B[in - 1] - AU[ik] * RHS; AU[ik] = 0.0; break; }
  }
  for (int32_t k = m->indexU[inode - 1]; k < m->indexU[inode]; k++) {
    AU[k] = 0.0;
    const int32_t in = m->itemU[k];
    for (int32_t ik = m->indexL[in - 1]; ik < m->indexL[in]; ik++)
      if (m->itemL[ik] == inode) { B[in - 1] = B[in - 1] - AL[ik] * RHS; AL[ik] = 0.0; break; }
  }
}

// fx_heat_assemble_groups (bc null) and fx_heat_assemble_groups_bc: one body, the surface stage between the element kernels and the copy-back
static int heat_assemble(const char *who, fx_context *c, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                         int32_t n_mat, const fx_heat_material_view *mats, const fx_heat_view *heat, const fx_matrix_view *mat,
                         const double *flux, int32_t n_fix, const int32_t *fix_node, const double *fix_val, const fx_heat_bc *bc,
                         float *ms_kernel) {
  if (!c || !heat || !mat) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  if (int rc = check_group_types(who, n_group, groups, SOLID_TYPES_ASCENDING)) return rc;
  if (mat->NDOF != 1) return fx_fail(who, FX_ERROR_UNSUPPORTED, "the heat matrix has NDOF = 1 (got %d)", (int)mat->NDOF);
  const bool cap = heat->dtime > 0.0;
  if (n_node < 1 || !coord) return fx_fail(who, FX_ERROR_RUNTIME, "empty mesh");
  if (mat->NP != n_node) return fx_fail(who, FX_ERROR_RUNTIME, "mesh/profile size mismatch");
  if (!mat->indexL || !mat->indexU || (mat->NPL > 0 && (!mat->itemL || !mat->AL)) || (mat->NPU > 0 && (!mat->itemU || !mat->AU)) || !mat->D ||
      !mat->B)
    return fx_fail(who, FX_ERROR_RUNTIME, "matrix arrays missing");
  if (!heat->temp) return fx_fail(who, FX_ERROR_RUNTIME, "temp missing");
  const double alfa = 1.0 - heat->beta;
  if (!heat->temp0 && (cap || alfa != 0.0)) return fx_fail(who, FX_ERROR_RUNTIME, "temp0 missing");
  if (int rc = heat_check_mats(who, n_mat, mats, cap)) return rc;
  if (n_fix < 0 || (n_fix > 0 && (!fix_node || !fix_val))) return fx_fail(who, FX_ERROR_RUNTIME, "fixed temperatures missing");
  for (int32_t k = 0; k < n_fix; k++)
    if (fix_node[k] < 1 || fix_node[k] > n_node) return fx_fail(who, FX_ERROR_RUNTIME, "fixed node id out of range");
  if (int rc = check_group_elements(who, n_node, n_group, groups, n_mat, false)) return rc;  // (no collapsed hexahedra here)
  if (bc)
    if (int rc = heat_bc_check(who, n_group, groups, bc)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HeatAsm &h = c->heat;
  h.n_calls++;
  if (heat_ensure_profile(c, mat)) return FX_ERROR_RUNTIME;
  // one cache entry per group, by position: a group whose connectivity and type are those of the last call keeps its colours and map
  for (size_t g = (size_t)n_group; g < h.ec.size(); g++) elem_colors_free(h.ec[g]);
  h.ec.resize((size_t)n_group);
  DevScratch tmp;
  HeatMatsDev md;
  double *d_coord = nullptr, *d_temp = nullptr, *d_temp0 = nullptr;
  int32_t *d_err = nullptr;
  const size_t np = (size_t)n_node;
  if (tmp.alloc(&d_coord, 3 * np) || tmp.alloc(&d_temp, np) || tmp.alloc(&d_err, 1)) return FX_ERROR_RUNTIME;
  if (heat->temp0 && tmp.alloc(&d_temp0, np)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(d_coord, coord, 3 * np * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_temp, heat->temp, np * 8, hipMemcpyHostToDevice, c->stream));
  if (heat->temp0) HIP_TRY(hipMemcpyAsync(d_temp0, heat->temp0, np * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(d_err, 0, 4, c->stream));
  if (int rc = heat_upload_mats(c, tmp, n_mat, mats, cap, md)) return rc;
  std::vector<const int32_t *> d_conn, d_emat;
  if (int rc = upload_group_conn(c, tmp, n_group, groups, d_conn, d_emat)) return rc;
  for (int32_t g = 0; g < n_group; g++) {
    const fx_elem_group &G = groups[g];
    ElemColors &ec = h.ec[g];
    if (G.n_elem < 1) { elem_colors_free(ec); continue; }
    const int nn = c3_nodes(G.etype);
    const uint64_t key0 = ec.key;
    const int32_t *order0 = ec.order;
    if (ensure_elem_colors(c, ec, G.n_elem, G.conn, n_node, nn, G.etype)) return FX_ERROR_RUNTIME;
    if (ec.order != order0 || ec.key != key0) h.n_colourings++;
    if (ec.offsets.empty())
      return fx_fail(who, FX_ERROR_RUNTIME, "group %d cannot be coloured (a node in more than 64 elements, or FX_ASM_ATOMIC set)", (int)g + 1);
    if (!ec.pos) {
      if (dev_alloc(&ec.pos, (size_t)nn * nn * G.n_elem)) return FX_ERROR_RUNTIME;
      launch_scatter_map(c, nn, G.n_elem, d_conn[g], h.indexL, h.itemL, h.indexU, h.itemU, ec.pos);
      HIP_TRY(hipGetLastError());
      h.n_maps++;
    }
  }
  if (bc) {
    if (int rc = heat_bc_prepare(c, who, n_node, n_group, groups, bc)) return rc;
    if (!h.ev_surf) HIP_TRY(hipEventCreate(&h.ev_surf));
  }
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  // hecmw_mat_clear, hecmw_mat_clear_b (heat_mat_ass_conductivity.f90:36-37)
  HIP_TRY(hipMemsetAsync(h.D, 0, np * 8, c->stream));
  HIP_TRY(hipMemsetAsync(h.AL, 0, (size_t)std::max(h.NPL, 1) * 8, c->stream));
  HIP_TRY(hipMemsetAsync(h.AU, 0, (size_t)std::max(h.NPU, 1) * 8, c->stream));
  HIP_TRY(hipMemsetAsync(h.B, 0, np * 8, c->stream));
  for (int32_t g = 0; g < n_group; g++) {
    const fx_elem_group &G = groups[g];
    if (G.n_elem < 1) continue;
    const ElemColors &ec = h.ec[g];
    HeatArgs a{};
    if (heat_rules(c, G.etype, a.rc, a.rk)) return FX_ERROR_RUNTIME;
    a.list = ec.order; a.coord = d_coord; a.conn = d_conn[g]; a.emat = d_emat[g]; a.temp = d_temp; a.temp0 = d_temp0;
    a.beta = heat->beta; a.alfa = alfa; a.dtime = heat->dtime; a.with_cap = cap ? 1 : 0;
    a.moff = md.moff; a.mntab = md.mntab; a.mblk = md.mblk; a.pos = ec.pos;
    a.D = h.D; a.AL = h.AL; a.AU = h.AU; a.B = h.B; a.err = d_err;
    for_colour_ranges(ec.offsets, false, HEAT_EPB, [&](dim3 grid, int32_t e0, int32_t e1) {
      a.e0 = e0; a.e1 = e1;
      heat_launch(c, G.etype, grid, a);
    });
  }
  HIP_TRY(hipGetLastError());
  if (bc) {  // heat_mat_ass_bc_DFLUX, _FILM, _RADIATE
    HIP_TRY(hipEventRecord(h.ev_surf, c->stream));
    if (int rc = heat_bc_launch(c, n_group, groups, bc, tmp, d_coord, d_temp, d_err)) return rc;
  }
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  int32_t herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  if (ms_kernel) *ms_kernel = ms;
  if (bc) {
    float ms_e = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_e, c->ev0, h.ev_surf));
    h.elem_us = (int64_t)(1e3 * ms_e);
    h.surf_us = (int64_t)(1e3 * (ms - ms_e));
  }
  if (herr) return fx_fail(who, FX_ERROR_RUNTIME, "###ERROR### : cannot find connectivity (element not covered by the profile)");
  // the result goes to the caller's arrays (fx_solve builds the NDOF = 1 layout from host pointers)
  double *D = const_cast<double *>(mat->D), *AL = const_cast<double *>(mat->AL), *AU = const_cast<double *>(mat->AU),
         *B = const_cast<double *>(mat->B);
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpy(D, h.D, np * 8, hipMemcpyDeviceToHost));
  if (h.NPL > 0) HIP_TRY(hipMemcpy(AL, h.AL, (size_t)h.NPL * 8, hipMemcpyDeviceToHost));
  if (h.NPU > 0) HIP_TRY(hipMemcpy(AU, h.AU, (size_t)h.NPU * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(B, h.B, np * 8, hipMemcpyDeviceToHost));
  h.copy_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  if (flux)  // heat_mat_ass_bc_CFLUX
    for (size_t i = 0; i < np; i++) B[i] = B[i] + flux[i];
  for (int32_t k = 0; k < n_fix; k++) heat_ass_bc(mat, D, AL, AU, B, fix_node[k], fix_val[k]);  // heat_mat_ass_bc_FIXT
  return 0;
}

extern "C" int fx_heat_assemble_groups(fx_context *c, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                                       int32_t n_mat, const fx_heat_material_view *mats, const fx_heat_view *heat, const fx_matrix_view *mat,
                                       const double *flux, int32_t n_fix, const int32_t *fix_node, const double *fix_val, float *ms_kernel) {
  return heat_assemble("fx_heat_assemble_groups", c, n_node, coord, n_group, groups, n_mat, mats, heat, mat, flux, n_fix, fix_node, fix_val,
                       nullptr, ms_kernel);
}
extern "C" int fx_heat_assemble_groups_bc(fx_context *c, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                                          int32_t n_mat, const fx_heat_material_view *mats, const fx_heat_view *heat,
                                          const fx_matrix_view *mat, const double *flux, int32_t n_fix, const int32_t *fix_node,
                                          const double *fix_val, const fx_heat_bc *bc, float *ms_kernel) {
  const char *who = "fx_heat_assemble_groups_bc";
  if (!bc) return fx_fail(who, FX_ERROR_RUNTIME, "bc missing (fx_heat_assemble_groups is the call without surface terms)");
  return heat_assemble(who, c, n_node, coord, n_group, groups, n_mat, mats, heat, mat, flux, n_fix, fix_node, fix_val, bc, ms_kernel);
}

extern "C" int fx_heat_element(fx_context *c, int32_t etype, const double *ecoord, const double *tt, const double *tt0,
                               const fx_heat_material_view *mat, double dtime, double *ss, double *s0) {
  const char *who = "fx_heat_element";
  if (!c || !ecoord || !tt || !mat || !ss) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  const int nn = c3_nodes(etype);
  if (nn == 0) return fx_fail(who, FX_ERROR_UNSUPPORTED, "element type %d not supported on the device (%s)", (int)etype, SOLID_TYPES_ASCENDING);
  const bool cap = dtime > 0.0;
  if (cap && (!tt0 || !s0)) return fx_fail(who, FX_ERROR_RUNTIME, "tt0 and s0 are needed with dtime > 0");
  if (int rc = heat_check_mats(who, 1, mat, cap)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  DevScratch tmp;
  HeatMatsDev md;
  double *d_coord = nullptr, *d_t = nullptr, *d_t0 = nullptr, *d_ss = nullptr, *d_s0 = nullptr;
  int32_t *d_conn = nullptr, *d_err = nullptr;
  if (tmp.alloc(&d_coord, (size_t)3 * nn) || tmp.alloc(&d_t, (size_t)nn) || tmp.alloc(&d_t0, (size_t)nn) || tmp.alloc(&d_ss, (size_t)nn * nn) ||
      tmp.alloc(&d_s0, (size_t)nn) || tmp.alloc(&d_conn, (size_t)nn) || tmp.alloc(&d_err, 1))
    return FX_ERROR_RUNTIME;
  const int32_t conn[20] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20};
  HIP_TRY(hipMemcpy(d_coord, ecoord, (size_t)3 * nn * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_t, tt, (size_t)nn * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_t0, tt0 ? tt0 : tt, (size_t)nn * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_conn, conn, (size_t)nn * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_err, 0, 4));
  if (int rc = heat_upload_mats(c, tmp, 1, mat, cap, md)) return rc;
  HeatArgs a{};
  if (heat_rules(c, etype, a.rc, a.rk)) return FX_ERROR_RUNTIME;
  a.e0 = 0; a.e1 = 1; a.coord = d_coord; a.conn = d_conn; a.temp = d_t; a.temp0 = d_t0;
  a.beta = 1.0; a.alfa = 0.0; a.dtime = dtime; a.with_cap = cap ? 1 : 0;
  a.moff = md.moff; a.mntab = md.mntab; a.mblk = md.mblk; a.ss_out = d_ss; a.s0_out = d_s0; a.err = d_err;
  heat_launch(c, etype, dim3(1), a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(ss, d_ss, (size_t)nn * nn * 8, hipMemcpyDeviceToHost));
  if (cap) HIP_TRY(hipMemcpy(s0, d_s0, (size_t)nn * 8, hipMemcpyDeviceToHost));
  return 0;
}

// out: colourings made, position maps made, profiles uploaded, calls of fx_heat_assemble_groups, microseconds of the last copy-back,
// lanes per element, elements per workgroup, 0
extern "C" int fx_heat_get_stats(fx_context *c, int64_t out[8]) {
  if (!c || !out) return fx_fail("fx_heat_get_stats", FX_ERROR_RUNTIME, "null argument");
  const HeatAsm &h = c->heat;
  const int64_t v[8] = {h.n_colourings, h.n_maps, h.n_profile, h.n_calls, h.copy_us, HEAT_LPE, HEAT_EPB, 0};
  for (int k = 0; k < 8; k++) out[k] = v[k];
  return 0;
}
