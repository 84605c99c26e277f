// Heat conduction, the surface terms of heat_mat_ass_boundary on the device: heat_mat_ass_bc_DFLUX (faces S1.. and the body flux
// BF, without the weld line), heat_mat_ass_bc_FILM and heat_mat_ass_bc_RADIATE for TYPE=341, 342, 351, 352, 361, 362 (included by
// fx_heat.h before its entry points).
//
// What is restated, routine by routine: heat_FILM_3xx (heat_LIB_FILM.f90), heat_RADIATE_3xx (heat_LIB_RADIATE.f90) and
// heat_DFLUX_3xx (heat_LIB_DFLUX.f90) with their own NOD tables, point sets and loop order.  The routines share four face shapes:
// the 3-node triangle (a closed form), the 6-node triangle (3 x 3 collapsed points; the normal is divided by its length and a
// determinant is taken of the result), the 4-node quadrilateral (2 x 2 points) and the 8-node quadrilateral (3 x 3 points);
// heat_DFLUX_352 alone integrates its triangles with a 6-node set collapsed from the 8-node quadrilateral, and its volume with a
// 15-node set collapsed from the 20-node hexahedron.  Every Gauss constant of the three files is a default-real literal (the
// `DATA XG/-0.5773502691896, .../` initialisers too): it reaches the arithmetic as the nearest float32.  The routines differ in
// the order of their products (heat_FILM_351 / _361 / _362 multiply XSUM WGT WGT H(IP) H(JP) HH, the others form WG first); the
// order is kept form by form, and the face kernel is compiled without contraction so that it repeats the routines' roundings.
//
// Lane mapping: HEATF_LPF = 8 lanes per face, 8 faces per workgroup of one wave.  Lane IP < mm owns row IP of TERM1 (mm <= 8
// accumulators), TERM2(IP) or VECT(NOD(IP)); every lane repeats the face's geometry of the point (two sums of mm terms per
// coordinate from LDS), which costs less than exchanging it.  The routines recompute the point's geometry for every (IP, JP);
// here the sums over the points run in the same order per entry with the geometry computed once per point.
// Scatter: a list's faces are elements of mm nodes -- coloured by ensure_elem_colors, mapped by k_scatter_map<mm> -- so the faces
// of one launch share no node, and the launches follow each other in the stream: plain read-modify-write, no atomics, the same
// bits from call to call.  A face that appears twice in a list is two elements on the same nodes: two colours, added twice.
// The body flux is one launch per colour of its own element list (16 lanes per element as k_heat) and writes only B.
#pragma once

namespace fxh {
struct FaceRule {  // one face shape's points: [nq][mm] tables and [nq][3] weights (w1, w2, g)
  int mm = 0, nq = 0;
  std::vector<double> H, d1, d2, W;
  void push(const double *h, const double *a, const double *b, double w1, double w2, double g) {
    H.insert(H.end(), h, h + mm); d1.insert(d1.end(), a, a + mm); d2.insert(d2.end(), b, b + mm);
    W.push_back(w1); W.push_back(w2); W.push_back(g);
    nq++;
  }
};
// the 4-node quadrilateral of heat_FILM_351 / _361 (heat_LIB_FILM.f90:566-608, :937-978), heat_RADIATE_351 / _361, heat_DFLUX_351 / _361
static void face_q4(FaceRule &r) {
#pragma clang fp contract(off)
  const double g = (double)0.5773502691896f;
  const double XG[2] = {-g, g}, WGT[2] = {1.0, 1.0};
  r.mm = 4;
  for (int IG2 = 0; IG2 < 2; IG2++) {
    const double SI = XG[IG2];
    for (int IG1 = 0; IG1 < 2; IG1++) {
      const double RI = XG[IG1];
      const double H[4] = {0.25 * (1.0 - RI) * (1.0 - SI), 0.25 * (1.0 + RI) * (1.0 - SI), 0.25 * (1.0 + RI) * (1.0 + SI),
                           0.25 * (1.0 - RI) * (1.0 + SI)};
      const double HR[4] = {-.25 * (1.0 - SI), .25 * (1.0 - SI), .25 * (1.0 + SI), -.25 * (1.0 + SI)};
      const double HS[4] = {-.25 * (1.0 - RI), -.25 * (1.0 + RI), .25 * (1.0 + RI), .25 * (1.0 - RI)};
      r.push(H, HR, HS, WGT[IG1], WGT[IG2], 1.0);
    }
  }
}
// the 8-node quadrilateral of heat_FILM_352 / _362 (heat_LIB_FILM.f90:719-773, :1078-1139), heat_RADIATE_352 / _362, heat_DFLUX_352 / _362;
// collapsed: the 6-node set of heat_DFLUX_352's triangles (heat_LIB_DFLUX.f90:1296-1351)
static void face_q8(FaceRule &r, bool collapsed) {
#pragma clang fp contract(off)
  const double *XG = XG3, *WGT = WGT3;
  r.mm = collapsed ? 6 : 8;
  for (int IG2 = 0; IG2 < 3; IG2++) {
    const double SI = XG[IG2];
    for (int IG1 = 0; IG1 < 3; IG1++) {
      const double RI = XG[IG1];
      const double RP = 1.0 + RI, SP = 1.0 + SI, RM = 1.0 - RI, SM = 1.0 - SI;
      if (!collapsed) {
        const double H[8] = {0.25 * RM * SM * (-1.0 - RI - SI), 0.25 * RP * SM * (-1.0 + RI - SI), 0.25 * RP * SP * (-1.0 + RI + SI),
                             0.25 * RM * SP * (-1.0 - RI + SI), 0.5 * (1.0 - RI * RI) * (1.0 - SI), 0.5 * (1.0 - SI * SI) * (1.0 + RI),
                             0.5 * (1.0 - RI * RI) * (1.0 + SI), 0.5 * (1.0 - SI * SI) * (1.0 - RI)};
        const double HR[8] = {-.25 * SM * (-1.0 - RI - SI) - 0.25 * RM * SM, .25 * SM * (-1.0 + RI - SI) + 0.25 * RP * SM,
                              .25 * SP * (-1.0 + RI + SI) + 0.25 * RP * SP, -.25 * SP * (-1.0 - RI + SI) - 0.25 * RM * SP,
                              -RI * (1.0 - SI), .5 * (1.0 - SI * SI), -RI * (1.0 + SI), -.5 * (1.0 - SI * SI)};
        const double HS[8] = {-.25 * RM * (-1.0 - RI - SI) - 0.25 * RM * SM, -.25 * RP * (-1.0 + RI - SI) - 0.25 * RP * SM,
                              .25 * RP * (-1.0 + RI + SI) + 0.25 * RP * SP, .25 * RM * (-1.0 - RI + SI) + 0.25 * RM * SP,
                              -.5 * (1.0 - RI * RI), -SI * (1.0 + RI), .5 * (1.0 - RI * RI), -SI * (1.0 - RI)};
        r.push(H, HR, HS, WGT[IG1], WGT[IG2], 1.0);
      } else {
        const double H[6] = {0.25 * RM * SM * (-1.0 - RI - SI), 0.25 * RP * SM * (-1.0 + RI - SI), 0.5 * SP * SI,
                             0.5 * (1.0 - RI * RI) * (1.0 - SI), 0.5 * (1.0 - SI * SI) * (1.0 + RI), 0.5 * (1.0 - SI * SI) * (1.0 - RI)};
        const double HR[6] = {-.25 * SM * (-1.0 - RI - SI) - 0.25 * RM * SM, .25 * SM * (-1.0 + RI - SI) + 0.25 * RP * SM, 0.0,
                              -RI * (1.0 - SI), 0.5 * (1.0 - SI * SI), -0.5 * (1.0 - SI * SI)};
        const double HS[6] = {-.25 * RM * (-1.0 - RI - SI) - 0.25 * RM * SM, -.25 * RP * (-1.0 + RI - SI) - 0.25 * RP * SM,
                              0.5 * (1.0 + 2.0 * SI), -0.5 * (1.0 - RI * RI), -SI * (1.0 + RI), -SI * (1.0 - RI)};
        r.push(H, HR, HS, WGT[IG1], WGT[IG2], 1.0);
      }
    }
  }
}
// the 6-node triangle of heat_FILM_342 / _352 (heat_LIB_FILM.f90:414-495, :785-865), heat_RADIATE_342 / _352, heat_DFLUX_342:
// derivatives HL1 - HL3, HL2 - HL3; g = (1 - X2)
static void face_t6(FaceRule &r) {
#pragma clang fp contract(off)
  const double *XG = XG3, *WGT = WGT3;
  r.mm = 6;
  for (int L2 = 0; L2 < 3; L2++) {
    const double XL2 = XG[L2], X2 = (XL2 + 1.0) * 0.5;
    for (int L1 = 0; L1 < 3; L1++) {
      const double XL1 = XG[L1], X1 = 0.5 * (1.0 - X2) * (XL1 + 1.0);
      const double X3 = 1.0 - X1 - X2;
      const double H[6] = {X1 * (2.0 * X1 - 1.), X2 * (2.0 * X2 - 1.), X3 * (2.0 * X3 - 1.), 4.0 * X1 * X2, 4.0 * X2 * X3, 4.0 * X1 * X3};
      const double HL1[6] = {4.0 * X1 - 1.0, 0.0, 0.0, 4.0 * X2, 0.0, 4.0 * X3};
      const double HL2[6] = {0.0, 4.0 * X2 - 1.0, 0.0, 4.0 * X1, 4.0 * X3, 0.0};
      const double HL3[6] = {0.0, 0.0, 4.0 * X3 - 1.0, 0.0, 4.0 * X2, 4.0 * X1};
      double a[6], b[6];
      for (int i = 0; i < 6; i++) { a[i] = HL1[i] - HL3[i]; b[i] = HL2[i] - HL3[i]; }
      r.push(H, a, b, WGT[L1], WGT[L2], (1.0 - X2));
    }
  }
}
// the volume load of heat_DFLUX_351 (heat_LIB_DFLUX.f90:1071-1139): heat_THERMAL_351's points, but DATA statements without D0
static void rule_351_bf(Rule &r) {
#pragma clang fp contract(off)
  const double g = (double)0.5773502691896f;
  const double XG[2] = {-g, g}, WGT[2] = {1.0, 1.0};
  const double XG1[3] = {(double)0.6666666667f, (double)0.16666666667f, (double)0.16666666667f};
  const double XG2[3] = {(double)0.1666666667f, (double)0.66666666667f, (double)0.16666666667f};
  const double WGT1[3] = {(double)0.1666666667f, (double)0.16666666667f, (double)0.16666666667f};
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
      r.push(H, HR, HS, HT, WGT1[L12], WGT[LZ], 1.0, 1.0, 1.0, 1.0);
    }
  }
}
// the volume load of heat_DFLUX_352 (heat_LIB_DFLUX.f90:1356-1468): 3 x 3 x 3 points of a 15-node set collapsed from the 20-node hexahedron
static void rule_352_bf(Rule &r) {
#pragma clang fp contract(off)
  const double *XG = XG3, *WGT = WGT3;
  r.nn = 15; r.sign = 1.0;
  for (int LX = 0; LX < 3; LX++) {
    const double RI = XG[LX];
    for (int LY = 0; LY < 3; LY++) {
      const double SI = XG[LY];
      for (int LZ = 0; LZ < 3; LZ++) {
        const double TI = XG[LZ];
        const double RP = 1.0 + RI, SP = 1.0 + SI, TP = 1.0 + TI, RM = 1.0 - RI, SM = 1.0 - SI, TM = 1.0 - TI;
        const double H[15] = {-0.125 * RM * SM * TM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM * (2.0 - RI + SI + TI), -0.25 * SP * TM * (1.0 - SI + TI),
                              -0.125 * RM * SM * TP * (2.0 + RI + SI - TI), -0.125 * RP * SM * TP * (2.0 - RI + SI - TI), 0.25 * SP * TP * (SI + TI - 1.0),
                              0.25 * (1.0 - RI * RI) * SM * TM, 0.25 * RP * (1.0 - SI * SI) * TM, 0.25 * RM * (1.0 - SI * SI) * TM,
                              0.25 * (1.0 - RI * RI) * SM * TP, 0.25 * RP * (1.0 - SI * SI) * TP, 0.25 * RM * (1.0 - SI * SI) * TP,
                              0.25 * RM * SM * (1.0 - TI * TI), 0.25 * RP * SM * (1.0 - TI * TI), 0.5 * SP * (1.0 - TI * TI)};
        const double HR[15] = {-0.125 * RM * SM * TM + 0.125 * SM * TM * (2.0 + RI + SI + TI), +0.125 * RP * SM * TM - 0.125 * SM * TM * (2.0 - RI + SI + TI), 0.0,
                               -0.125 * RM * SM * TP + 0.125 * SM * TP * (2.0 + RI + SI - TI), +0.125 * RP * SM * TP - 0.125 * SM * TP * (2.0 - RI + SI - TI), 0.0,
                               -0.50 * RI * SM * TM, +0.25 * (1.0 - SI * SI) * TM, -0.25 * (1.0 - SI * SI) * TM,
                               -0.50 * RI * SM * TP, +0.25 * (1.0 - SI * SI) * TP, -0.25 * (1.0 - SI * SI) * TP,
                               -0.25 * SM * (1.0 - TI * TI), +0.25 * SM * (1.0 - TI * TI), 0.0};
        const double HS[15] = {-0.125 * RM * SM * TM + 0.125 * RM * TM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM + 0.125 * RP * TM * (2.0 - RI + SI + TI),
                               +0.25 * TM * (2.0 * SI - TI),
                               -0.125 * RM * SM * TP + 0.125 * RM * TP * (2.0 + RI + SI - TI), -0.125 * RP * SM * TP + 0.125 * RP * TP * (2.0 - RI + SI - TI),
                               +0.25 * TP * (2.0 * SI + TI),
                               -0.25 * (1.0 - RI * RI) * TM, -0.50 * RP * SI * TM, -0.50 * RM * SI * TM,
                               -0.25 * (1.0 - RI * RI) * TP, -0.50 * RP * SI * TP, -0.50 * RM * SI * TP,
                               -0.25 * RM * (1.0 - TI * TI), -0.25 * RP * (1.0 - TI * TI), +0.50 * (1.0 - TI * TI)};
        const double HT[15] = {-0.125 * RM * SM * TM + 0.125 * RM * SM * (2.0 + RI + SI + TI), -0.125 * RP * SM * TM + 0.125 * RP * SM * (2.0 - RI + SI + TI),
                               +0.25 * SP * (2.0 * TI - SI),
                               +0.125 * RM * SM * TP - 0.125 * RM * SM * (2.0 + RI + SI - TI), +0.125 * RP * SM * TP - 0.125 * RP * SM * (2.0 - RI + SI - TI),
                               +0.25 * SP * (SI + 2.0 * TI),
                               -0.25 * (1.0 - RI * RI) * SM, -0.25 * RP * (1.0 - SI * SI), -0.25 * RM * (1.0 - SI * SI),
                               0.25 * (1.0 - RI * RI) * SM, 0.25 * RP * (1.0 - SI * SI), 0.25 * RM * (1.0 - SI * SI),
                               -0.5 * RM * SM * TI, -0.5 * RP * SM * TI, -SP * TI};
        r.push(H, HR, HS, HT, WGT[LX], WGT[LY], WGT[LZ], 1.0, 1.0, 1.0);
      }
    }
  }
}
// the volume points of heat_DFLUX_<etype>: 341, 342, 361, 362 integrate over the points of heat_CAPACITY_<etype>
static bool make_bf_rule(int32_t etype, Rule &r) {
  if (etype == 351) { rule_351_bf(r); return true; }
  if (etype == 352) { rule_352_bf(r); return true; }
  return make_rule(etype, true, r);
}
}  // namespace fxh

// ---- device ---------------------------------------------------------------------------------------------------------------------
#define HEATF_LPF 8  // lanes per face
#define HEATF_BS 64  // lanes per workgroup (one wave)
#define HEATF_FPB (HEATF_BS / HEATF_LPF)
enum { HEATF_DFLUX = 0, HEATF_FILM = 1, HEATF_RADIATE = 2 };
// the order of the products: the closed form of the 3-node triangle; WG = XSUM w1 w2 CF first (heat_FILM_352's quadrilaterals,
// every heat_RADIATE quadrilateral; heat_DFLUX: XSUM val w1 w2 H); XSUM w1 w2 H(IP) H(JP) HH (heat_FILM_351 / _361 / _362); the
// 6-node triangle's WG = w1 w2 DET (1 - X2) 0.25 CF
enum { HEATF_T3 = 0, HEATF_WG = 1, HEATF_SPLIT = 2, HEATF_T6 = 3 };

struct HeatFaceArgs {
  int32_t e0, e1;
  const int32_t *list;  // face ids of the positions [e0, e1) (a colour), or null: the position is the id
  const int32_t *conn;  // mm node ids per face, in NOD order
  const int32_t *src;   // position of the face in val / sink, or null: the face id
  const double *coord, *temp, *val, *sink;
  double tzero;
  int32_t kind, form, nq;
  const double *H, *d1, *d2, *W;
  const int32_t *pos;
  double *D, *AL, *AU, *B;
  double *t1_out, *t2_out;  // TERM1, TERM2 (or the face's VECT) out (fx_heat_face): nothing is scattered
  int32_t *err;
};

template <int MM>
__global__ __launch_bounds__(HEATF_BS) void k_heat_face(const HeatFaceArgs a) {
#pragma clang fp contract(off)
  __shared__ double sX[HEATF_FPB][3][MM], sT[HEATF_FPB][MM];
  __shared__ int32_t sNode[HEATF_FPB][MM];
  const int lf = threadIdx.x / HEATF_LPF, lane = threadIdx.x % HEATF_LPF;
  const int64_t p = (int64_t)a.e0 + (int64_t)blockIdx.x * HEATF_FPB + lf;
  const bool valid = p < a.e1;
  const int32_t f = valid ? (a.list ? a.list[p] : (int32_t)p) : 0;
  if (valid && lane < MM) {
    const int32_t node = a.conn[(size_t)MM * f + lane];
    sNode[lf][lane] = node;
    for (int k = 0; k < 3; k++) sX[lf][k][lane] = a.coord[(size_t)3 * (node - 1) + k];
    sT[lf][lane] = a.temp ? a.temp[node - 1] : 0.0;
  }
  __syncthreads();
  if (!valid || lane >= MM) return;
  const int32_t s = a.src ? a.src[f] : f;
  const double val = a.val[s], SINK = a.sink ? a.sink[s] : 0.0;
  const double(*X)[MM] = sX[lf];
  const double *T = sT[lf];
  double t1[MM], t2 = 0.0;
#pragma unroll
  for (int j = 0; j < MM; j++) t1[j] = 0.0;

  if (MM == 3) {  // heat_FILM_341 (heat_LIB_FILM.f90:330-346), heat_RADIATE_341, heat_DFLUX_341 (heat_LIB_DFLUX.f90:582-594) and the triangles of 351
    const double AX = X[0][1] - X[0][0], AY = X[1][1] - X[1][0], AZ = X[2][1] - X[2][0];
    const double BX = X[0][2] - X[0][0], BY = X[1][2] - X[1][0], BZ = X[2][2] - X[2][0];
    const double c1 = AY * BZ - AZ * BY, c2 = AZ * BX - AX * BZ, c3 = AX * BY - AY * BX;
    if (a.kind == HEATF_DFLUX) {
      const double AA = 0.5 * sqrt(c1 * c1 + c2 * c2 + c3 * c3);
      t2 = -(val * AA / 3.0);
    } else {
      const double AA = sqrt(c1 * c1 + c2 * c2 + c3 * c3) / 6.0;
      double CF = val;
      if (a.kind == HEATF_RADIATE) {
        const double TT = (T[0] + T[1] + T[2]) / 3.0, T1 = TT - a.tzero, T2 = SINK - a.tzero;
        CF = (T1 + T2) * (T1 * T1 + T2 * T2) * val;
      }
      t2 = -(AA * CF * SINK);
#pragma unroll
      for (int j = 0; j < MM; j++) t1[j] = -(AA * CF / 3.0);
    }
  } else {
    for (int q = 0; q < a.nq; q++) {
      const double *h = a.H + (size_t)q * MM, *d1 = a.d1 + (size_t)q * MM, *d2 = a.d2 + (size_t)q * MM, *w = a.W + (size_t)3 * q;
      double G1X = 0.0, G1Y = 0.0, G1Z = 0.0, G2X = 0.0, G2Y = 0.0, G2Z = 0.0;
#pragma unroll
      for (int i = 0; i < MM; i++) {
        G1X = G1X + d1[i] * X[0][i]; G1Y = G1Y + d1[i] * X[1][i]; G1Z = G1Z + d1[i] * X[2][i];
        G2X = G2X + d2[i] * X[0][i]; G2Y = G2Y + d2[i] * X[1][i]; G2Z = G2Z + d2[i] * X[2][i];
      }
      double G3X = G1Y * G2Z - G1Z * G2Y, G3Y = G1Z * G2X - G1X * G2Z, G3Z = G1X * G2Y - G1Y * G2X;
      const double XSUM = sqrt(G3X * G3X + G3Y * G3Y + G3Z * G3Z);
      double geo = XSUM;  // HEATF_T6: DET of (G1, G2, G3 / XSUM)
      if (a.form == HEATF_T6) {
        G3X = G3X / XSUM; G3Y = G3Y / XSUM; G3Z = G3Z / XSUM;
        geo = G1X * G2Y * G3Z + G1Y * G2Z * G3X + G1Z * G2X * G3Y - G1Z * G2Y * G3X - G1Y * G2X * G3Z - G1X * G2Z * G3Y;
      }
      const double hi = h[lane];
      if (a.kind == HEATF_DFLUX) {
        if (a.form == HEATF_T6) {
          const double WG = w[0] * w[1] * geo * w[2] * 0.25;
          t2 = t2 - val * WG * hi;
        } else {
          t2 = t2 - XSUM * val * w[0] * w[1] * hi;
        }
        continue;
      }
      double CF = val;
      if (a.kind == HEATF_RADIATE) {
        double TT = h[0] * T[0];
#pragma unroll
        for (int i = 1; i < MM; i++) TT = TT + h[i] * T[i];
        const double T1 = TT - a.tzero, T2 = SINK - a.tzero;
        CF = (T1 + T2) * (T1 * T1 + T2 * T2) * val;
      }
      if (a.form == HEATF_SPLIT) {
#pragma unroll
        for (int j = 0; j < MM; j++) t1[j] = t1[j] - XSUM * w[0] * w[1] * hi * h[j] * CF;
        t2 = t2 - XSUM * w[0] * w[1] * hi * CF * SINK;
      } else {
        const double WG = a.form == HEATF_T6 ? w[0] * w[1] * geo * w[2] * 0.25 * CF : XSUM * w[0] * w[1] * CF;
#pragma unroll
        for (int j = 0; j < MM; j++) t1[j] = t1[j] - WG * hi * h[j];
        t2 = t2 - WG * hi * SINK;
      }
    }
  }

  if (a.t2_out) {  // fx_heat_face
    a.t2_out[(size_t)MM * f + lane] = t2;
    if (a.t1_out)
#pragma unroll
      for (int j = 0; j < MM; j++) a.t1_out[(size_t)MM * MM * f + MM * lane + j] = t1[j];
    return;
  }
  const int32_t ni = sNode[lf][lane];
  if (a.kind == HEATF_DFLUX) {  // heat_mat_ass_bc_DFLUX.f90:108-110
    a.B[ni - 1] = a.B[ni - 1] - t2;
    return;
  }
  // heat_mat_ass_bc_FILM.f90:111-139
  const int32_t *pos = a.pos + (size_t)MM * MM * f + MM * lane;
#pragma unroll
  for (int j = 0; j < MM; j++) {
    const int32_t nj = sNode[lf][j];
    if (nj == ni) {
      a.D[ni - 1] = a.D[ni - 1] - t1[j];
      a.B[ni - 1] = a.B[ni - 1] - t2;
    } else {
      const int32_t k = pos[j];
      if (k < 0) { atomicExch(a.err, 2); continue; }
      double *x = (nj > ni ? a.AU : a.AL) + k;
      *x = *x - t1[j];
    }
  }
}

struct HeatBfArgs {
  int32_t e0, e1;
  const int32_t *list;
  const int32_t *conn;  // nn node ids per listed element
  const int32_t *src;
  const double *coord, *val;
  HeatRuleDev r;
  int32_t etype, nq;
  double *B, *v_out;
};

// heat_DFLUX_3xx, LTYPE = 0: lanes 0..8 sum the Jacobian of the point, lane i adds the point's term to VECT(i) (and VECT(i + 16))
template <int NN>
__global__ __launch_bounds__(HEAT_BS) void k_heat_bf(const HeatBfArgs a) {
  constexpr int NPL = (NN + HEAT_LPE - 1) / HEAT_LPE;
  __shared__ double sX[HEAT_EPB][3][NN], sJ[HEAT_EPB][12];
  __shared__ int32_t sNode[HEAT_EPB][NN];
  const int le = threadIdx.x / HEAT_LPE, lane = threadIdx.x % HEAT_LPE;
  const int64_t p = (int64_t)a.e0 + (int64_t)blockIdx.x * HEAT_EPB + le;
  const bool valid = p < a.e1;
  const int32_t e = valid ? (a.list ? a.list[p] : (int32_t)p) : 0;
  if (valid)
    for (int i = lane; i < NN; i += HEAT_LPE) {
      const int32_t node = a.conn[(size_t)NN * e + i];
      sNode[le][i] = node;
      for (int k = 0; k < 3; k++) sX[le][k][i] = a.coord[(size_t)3 * (node - 1) + k];
    }
  const double val = valid ? a.val[a.src ? a.src[e] : e] : 0.0;
  double v[NPL];
#pragma unroll
  for (int k = 0; k < NPL; k++) v[k] = 0.0;
  for (int q = 0; q < a.nq; q++) {
    __syncthreads();  // sX is loaded; sJ of the point before has been read
    if (valid && lane < 9) heat_jacobian_entry<NN>(a.r, q, lane, sX[le], sJ[le]);
    __syncthreads();
    if (!valid) continue;
    const double DET = heat_det(sJ[le]);
    const double *w = a.r.W + (size_t)6 * q, *h = a.r.H + (size_t)q * NN;
#pragma unroll
    for (int k = 0; k < NPL; k++) {
      const int i = lane + HEAT_LPE * k;
      if (i >= NN) continue;
      switch (a.etype) {
        case 341: v[k] = v[k] + val * h[i] * DET * w[4] * w[3] * 0.125; break;  // (1 - X3), (1 - X2 - X3); no DET = -DET here
        case 342: { const double WG = (-DET) * w[0] * w[1] * w[2] * w[3] * w[4] * 0.125; v[k] = v[k] - val * WG * h[i]; } break;
        case 351: { const double WG = w[0] * w[1] * DET; v[k] = v[k] - val * h[i] * WG; } break;
        case 352: { const double WG = DET * w[0] * w[1] * w[2]; v[k] = v[k] - val * WG * h[i]; } break;
        default: { const double WG = w[0] * w[1] * w[2] * DET; v[k] = v[k] - h[i] * WG * val; } break;
      }
    }
  }
  if (!valid) return;
#pragma unroll
  for (int k = 0; k < NPL; k++) {
    const int i = lane + HEAT_LPE * k;
    if (i >= NN) continue;
    if (a.v_out) a.v_out[(size_t)NN * e + i] = v[k];
    else a.B[sNode[le][i] - 1] = a.B[sNode[le][i] - 1] - v[k];
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// The routines' NOD tables are getSubFace's (C3_FACE_NOD), mm of heat_mat_ass_bc_FILM.f90:75-94 is c3_face_nodes.
static int heat_face_form(int kind, int32_t etype, int mm) {
  if (mm == 3) return HEATF_T3;
  if (kind == HEATF_DFLUX) return etype == 342 ? HEATF_T6 : HEATF_WG;
  if (mm == 6) return HEATF_T6;
  if (kind == HEATF_FILM && !(etype == 352)) return HEATF_SPLIT;
  return HEATF_WG;
}

static void heat_face_list_free(HeatFaceList &l) {
  dev_free(l.conn); dev_free(l.src);
  elem_colors_free(l.ec);
  l = HeatFaceList();
}
static void heat_bc_free(HeatAsm &h) {
  for (HeatFaceList &l : h.fl) heat_face_list_free(l);
  h.fl.clear();
  for (int k = 0; k < 4; k++) dev_free(h.frule[k]);
  for (int t = 0; t < 6; t++) dev_free(h.bfrule[t]);
  if (h.ev_surf) { (void)hipEventDestroy(h.ev_surf); h.ev_surf = nullptr; }
}

// the point tables of a face of mm nodes on the device, made at first use
static int heat_face_rule(fx_context *c, int kind, int32_t etype, int mm, HeatFaceArgs &a) {
  a.nq = 0; a.H = a.d1 = a.d2 = a.W = nullptr;
  if (mm == 3) return 0;
  HeatAsm &h = c->heat;
  const int id = mm == 4 ? 0 : (mm == 8 ? 1 : (kind == HEATF_DFLUX && etype == 352 ? 3 : 2));
  fxh::FaceRule r;
  if (id == 0) fxh::face_q4(r);
  else if (id == 2) fxh::face_t6(r);
  else fxh::face_q8(r, id == 3);
  if (upload_tables_once(&h.frule[id], {&r.H, &r.d1, &r.d2, &r.W})) return FX_ERROR_RUNTIME;
  const size_t n = (size_t)r.mm * r.nq;
  const double *b = h.frule[id];
  a.nq = r.nq; a.H = b; a.d1 = b + n; a.d2 = b + 2 * n; a.W = b + 3 * n;
  return 0;
}
static int heat_bf_rule(fx_context *c, int32_t etype, HeatBfArgs &a) {
  fxh::Rule r;
  fxh::make_bf_rule(etype, r);
  a.nq = r.nq; a.etype = etype;
  return heat_rule_dev(&c->heat.bfrule[c3_type_index(etype)], r, a.r);
}

// grid: HEATF_FPB faces, HEAT_EPB elements per workgroup
static void heat_face_launch(fx_context *c, int mm, dim3 grid, const HeatFaceArgs &a) {
  with_face_nodes(mm, [&](auto m) { hipLaunchKernelGGL((k_heat_face<decltype(m)::value>), grid, dim3(HEATF_BS), 0, c->stream, a); });
}
static void heat_bf_launch(fx_context *c, dim3 grid, const HeatBfArgs &a) {
  with_solid_type(a.etype, [&](auto t) { hipLaunchKernelGGL((k_heat_bf<C3El<decltype(t)::value>::NN>), grid, dim3(HEAT_BS), 0, c->stream, a); });
}

static const fx_heat_surface *heat_bc_list(const fx_heat_bc *bc, int kind) {
  return kind == HEATF_DFLUX ? &bc->dflux : (kind == HEATF_FILM ? &bc->film : &bc->radiate);
}
// every index of the three lists, before anything is made or written
static int heat_bc_check(const char *who, int32_t n_group, const fx_elem_group *groups, const fx_heat_bc *bc) {
  static const char *name[3] = {"dflux", "film", "radiate"};
  for (int kind = 0; kind < 3; kind++) {
    const fx_heat_surface &s = *heat_bc_list(bc, kind);
    if (s.n < 0) return fx_fail(who, FX_ERROR_RUNTIME, "%s: n < 0", name[kind]);
    if (s.n == 0) continue;
    if (!s.group || !s.elem || !s.face || !s.val || (kind != HEATF_DFLUX && !s.sink))
      return fx_fail(who, FX_ERROR_RUNTIME, "%s: list arrays missing", name[kind]);
    for (int32_t k = 0; k < s.n; k++) {
      if (int rc = check_list_entry(who, name[kind], k, s.group[k], s.elem[k], n_group, groups)) return rc;
      const fx_elem_group &G = groups[s.group[k]];
      if (s.face[k] < (kind == HEATF_DFLUX ? 0 : 1) || s.face[k] > c3_faces(G.etype))
        return fx_fail(who, FX_ERROR_RUNTIME, "%s, entry %d: TYPE=%d has no face %d", name[kind], (int)k + 1, (int)G.etype, (int)s.face[k]);
    }
  }
  return 0;
}

// The lists of this call as h.fl[(kind * n_group + g) * 3 + shape] (shape 0: the group's triangles, 1: its quadrilaterals, 2: its
// elements under a body flux): a list whose entries and whose group are those of the last call keeps its colouring and map.
static int heat_bc_prepare(fx_context *c, const char *who, int32_t n_node, int32_t n_group, const fx_elem_group *groups, const fx_heat_bc *bc) {
  HeatAsm &h = c->heat;
  const size_t nslot = (size_t)9 * n_group;
  for (size_t k = nslot; k < h.fl.size(); k++) heat_face_list_free(h.fl[k]);
  h.fl.resize(nslot);
  std::vector<std::vector<int32_t>> pick(nslot);
  for (int kind = 0; kind < 3; kind++) {
    const fx_heat_surface &s = *heat_bc_list(bc, kind);
    for (int32_t k = 0; k < s.n; k++) {
      const int32_t et = groups[s.group[k]].etype;
      const int shape = s.face[k] == 0 ? 2 : (c3_face_nodes(et, s.face[k]) % 3 == 0 ? 0 : 1);
      pick[((size_t)kind * n_group + s.group[k]) * 3 + shape].push_back(k);
    }
  }
  for (int kind = 0; kind < 3; kind++) {
    const fx_heat_surface &s = *heat_bc_list(bc, kind);
    for (int32_t g = 0; g < n_group; g++)
      for (int shape = 0; shape < 3; shape++) {
        const size_t slot = ((size_t)kind * n_group + g) * 3 + shape;
        HeatFaceList &l = h.fl[slot];
        const std::vector<int32_t> &idx = pick[slot];
        if (idx.empty()) { heat_face_list_free(l); continue; }
        const fx_elem_group &G = groups[g];
        const int nne = c3_nodes(G.etype), t = c3_type_index(G.etype);
        const int nn = shape == 2 ? nne : c3_face_nodes(G.etype, s.face[idx[0]]);
        uint64_t key = fnv_mix(fnv_mix(fnv_mix(1469598103934665603ull, h.ec[g].key), (uint64_t)G.etype), h.prof_key);
        for (int32_t k : idx) key = fnv_mix(fnv_mix(fnv_mix(key, (uint64_t)k), (uint64_t)s.elem[k]), (uint64_t)s.face[k]);
        key |= 1;
        if (l.key == key && l.n == (int32_t)idx.size() && l.conn && !l.ec.offsets.empty() && (kind == HEATF_DFLUX || l.ec.pos)) continue;
        heat_face_list_free(l);
        l.n = (int32_t)idx.size(); l.nn = nn;
        std::vector<int32_t> conn((size_t)nn * l.n);
        for (int32_t q = 0; q < l.n; q++) {
          const int32_t *en = G.conn + (size_t)nne * s.elem[idx[q]];
          for (int i = 0; i < nn; i++) conn[(size_t)nn * q + i] = shape == 2 ? en[i] : en[C3_FACE_NOD[t][s.face[idx[q]] - 1][i] - 1];
        }
        if (dev_alloc(&l.conn, conn.size()) || dev_alloc(&l.src, idx.size())) return FX_ERROR_RUNTIME;
        HIP_TRY(hipMemcpy(l.conn, conn.data(), conn.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(l.src, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
        if (ensure_elem_colors(c, l.ec, l.n, conn.data(), n_node, nn, G.etype)) return FX_ERROR_RUNTIME;
        h.n_face_colourings++;
        if (l.ec.offsets.empty())
          return fx_fail(who, FX_ERROR_RUNTIME, "a surface list of group %d cannot be coloured (a node in more than 64 of its faces, or FX_ASM_ATOMIC set)",
                         (int)g + 1);
        if (kind != HEATF_DFLUX) {
          if (dev_alloc(&l.ec.pos, (size_t)nn * nn * l.n)) return FX_ERROR_RUNTIME;
          launch_scatter_map(c, nn, l.n, l.conn, h.indexL, h.itemL, h.indexU, h.itemU, l.ec.pos);
          HIP_TRY(hipGetLastError());
          h.n_face_maps++;
        }
        l.key = key;
      }
  }
  return 0;
}

// heat_mat_ass_bc_DFLUX, _FILM, _RADIATE into the device copy of the matrix, in this order, list after list, colour after colour
static int heat_bc_launch(fx_context *c, int32_t n_group, const fx_elem_group *groups, const fx_heat_bc *bc, DevScratch &tmp, const double *d_coord,
                          const double *d_temp, int32_t *d_err) {
  HeatAsm &h = c->heat;
  for (int kind = 0; kind < 3; kind++) {
    const fx_heat_surface &s = *heat_bc_list(bc, kind);
    if (s.n < 1) continue;
    double *d_val = nullptr, *d_sink = nullptr;
    if (tmp.alloc(&d_val, (size_t)s.n)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpyAsync(d_val, s.val, (size_t)s.n * 8, hipMemcpyHostToDevice, c->stream));
    if (kind != HEATF_DFLUX) {
      if (tmp.alloc(&d_sink, (size_t)s.n)) return FX_ERROR_RUNTIME;
      HIP_TRY(hipMemcpyAsync(d_sink, s.sink, (size_t)s.n * 8, hipMemcpyHostToDevice, c->stream));
    }
    for (int32_t g = 0; g < n_group; g++)
      for (int shape = 0; shape < 3; shape++) {
        const HeatFaceList &l = h.fl[((size_t)kind * n_group + g) * 3 + shape];
        if (l.n < 1) continue;
        const std::vector<int32_t> &off = l.ec.offsets;
        if (shape == 2) {
          HeatBfArgs a{};
          if (heat_bf_rule(c, groups[g].etype, a)) return FX_ERROR_RUNTIME;
          a.list = l.ec.order; a.conn = l.conn; a.src = l.src; a.coord = d_coord; a.val = d_val; a.B = h.B;
          for_colour_ranges(off, false, HEAT_EPB, [&](dim3 grid, int32_t e0, int32_t e1) {
            a.e0 = e0; a.e1 = e1;
            heat_bf_launch(c, grid, a);
          });
          continue;
        }
        HeatFaceArgs a{};
        if (heat_face_rule(c, kind, groups[g].etype, l.nn, a)) return FX_ERROR_RUNTIME;
        a.list = l.ec.order; a.conn = l.conn; a.src = l.src; a.coord = d_coord; a.temp = d_temp; a.val = d_val; a.sink = d_sink;
        a.tzero = bc->tzero; a.kind = kind; a.form = heat_face_form(kind, groups[g].etype, l.nn);
        a.pos = l.ec.pos; a.D = h.D; a.AL = h.AL; a.AU = h.AU; a.B = h.B; a.err = d_err;
        for_colour_ranges(off, false, HEATF_FPB, [&](dim3 grid, int32_t e0, int32_t e1) {
          a.e0 = e0; a.e1 = e1;
          heat_face_launch(c, l.nn, grid, a);
        });
      }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int fx_heat_face(fx_context *c, int32_t etype, int32_t kind, int32_t face, const double *ecoord, const double *tt, double val,
                            double sink, double tzero, double *term1, double *term2, int32_t *nsuf, int32_t *mm_out) {
  const char *who = "fx_heat_face";
  if (!c || !ecoord || !term2 || !nsuf || !mm_out) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  const int nn = c3_nodes(etype), t = c3_type_index(etype);
  if (nn == 0) return fx_fail(who, FX_ERROR_UNSUPPORTED, "element type %d not supported on the device (%s)", (int)etype, SOLID_TYPES_ASCENDING);
  if (kind < HEATF_DFLUX || kind > HEATF_RADIATE) return fx_fail(who, FX_ERROR_RUNTIME, "kind must be 0 (dflux), 1 (film) or 2 (radiate)");
  if (face < (kind == HEATF_DFLUX ? 0 : 1) || face > c3_faces(etype)) return fx_fail(who, FX_ERROR_RUNTIME, "TYPE=%d has no face %d", (int)etype, (int)face);
  if (kind != HEATF_DFLUX && !term1) return fx_fail(who, FX_ERROR_RUNTIME, "term1 missing");
  if (kind == HEATF_RADIATE && !tt) return fx_fail(who, FX_ERROR_RUNTIME, "radiate needs the node temperatures");
  HIP_TRY(hipSetDevice(c->device));
  DevScratch tmp;
  const int mm = face == 0 ? nn : c3_face_nodes(etype, face);
  int32_t conn[20];
  for (int i = 0; i < mm; i++) conn[i] = face == 0 ? i + 1 : C3_FACE_NOD[t][face - 1][i];
  double *d_coord = nullptr, *d_t = nullptr, *d_v = nullptr, *d_t1 = nullptr, *d_t2 = nullptr;
  int32_t *d_conn = nullptr, *d_err = nullptr;
  const double vs[2] = {val, sink};
  if (tmp.alloc(&d_coord, (size_t)3 * nn) || tmp.alloc(&d_t, (size_t)nn) || tmp.alloc(&d_v, 2) || tmp.alloc(&d_t1, (size_t)mm * mm) ||
      tmp.alloc(&d_t2, (size_t)mm) || tmp.alloc(&d_conn, (size_t)mm) || tmp.alloc(&d_err, 1))
    return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpy(d_coord, ecoord, (size_t)3 * nn * 8, hipMemcpyHostToDevice));
  if (tt) HIP_TRY(hipMemcpy(d_t, tt, (size_t)nn * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_v, vs, 16, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_conn, conn, (size_t)mm * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_err, 0, 4));
  std::vector<double> t2((size_t)mm);
  if (face == 0) {
    HeatBfArgs a{};
    if (heat_bf_rule(c, etype, a)) return FX_ERROR_RUNTIME;
    a.e0 = 0; a.e1 = 1; a.conn = d_conn; a.coord = d_coord; a.val = d_v; a.v_out = d_t2;
    heat_bf_launch(c, dim3(1), a);
  } else {
    HeatFaceArgs a{};
    if (heat_face_rule(c, kind, etype, mm, a)) return FX_ERROR_RUNTIME;
    a.e0 = 0; a.e1 = 1; a.conn = d_conn; a.coord = d_coord; a.temp = tt ? d_t : nullptr; a.val = d_v; a.sink = d_v + 1;
    a.tzero = tzero; a.kind = kind; a.form = heat_face_form(kind, etype, mm);
    a.t1_out = kind == HEATF_DFLUX ? nullptr : d_t1; a.t2_out = d_t2; a.err = d_err;
    heat_face_launch(c, mm, dim3(1), a);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(t2.data(), d_t2, (size_t)mm * 8, hipMemcpyDeviceToHost));
  if (kind == HEATF_DFLUX) {  // VECT(nn) of the routine: zero off the face
    for (int i = 0; i < nn; i++) term2[i] = 0.0;
    for (int i = 0; i < mm; i++) term2[conn[i] - 1] = t2[i];
  } else {
    for (int i = 0; i < mm; i++) term2[i] = t2[i];
    HIP_TRY(hipMemcpy(term1, d_t1, (size_t)mm * mm * 8, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < mm; i++) nsuf[i] = conn[i];
  *mm_out = mm;
  return 0;
}

// out: face colourings made, face position maps made, microseconds of the element kernels and of the surface kernels of the last
// call of fx_heat_assemble_groups_bc, lanes per face, faces per workgroup, 0, 0
extern "C" int fx_heat_get_bc_stats(fx_context *c, int64_t out[8]) {
  if (!c || !out) return fx_fail("fx_heat_get_bc_stats", FX_ERROR_RUNTIME, "null argument");
  const HeatAsm &h = c->heat;
  const int64_t v[8] = {h.n_face_colourings, h.n_face_maps, h.elem_us, h.surf_us, HEATF_LPF, HEATF_FPB, 0, 0};
  for (int k = 0; k < 8; k++) out[k] = v[k];
  return 0;
}
