// Distributed loads (!DLOAD) on the device: the DLOAD block of fstr_ass_load (fstr_ass_load.f90:138-257) with DL_C3
// (static_LIB_3d.f90:210-377) restated for TYPE=341, 342, 351, 352, 361, 362 (included by fistr_hip.hip before fx_nonlinear_host.h,
// whose begin / update steps rebuild GL through nl_dload_rebuild).
//
// Volume loads (LTYPE 1 BX, 2 BY, 3 BZ, 4 GRAV, 5 CENT) integrate over the element's own rule (NumOfQuadPoints / getQuadPoint /
// getWeight: fx_c3_element.h's point sets; 361 the 8 points of gauss3d2 whatever its elemopt) with getShapeFunc and the determinant
// as :311-316 spells it; the products keep the order of :339-341 and :344-374.  BX / BY / BZ are not multiplied by RHO; GRAV is,
// and every component is scaled by the normalised PARAMS(1:3); CENT is RHO val^2 (x - foot of x on the axis) in all three components.
// Face loads (LTYPE = 10 f) take getSubFace's node tables (element.f90:181-315, C3_FACE_NOD, resolved on the host), the face type's
// rule (gauss2d4: 1 point, gauss2d5: 3, gauss2d2: 4, gauss2d3: 9) and SurfaceNormal's un-normalised cross product (:849-852):
// VECT += val WG H(I) normal(k).  The kernels are compiled without contraction, as the reference's x86 build has none.
//
// Lane mapping.  k_dload_face<MM>: DLF_LPF = 8 lanes per face, 8 faces per one-wave workgroup; lane I < MM owns node I's three sums
// and repeats the point's normal (two sums of MM terms per coordinate from LDS), as k_heat_face does.  k_dload_vol<ETYPE>: L =
// 4 / 16 / 8 / 16 / 8 / 32 lanes per element (341 / 342 / 351 / 352 / 361 / 362), 256 / L elements per workgroup.  Lane q < NQ takes
// quadrature point q (the `ulpe` precedent): its Jacobian, WG = weight DET and, for CENT, the three coefficients, left in LDS; then
// lane I < NN sums PLX, PLY, PLZ of node I over the points in the routine's order.
// Scatter: every entry's vector times its factor (fstr_ass_load.f90:141-142, :254) is added to the 3 n_node vector with fp64 atomics,
// as fx_thermal_load_groups and QFORCE are: equal to rounding from call to call, not bit for bit.  The resident list of the
// nonlinear loop is the exception: its batches are launched colour by colour (dload_colour: no two entries of a launch share a node),
// so the same inputs give the same GL bit for bit, which a cutback relies on.  An entry that appears twice is
// added twice.  The kernels cannot fail (the routine has no check of DET either): they leave the context's error word alone.
#pragma once

#define DLF_LPF 8
#define DLF_BS 64
#define DLF_FPB (DLF_BS / DLF_LPF)
#define DLV_BS 256

// per entry: nodes (MM or NN global ids, 1-based), par (PARAMS(0:6), RHO), held, ltype (volume batches)
struct DloadArgs {
  int32_t n;
  const int32_t *nodes;
  const double *par;
  const uint8_t *held;
  const int32_t *ltype;
  const double *coord, *u1, *u2;  // the configuration: coord (+ u1 (+ u2)), 3 n_node each; u1, u2 may be null
  double factor;
  double *out;       // 3 n_node, added to with atomics; or null:
  double *vect_out;  // 3 MM (3 NN) per entry, DL_C3's VECT without the factor (fx_dload_element)
};

__device__ __forceinline__ double dl_coord(const DloadArgs &a, int32_t node, int k) {
#pragma clang fp contract(off)
  const size_t i = (size_t)3 * (node - 1) + k;
  double x = a.coord[i];
  if (a.u1) x = x + a.u1[i];
  if (a.u2) x = x + a.u2[i];
  return x;
}

// getQuadPoint / getWeight of the face types: gauss2d4 / weight2d4, gauss2d2 / weight2d2, gauss2d5 / weight2d5, gauss2d3 / weight2d3
template <int MM>
__host__ __device__ __forceinline__ void dl_face_point(int q, double &r, double &s, double &w) {
  if (MM == 3) {
    r = s = 0.333333333333333; w = 0.5;
  } else if (MM == 4) {
    const double G = 0.577350269189626;
    r = (q & 1) ? G : -G; s = (q & 2) ? G : -G; w = 1.0;
  } else if (MM == 6) {
    const double A = 0.166666666666667, B = 0.666666666666667;
    r = q == 1 ? B : A; s = q == 2 ? B : A; w = 0.166666666666666;
  } else {
    const double G = 0.774596669241483;
    const int i = q % 3, j = q / 3;
    r = i == 0 ? -G : (i == 1 ? -0.0 : G);
    s = j == 0 ? -G : (j == 1 ? 0.0 : G);
    const int mid = (i == 1) + (j == 1);
    w = mid == 0 ? 0.308641975308642 : (mid == 1 ? 0.493827160493827 : 0.790123456790123);
  }
}
// ShapeFunc_tri3n, _quad4n, _tri6n, _quad8n
template <int MM>
__host__ __device__ __forceinline__ double dl_face_func(int n, double r, double s) {
  if (MM == 3) {
    return n == 0 ? r : (n == 1 ? s : 1.0 - r - s);
  } else if (MM == 4) {
    switch (n) {
      case 0: return 0.25 * (1.0 - r) * (1.0 - s);
      case 1: return 0.25 * (1.0 + r) * (1.0 - s);
      case 2: return 0.25 * (1.0 + r) * (1.0 + s);
      default: return 0.25 * (1.0 - r) * (1.0 + s);
    }
  } else if (MM == 6) {
    const double st = 1.0 - r - s;
    switch (n) {
      case 0: return st * (2.0 * st - 1.0);
      case 1: return r * (2.0 * r - 1.0);
      case 2: return s * (2.0 * s - 1.0);
      case 3: return 4.0 * r * st;
      case 4: return 4.0 * r * s;
      default: return 4.0 * s * st;
    }
  } else {
    const double RP = 1.0 + r, SP = 1.0 + s, RM = 1.0 - r, SM = 1.0 - s;
    switch (n) {
      case 0: return 0.25 * RM * SM * (-1.0 - r - s);
      case 1: return 0.25 * RP * SM * (-1.0 + r - s);
      case 2: return 0.25 * RP * SP * (-1.0 + r + s);
      case 3: return 0.25 * RM * SP * (-1.0 - r + s);
      case 4: return 0.5 * (1.0 - r * r) * (1.0 - s);
      case 5: return 0.5 * (1.0 - s * s) * (1.0 + r);
      case 6: return 0.5 * (1.0 - r * r) * (1.0 + s);
      default: return 0.5 * (1.0 - s * s) * (1.0 - r);
    }
  }
}
// ShapeDeriv_tri3n, _quad4n, _tri6n, _quad8n
template <int MM>
__host__ __device__ __forceinline__ void dl_face_deriv(int n, double r, double s, double &d1, double &d2) {
  if (MM == 3) {
    d1 = n == 0 ? 1.0 : (n == 1 ? 0.0 : -1.0);
    d2 = n == 0 ? 0.0 : (n == 1 ? 1.0 : -1.0);
  } else if (MM == 4) {
    switch (n) {
      case 0: d1 = -0.25 * (1.0 - s); d2 = -0.25 * (1.0 - r); break;
      case 1: d1 = 0.25 * (1.0 - s); d2 = -0.25 * (1.0 + r); break;
      case 2: d1 = 0.25 * (1.0 + s); d2 = 0.25 * (1.0 + r); break;
      default: d1 = -0.25 * (1.0 + s); d2 = 0.25 * (1.0 - r); break;
    }
  } else if (MM == 6) {
    const double st = 1.0 - r - s;
    switch (n) {
      case 0: d1 = 1.0 - 4.0 * st; d2 = 1.0 - 4.0 * st; break;
      case 1: d1 = 4.0 * r - 1.0; d2 = 0.0; break;
      case 2: d1 = 0.0; d2 = 4.0 * s - 1.0; break;
      case 3: d1 = 4.0 * (st - r); d2 = -4.0 * r; break;
      case 4: d1 = 4.0 * s; d2 = 4.0 * r; break;
      default: d1 = -4.0 * s; d2 = 4.0 * (st - s); break;
    }
  } else {
    switch (n) {
      case 0: d1 = .25 * (1.0 - s) * (2.0 * r + s); d2 = .25 * (1.0 - r) * (r + 2.0 * s); break;
      case 1: d1 = .25 * (1.0 - s) * (2.0 * r - s); d2 = -.25 * (1.0 + r) * (r - 2.0 * s); break;
      case 2: d1 = .25 * (1.0 + s) * (2.0 * r + s); d2 = .25 * (1.0 + r) * (r + 2.0 * s); break;
      case 3: d1 = .25 * (1.0 + s) * (2.0 * r - s); d2 = -.25 * (1.0 - r) * (r - 2.0 * s); break;
      case 4: d1 = -r * (1.0 - s); d2 = -0.5 * (1.0 - r * r); break;
      case 5: d1 = 0.5 * (1.0 - s * s); d2 = -s * (1.0 + r); break;
      case 6: d1 = -r * (1.0 + s); d2 = 0.5 * (1.0 - r * r); break;
      default: d1 = -0.5 * (1.0 - s * s); d2 = -s * (1.0 - r); break;
    }
  }
}

// DL_C3's surface branch (static_LIB_3d.f90:276-295) for one face of MM nodes
template <int MM>
__global__ __launch_bounds__(DLF_BS) void k_dload_face(const DloadArgs a) {
#pragma clang fp contract(off)
  constexpr int NQ = MM == 3 ? 1 : (MM == 6 ? 3 : (MM == 4 ? 4 : 9));
  __shared__ double sX[DLF_FPB][3][MM];
  const int lf = threadIdx.x / DLF_LPF, lane = threadIdx.x % DLF_LPF;
  const int64_t f = (int64_t)blockIdx.x * DLF_FPB + lf;
  const bool valid = f < a.n;
  int32_t node = 1;
  if (valid && lane < MM) {
    node = a.nodes[(size_t)MM * f + lane];
    for (int k = 0; k < 3; k++) sX[lf][k][lane] = dl_coord(a, node, k);
  }
  __syncthreads();
  if (!valid || lane >= MM) return;
  const double(*X)[MM] = sX[lf];
  const double val = a.par[(size_t)8 * f];
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  for (int q = 0; q < NQ; q++) {
    double r, s, WG;
    dl_face_point<MM>(q, r, s, WG);
    double g11 = 0.0, g21 = 0.0, g31 = 0.0, g12 = 0.0, g22 = 0.0, g32 = 0.0;  // gderiv = matmul(elecoord, deriv)
#pragma unroll
    for (int i = 0; i < MM; i++) {
      double d1, d2;
      dl_face_deriv<MM>(i, r, s, d1, d2);
      g11 = g11 + X[0][i] * d1; g21 = g21 + X[1][i] * d1; g31 = g31 + X[2][i] * d1;
      g12 = g12 + X[0][i] * d2; g22 = g22 + X[1][i] * d2; g32 = g32 + X[2][i] * d2;
    }
    const double n1 = g21 * g32 - g31 * g22, n2 = g31 * g12 - g11 * g32, n3 = g11 * g22 - g21 * g12;
    const double H = dl_face_func<MM>(lane, r, s);
    v0 = v0 + val * WG * H * n1;
    v1 = v1 + val * WG * H * n2;
    v2 = v2 + val * WG * H * n3;
  }
  if (a.vect_out) {
    double *o = a.vect_out + (size_t)3 * MM * f + 3 * lane;
    o[0] = v0; o[1] = v1; o[2] = v2;
    return;
  }
  const double fac = (a.held && a.held[f]) ? 1.0 : a.factor;
  double *o = a.out + (size_t)3 * (node - 1);
  unsafeAtomicAdd(o + 0, fac * v0);
  unsafeAtomicAdd(o + 1, fac * v1);
  unsafeAtomicAdd(o + 2, fac * v2);
}

template <int ETYPE>
struct DlVol {
  static constexpr int NN = c3_facts(ETYPE).nn;
  static constexpr int NQ = ETYPE == 361 ? 8 : c3_facts(ETYPE).nq;
  static constexpr int L = ETYPE == 341 ? 4 : (ETYPE == 342 ? 16 : (ETYPE == 351 ? 8 : (ETYPE == 352 ? 16 : (ETYPE == 361 ? 8 : 32))));
  static constexpr int EPB = DLV_BS / L;
  static_assert(L >= NN && L >= NQ, "a lane per node and a lane per quadrature point");
};
template <int ETYPE>
__host__ __device__ __forceinline__ void dl_gauss(int q, double &xi, double &et, double &ze, double &w) {
  if (ETYPE == 361) {  // gauss3d2 / weight3d2
    const double G = 0.577350269189626;
    xi = (q & 1) ? G : -G; et = (q & 2) ? G : -G; ze = (q & 4) ? G : -G; w = 1.0;
  } else {
    c3_gauss<ETYPE>(q, xi, et, ze, w);
  }
}
// ShapeFunc_prism6n / ShapeDeriv_prism6n (prism6n.f90), written out here
__device__ __forceinline__ double dl_prism6_func(int n, double xi, double et, double ze) {
  const double a = 1.0 - xi - et;
  switch (n) {
    case 0: return 0.5 * a * (1.0 - ze);
    case 1: return 0.5 * xi * (1.0 - ze);
    case 2: return 0.5 * et * (1.0 - ze);
    case 3: return 0.5 * a * (1.0 + ze);
    case 4: return 0.5 * xi * (1.0 + ze);
    default: return 0.5 * et * (1.0 + ze);
  }
}
__device__ __forceinline__ void dl_prism6_deriv(int n, double xi, double et, double ze, double *d) {
  const double a = 1.0 - xi - et, m = 0.5 * (1.0 - ze), p = 0.5 * (1.0 + ze);
  switch (n) {
    case 0: d[0] = -m; d[1] = -m; d[2] = -0.5 * a; break;
    case 1: d[0] = m; d[1] = 0.0; d[2] = -0.5 * xi; break;
    case 2: d[0] = 0.0; d[1] = m; d[2] = -0.5 * et; break;
    case 3: d[0] = -p; d[1] = -p; d[2] = 0.5 * a; break;
    case 4: d[0] = p; d[1] = 0.0; d[2] = 0.5 * xi; break;
    default: d[0] = 0.0; d[1] = p; d[2] = 0.5 * et; break;
  }
}
template <int ETYPE>
__device__ __forceinline__ double dl_shape_func(int n, double xi, double et, double ze) {
  if (ETYPE == 361) return hex8_shape_func(n, xi, et, ze);
  if (ETYPE == 351) return dl_prism6_func(n, xi, et, ze);
  return c3_shape_func<ETYPE>(n, xi, et, ze);
}

// DL_C3's volume branch (static_LIB_3d.f90:297-375)
template <int ETYPE>
__global__ __launch_bounds__(DLV_BS) void k_dload_vol(const DloadArgs a) {
#pragma clang fp contract(off)
  using V = DlVol<ETYPE>;
  constexpr int NN = V::NN, NQ = V::NQ, L = V::L, EPB = V::EPB;
  __shared__ double sX[EPB][3][NN], sW[EPB][NQ][4];
  __shared__ int32_t sNode[EPB][NN];
  const int le = threadIdx.x / L, lane = threadIdx.x % L;
  const int64_t e = (int64_t)blockIdx.x * EPB + le;
  const bool valid = e < a.n;
  if (valid)
    for (int i = lane; i < NN; i += L) {
      const int32_t node = a.nodes[(size_t)NN * e + i];
      sNode[le][i] = node;
      for (int k = 0; k < 3; k++) sX[le][k][i] = dl_coord(a, node, k);
    }
  __syncthreads();
  const int32_t LTYPE = valid ? a.ltype[e] : 1;
  const double *P = a.par + (size_t)8 * (valid ? e : 0);
  const double val = P[0], RHO = P[7];
  const double(*X)[NN] = sX[le];
  if (valid && lane < NQ) {
    double xi, et, ze, w;
    dl_gauss<ETYPE>(lane, xi, et, ze, w);
    double XJ[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    double dN8[8][3];
    if (ETYPE == 361) hex8_shape_deriv(xi, et, ze, dN8);
#pragma unroll
    for (int n = 0; n < NN; n++) {
      double d[3];
      if (ETYPE == 361) { d[0] = dN8[n & 7][0]; d[1] = dN8[n & 7][1]; d[2] = dN8[n & 7][2]; }
      else if (ETYPE == 351) dl_prism6_deriv(n, xi, et, ze, d);
      else c3_shape_deriv<(ETYPE == 361 || ETYPE == 351) ? 362 : ETYPE>(n, xi, et, ze, d);
#pragma unroll
      for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) XJ[k][j] = XJ[k][j] + X[k][n] * d[j];
    }
    const double DET = XJ[0][0] * XJ[1][1] * XJ[2][2] + XJ[1][0] * XJ[2][1] * XJ[0][2] + XJ[2][0] * XJ[0][1] * XJ[1][2] -
                       XJ[2][0] * XJ[1][1] * XJ[0][2] - XJ[1][0] * XJ[0][1] * XJ[2][2] - XJ[0][0] * XJ[2][1] * XJ[1][2];
    double COEFX = 1.0, COEFY = 1.0, COEFZ = 1.0;
    if (LTYPE == 5) {
      const double AX = P[1], AY = P[2], AZ = P[3], RX = P[4], RY = P[5], RZ = P[6];
      double XCOD = 0.0, YCOD = 0.0, ZCOD = 0.0;
#pragma unroll
      for (int n = 0; n < NN; n++) {
        const double H = dl_shape_func<ETYPE>(n, xi, et, ze);
        XCOD = XCOD + H * X[0][n]; YCOD = YCOD + H * X[1][n]; ZCOD = ZCOD + H * X[2][n];
      }
      const double t = ((XCOD - AX) * RX + (YCOD - AY) * RY + (ZCOD - AZ) * RZ) / (RX * RX + RY * RY + RZ * RZ);
      const double HX = AX + t * RX, HY = AY + t * RY, HZ = AZ + t * RZ;
      const double PHX = XCOD - HX, PHY = YCOD - HY, PHZ = ZCOD - HZ;
      COEFX = RHO * val * val * PHX;
      COEFY = RHO * val * val * PHY;
      COEFZ = RHO * val * val * PHZ;
    }
    double *W = sW[le][lane];
    W[0] = w * DET; W[1] = COEFX; W[2] = COEFY; W[3] = COEFZ;
  }
  __syncthreads();
  if (!valid || lane >= NN) return;
  double PLX = 0.0, PLY = 0.0, PLZ = 0.0;
  for (int q = 0; q < NQ; q++) {
    double xi, et, ze, w;
    dl_gauss<ETYPE>(q, xi, et, ze, w);
    const double H = dl_shape_func<ETYPE>(lane, xi, et, ze);
    const double *W = sW[le][q];
    PLX = PLX + H * W[0] * W[1];
    PLY = PLY + H * W[0] * W[2];
    PLZ = PLZ + H * W[0] * W[3];
  }
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  if (LTYPE == 1) v0 = val * PLX;
  else if (LTYPE == 2) v1 = val * PLY;
  else if (LTYPE == 3) v2 = val * PLZ;
  else if (LTYPE == 4) {
    const double len = sqrt(P[1] * P[1] + P[2] * P[2] + P[3] * P[3]);
    const double VX = P[1] / len, VY = P[2] / len, VZ = P[3] / len;
    v0 = val * PLX * RHO * VX; v1 = val * PLY * RHO * VY; v2 = val * PLZ * RHO * VZ;
  } else { v0 = PLX; v1 = PLY; v2 = PLZ; }
  if (a.vect_out) {
    double *o = a.vect_out + (size_t)3 * NN * e + 3 * lane;
    o[0] = v0; o[1] = v1; o[2] = v2;
    return;
  }
  const double fac = (a.held && a.held[e]) ? 1.0 : a.factor;
  double *o = a.out + (size_t)3 * (sNode[le][lane] - 1);
  if (LTYPE != 2 && LTYPE != 3) unsafeAtomicAdd(o + 0, fac * v0);
  if (LTYPE != 1 && LTYPE != 3) unsafeAtomicAdd(o + 1, fac * v1);
  if (LTYPE != 1 && LTYPE != 2) unsafeAtomicAdd(o + 2, fac * v2);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// getSubFace's node tables are C3_FACE_NOD.  Batch kinds 0..3: faces of DL_FACE_MM[kind] nodes; 4..9: volume entries of the type at
// place kind - 4 of the order 341, 342, 351, 352, 361, 362 (c3_type_at).
static const int DL_FACE_MM[4] = {3, 4, 6, 8};
static int dl_face_kind(int mm) { return mm == 3 ? 0 : (mm == 4 ? 1 : (mm == 6 ? 2 : 3)); }
// 0: not an LTYPE of DL_C3 for this type; else nodes of the entry (face nodes, or the element's)
static int dl_entry_nodes(int32_t etype, int32_t ltype) {
  if (ltype >= 1 && ltype <= 5) return c3_nodes(etype);
  if (ltype >= 10 && ltype % 10 == 0 && ltype / 10 <= c3_faces(etype)) return c3_face_nodes(etype, ltype / 10);
  return 0;
}

static void dload_list_free(DloadList &l) {
  for (DloadBatch &b : l.b) { dev_free(b.nodes); dev_free(b.par); dev_free(b.held); dev_free(b.ltype); }
  l = DloadList();
}

// Every refusal of a list, before anything is made or written.  groups: host views (etype, n_elem, conn, elem_mat).
static int dload_check(const char *who, int32_t n_group, const fx_elem_group *groups, int32_t n_mat, const double *rho, const fx_dload *dl) {
  if (dl->n < 0) return fx_fail(who, FX_ERROR_RUNTIME, "dload: n < 0");
  if (dl->n == 0) return 0;
  if (!dl->group || !dl->elem || !dl->ltype || !dl->params) return fx_fail(who, FX_ERROR_RUNTIME, "dload: list arrays missing");
  for (int32_t k = 0; k < dl->n; k++) {
    const int g = dl->group[k];
    if (int rc = check_list_entry(who, "dload", k, g, dl->elem[k], n_group, groups)) return rc;
    const fx_elem_group &G = groups[g];
    const int32_t lt = dl->ltype[k];
    if (dl_entry_nodes(G.etype, lt) == 0)
      return fx_fail(who, FX_ERROR_RUNTIME, "dload, entry %d (group %d): TYPE=%d has no LTYPE %d", (int)k + 1, g + 1, (int)G.etype, (int)lt);
    const double *p = dl->params + (size_t)7 * k;
    if (lt == 4 || lt == 5) {
      if (!rho || n_mat < 1) return fx_fail(who, FX_ERROR_RUNTIME, "dload, entry %d (group %d): GRAV and CENT need rho", (int)k + 1, g + 1);
      if (G.elem_mat && (G.elem_mat[dl->elem[k]] < 1 || G.elem_mat[dl->elem[k]] > n_mat))
        return fx_fail(who, FX_ERROR_RUNTIME, "dload, entry %d (group %d): material id out of range", (int)k + 1, g + 1);
      const double *d = lt == 4 ? p + 1 : p + 4;
      if (!(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] > 0.0))
        return fx_fail(who, FX_ERROR_RUNTIME, "dload, entry %d (group %d): %s", (int)k + 1, g + 1,
                       lt == 4 ? "GRAV with a zero direction" : "CENT with a zero axis direction");
    }
  }
  return 0;
}

// The entries `idx` of one batch (nn nodes each, node(k, i) the 1-based id of node i of entry k) sorted by colour, stably: greedy,
// every entry takes the lowest colour that none of its nodes holds yet.  -> the colour offsets.  The bit masks grow by 64 colours
// (one word per node) whenever an entry finds none free: a node of a Kuhn mesh with GRAV, CENT and a body force on every
// element around it holds more than 64 entries.
template <class Node>
static std::vector<int32_t> dload_colour(std::vector<int32_t> &idx, int nn, int32_t n_node, Node node) {
  std::vector<std::vector<uint64_t>> used;
  std::vector<int32_t> colour(idx.size());
  int32_t ncol = 0;
  for (size_t q = 0; q < idx.size(); q++) {
    int32_t col = -1;
    for (size_t w = 0; col < 0; w++) {
      if (w == used.size()) used.emplace_back((size_t)n_node, (uint64_t)0);
      uint64_t m = 0;
      for (int i = 0; i < nn; i++) m |= used[w][(size_t)node(idx[q], i) - 1];
      if (~m) col = (int32_t)(64 * w) + __builtin_ctzll(~m);
    }
    for (int i = 0; i < nn; i++) used[(size_t)col / 64][(size_t)node(idx[q], i) - 1] |= (uint64_t)1 << (col % 64);
    colour[q] = col;
    ncol = std::max(ncol, col + 1);
  }
  std::vector<int32_t> off((size_t)ncol + 1, 0), sorted(idx.size());
  for (int32_t col : colour) off[(size_t)col + 1]++;
  for (int32_t k = 0; k < ncol; k++) off[(size_t)k + 1] += off[k];
  std::vector<int32_t> at(off.begin(), off.end() - 1);
  for (size_t q = 0; q < idx.size(); q++) sorted[(size_t)at[colour[q]]++] = idx[q];
  idx.swap(sorted);
  return off;
}

// The checked list as batches on the device: faces by shape (all groups together), volume entries by element type.
// coloured (the resident list of fx_nl_set_dload, n_node its node count): every batch is cut into colours of entries that share no
// node, one launch each, so that a rebuilt GL is the same bit for bit whenever its inputs are (an entry that names a node twice --
// a collapsed hexahedron -- still adds to it twice in one launch).
static int dload_build(fx_context *c, int32_t n_group, const fx_elem_group *groups, int32_t n_mat, const double *rho, const fx_dload *dl,
                       DloadList &L, bool coloured = false, int32_t n_node = 0) {
  dload_list_free(L);
  std::vector<std::vector<int32_t>> pick(10);
  for (int32_t k = 0; k < dl->n; k++) {
    const int32_t et = groups[dl->group[k]].etype, lt = dl->ltype[k];
    if (lt < 10) {
      pick[4 + c3_type_index(et)].push_back(k);
      L.count[lt <= 3 ? 2 : lt - 1]++;
    } else {
      const int mm = c3_face_nodes(et, lt / 10);
      pick[dl_face_kind(mm)].push_back(k);
      L.count[mm % 3 == 0 ? 0 : 1]++;
    }
  }
  for (int kind = 0; kind < 10; kind++) {
    std::vector<int32_t> &idx = pick[kind];
    if (idx.empty()) continue;
    DloadBatch b;
    b.kind = kind; b.n = (int32_t)idx.size();
    const int nn = kind < 4 ? DL_FACE_MM[kind] : c3_nodes(c3_type_at(kind - 4));
    if (coloured)
      b.color_off = dload_colour(idx, nn, n_node, [&](int32_t k, int i) {
        const fx_elem_group &G = groups[dl->group[k]];
        const int32_t *en = G.conn + (size_t)c3_nodes(G.etype) * dl->elem[k];
        return kind < 4 ? en[C3_FACE_NOD[c3_type_index(G.etype)][dl->ltype[k] / 10 - 1][i] - 1] : en[i];
      });
    std::vector<int32_t> nodes((size_t)nn * b.n), lts((size_t)b.n);
    std::vector<double> par((size_t)8 * b.n);
    std::vector<uint8_t> held((size_t)b.n);
    for (int32_t q = 0; q < b.n; q++) {
      const int32_t k = idx[q];
      const fx_elem_group &G = groups[dl->group[k]];
      const int nne = c3_nodes(G.etype), t = c3_type_index(G.etype);
      const int32_t *en = G.conn + (size_t)nne * dl->elem[k];
      for (int i = 0; i < nn; i++) nodes[(size_t)nn * q + i] = kind < 4 ? en[C3_FACE_NOD[t][dl->ltype[k] / 10 - 1][i] - 1] : en[i];
      for (int i = 0; i < 7; i++) par[(size_t)8 * q + i] = dl->params[(size_t)7 * k + i];
      const bool needs_rho = dl->ltype[k] == 4 || dl->ltype[k] == 5;  // dload_check has validated the material id of exactly these
      par[(size_t)8 * q + 7] = needs_rho ? rho[G.elem_mat ? G.elem_mat[dl->elem[k]] - 1 : 0] : 0.0;
      held[q] = dl->held ? dl->held[k] : 0;
      lts[q] = dl->ltype[k];
    }
    L.b.push_back(b);
    DloadBatch &d = L.b.back();
    if (dev_alloc(&d.nodes, nodes.size()) || dev_alloc(&d.par, par.size()) || dev_alloc(&d.held, held.size()) || dev_alloc(&d.ltype, lts.size()))
      return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpy(d.nodes, nodes.data(), nodes.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.par, par.data(), par.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.held, held.data(), held.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.ltype, lts.data(), lts.size() * 4, hipMemcpyHostToDevice));
  }
  return 0;
}

// The entries e0 .. e1 of a batch in one launch
static void dload_launch_range(fx_context *c, const DloadBatch &b, DloadArgs a, int32_t e0, int32_t e1) {
  const int32_t n = e1 - e0;
  if (n <= 0) return;
  const int nn = b.kind < 4 ? DL_FACE_MM[b.kind] : c3_nodes(c3_type_at(b.kind - 4));
  a.n = n; a.nodes = b.nodes + (size_t)nn * e0; a.par = b.par + (size_t)8 * e0; a.held = b.held + e0; a.ltype = b.ltype + e0;
  if (b.kind < 4) {
    const dim3 grid((unsigned)((n + DLF_FPB - 1) / DLF_FPB));
    with_face_nodes(DL_FACE_MM[b.kind], [&](auto m) { hipLaunchKernelGGL((k_dload_face<decltype(m)::value>), grid, dim3(DLF_BS), 0, c->stream, a); });
    return;
  }
  with_solid_type(c3_type_at(b.kind - 4), [&](auto t) {
    constexpr int T = decltype(t)::value, EPB = DlVol<T>::EPB;
    hipLaunchKernelGGL((k_dload_vol<T>), dim3((unsigned)((n + EPB - 1) / EPB)), dim3(DLV_BS), 0, c->stream, a);
  });
}
// One launch, or one per colour of a coloured batch
static void dload_launch_batch(fx_context *c, const DloadBatch &b, const DloadArgs &a) {
  if (b.color_off.empty()) { dload_launch_range(c, b, a, 0, b.n); return; }
  for (size_t k = 0; k + 1 < b.color_off.size(); k++) dload_launch_range(c, b, a, b.color_off[k], b.color_off[k + 1]);
}
// Every batch of the list on the context's stream, the faces first; ev_mid (may be null) is recorded between the two families.
static int dload_launch(fx_context *c, const DloadList &L, const DloadArgs &a, hipEvent_t ev_mid) {
  for (const DloadBatch &b : L.b)
    if (b.kind < 4) dload_launch_batch(c, b, a);
  if (ev_mid) HIP_TRY(hipEventRecord(ev_mid, c->stream));
  for (const DloadBatch &b : L.b)
    if (b.kind >= 4) dload_launch_batch(c, b, a);
  HIP_TRY(hipGetLastError());
  return 0;
}
static int dload_single_rank(const char *who, const fx_context *c) {
  if (c->nranks > 1 || c->view_petot > 1)
    return fx_fail(who, FX_ERROR_UNSUPPORTED, "distributed loads on a decomposed mesh are not served (fstr_ass_load exchanges GL with hecmw_update_3_R)");
  return 0;
}
static int dload_times(fx_context *c, hipEvent_t e0, hipEvent_t mid, hipEvent_t e1) {
  float f = 0.f, v = 0.f;
  HIP_TRY(hipEventElapsedTime(&f, e0, mid));
  HIP_TRY(hipEventElapsedTime(&v, mid, e1));
  c->dload.face_us = (int64_t)(1000.0 * f + 0.5);
  c->dload.vol_us = (int64_t)(1000.0 * v + 0.5);
  return 0;
}

// The device part of fx_dload_groups: uploads, the kernels between the context's events, the result into `out` (host).  The stream
// is idle when it returns, whatever it returns: `out` and the scratch arrays may be released.
static int dload_groups_run(fx_context *c, const DloadList &L, size_t np3, const double *coord, const double *disp, double factor,
                            const double *load, double *out) {
  DloadCtx &dc = c->dload;
  DevScratch tmp;
  double *d_coord = nullptr, *d_disp = nullptr, *d_out = nullptr;
  if (tmp.alloc(&d_coord, np3) || tmp.alloc(&d_out, np3) || (disp && tmp.alloc(&d_disp, np3))) return FX_ERROR_RUNTIME;
  int rc = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(d_coord, coord, np3 * 8, hipMemcpyHostToDevice, c->stream));
    if (disp) HIP_TRY(hipMemcpyAsync(d_disp, disp, np3 * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_out, load, np3 * 8, hipMemcpyHostToDevice, c->stream));
    DloadArgs a{};
    a.coord = d_coord; a.u1 = d_disp; a.factor = factor; a.out = d_out;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    if (int e = dload_launch(c, L, a, dc.ev_mid)) return e;
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipMemcpyAsync(out, d_out, np3 * 8, hipMemcpyDeviceToHost, c->stream));
    return 0;
  }();
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fx_fail("fx_dload_groups", FX_ERROR_RUNTIME, "hipStreamSynchronize failed");
  if (!rc) rc = dload_times(c, c->ev0, dc.ev_mid, c->ev1);
  return rc;
}
static void dload_list_free_keep_counts(DloadList &L, DloadCtx &dc) {
  for (int k = 0; k < 5; k++) dc.count[k] = L.count[k];
  dload_list_free(L);
}

extern "C" int fx_dload_groups(fx_context *c, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups, int32_t n_mat,
                               const double *rho, const fx_dload *dl, double factor, const double *disp, double *load_inout, float *ms_kernel) {
  const char *who = "fx_dload_groups";
  if (!c || !dl || !load_inout) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  if (n_group < 1 || !groups) return fx_fail(who, FX_ERROR_RUNTIME, "n_group must be >= 1");
  std::vector<fx_elem_group> gv(groups, groups + n_group);
  if (!rho)
    for (fx_elem_group &G : gv) G.elem_mat = nullptr;
  if (int rc = check_groups(who, n_node, coord, n_group, gv.data(), rho ? n_mat : 1, true, true)) return rc;  // (elemopt is not read)
  if (int rc = dload_single_rank(who, c)) return rc;
  if (int rc = dload_check(who, n_group, gv.data(), n_mat, rho, dl)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  DloadCtx &dc = c->dload;
  if (!dc.ev_mid) HIP_TRY(hipEventCreate(&dc.ev_mid));
  DloadList L;  // lives for this call: nothing would reuse it
  int rc = dload_build(c, n_group, gv.data(), n_mat, rho, dl, L);
  const size_t np3 = (size_t)3 * n_node;
  std::vector<double> out(np3);  // the caller's vector changes only when everything went well
  if (!rc) rc = dload_groups_run(c, L, np3, coord, disp, factor, load_inout, out.data());
  dload_list_free_keep_counts(L, dc);
  if (rc) return rc;
  if (ms_kernel) *ms_kernel = 1.0e-3f * (float)(dc.face_us + dc.vol_us);
  memcpy(load_inout, out.data(), np3 * 8);
  return 0;
}

extern "C" int fx_dload_element(fx_context *c, int32_t etype, int32_t ltype, const double *ecoord, double rho, const double *params, double *vect) {
  const char *who = "fx_dload_element";
  if (!c || !ecoord || !params || !vect) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  const int nn = c3_nodes(etype), t = c3_type_index(etype);
  if (nn == 0) return fx_fail(who, FX_ERROR_UNSUPPORTED, "element type %d not supported on the device (%s)", (int)etype, SOLID_TYPES_ASCENDING);
  std::vector<int32_t> conn((size_t)nn);
  for (int i = 0; i < nn; i++) conn[i] = i + 1;
  const fx_elem_group G = {etype, 0, 1, conn.data(), nullptr};
  const int32_t zero = 0;
  const fx_dload dl = {1, &zero, &zero, &ltype, params, nullptr};
  if (int rc = dload_check(who, 1, &G, 1, &rho, &dl)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  DloadList L;
  if (int rc = dload_build(c, 1, &G, 1, &rho, &dl, L)) { dload_list_free(L); return rc; }
  const int mm = dl_entry_nodes(etype, ltype);
  double *d_coord = nullptr, *d_v = nullptr;
  int rc = 0;
  std::vector<double> v((size_t)3 * mm);
  if (dev_alloc(&d_coord, (size_t)3 * nn) || dev_alloc(&d_v, (size_t)3 * mm)) rc = FX_ERROR_RUNTIME;
  if (!rc && hipMemcpy(d_coord, ecoord, (size_t)3 * nn * 8, hipMemcpyHostToDevice) != hipSuccess) rc = FX_ERROR_RUNTIME;
  if (!rc) {
    DloadArgs a{};
    a.coord = d_coord; a.factor = 1.0; a.vect_out = d_v;
    rc = dload_launch(c, L, a, nullptr);
  }
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = FX_ERROR_RUNTIME;
  if (!rc && hipMemcpy(v.data(), d_v, v.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FX_ERROR_RUNTIME;
  dev_free(d_coord); dev_free(d_v);
  dload_list_free(L);
  if (rc) return fx_fail(who, FX_ERROR_RUNTIME, "device error");
  for (int i = 0; i < 3 * nn; i++) vect[i] = 0.0;  // VECT(1:NSIZE) = 0 (:273-274)
  for (int i = 0; i < mm; i++) {
    const int node = ltype >= 10 ? C3_FACE_NOD[t][ltype / 10 - 1][i] - 1 : i;
    for (int k = 0; k < 3; k++) vect[3 * node + k] = v[(size_t)3 * i + k];
  }
  return 0;
}

// out: entries on triangles, on quadrilaterals, BX / BY / BZ entries, GRAV entries, CENT entries of the last list built,
// microseconds of the face kernels and of the volume kernels of the last fx_dload_groups, lanes per face
extern "C" int fx_dload_get_stats(fx_context *c, int64_t out[8]) {
  if (!c || !out) return fx_fail("fx_dload_get_stats", FX_ERROR_RUNTIME, "null argument");
  const DloadCtx &d = c->dload;
  const int64_t v[8] = {d.count[0], d.count[1], d.count[2], d.count[3], d.count[4], d.face_us, d.vol_us, DLF_LPF};
  for (int k = 0; k < 8; k++) out[k] = v[k];
  return 0;
}
static void dload_free(fx_context *c) {
  if (c->dload.ev_mid) { (void)hipEventDestroy(c->dload.ev_mid); c->dload.ev_mid = nullptr; }
}

// ---- the nonlinear loop -------------------------------------------------------------------------------------------------------------
static int nl_parts_to_host(const NlDev &n, bool with_emat, std::vector<std::vector<int32_t>> &conn,
                            std::vector<std::vector<int32_t>> &emat);  // fx_nonlinear_host.h
static void nl_dload_free(NlDev &n) {
  dload_list_free(n.dl.list);
  dev_free(n.dl.nodal);
  n.dl = NlDev::Dload();
}
// GL = nodal part + factor DLOAD on coord (+ unode (+ dunode)): fstr_ass_load.f90:64-257 with the nodal part kept aside.
// begin: GL holds the nodal load just uploaded and becomes the nodal part; the configuration is coord + unode when the load follows.
// Otherwise (fstr_solve_NonLinear.f90:103, follower only) the configuration is coord + unode + dunode.
static int nl_dload_rebuild(fx_context *c, bool begin) {
  NlDev &n = c->nl;
  const size_t np3 = (size_t)3 * c->A.NP;
  if (begin) HIP_TRY(hipMemcpyAsync(n.dl.nodal, n.GL, np3 * 8, hipMemcpyDeviceToDevice, c->stream));
  else HIP_TRY(hipMemcpyAsync(n.GL, n.dl.nodal, np3 * 8, hipMemcpyDeviceToDevice, c->stream));
  DloadArgs a{};
  a.coord = n.coord;
  a.u1 = n.dl.follow ? n.unode : nullptr;
  a.u2 = n.dl.follow && !begin ? n.dunode : nullptr;
  a.factor = n.dl.factor; a.out = n.GL;
  return dload_launch(c, n.dl.list, a, nullptr);
}

extern "C" int fx_nl_set_dload(fx_context *c, int32_t n_mat, const double *rho, const fx_dload *dl, int follow) {
  const char *who = "fx_nl_set_dload";
  if (!c) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->nl.ready) return fx_fail(who, FX_ERROR_RUNTIME, "call fx_nl_init first");
  NlDev &n = c->nl;
  if (!dl) { nl_dload_free(n); return 0; }
  if (int rc = dload_single_rank(who, c)) return rc;
  // the parts' connectivity and material ids back on the host: the list is resolved to node ids once
  std::vector<std::vector<int32_t>> conn, emat;
  if (int rc = nl_parts_to_host(n, rho != nullptr, conn, emat)) return rc;
  // the group table in the caller's numbering: an empty group has no part, and keeps its place with no element
  std::vector<fx_elem_group> gv;
  for (size_t g = 0; g < n.group_part.size(); g++) {
    const int32_t p = n.group_part[g];
    if (p < 0) gv.push_back({n.group_etype[g], 2, 0, nullptr, nullptr});
    else gv.push_back({n.parts[p].etype, 2, n.parts[p].n_elem, conn[p].data(), emat[p].empty() ? nullptr : emat[p].data()});
  }
  if (int rc = dload_check(who, (int32_t)gv.size(), gv.data(), n_mat, rho, dl)) return rc;
  DloadList L;
  double *nodal = nullptr;
  int rc = dload_build(c, (int32_t)gv.size(), gv.data(), n_mat, rho, dl, L, true, (int32_t)c->A.NP);  // coloured: GL is rebuilt, not summed up
  if (!rc && dev_alloc(&nodal, (size_t)3 * c->A.NP)) rc = FX_ERROR_RUNTIME;
  if (!rc && hipMemsetAsync(nodal, 0, (size_t)3 * c->A.NP * 8, c->stream) != hipSuccess)
    rc = fx_fail(who, FX_ERROR_RUNTIME, "hipMemsetAsync failed");
  if (rc) { dload_list_free(L); dev_free(nodal); return rc; }  // the context keeps the list it had
  const double factor = n.dl.factor;
  nl_dload_free(n);
  n.dl.on = true; n.dl.follow = follow != 0; n.dl.factor = factor; n.dl.list = L; n.dl.nodal = nodal;
  for (int k = 0; k < 5; k++) c->dload.count[k] = L.count[k];
  return 0;
}
extern "C" int fx_nl_set_dload_factor(fx_context *c, double factor) {
  if (!c) return fx_fail("fx_nl_set_dload_factor", FX_ERROR_RUNTIME, "null argument");
  if (!c->nl.ready) return fx_fail("fx_nl_set_dload_factor", FX_ERROR_RUNTIME, "call fx_nl_init first");
  c->nl.dl.factor = factor;
  return 0;
}
extern "C" int fx_nl_get_load(fx_context *c, double *GL) {
  if (!c || !GL) return fx_fail("fx_nl_get_load", FX_ERROR_RUNTIME, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->nl.ready) return fx_fail("fx_nl_get_load", FX_ERROR_RUNTIME, "call fx_nl_init first");
  HIP_TRY(hipMemcpyAsync(GL, c->nl.GL, (size_t)3 * c->A.NP * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
