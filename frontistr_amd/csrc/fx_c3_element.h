// What the kernels and the host know about the solid element types, in one place: the table of nodes, quadrature points
// and lanes per element (TYPE=361, 341, 342, 351, 352, 362), their faces (host), quadrature and shape-function derivatives of the five types
// that STF_C3 (static_LIB_3d.f90:47-205) and UPDATE_C3 (:516-837) serve, and the small steps every element kernel repeats:
// determinant and inverse of the Jacobian, strain from the displacement gradient, isotropic stress, elastic constants.
//
// Element data, restated in FrontISTR's node order: ShapeDeriv_tet4n (tet4n.f90), ShapeDeriv_tet10n (tet10n.f90: vertices
// 1-4 = origin, xi, eta, zeta, then the mid-edge nodes of (1,2), (2,3), (3,1), (1,4), (2,4), (3,4)), ShapeDeriv_prism6n
// (prism6n.f90: bottom triangle origin, xi, eta at zeta = -1, then the top triangle), ShapeDeriv_prism15n (prism15n.f90: the
// six vertices, the mid-edge nodes of the bottom triangle (1,2), (2,3), (3,1), of the top triangle (4,5), (5,6), (6,4), then
// of the vertical edges (1,4), (2,5), (3,6)), ShapeDeriv_hex20n (hex20n.f90: the eight vertices as TYPE=361, the mid-edge
// nodes of the bottom face (1,2), (2,3), (3,4), (4,1), of the top face (5,6), (6,7), (7,8), (8,5), then of the vertical edges
// (1,5), (2,6), (3,7), (4,8)); quadrature of quadrature.f90, positions and weights as the reference prints them: gauss3d4 /
// weight3d4 (341), gauss3d5 / weight3d5 (342), gauss3d7 / weight3d7 (351), gauss3d8 / weight3d8 (352: three points of the
// triangle at each of three heights, the triangle index running fastest), gauss3d3 / weight3d3 (362: xi fastest, zeta slowest).
// TYPE=361 has its row in the table only; its shape code is fx_assemble.h's.
#pragma once
#include "fx_internal.h"

// lpe: lanes per element of the assembly kernel (one lane per upper block; 341: six elements per wave64, lanes 60..63 idle;
// 351: three per wave; 352: two waves; 362: one 256-lane workgroup); ulpe: lanes per element of the linear update kernel
// (341 / 342: one per quadrature point; 362: two elements' 34 KB of LDS per workgroup).  361: 8 lanes in both (fx_assemble.h).
struct C3Facts {
  int etype, nn, nq, lpe, ulpe;  // nodes, quadrature points (NumOfQuadPoints, element.f90:415-447), lanes
};
constexpr C3Facts C3_TABLE[] = {{361, 8, 8, 8, 8},    {341, 4, 1, 10, 1},      {342, 10, 4, 64, 4},
                                {351, 6, 2, 21, 8},   {352, 15, 9, 128, 32},   {362, 20, 27, 256, 128}};
constexpr C3Facts c3_facts(int etype) {  // all zero: not a type the device knows
  for (const C3Facts &f : C3_TABLE)
    if (f.etype == etype) return f;
  return C3Facts{0, 0, 0, 0, 0};
}
// The same types in the order 341, 342, 351, 352, 361, 362 (the rows above are in another: 361 first), in which the per-type caches
// and tables of the host are indexed: ti is the type's place in it.  Faces (getSubFace, element.f90:181-315): nf of them, the
// first ntri are triangles of tn nodes, the others quadrilaterals of qn nodes.
struct C3FaceFacts {
  int etype, ti, nf, ntri, tn, qn;
};
constexpr C3FaceFacts C3_FACE_TABLE[] = {{341, 0, 4, 4, 3, 0}, {342, 1, 4, 4, 6, 0}, {351, 2, 5, 2, 3, 4},
                                         {352, 3, 5, 2, 6, 8}, {361, 4, 6, 0, 0, 4}, {362, 5, 6, 0, 0, 8}};
constexpr C3FaceFacts c3_face_facts(int etype) {  // ti = -1, no faces: not a type the device knows
  for (const C3FaceFacts &f : C3_FACE_TABLE)
    if (f.etype == etype) return f;
  return C3FaceFacts{0, -1, 0, 0, 0, 0};
}
constexpr int c3_type_index(int etype) { return c3_face_facts(etype).ti; }
constexpr int c3_type_at(int ti) { return C3_FACE_TABLE[ti].etype; }
constexpr int c3_faces(int etype) { return c3_face_facts(etype).nf; }
// nodes of face `face` (1-based) of a type the device knows
constexpr int c3_face_nodes(int etype, int face) { return face <= c3_face_facts(etype).ntri ? c3_face_facts(etype).tn : c3_face_facts(etype).qn; }
// getSubFace's node tables, which heat_FILM_3xx / heat_RADIATE_3xx / heat_DFLUX_3xx repeat as their NOD: 1-based positions in the
// element, by ti and face (host side)
static const int8_t C3_FACE_NOD[6][6][8] = {
    {{1, 2, 3}, {4, 2, 1}, {4, 3, 2}, {4, 1, 3}},
    {{1, 2, 3, 5, 6, 7}, {4, 2, 1, 9, 5, 8}, {4, 3, 2, 10, 6, 9}, {4, 1, 3, 8, 7, 10}},
    {{1, 2, 3}, {6, 5, 4}, {4, 5, 2, 1}, {5, 6, 3, 2}, {6, 4, 1, 3}},
    {{1, 2, 3, 7, 8, 9}, {6, 5, 4, 11, 10, 12}, {4, 5, 2, 1, 10, 14, 7, 13}, {5, 6, 3, 2, 11, 15, 8, 14}, {6, 4, 1, 3, 12, 13, 9, 15}},
    {{1, 2, 3, 4}, {8, 7, 6, 5}, {5, 6, 2, 1}, {6, 7, 3, 2}, {7, 8, 4, 3}, {8, 5, 1, 4}},
    {{1, 2, 3, 4, 9, 10, 11, 12}, {8, 7, 6, 5, 15, 14, 13, 16}, {5, 6, 2, 1, 13, 18, 9, 17}, {6, 7, 3, 2, 14, 19, 10, 18},
     {7, 8, 4, 3, 15, 20, 11, 19}, {8, 5, 1, 4, 16, 17, 12, 20}}};

template <int ETYPE>
struct C3El {
  static constexpr int NN = c3_facts(ETYPE).nn, NQ = c3_facts(ETYPE).nq, LPE = c3_facts(ETYPE).lpe, ULPE = c3_facts(ETYPE).ulpe;
  static constexpr bool TET = ETYPE == 341 || ETYPE == 342;  // k_assemble_tet / k_update_tet (registers), else k_assemble_c3 / k_update_c3 (LDS)
  static constexpr int BS = 256;                              // workgroup size of the STF_C3 kernels
  static constexpr int NB = NN * (NN + 1) / 2;                // upper blocks a <= b
  static constexpr int EPW = LPE < 64 ? 64 / LPE : 1;         // whole elements per wave64 where several fit
  static constexpr int EPB = LPE < 64 ? BS / 64 * EPW : BS / LPE;  // elements per workgroup (assembly)
  static constexpr int UEPB = BS / ULPE;                      // elements per workgroup (linear update)
};

// quadrature point q in natural (tetrahedra: volume) coordinates and its weight (getQuadPoint / getWeight)
template <int ETYPE>
__host__ __device__ __forceinline__ void c3_gauss(int q, double &xi, double &et, double &ze, double &w) {
  const double G2 = 0.577350269189626, G3 = 0.774596669241483;
  if (ETYPE == 341) {
    xi = et = ze = 0.25;
    w = 0.166666666666667;
  } else if (ETYPE == 342) {
    const double A = 0.138196601125011, B = 0.585410196624968;
    xi = q == 1 ? B : A; et = q == 2 ? B : A; ze = q == 3 ? B : A;
    w = 0.041666666666667;
  } else if (ETYPE == 351) {
    xi = et = 0.333333333333333;
    ze = q == 0 ? -G2 : G2;
    w = 0.5;
  } else if (ETYPE == 352) {
    const double A = 0.166666666666667, B = 0.666666666666667;
    const int t = q % 3, h = q / 3;
    xi = t == 1 ? B : A; et = t == 2 ? B : A;
    ze = h == 0 ? -G3 : (h == 1 ? 0.0 : G3);
    w = h == 1 ? 0.148148148148148 : 0.092592592592593;
  } else {
    const int i = q % 3, j = q / 3 % 3, k = q / 9;
    xi = i == 0 ? -G3 : (i == 1 ? 0.0 : G3);
    et = j == 0 ? -G3 : (j == 1 ? 0.0 : G3);
    ze = k == 0 ? -G3 : (k == 1 ? 0.0 : G3);
    const int mid = (i == 1) + (j == 1) + (k == 1);  // how many of the three coordinates sit at the centre point of the 1-d rule
    w = mid == 0 ? 0.171467764060357 : (mid == 1 ? 0.274348422496571 : (mid == 2 ? 0.438957475994513 : 0.702331961591221));
  }
}

// derivatives of node n's shape function with respect to the natural coordinates
template <int ETYPE>
__device__ __forceinline__ void c3_shape_deriv(int n, double xi, double et, double ze, double *d) {
  if (ETYPE == 341) {  // ShapeDeriv_tet4n
    d[0] = n == 0 ? -1.0 : (n == 1 ? 1.0 : 0.0);
    d[1] = n == 0 ? -1.0 : (n == 2 ? 1.0 : 0.0);
    d[2] = n == 0 ? -1.0 : (n == 3 ? 1.0 : 0.0);
  } else if (ETYPE == 342) {  // ShapeDeriv_tet10n
    const double a = 1.0 - xi - et - ze;
    switch (n) {
      case 0: d[0] = 1.0 - 4.0 * a; d[1] = 1.0 - 4.0 * a; d[2] = 1.0 - 4.0 * a; break;
      case 1: d[0] = 4.0 * xi - 1.0; d[1] = 0.0; d[2] = 0.0; break;
      case 2: d[0] = 0.0; d[1] = 4.0 * et - 1.0; d[2] = 0.0; break;
      case 3: d[0] = 0.0; d[1] = 0.0; d[2] = 4.0 * ze - 1.0; break;
      case 4: d[0] = 4.0 * (1.0 - 2.0 * xi - et - ze); d[1] = -4.0 * xi; d[2] = -4.0 * xi; break;
      case 5: d[0] = 4.0 * et; d[1] = 4.0 * xi; d[2] = 0.0; break;
      case 6: d[0] = -4.0 * et; d[1] = 4.0 * (1.0 - xi - 2.0 * et - ze); d[2] = -4.0 * et; break;
      case 7: d[0] = -4.0 * ze; d[1] = -4.0 * ze; d[2] = 4.0 * (1.0 - xi - et - 2.0 * ze); break;
      case 8: d[0] = 4.0 * ze; d[1] = 0.0; d[2] = 4.0 * xi; break;
      default: d[0] = 0.0; d[1] = 4.0 * ze; d[2] = 4.0 * et; break;
    }
  } else if (ETYPE == 351) {  // ShapeDeriv_prism6n
    const double a = 1.0 - xi - et;
    const double s = n < 3 ? -1.0 : 1.0, f = 0.5 * (1.0 + s * ze);  // 0.5 (1 -+ zeta): bottom / top triangle
    const int i = n % 3;
    d[0] = i == 0 ? -f : (i == 1 ? f : 0.0);
    d[1] = i == 0 ? -f : (i == 2 ? f : 0.0);
    d[2] = s * 0.5 * (i == 0 ? a : (i == 1 ? xi : et));
  } else if (ETYPE == 352) {  // ShapeDeriv_prism15n
    const double a = 1.0 - xi - et;
    const double zm = 1.0 - ze, zp = 1.0 + ze, zz = 1.0 - ze * ze;
    switch (n) {
      case 0: d[0] = -0.5 * zm * (4.0 * a - ze - 2.0); d[1] = d[0]; d[2] = a * (xi + et + ze - 0.5); break;
      case 1: d[0] = 0.5 * zm * (4.0 * xi - ze - 2.0); d[1] = 0.0; d[2] = xi * (-xi + ze + 0.5); break;
      case 2: d[0] = 0.0; d[1] = 0.5 * zm * (4.0 * et - ze - 2.0); d[2] = et * (-et + ze + 0.5); break;
      case 3: d[0] = -0.5 * zp * (4.0 * a + ze - 2.0); d[1] = d[0]; d[2] = a * (-xi - et + ze + 0.5); break;
      case 4: d[0] = 0.5 * zp * (4.0 * xi + ze - 2.0); d[1] = 0.0; d[2] = xi * (xi + ze - 0.5); break;
      case 5: d[0] = 0.0; d[1] = 0.5 * zp * (4.0 * et + ze - 2.0); d[2] = et * (et + ze - 0.5); break;
      case 6: d[0] = 2.0 * zm * (1.0 - 2.0 * xi - et); d[1] = -2.0 * xi * zm; d[2] = -2.0 * xi * a; break;
      case 7: d[0] = 2.0 * et * zm; d[1] = 2.0 * xi * zm; d[2] = -2.0 * xi * et; break;
      case 8: d[0] = -2.0 * et * zm; d[1] = 2.0 * zm * (1.0 - xi - 2.0 * et); d[2] = -2.0 * et * a; break;
      case 9: d[0] = 2.0 * zp * (1.0 - 2.0 * xi - et); d[1] = -2.0 * xi * zp; d[2] = 2.0 * xi * a; break;
      case 10: d[0] = 2.0 * et * zp; d[1] = 2.0 * xi * zp; d[2] = 2.0 * xi * et; break;
      case 11: d[0] = -2.0 * et * zp; d[1] = 2.0 * zp * (1.0 - xi - 2.0 * et); d[2] = 2.0 * et * a; break;
      case 12: d[0] = -zz; d[1] = -zz; d[2] = -2.0 * a * ze; break;
      case 13: d[0] = zz; d[1] = 0.0; d[2] = -2.0 * xi * ze; break;
      default: d[0] = 0.0; d[1] = zz; d[2] = -2.0 * et * ze; break;
    }
  } else {  // ShapeDeriv_hex20n, by the node's place: a vertex, or the middle of an edge along xi, eta or zeta
    if (n < 8) {
      const int c = n & 3;
      const double sx = (c == 1 || c == 2) ? 1.0 : -1.0, sy = c >= 2 ? 1.0 : -1.0, sz = n >= 4 ? 1.0 : -1.0;
      const double X = 1.0 + sx * xi, Y = 1.0 + sy * et, Z = 1.0 + sz * ze, P = 2.0 - sx * xi - sy * et - sz * ze;
      const double xyz = 0.125 * X * Y * Z;
      d[0] = sx * xyz - sx * (0.125 * Y * Z * P);
      d[1] = sy * xyz - sy * (0.125 * X * Z * P);
      d[2] = sz * xyz - sz * (0.125 * X * Y * P);
    } else if (n < 16) {
      const int c = (n - 8) & 3;
      const double sz = n >= 12 ? 1.0 : -1.0, Z = 1.0 + sz * ze;
      if ((c & 1) == 0) {  // along xi, at eta = sy
        const double sy = c == 2 ? 1.0 : -1.0, Y = 1.0 + sy * et, r2 = 1.0 - xi * xi;
        d[0] = -0.50 * xi * Y * Z; d[1] = sy * (0.25 * r2 * Z); d[2] = sz * (0.25 * r2 * Y);
      } else {  // along eta, at xi = sx
        const double sx = c == 1 ? 1.0 : -1.0, X = 1.0 + sx * xi, s2 = 1.0 - et * et;
        d[0] = sx * (0.25 * s2 * Z); d[1] = -0.50 * X * et * Z; d[2] = sz * (0.25 * X * s2);
      }
    } else {  // along zeta
      const int c = n - 16;
      const double sx = (c == 1 || c == 2) ? 1.0 : -1.0, sy = c >= 2 ? 1.0 : -1.0;
      const double X = 1.0 + sx * xi, Y = 1.0 + sy * et, t2 = 1.0 - ze * ze;
      d[0] = sx * (0.25 * Y * t2); d[1] = sy * (0.25 * X * t2); d[2] = -0.5 * X * Y * ze;
    }
  }
}

// determinant and inverse of the Jacobian J = X^T dN: getJacobian's expressions in its order (element.f90:772-818)
__device__ __forceinline__ void invert3(const double (&J)[3][3], double &det, double (&inv)[3][3]) {
  det = J[0][0] * J[1][1] * J[2][2] + J[1][0] * J[2][1] * J[0][2] + J[2][0] * J[0][1] * J[1][2] -
        J[2][0] * J[1][1] * J[0][2] - J[1][0] * J[0][1] * J[2][2] - J[0][0] * J[2][1] * J[1][2];
  const double dum = 1.0 / det;
  inv[0][0] = dum * (J[1][1] * J[2][2] - J[2][1] * J[1][2]);
  inv[0][1] = dum * (-J[0][1] * J[2][2] + J[2][1] * J[0][2]);
  inv[0][2] = dum * (J[0][1] * J[1][2] - J[1][1] * J[0][2]);
  inv[1][0] = dum * (-J[1][0] * J[2][2] + J[2][0] * J[1][2]);
  inv[1][1] = dum * (J[0][0] * J[2][2] - J[2][0] * J[0][2]);
  inv[1][2] = dum * (-J[0][0] * J[1][2] + J[1][0] * J[0][2]);
  inv[2][0] = dum * (J[1][0] * J[2][1] - J[2][0] * J[1][1]);
  inv[2][1] = dum * (-J[0][0] * J[2][1] + J[2][0] * J[0][1]);
  inv[2][2] = dum * (J[0][0] * J[1][1] - J[1][0] * J[0][1]);
}

// upper block number k (0 .. NN (NN + 1) / 2 - 1, row by row) -> (a, b), a <= b
template <int NN>
__device__ __forceinline__ void upper_block(int k, int &a, int &b) {
  a = 0;
  while (k >= NN - a) { k -= NN - a; a++; }
  b = a + k;
}

// small strain (xx, yy, zz, xy, yz, zx) from the displacement gradient gu = matmul(disp, gderiv) (static_LIB_3d.f90:648-668)
__device__ __forceinline__ void small_strain(const double (&gu)[3][3], double (&eps)[6]) {
  eps[0] = gu[0][0]; eps[1] = gu[1][1]; eps[2] = gu[2][2];
  eps[3] = gu[0][1] + gu[1][0]; eps[4] = gu[1][2] + gu[2][1]; eps[5] = gu[2][0] + gu[0][2];
}
// stress = D strain of an isotropic elastic material (D of calElasticMatrix)
__device__ __forceinline__ void iso_stress(double D11, double D12, double D44, const double *e, double *s) {
  s[0] = D11 * e[0] + D12 * e[1] + D12 * e[2];
  s[1] = D12 * e[0] + D11 * e[1] + D12 * e[2];
  s[2] = D12 * e[0] + D12 * e[1] + D11 * e[2];
  s[3] = D44 * e[3]; s[4] = D44 * e[4]; s[5] = D44 * e[5];
}
// The same with its fused multiply-adds written out instead of left to the compiler: the product of the yy strain is rounded, the
// xx and zz products are fused onto it in that order.  Two instantiations of a kernel that both use this form give the same bits
// for the same strain, which contraction left to the compiler does not promise (it chooses by the use counts of the products in
// the surrounding code).  This is the form the compiler had chosen in the linear update kernels of every type but 341, whose machine code is unchanged by it.
__device__ __forceinline__ void iso_stress_fixed(double D11, double D12, double D44, const double *e, double *s) {
  s[0] = __builtin_fma(D12, e[2], __builtin_fma(D11, e[0], D12 * e[1]));
  s[1] = __builtin_fma(D12, e[2], __builtin_fma(D12, e[0], D11 * e[1]));
  s[2] = __builtin_fma(D11, e[2], __builtin_fma(D12, e[0], D12 * e[1]));
  s[3] = D44 * e[3]; s[4] = D44 * e[4]; s[5] = D44 * e[5];
}
// calElasticMatrix, 3-D case (ElasticLinear.f90:43-55)
__host__ __device__ __forceinline__ void elastic_constants(double E, double nu, double &D11, double &D12, double &D44) {
  D11 = E * (1.0 - nu) / (1.0 - 2.0 * nu) / (1.0 + nu);
  D12 = E * nu / (1.0 - 2.0 * nu) / (1.0 + nu);
  D44 = E / (1.0 + nu) * 0.5;
}
