// Device assembly and linear stress update of the wedges TYPE=351 (6 nodes, 2 quadrature points), TYPE=352 (15 nodes, 9
// points) and of the quadratic hexahedron TYPE=362 (20 nodes, 27 points): STF_C3 (static_LIB_3d.f90:47-205) and UPDATE_C3
// (:516-837), small strain, isotropic ELASTIC -- with the tetrahedra of fx_assemble_tet.h the five types that
// fstr_StiffMatrix.f90:134-144 and fstr_Update.f90:182-189 send through these two routines.
//
// Element data, restated in FrontISTR's node order: ShapeDeriv_prism6n (prism6n.f90: bottom triangle origin, xi, eta at
// zeta = -1, then the top triangle), ShapeDeriv_prism15n (prism15n.f90: the six vertices, the mid-edge nodes of the bottom
// triangle (1,2), (2,3), (3,1), of the top triangle (4,5), (5,6), (6,4), then of the vertical edges (1,4), (2,5), (3,6)),
// ShapeDeriv_hex20n (hex20n.f90: the eight vertices as TYPE=361, the mid-edge nodes of the bottom face (1,2), (2,3), (3,4),
// (4,1), of the top face (5,6), (6,7), (7,8), (8,5), then of the vertical edges (1,5), (2,6), (3,7), (4,8)); quadrature
// gauss3d7 / weight3d7 (351), gauss3d8 / weight3d8 (352: three points of the triangle at each of three heights, the
// triangle index running fastest) and gauss3d3 / weight3d3 (362: xi fastest, zeta slowest) of quadrature.f90, positions
// and weights as the reference prints them.
//
// k_assemble_c3: as k_assemble_tet one lane per upper block (a <= b) of the symmetric element matrix -- 21 at 351 (three
// elements per wave64), 120 at 352 (two waves per element, two elements per workgroup), 210 at 362 (one 256-lane
// workgroup per element).  The element's lanes first stage the natural derivatives of every node at every point in LDS,
// lanes 0..NQ-1 then form and invert the Jacobian of their point (J = X^T dN summed over the nodes in order, as getJacobian),
// the lanes turn the staged derivatives into global ones in place, and lane (a, b) loops over the points in the reference's
// order with the two nodes' derivative rows re-read from LDS each time (btdb_accumulate): nine accumulators and the old
// values of two destination blocks are all a lane keeps, so the 27-point element needs no more registers than the 4-point
// tetrahedron.  The scatter is k_assemble_tet's.
#pragma once
#include "fx_internal.h"

template <int ETYPE>
struct C3El;
template <>
struct C3El<351> {
  static constexpr int NN = 6, NQ = 2, LPE = 21, ULPE = 8;  // nodes, points, lanes per element (assembly), lanes per element (update)
};
template <>
struct C3El<352> {
  static constexpr int NN = 15, NQ = 9, LPE = 128, ULPE = 32;
};
template <>
struct C3El<362> {
  static constexpr int NN = 20, NQ = 27, LPE = 256, ULPE = 128;  // (update: two elements' 34 KB of LDS per workgroup)
};
#define FXC_BS 256
#define FXC_NB(ET) (C3El<ET>::NN * (C3El<ET>::NN + 1) / 2)                                             // upper blocks a <= b
#define FXC_EPB(ET) (C3El<ET>::LPE < 64 ? FXC_BS / 64 * (64 / C3El<ET>::LPE) : FXC_BS / C3El<ET>::LPE)  // elements per workgroup
#define FXC_UEPB(ET) (FXC_BS / C3El<ET>::ULPE)

// quadrature point q in natural coordinates and its weight (getQuadPoint / getWeight)
template <int ETYPE>
__device__ __forceinline__ void c3_gauss(int q, double &xi, double &et, double &ze, double &w) {
  const double G2 = 0.577350269189626, G3 = 0.774596669241483;
  if (ETYPE == 351) {
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
  if (ETYPE == 351) {  // ShapeDeriv_prism6n
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

// determinant and inverse of J (getJacobian, element.f90:772-818; the expressions of tet_jacobian)
__device__ __forceinline__ void c3_invert(const double (&J)[3][3], double &det, double *inv) {
  det = J[0][0] * J[1][1] * J[2][2] + J[1][0] * J[2][1] * J[0][2] + J[2][0] * J[0][1] * J[1][2] -
        J[2][0] * J[1][1] * J[0][2] - J[1][0] * J[0][1] * J[2][2] - J[0][0] * J[2][1] * J[1][2];
  const double dum = 1.0 / det;
  inv[0] = dum * (J[1][1] * J[2][2] - J[2][1] * J[1][2]);
  inv[1] = dum * (-J[0][1] * J[2][2] + J[2][1] * J[0][2]);
  inv[2] = dum * (J[0][1] * J[1][2] - J[1][1] * J[0][2]);
  inv[3] = dum * (-J[1][0] * J[2][2] + J[2][0] * J[1][2]);
  inv[4] = dum * (J[0][0] * J[2][2] - J[2][0] * J[0][2]);
  inv[5] = dum * (-J[0][0] * J[1][2] + J[1][0] * J[0][2]);
  inv[6] = dum * (J[1][0] * J[2][1] - J[2][0] * J[1][1]);
  inv[7] = dum * (-J[0][0] * J[2][1] + J[2][0] * J[0][1]);
  inv[8] = dum * (J[0][0] * J[1][1] - J[1][0] * J[0][1]);
}

// The three staging steps both kernels share, for the element whose LPE lanes call this together (k = lane of the element,
// `active`: the element exists).  In: nothing staged.  Out: X = node coordinates, Jq[q] = inverse Jacobian (row-major) and
// weight * determinant, G[q][n] = global derivatives (getGlobalDeriv, element.f90:693-744).  Every lane of the workgroup
// must call it (it holds the barriers).
template <int ETYPE, int LPE>
__device__ __forceinline__ void c3_stage(bool active, int k, int32_t elem, const double *__restrict__ coord,
                                         const int32_t *__restrict__ conn, double (*X)[3], double (*Jq)[10],
                                         double (*G)[C3El<ETYPE>::NN][3]) {
  constexpr int NN = C3El<ETYPE>::NN, NQ = C3El<ETYPE>::NQ;
  if (active) {
    for (int t = k; t < NN; t += LPE) {
      const int32_t nd = conn[(size_t)NN * elem + t];
#pragma unroll
      for (int d = 0; d < 3; d++) X[t][d] = coord[(size_t)3 * (nd - 1) + d];
    }
    for (int t = k; t < NQ * NN; t += LPE) {  // natural derivatives of node n at point q
      const int q = t / NN, n = t % NN;
      double xi, et, ze, w, d[3];
      c3_gauss<ETYPE>(q, xi, et, ze, w);
      c3_shape_deriv<ETYPE>(n, xi, et, ze, d);
#pragma unroll
      for (int j = 0; j < 3; j++) G[q][n][j] = d[j];
    }
  }
  __syncthreads();
  if (active) {
    for (int q = k; q < NQ; q += LPE) {
      double J[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll 1
      for (int a = 0; a < NN; a++) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) J[i][j] += X[a][i] * G[q][a][j];
      }
      double det, inv[9], xi, et, ze, w;
      c3_invert(J, det, inv);
      c3_gauss<ETYPE>(q, xi, et, ze, w);
#pragma unroll
      for (int e = 0; e < 9; e++) Jq[q][e] = inv[e];
      Jq[q][9] = w * det;  // wg = getWeight * det
    }
  }
  __syncthreads();
  if (active) {
    for (int t = k; t < NQ * NN; t += LPE) {
      const int q = t / NN, n = t % NN;
      const double *inv = Jq[q];
      const double d0 = G[q][n][0], d1 = G[q][n][1], d2 = G[q][n][2];
#pragma unroll
      for (int j = 0; j < 3; j++) G[q][n][j] = d0 * inv[j] + d1 * inv[3 + j] + d2 * inv[6 + j];
    }
  }
  __syncthreads();
}

// Element stiffness and scatter (see the head of this file); the arguments are k_assemble_tet's.
template <int ETYPE>
__global__ __launch_bounds__(FXC_BS) void k_assemble_c3(int32_t n_elem, const double *__restrict__ coord,
                                                       const int32_t *__restrict__ conn, double D11, double D12, double D44,
                                                       const int32_t *__restrict__ indexL, const int32_t *__restrict__ itemL,
                                                       const int32_t *__restrict__ indexU, const int32_t *__restrict__ itemU,
                                                       double *__restrict__ D, double *__restrict__ AL, double *__restrict__ AU,
                                                       double *__restrict__ Kout, int32_t *__restrict__ err,
                                                       const int32_t *__restrict__ elem_mat, const double *__restrict__ mat_tab,
                                                       const int32_t *__restrict__ elem_list, int32_t e0,
                                                       const int32_t *__restrict__ pos_map) {
  constexpr int NN = C3El<ETYPE>::NN, NQ = C3El<ETYPE>::NQ, LPE = C3El<ETYPE>::LPE, EPB = FXC_EPB(ETYPE), NB = FXC_NB(ETYPE);
  __shared__ double Xsh[EPB][NN][3];
  __shared__ double Jsh[EPB][NQ][10];
  __shared__ double Gsh[EPB][NQ][NN][3];
  int el, k;
  bool lane_ok = true;
  if (LPE < 64) {  // whole elements per wave; the wave's last 64 % LPE lanes idle
    const int wl = threadIdx.x & 63;
    el = (threadIdx.x >> 6) * (64 / LPE) + wl / LPE;
    k = wl % LPE;
    lane_ok = wl < 64 / LPE * LPE;
  } else {
    el = threadIdx.x / LPE;
    k = threadIdx.x % LPE;
  }
  if (!lane_ok) el = 0;  // (never indexes LDS: not active)
  const int32_t epos = e0 + blockIdx.x * EPB + el;
  const bool active = lane_ok && epos < n_elem;
  const int32_t elem = !active ? 0 : (elem_list ? elem_list[epos] : epos);
  c3_stage<ETYPE, LPE>(active, k, elem, coord, conn, Xsh[el], Jsh[el], Gsh[el]);
  if (!active || k >= NB) return;
  if (elem_mat) {  // several sections: (D11, D12, D44) of this element's material
    const int32_t mid = elem_mat[elem] - 1;
    D11 = mat_tab[3 * mid]; D12 = mat_tab[3 * mid + 1]; D44 = mat_tab[3 * mid + 2];
  }
  int a, b;
  upper_block<NN>(k, a, b);
  const int32_t inod = conn[(size_t)NN * elem + a], jnod = conn[(size_t)NN * elem + b];
  auto block_ptr = [&](int ra, int rb, int32_t rnod, int32_t cnod, bool &first) -> double * {  // hecmw_mat_add_node
    const int32_t raw = pos_map ? pos_map[(size_t)(NN * NN) * elem + NN * ra + rb] : 0;
    first = pos_map && raw >= 0 && (raw & FXA_FIRST_BIT);
    if (rnod == cnod) return D + (size_t)9 * (rnod - 1);
    if (cnod < rnod) {
      const int32_t p = pos_map ? (raw < 0 ? raw : (raw & ~FXA_FIRST_BIT)) : item_search(itemL, indexL[rnod - 1], indexL[rnod], cnod);
      return p < 0 ? nullptr : AL + (size_t)9 * p;
    }
    const int32_t p = pos_map ? (raw < 0 ? raw : (raw & ~FXA_FIRST_BIT)) : item_search(itemU, indexU[rnod - 1], indexU[rnod], cnod);
    return p < 0 ? nullptr : AU + (size_t)9 * p;
  };
  double *dst = nullptr, *dstT = nullptr;
  double old[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, oldT[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (!Kout) {  // destinations and old values first: the reads' latency runs under the arithmetic
    bool first = false, firstT = false;
    dst = block_ptr(a, b, inod, jnod, first);
    if (a != b) dstT = block_ptr(b, a, jnod, inod, firstT);
    if (!dst || (a != b && !dstT)) { if (err) atomicExch(err, 2); return; }
    if (elem_list && !first) {
#pragma unroll
      for (int e = 0; e < 9; e++) old[e] = dst[e];
    }
    if (elem_list && a != b && !firstT) {
#pragma unroll
      for (int e = 0; e < 9; e++) oldT[e] = dstT[e];
    }
  }
  double K[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int q = 0; q < NQ; q++) {
    const double h0[3] = {0.0, 0.0, 0.0};
    double Ba[6][3], Bb[6][3];
    node_B(Gsh[el][q][a], h0, Ba);
    node_B(Gsh[el][q][b], h0, Bb);
    btdb_accumulate(Ba, Bb, D11, D12, D44, Jsh[el][q][9], K);
  }
  if (Kout) {
    constexpr int W = 3 * NN;
    const size_t ko = (size_t)elem * W * W;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        Kout[ko + (size_t)(3 * a + i) * W + 3 * b + j] = K[3 * i + j];
        if (a != b) Kout[ko + (size_t)(3 * b + j) * W + 3 * a + i] = K[3 * i + j];
      }
    return;
  }
  if (elem_list) {
#pragma unroll
    for (int e = 0; e < 9; e++) dst[e] = old[e] + K[e];
    if (a != b) {
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) dstT[3 * j + i] = oldT[3 * j + i] + K[3 * i + j];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 9; e++) unsafeAtomicAdd(dst + e, K[e]);
    if (a != b) {
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) unsafeAtomicAdd(dstT + 3 * j + i, K[3 * i + j]);
    }
  }
}

// UPDATE_C3 of a linear static analysis.  ULPE lanes per element (8 / 32 / 128); the staging is the assembly's.  Lane g < NQ
// then computes strain = B u (total displacement) and stress = D strain at its point, writes both out and leaves the stress
// in LDS; lane t < 3 NN sums component t % 3 of node t / 3's internal force wg B_a^T stress over the points in the
// reference's order and adds it to QFORCE with an fp64 atomic (elements share nodes).  strain / stress: [n_elem][NQ][6].
template <int ETYPE>
__global__ __launch_bounds__(FXC_BS) void k_update_c3(int32_t n_elem, const double *__restrict__ coord,
                                                     const int32_t *__restrict__ conn, double D11, double D12, double D44,
                                                     const int32_t *__restrict__ elem_mat, const double *__restrict__ mat_tab,
                                                     const double *__restrict__ disp, double *__restrict__ strain,
                                                     double *__restrict__ stress, double *__restrict__ qforce) {
  constexpr int NN = C3El<ETYPE>::NN, NQ = C3El<ETYPE>::NQ, LPE = C3El<ETYPE>::ULPE, EPB = FXC_UEPB(ETYPE);
  __shared__ double Xsh[EPB][NN][3];
  __shared__ double Jsh[EPB][NQ][10];
  __shared__ double Gsh[EPB][NQ][NN][3];
  __shared__ double Ssh[EPB][NQ][6];  // stress at every point
  const int el = threadIdx.x / LPE, k = threadIdx.x % LPE;
  const int64_t e_raw = (int64_t)blockIdx.x * EPB + el;
  const bool active = e_raw < n_elem;
  const int32_t elem = active ? (int32_t)e_raw : 0;
  c3_stage<ETYPE, LPE>(active, k, elem, coord, conn, Xsh[el], Jsh[el], Gsh[el]);
  if (active) {
    if (elem_mat) {
      const int32_t mid = elem_mat[elem] - 1;
      D11 = mat_tab[3 * mid]; D12 = mat_tab[3 * mid + 1]; D44 = mat_tab[3 * mid + 2];
    }
    for (int g = k; g < NQ; g += LPE) {
      double gu[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // gdispderiv = matmul(totaldisp, gderiv)
#pragma unroll 2
      for (int a = 0; a < NN; a++) {
        const int32_t nd = conn[(size_t)NN * elem + a];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const double u = disp[(size_t)3 * (nd - 1) + i];
#pragma unroll
          for (int j = 0; j < 3; j++) gu[i][j] += u * Gsh[el][g][a][j];
        }
      }
      double eps[6], sg[6];
      eps[0] = gu[0][0]; eps[1] = gu[1][1]; eps[2] = gu[2][2];
      eps[3] = gu[0][1] + gu[1][0]; eps[4] = gu[1][2] + gu[2][1]; eps[5] = gu[2][0] + gu[0][2];
      sg[0] = D11 * eps[0] + D12 * eps[1] + D12 * eps[2];
      sg[1] = D12 * eps[0] + D11 * eps[1] + D12 * eps[2];
      sg[2] = D12 * eps[0] + D12 * eps[1] + D11 * eps[2];
      sg[3] = D44 * eps[3]; sg[4] = D44 * eps[4]; sg[5] = D44 * eps[5];
      double *se = strain + ((size_t)NQ * elem + g) * 6, *ss = stress + ((size_t)NQ * elem + g) * 6;
#pragma unroll
      for (int c = 0; c < 6; c++) { se[c] = eps[c]; ss[c] = sg[c]; Ssh[el][g][c] = sg[c]; }
    }
  }
  __syncthreads();
  if (!active) return;
  for (int t = k; t < 3 * NN; t += LPE) {
    const int a = t / 3, d = t % 3;
    double f = 0.0;
#pragma unroll 3
    for (int g = 0; g < NQ; g++) {
      const double *q = Gsh[el][g][a], *sg = Ssh[el][g];
      const double o = d == 0 ? q[0] * sg[0] + q[1] * sg[3] + q[2] * sg[5]
                              : (d == 1 ? q[1] * sg[1] + q[0] * sg[3] + q[2] * sg[4] : q[2] * sg[2] + q[1] * sg[4] + q[0] * sg[5]);
      f += o * Jsh[el][g][9];
    }
    const int32_t nd = conn[(size_t)NN * elem + a];
    unsafeAtomicAdd(qforce + (size_t)3 * (nd - 1) + d, f);
  }
}
