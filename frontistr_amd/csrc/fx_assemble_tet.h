// Device assembly and linear stress update of the tetrahedra TYPE=341 (4 nodes, one quadrature point) and TYPE=342 (10 nodes,
// four points): STF_C3 (static_LIB_3d.f90:47-205) and UPDATE_C3 (:516-837) with etype 341 / 342, small strain, isotropic
// ELASTIC -- what fstr_StiffMatrix.f90:134-144 and fstr_Update.f90:182-189 call for these elements.
//
// Element data: ShapeDeriv_tet4n (tet4n.f90), ShapeDeriv_tet10n (tet10n.f90; FrontISTR's node order: vertices 1-4 = origin, xi,
// eta, zeta, then the mid-edge nodes of (1,2), (2,3), (3,1), (1,4), (2,4), (3,4)); quadrature gauss3d4 / weight3d4 and
// gauss3d5 / weight3d5 (quadrature.f90), the weights as the reference prints them.
//
// k_assemble_tet: the element matrix is symmetric, so only its NN (NN + 1) / 2 upper blocks (a <= b) are computed: 10 at 341,
// 55 at 342.  One lane per upper block -- 342: one element per wave64 (55 of 64 lanes busy), 341: six elements per wave (60).
// First the lanes 0..NQ-1 of an element compute their quadrature point's Jacobian (inverse and determinant, LDS), then lanes
// 0..NQ*NN-1 the global derivatives of one node at one point (LDS), then lane (a, b) accumulates K_ab = sum_g wg B_a^T D B_b
// over the points in the reference's order (btdb_accumulate) and scatters it at (a, b) and, transposed, at (b, a).  The
// scatter is that of k_assemble_c3d8: colour by colour with plain read-modify-writes (first-write flags from the position
// map), or hardware fp64 atomics.  A tetrahedron that names a node twice has zero volume: the host refuses it, so the NN^2
// blocks of an element are always distinct blocks of the matrix.
#pragma once
#include "fx_internal.h"

template <int ETYPE>
struct TetEl;
template <>
struct TetEl<341> {
  static constexpr int NN = 4, NQ = 1, EPW = 6;  // nodes, quadrature points, elements per wave64
};
template <>
struct TetEl<342> {
  static constexpr int NN = 10, NQ = 4, EPW = 1;
};
#define FXT_BS 256
#define FXT_NB(ET) (TetEl<ET>::NN * (TetEl<ET>::NN + 1) / 2)       // upper blocks a <= b
#define FXT_LPE(ET) (64 / TetEl<ET>::EPW)                           // lanes per element (341: 10, lanes 60..63 idle)
#define FXT_EPB(ET) (FXT_BS / 64 * TetEl<ET>::EPW)                  // elements per workgroup

// quadrature point q in volume coordinates (gauss3d4, gauss3d5) and its weight
template <int ETYPE>
__device__ __forceinline__ void tet_gauss(int q, double &xi, double &et, double &ze, double &w) {
  if (ETYPE == 341) {
    xi = et = ze = 0.25;
    w = 0.166666666666667;
  } else {
    const double A = 0.138196601125011, B = 0.585410196624968;
    xi = q == 1 ? B : A; et = q == 2 ? B : A; ze = q == 3 ? B : A;
    w = 0.041666666666667;
  }
}

// derivatives of node n's shape function with respect to the volume coordinates (ShapeDeriv_tet4n / ShapeDeriv_tet10n)
template <int ETYPE>
__device__ __forceinline__ void tet_shape_deriv(int n, double xi, double et, double ze, double *d) {
  if (ETYPE == 341) {
    d[0] = n == 0 ? -1.0 : (n == 1 ? 1.0 : 0.0);
    d[1] = n == 0 ? -1.0 : (n == 2 ? 1.0 : 0.0);
    d[2] = n == 0 ? -1.0 : (n == 3 ? 1.0 : 0.0);
    return;
  }
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
}

// Jacobian J = X^T dN at quadrature point q of the element with node coordinates ec, its determinant and inverse (getJacobian,
// element.f90:772-818, the same expressions as hex8_global_deriv)
template <int ETYPE>
__device__ __forceinline__ void tet_jacobian(const double (&ec)[TetEl<ETYPE>::NN][3], int q, double &det, double (&inv)[3][3]) {
  constexpr int NN = TetEl<ETYPE>::NN;
  double xi, et, ze, w;
  tet_gauss<ETYPE>(q, xi, et, ze, w);
  double J[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
  for (int a = 0; a < NN; a++) {
    double d[3];
    tet_shape_deriv<ETYPE>(a, xi, et, ze, d);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) J[i][j] += ec[a][i] * d[j];
  }
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

// Element stiffness and scatter (see the head of this file).  Arguments as k_assemble_c3d8; elem_list != nullptr: positions
// [e0, n_elem) of elem_list are the elements of ONE colour; nullptr: elements e0..n_elem-1 with fp64 atomics.  Kout: element
// matrices out ((3 NN)^2 each, row-major, by element id), no scatter.
template <int ETYPE>
__global__ __launch_bounds__(FXT_BS) void k_assemble_tet(int32_t n_elem, const double *__restrict__ coord,
                                                        const int32_t *__restrict__ conn, double D11, double D12, double D44,
                                                        const int32_t *__restrict__ indexL, const int32_t *__restrict__ itemL,
                                                        const int32_t *__restrict__ indexU, const int32_t *__restrict__ itemU,
                                                        double *__restrict__ D, double *__restrict__ AL, double *__restrict__ AU,
                                                        double *__restrict__ Kout, int32_t *__restrict__ err,
                                                        const int32_t *__restrict__ elem_mat, const double *__restrict__ mat_tab,
                                                        const int32_t *__restrict__ elem_list, int32_t e0,
                                                        const int32_t *__restrict__ pos_map) {
  constexpr int NN = TetEl<ETYPE>::NN, NQ = TetEl<ETYPE>::NQ, EPB = FXT_EPB(ETYPE), LPE = FXT_LPE(ETYPE);
  constexpr int NB = FXT_NB(ETYPE);
  __shared__ double Jsh[EPB][NQ][10];     // per quadrature point: inverse Jacobian (row-major), weight * determinant
  __shared__ double Gsh[EPB][NQ][NN][3];  // global derivatives of every node at every point
  const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63;
  const int el = wave * TetEl<ETYPE>::EPW + wl / LPE, k = wl % LPE;
  const int32_t epos = e0 + blockIdx.x * EPB + el;
  const bool active = wl < TetEl<ETYPE>::EPW * LPE && epos < n_elem;
  const int32_t elem = !active ? 0 : (elem_list ? elem_list[epos] : epos);
  if (active && k < NQ) {
    double ec[NN][3];
#pragma unroll
    for (int j = 0; j < NN; j++) {
      const int32_t nd = conn[(size_t)NN * elem + j];
#pragma unroll
      for (int d = 0; d < 3; d++) ec[j][d] = coord[(size_t)3 * (nd - 1) + d];
    }
    double det, inv[3][3], xi, et, ze, w;
    tet_jacobian<ETYPE>(ec, k, det, inv);
    tet_gauss<ETYPE>(k, xi, et, ze, w);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Jsh[el][k][3 * i + j] = inv[i][j];
    Jsh[el][k][9] = w * det;  // wg = getWeight * det
  }
  __syncthreads();
  if (active && k < NQ * NN) {  // global derivatives of node n at point q (getGlobalDeriv, element.f90:693-744)
    const int q = k / NN, n = k % NN;
    double xi, et, ze, w, d[3];
    tet_gauss<ETYPE>(q, xi, et, ze, w);
    tet_shape_deriv<ETYPE>(n, xi, et, ze, d);
    const double *inv = Jsh[el][q];
#pragma unroll
    for (int j = 0; j < 3; j++) Gsh[el][q][n][j] = d[0] * inv[j] + d[1] * inv[3 + j] + d[2] * inv[6 + j];
  }
  __syncthreads();
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
#pragma unroll
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

// UPDATE_C3 of a linear static analysis: one lane per quadrature point (341: one lane per element, 342: four).  Lane g computes
// the global derivatives at its point, strain = B u (total displacement), stress = D strain, and its share wg B_a^T stress of
// every node's internal force; the shares are summed over the element's lanes (xor shuffles) and lane g adds the nodes a with
// a % NQ == g to QFORCE with fp64 atomics (elements share nodes).  strain / stress: [n_elem][NQ][6].
#define FXU_TET_BS 256
template <int ETYPE>
__global__ __launch_bounds__(FXU_TET_BS) void k_update_tet(int32_t n_elem, const double *__restrict__ coord,
                                                          const int32_t *__restrict__ conn, double D11, double D12, double D44,
                                                          const int32_t *__restrict__ elem_mat, const double *__restrict__ mat_tab,
                                                          const double *__restrict__ disp, double *__restrict__ strain,
                                                          double *__restrict__ stress, double *__restrict__ qforce) {
  constexpr int NN = TetEl<ETYPE>::NN, NQ = TetEl<ETYPE>::NQ;
  const int64_t t = (int64_t)blockIdx.x * FXU_TET_BS + threadIdx.x;
  const int g = (int)(t % NQ);
  const bool active = t / NQ < n_elem;
  const int32_t elem = active ? (int32_t)(t / NQ) : n_elem - 1;  // idle lanes shadow the last element (uniform shuffles), write nothing
  if (elem_mat) {
    const int32_t mid = elem_mat[elem] - 1;
    D11 = mat_tab[3 * mid]; D12 = mat_tab[3 * mid + 1]; D44 = mat_tab[3 * mid + 2];
  }
  int32_t nod[NN];
  double ec[NN][3];
#pragma unroll
  for (int j = 0; j < NN; j++) {
    nod[j] = conn[(size_t)NN * elem + j];
#pragma unroll
    for (int d = 0; d < 3; d++) ec[j][d] = coord[(size_t)3 * (nod[j] - 1) + d];
  }
  double det, inv[3][3], xi, et, ze, w;
  tet_jacobian<ETYPE>(ec, g, det, inv);
  tet_gauss<ETYPE>(g, xi, et, ze, w);
  const double wg = w * det;
  double gd[NN][3], gu[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // gdispderiv = matmul(totaldisp, gderiv)
#pragma unroll
  for (int a = 0; a < NN; a++) {
    double d[3];
    tet_shape_deriv<ETYPE>(a, xi, et, ze, d);
#pragma unroll
    for (int j = 0; j < 3; j++) gd[a][j] = d[0] * inv[0][j] + d[1] * inv[1][j] + d[2] * inv[2][j];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double u = disp[(size_t)3 * (nod[a] - 1) + i];
#pragma unroll
      for (int j = 0; j < 3; j++) gu[i][j] += u * gd[a][j];
    }
  }
  double eps[6], sg[6];
  eps[0] = gu[0][0]; eps[1] = gu[1][1]; eps[2] = gu[2][2];
  eps[3] = gu[0][1] + gu[1][0]; eps[4] = gu[1][2] + gu[2][1]; eps[5] = gu[2][0] + gu[0][2];
  sg[0] = D11 * eps[0] + D12 * eps[1] + D12 * eps[2];
  sg[1] = D12 * eps[0] + D11 * eps[1] + D12 * eps[2];
  sg[2] = D12 * eps[0] + D12 * eps[1] + D11 * eps[2];
  sg[3] = D44 * eps[3]; sg[4] = D44 * eps[4]; sg[5] = D44 * eps[5];
  if (active) {
    double *se = strain + ((size_t)NQ * elem + g) * 6, *ss = stress + ((size_t)NQ * elem + g) * 6;
#pragma unroll
    for (int k = 0; k < 6; k++) { se[k] = eps[k]; ss[k] = sg[k]; }
  }
#pragma unroll
  for (int a = 0; a < NN; a++) {
    const double *q = gd[a];
    double o[3];
    o[0] = (q[0] * sg[0] + q[1] * sg[3] + q[2] * sg[5]) * wg;
    o[1] = (q[1] * sg[1] + q[0] * sg[3] + q[2] * sg[4]) * wg;
    o[2] = (q[2] * sg[2] + q[1] * sg[4] + q[0] * sg[5]) * wg;
#pragma unroll
    for (int d = 0; d < 3; d++) {
#pragma unroll
      for (int s = 1; s < NQ; s <<= 1) o[d] += __shfl_xor(o[d], s, 64);
    }
    if (active && a % NQ == g) {
#pragma unroll
      for (int d = 0; d < 3; d++) unsafeAtomicAdd(qforce + (size_t)3 * (nod[a] - 1) + d, o[d]);
    }
  }
}
