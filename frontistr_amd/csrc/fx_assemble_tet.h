// Device assembly and linear stress update of the tetrahedra TYPE=341 (4 nodes, one quadrature point) and TYPE=342 (10 nodes,
// four points): STF_C3 (static_LIB_3d.f90:47-205) and UPDATE_C3 (:516-837) with etype 341 / 342, small strain, isotropic
// ELASTIC -- what fstr_StiffMatrix.f90:134-144 and fstr_Update.f90:182-189 call for these elements.
//
// Element data (shape functions, quadrature, lanes per element): fx_c3_element.h.
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
#include "fx_assemble.h"

// Jacobian J = X^T dN at quadrature point q of the element with node coordinates ec (in registers), its determinant and inverse
template <int ETYPE>
__device__ __forceinline__ void tet_jacobian(const double (&ec)[C3El<ETYPE>::NN][3], int q, double &det, double (&inv)[3][3]) {
  constexpr int NN = C3El<ETYPE>::NN;
  double xi, et, ze, w;
  c3_gauss<ETYPE>(q, xi, et, ze, w);
  double J[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
  for (int a = 0; a < NN; a++) {
    double d[3];
    c3_shape_deriv<ETYPE>(a, xi, et, ze, d);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) J[i][j] += ec[a][i] * d[j];
  }
  invert3(J, det, inv);
}

// Element stiffness and scatter (see the head of this file).  Arguments as k_assemble_c3d8; elem_list != nullptr: positions
// [e0, n_elem) of elem_list are the elements of ONE colour; nullptr: elements e0..n_elem-1 with fp64 atomics.  Kout: element
// matrices out ((3 NN)^2 each, row-major, by element id), no scatter.
template <int ETYPE>
__global__ __launch_bounds__(C3El<ETYPE>::BS) void k_assemble_tet(int32_t n_elem, const double *__restrict__ coord,
                                                        const int32_t *__restrict__ conn, double D11, double D12, double D44,
                                                        const int32_t *__restrict__ indexL, const int32_t *__restrict__ itemL,
                                                        const int32_t *__restrict__ indexU, const int32_t *__restrict__ itemU,
                                                        double *__restrict__ D, double *__restrict__ AL, double *__restrict__ AU,
                                                        double *__restrict__ Kout, int32_t *__restrict__ err,
                                                        const int32_t *__restrict__ elem_mat, const double *__restrict__ mat_tab,
                                                        const int32_t *__restrict__ elem_list, int32_t e0,
                                                        const int32_t *__restrict__ pos_map) {
  using El = C3El<ETYPE>;
  constexpr int NN = El::NN, NQ = El::NQ, EPB = El::EPB, LPE = El::LPE, NB = El::NB;
  __shared__ double Jsh[EPB][NQ][10];     // per quadrature point: inverse Jacobian (row-major), weight * determinant
  __shared__ double Gsh[EPB][NQ][NN][3];  // global derivatives of every node at every point
  const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63;
  const int el = wave * El::EPW + wl / LPE, k = wl % LPE;
  const int32_t epos = e0 + blockIdx.x * EPB + el;
  const bool active = wl < El::EPW * LPE && epos < n_elem;
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
    c3_gauss<ETYPE>(k, xi, et, ze, w);
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
    c3_gauss<ETYPE>(q, xi, et, ze, w);
    c3_shape_deriv<ETYPE>(n, xi, et, ze, d);
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
  BlockScatter<NN> sc;  // destinations and old values first: the reads' latency runs under the arithmetic
  if (!sc.prepare({indexL, itemL, indexU, itemU, D, AL, AU, pos_map}, Kout != nullptr, conn + (size_t)NN * elem, elem, a, b, a != b,
                  elem_list != nullptr, err))
    return;
  double K[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const double h0[3] = {0.0, 0.0, 0.0};
    double Ba[6][3], Bb[6][3];
    node_B(Gsh[el][q][a], h0, Ba);
    node_B(Gsh[el][q][b], h0, Bb);
    btdb_accumulate(Ba, Bb, D11, D12, D44, Jsh[el][q][9], K);
  }
  sc.commit(K, Kout, (size_t)elem * (9 * NN * NN));
}

// UPDATE_C3 of a linear static analysis: one lane per quadrature point (341: one lane per element, 342: four).  Lane g computes
// the global derivatives at its point, strain = B u (total displacement), stress = D strain, and its share wg B_a^T stress of
// every node's internal force; the shares are summed over the element's lanes (xor shuffles) and lane g adds the nodes a with
// a % NQ == g to QFORCE with fp64 atomics (elements share nodes).  strain / stress: [n_elem][NQ][6].
// TH: the thermal switch of k_update_c3d8_linear (1: stress = D (strain - EPSTH); 2: TLOAD_C3, qforce += sum_g wg B^T D EPSTH).
template <int ETYPE, int TH = 0>
__global__ __launch_bounds__(C3El<ETYPE>::BS) void k_update_tet(int32_t n_elem, const double *__restrict__ coord,
                                                          const int32_t *__restrict__ conn, double D11, double D12, double D44,
                                                          const int32_t *__restrict__ elem_mat, const double *__restrict__ mat_tab,
                                                          const double *__restrict__ disp, double *__restrict__ strain,
                                                          double *__restrict__ stress, double *__restrict__ qforce,
                                                          ThermalDev th) {
  constexpr int NN = C3El<ETYPE>::NN, NQ = C3El<ETYPE>::NQ;
  const int64_t t = (int64_t)blockIdx.x * C3El<ETYPE>::BS + threadIdx.x;
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
  c3_gauss<ETYPE>(g, xi, et, ze, w);
  const double wg = w * det;
  double gd[NN][3], gu[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // gdispderiv = matmul(totaldisp, gderiv)
#pragma unroll
  for (int a = 0; a < NN; a++) {
    double d[3];
    c3_shape_deriv<ETYPE>(a, xi, et, ze, d);
#pragma unroll
    for (int j = 0; j < 3; j++) gd[a][j] = d[0] * inv[0][j] + d[1] * inv[1][j] + d[2] * inv[2][j];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double u = TH == 2 ? 0.0 : disp[(size_t)3 * (nod[a] - 1) + i];
#pragma unroll
      for (int j = 0; j < 3; j++) gu[i][j] += u * gd[a][j];
    }
  }
  double eps[6], sg[6];
  small_strain(gu, eps);
  // the stored stress in the written-out form (fx_c3_element.h) where that is what the compiler had made of iso_stress (342); 341,
  // where it had chosen another, keeps iso_stress and with it the bits it always gave
  auto stress_of = [&](const double *e, double *s) {
    if (ETYPE == 341) iso_stress(D11, D12, D44, e, s);
    else iso_stress_fixed(D11, D12, D44, e, s);
  };
  if (TH) {
    double tc = 0.0, t0 = 0.0;
#pragma unroll
    for (int a = 0; a < NN; a++) {
      const double h = c3_shape_func<ETYPE>(a, xi, et, ze);
      tc += h * th.temp[nod[a] - 1];
      t0 += h * th.temp0[nod[a] - 1];
    }
    double e;
    if (TH == 2 && th.tab_idx) {  // tables (the nonlinear loop's load, the only caller with any): the coefficients and D at this point's temperatures
      double alp, alp0, E, nu;
      if (thermal_coefficients(th, elem_mat ? elem_mat[elem] - 1 : 0, tc, t0, alp, alp0, E, nu)) elastic_constants(E, nu, D11, D12, D44);
      e = thermal_eps(alp, alp0, tc, t0, th.ref_temp);
    } else {
      e = thermal_eps(th.alpha[elem_mat ? elem_mat[elem] - 1 : 0], tc, t0, th.ref_temp);
    }
    double em[6] = {e, e, e, 0.0, 0.0, 0.0};
    if (TH == 1) {
#pragma unroll
      for (int k = 0; k < 6; k++) em[k] = eps[k] - em[k];
    }
    stress_of(em, sg);
  } else {
    stress_of(eps, sg);
  }
  if (active && TH != 2) {
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
