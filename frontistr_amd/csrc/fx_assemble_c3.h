// Device assembly and linear stress update of the wedges TYPE=351 (6 nodes, 2 quadrature points), TYPE=352 (15 nodes, 9
// points) and of the quadratic hexahedron TYPE=362 (20 nodes, 27 points): STF_C3 (static_LIB_3d.f90:47-205) and UPDATE_C3
// (:516-837), small strain, isotropic ELASTIC -- with the tetrahedra of fx_assemble_tet.h the five types that
// fstr_StiffMatrix.f90:134-144 and fstr_Update.f90:182-189 send through these two routines.
//
// Element data (shape functions, quadrature, lanes per element): fx_c3_element.h.
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
#include "fx_assemble.h"

// The three staging steps both kernels share, for the element whose LPE lanes call this together (k = lane of the element,
// `active`: the element exists).  In: nothing staged.  Out: X = node coordinates, Jq[q] = inverse Jacobian (row-major) and
// weight * determinant, G[q][n] = global derivatives (getGlobalDeriv, element.f90:693-744).  Every lane of the workgroup
// must call it (it holds the barriers).  DISP (the nonlinear kernels' updated Lagrange branch, fx_nonlinear_c3.h): the
// configuration is X = (alpha dunode + unode) + coord instead of the initial coordinates.
template <int ETYPE, int LPE, bool DISP = false>
__device__ __forceinline__ void c3_stage(bool active, int k, int32_t elem, const double *__restrict__ coord,
                                         const int32_t *__restrict__ conn, double (*X)[3], double (*Jq)[10],
                                         double (*G)[C3El<ETYPE>::NN][3], const double *__restrict__ unode = nullptr,
                                         const double *__restrict__ dunode = nullptr, double alpha = 0.0) {
  constexpr int NN = C3El<ETYPE>::NN, NQ = C3El<ETYPE>::NQ;
  if (active) {
    for (int t = k; t < NN; t += LPE) {
      const int32_t nd = conn[(size_t)NN * elem + t];
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const size_t o = (size_t)3 * (nd - 1) + d;
        if (DISP) X[t][d] = (alpha * dunode[o] + unode[o]) + coord[o];
        else X[t][d] = coord[o];
      }
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
      double det, inv[3][3], xi, et, ze, w;
      invert3(J, det, inv);
      c3_gauss<ETYPE>(q, xi, et, ze, w);
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Jq[q][3 * i + j] = inv[i][j];
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
__global__ __launch_bounds__(C3El<ETYPE>::BS) void k_assemble_c3(int32_t n_elem, const double *__restrict__ coord,
                                                       const int32_t *__restrict__ conn, double D11, double D12, double D44,
                                                       const int32_t *__restrict__ indexL, const int32_t *__restrict__ itemL,
                                                       const int32_t *__restrict__ indexU, const int32_t *__restrict__ itemU,
                                                       double *__restrict__ D, double *__restrict__ AL, double *__restrict__ AU,
                                                       double *__restrict__ Kout, int32_t *__restrict__ err,
                                                       const int32_t *__restrict__ elem_mat, const double *__restrict__ mat_tab,
                                                       const int32_t *__restrict__ elem_list, int32_t e0,
                                                       const int32_t *__restrict__ pos_map) {
  constexpr int NN = C3El<ETYPE>::NN, NQ = C3El<ETYPE>::NQ, LPE = C3El<ETYPE>::LPE, EPB = C3El<ETYPE>::EPB, NB = C3El<ETYPE>::NB;
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
  BlockScatter<NN> sc;  // destinations and old values first: the reads' latency runs under the arithmetic
  if (!sc.prepare({indexL, itemL, indexU, itemU, D, AL, AU, pos_map}, Kout != nullptr, conn + (size_t)NN * elem, elem, a, b, a != b,
                  elem_list != nullptr, err))
    return;
  double K[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int q = 0; q < NQ; q++) {
    const double h0[3] = {0.0, 0.0, 0.0};
    double Ba[6][3], Bb[6][3];
    node_B(Gsh[el][q][a], h0, Ba);
    node_B(Gsh[el][q][b], h0, Bb);
    btdb_accumulate(Ba, Bb, D11, D12, D44, Jsh[el][q][9], K);
  }
  sc.commit(K, Kout, (size_t)elem * (9 * NN * NN));
}

// UPDATE_C3 of a linear static analysis.  ULPE lanes per element (8 / 32 / 128); the staging is the assembly's.  Lane g < NQ
// then computes strain = B u (total displacement) and stress = D strain at its point, writes both out and leaves the stress
// in LDS; lane t < 3 NN sums component t % 3 of node t / 3's internal force wg B_a^T stress over the points in the
// reference's order and adds it to QFORCE with an fp64 atomic (elements share nodes).  strain / stress: [n_elem][NQ][6].
// TH: the thermal switch of k_update_c3d8_linear (1: stress = D (strain - EPSTH); 2: TLOAD_C3, qforce += sum_g wg B^T D EPSTH).
template <int ETYPE, int TH = 0>
__global__ __launch_bounds__(C3El<ETYPE>::BS) void k_update_c3(int32_t n_elem, const double *__restrict__ coord,
                                                     const int32_t *__restrict__ conn, double D11, double D12, double D44,
                                                     const int32_t *__restrict__ elem_mat, const double *__restrict__ mat_tab,
                                                     const double *__restrict__ disp, double *__restrict__ strain,
                                                     double *__restrict__ stress, double *__restrict__ qforce, ThermalDev th) {
  constexpr int NN = C3El<ETYPE>::NN, NQ = C3El<ETYPE>::NQ, LPE = C3El<ETYPE>::ULPE, EPB = C3El<ETYPE>::UEPB;
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
      double tc = 0.0, t0 = 0.0, xi, et, ze, w;                              // TH: TEMPC, TEMP0 at this point
      if (TH) c3_gauss<ETYPE>(g, xi, et, ze, w);
#pragma unroll 2
      for (int a = 0; a < NN; a++) {
        const int32_t nd = conn[(size_t)NN * elem + a];
        if (TH != 2) {
#pragma unroll
          for (int i = 0; i < 3; i++) {
            const double u = disp[(size_t)3 * (nd - 1) + i];
#pragma unroll
            for (int j = 0; j < 3; j++) gu[i][j] += u * Gsh[el][g][a][j];
          }
        }
        if (TH) {
          const double h = c3_shape_func<ETYPE>(a, xi, et, ze);
          tc += h * th.temp[nd - 1];
          t0 += h * th.temp0[nd - 1];
        }
      }
      double eps[6], sg[6];
      small_strain(gu, eps);
      if (TH) {
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
          for (int c = 0; c < 6; c++) em[c] = eps[c] - em[c];
        }
        iso_stress_fixed(D11, D12, D44, em, sg);
      } else {
        iso_stress_fixed(D11, D12, D44, eps, sg);
      }
      if (TH != 2) {
        double *se = strain + ((size_t)NQ * elem + g) * 6, *ss = stress + ((size_t)NQ * elem + g) * 6;
#pragma unroll
        for (int c = 0; c < 6; c++) { se[c] = eps[c]; ss[c] = sg[c]; }
      }
#pragma unroll
      for (int c = 0; c < 6; c++) Ssh[el][g][c] = sg[c];
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
