// Nonlinear (total / updated Lagrange, Mises elastoplastic) path of the tetrahedra TYPE=341 and TYPE=342: STF_C3
// (static_LIB_3d.f90:47-205) with `u` present and UPDATE_C3 (:516-837) without temperatures, as fstr_StiffMatrix.f90:134-144 and
// fstr_Update.f90:182-189 call them inside fstr_Newton.  The element data (shape functions, quadrature) is that of
// fx_c3_element.h, the Jacobian fx_assemble_tet.h's, the material point (nl_block_point; MatlMatrix with its latch, GEOMAT_C3, BackwardEuler, hardening) that of fx_nl_point.h.
//
// k_nl_stiffness_tet keeps the lane mapping of k_assemble_tet: the element matrix is symmetric in all three branches (D is held
// as 21 entries, the initial-stress term is symmetric), so one lane owns one upper block a <= b (10 lanes at 341, 55 at 342) and
// stores it at (a, b) and, transposed, at (b, a).  What is new against the linear kernel is data per quadrature point: the
// material matrix (21 doubles: it differs between plastic points), the stress (6) and, for TOTALLAG, the displacement gradient
// (9).  The lanes 0..NQ-1 of an element compute them with the Jacobian and stage them in LDS beside the inverse Jacobian,
// weight * determinant and global derivatives; the block lanes read them from there.
//
// k_nl_update_tet: one lane per quadrature point, as k_update_tet.  The internal force is summed over the element's lanes with
// xor shuffles and added to QFORCE with fp64 atomics.
//
// UPDATE_C3's UPDATELAG branch computes `dstress = real( matmul(D, dstrain) )` (:718): REAL() of a double-precision argument
// without KIND is default real, so the reference rounds the stress increment to single precision before it adds it to the
// stress of the last converged sub-step (Update_C3D8Bbar has no real() there).  fx_real_default() (fx_nl_point.h) restates that.
#pragma once
#include "fx_assemble_tet.h"
#include "fx_nl_point.h"

// global derivatives of node n at a point whose inverse Jacobian is inv (row-major 3x3): getGlobalDeriv, element.f90:693-744
template <int ETYPE>
__device__ __forceinline__ void tet_node_gderiv(int n, double xi, double et, double ze, const double *inv, double *g) {
  double d[3];
  c3_shape_deriv<ETYPE>(n, xi, et, ze, d);
#pragma unroll
  for (int j = 0; j < 3; j++) g[j] = d[0] * inv[j] + d[1] * inv[3 + j] + d[2] * inv[6 + j];
}

// Arguments as k_nl_stiffness.  Positions [e0, n_elem) of elem_list: elements of one NLGEOM group; atomic == 0: they are of one
// colour, scattered with plain read-modify-writes (a block whose first-write flag is set in pos_map is stored, not added to).
// Kout: element matrices out ((3 NN)^2 each, row-major, by element id), no scatter.  G: the group (nl_group_flag); strain: group 3.
// TH: MatlMatrix with E, nu at the point's temperature (nl_thermal_matrix, fx_nl_point.h); th is read by TH = 1 alone.
template <int ETYPE, int G, int TH = 0>
__global__ __launch_bounds__(C3El<ETYPE>::BS) void k_nl_stiffness_tet(int32_t n_elem, const double *__restrict__ coord,
                                                            const int32_t *__restrict__ conn, const double *__restrict__ unode,
                                                            const double *__restrict__ dunode, NlMat m, int latch,
                                                            const double *__restrict__ stress, const double *__restrict__ fstat,
                                                            const int32_t *__restrict__ istat, const int32_t *__restrict__ indexL,
                                                            const int32_t *__restrict__ itemL, const int32_t *__restrict__ indexU,
                                                            const int32_t *__restrict__ itemU, double *__restrict__ D,
                                                            double *__restrict__ AL, double *__restrict__ AU,
                                                            double *__restrict__ Kout, int32_t *__restrict__ err,
                                                            const int32_t *__restrict__ elem_list, int32_t e0,
                                                            const int32_t *__restrict__ pos_map, int atomic,
                                                            const NlMat *__restrict__ mats, const int32_t *__restrict__ emat,
                                                            const double *__restrict__ strain, ThermalDev th, NlHist hs) {
  using El = C3El<ETYPE>;
  constexpr int NLGEOM = nl_group_flag(G);
  constexpr int NN = El::NN, NQ = El::NQ, EPB = El::EPB, LPE = El::LPE, NB = El::NB;
  constexpr int NF = NLGEOM == 1 ? 9 : 1, NS = NLGEOM != 0 ? 6 : 1;
  __shared__ double Jsh[EPB][NQ][10];     // per quadrature point: inverse Jacobian (row-major), weight * determinant
  __shared__ double Gsh[EPB][NQ][NN][3];  // global derivatives of every node at every point
  __shared__ double Dsh[EPB][NQ][21];     // material matrix (MatlMatrix, minus GEOMAT_C3 for UPDATELAG), upper triangle
  __shared__ double Ssh[EPB][NQ][NS];     // stress (initial-stress term)
  __shared__ double Fsh[EPB][NQ][NF];     // gdispderiv = u . gderiv (TOTALLAG)
  const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63;
  const int el = wave * El::EPW + wl / LPE, k = wl % LPE;
  const int32_t epos = e0 + blockIdx.x * EPB + el;
  const bool active = wl < El::EPW * LPE && epos < n_elem;
  const int32_t elem = !active ? 0 : (elem_list ? elem_list[epos] : epos);
  if (active && k < NQ) {
    if (mats) m = mats[emat[elem] - 1];
    double ec[NN][3], ut[NN][3];
#pragma unroll
    for (int j = 0; j < NN; j++) {
      const int32_t nd = conn[(size_t)NN * elem + j];
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const size_t o = (size_t)3 * (nd - 1) + d;
        ec[j][d] = coord[o];
        if (NLGEOM != 0) {
          ut[j][d] = unode[o] + dunode[o];
          if (NLGEOM == 2) ec[j][d] += ut[j][d];  // elem = ecoord + u (:91)
        }
      }
    }
    double det, inv[3][3], xi, et, ze, w;
    tet_jacobian<ETYPE>(ec, k, det, inv);
    c3_gauss<ETYPE>(k, xi, et, ze, w);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Jsh[el][k][3 * i + j] = inv[i][j];
    Jsh[el][k][9] = w * det;  // wg = getWeight * det
    const size_t gp = (size_t)NQ * elem + k;
    double S[6], Dm[21];
#pragma unroll
    for (int i = 0; i < 6; i++) S[i] = stress[gp * 6 + i];
    if (G == 3) {  // MatlMatrix of a hyperelastic point: from the stored strain (calMatMatrix.f90:81-86)
      double E[6];
#pragma unroll
      for (int i = 0; i < 6; i++) E[i] = strain[gp * 6 + i];
      hyper_tangent(nl_hyper_kind(m), m.pl, E, Dm);
    } else {
      if constexpr (TH != 0)
        nl_thermal_matrix<NN>(th, m, mats ? emat[elem] - 1 : 0, [&](int j) { return conn[(size_t)NN * elem + j]; },
                              [&](int j) { return c3_shape_func<ETYPE>(j, xi, et, ze); });
      // (inside `if (active && k < NQ)`: only lanes that own a real point get here, so err needs no `active ?` guard)
      nl_point_matrix<nl_group_yield(G)>(m, latch, NLGEOM, S, m.plastic ? istat[gp] : 0, m.plastic ? fstat[gp] : 0.0, Dm, err, nl_group_creep(G) ? hs.plstrain[gp] : 0.0);
    }
#pragma unroll
    for (int i = 0; i < 21; i++) Dsh[el][k][i] = Dm[i];
    if (NLGEOM != 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) Ssh[el][k][i % NS] = S[i];
    }
    if (NLGEOM == 1) {  // gdispderiv = matmul(u, gderiv) (:136)
      double F[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int a = 0; a < NN; a++) {
        double g[3];
        tet_node_gderiv<ETYPE>(a, xi, et, ze, &inv[0][0], g);
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
          for (int d = 0; d < 3; d++) F[3 * c + d] += ut[a][c] * g[d];
      }
#pragma unroll
      for (int i = 0; i < 9; i++) Fsh[el][k][i % NF] = F[i];
    }
  }
  __syncthreads();
  if (active && k < NQ * NN) {
    const int q = k / NN, n = k % NN;
    double xi, et, ze, w;
    c3_gauss<ETYPE>(q, xi, et, ze, w);
    tet_node_gderiv<ETYPE>(n, xi, et, ze, Jsh[el][q], Gsh[el][q][n]);
  }
  __syncthreads();
  if (!active || k >= NB) return;
  int a, b;
  upper_block<NN>(k, a, b);
  BlockScatter<NN> sc;  // destinations and old values first: the reads' latency runs under the arithmetic
  if (!sc.prepare({indexL, itemL, indexU, itemU, D, AL, AU, pos_map}, Kout != nullptr, conn + (size_t)NN * elem, elem, a, b, a != b,
                  !atomic, err))
    return;
  double K[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < NQ; q++)
    nl_block_point<NLGEOM>(Gsh[el][q][a], Gsh[el][q][b], Dsh[el][q], Ssh[el][q], Fsh[el][q], Jsh[el][q][9], K);
  sc.commit(K, Kout, (size_t)elem * (9 * NN * NN));
}

// Node coordinates of the configuration x + (u + alpha du) the derivatives are taken in, and the Jacobian of point g there.
// alpha = 0.5: `(0.5 ddu + u) + ecoord` (:563), alpha = 1: `(ddu + u) + ecoord` (:564); UPDATELAG only, else the initial coordinates.
template <int ETYPE, int NLGEOM>
__device__ __forceinline__ void nl_tet_config_jacobian(const int32_t (&nod)[C3El<ETYPE>::NN], const double *__restrict__ coord,
                                                       const double *__restrict__ unode, const double *__restrict__ dunode, double alpha,
                                                       int g, double &det, double (&inv)[3][3]) {
  constexpr int NN = C3El<ETYPE>::NN;
  double ec[NN][3];
#pragma unroll
  for (int j = 0; j < NN; j++)
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const size_t o = (size_t)3 * (nod[j] - 1) + d;
      ec[j][d] = coord[o];
      if (NLGEOM == 2) ec[j][d] = (alpha * dunode[o] + unode[o]) + coord[o];
    }
  tet_jacobian<ETYPE>(ec, g, det, inv);
}

// UPDATE_C3 + scatter of the internal force.  Arguments as k_nl_update; state arrays [elem][NQ][.]; qf_out (tests): per-element
// qf[3 NN] instead of the scatter.
// TH: the routine's thermal branch (nl_thermal_point, fx_nl_point.h); th is read by TH = 1 alone.
template <int ETYPE, int G, int TH = 0>
__global__ __launch_bounds__(C3El<ETYPE>::BS) void k_nl_update_tet(int32_t n_elem, const double *__restrict__ coord,
                                                             const int32_t *__restrict__ conn, const double *__restrict__ unode,
                                                             const double *__restrict__ dunode, NlMat m, double *__restrict__ stress,
                                                             double *__restrict__ strain, const double *__restrict__ stress_bak,
                                                             const double *__restrict__ strain_bak, const double *__restrict__ plstrain,
                                                             double *__restrict__ fstat, int32_t *__restrict__ istat,
                                                             double *__restrict__ qforce, double *__restrict__ qf_out,
                                                             const int32_t *__restrict__ elem_list, int32_t e0,
                                                             const NlMat *__restrict__ mats, const int32_t *__restrict__ emat,
                                                             int32_t *__restrict__ err, ThermalDev th, NlHist hs) {
  constexpr int NLGEOM = nl_group_flag(G);
  constexpr int NN = C3El<ETYPE>::NN, NQ = C3El<ETYPE>::NQ;
  const int64_t t = (int64_t)blockIdx.x * C3El<ETYPE>::BS + threadIdx.x;
  const int g = (int)(t % NQ);
  int64_t epos = e0 + t / NQ;
  const bool active = epos < n_elem;
  if (!active) epos = n_elem - 1;  // idle lanes shadow the last element's geometry (uniform shuffles); they read no state and write nothing
  const int32_t elem = elem_list ? elem_list[epos] : (int32_t)epos;
  if (mats) m = mats[emat[elem] - 1];
  int32_t nod[NN];
#pragma unroll
  for (int j = 0; j < NN; j++) nod[j] = conn[(size_t)NN * elem + j];
  double det, inv[3][3], xi, et, ze, w;
  c3_gauss<ETYPE>(g, xi, et, ze, w);
  nl_tet_config_jacobian<ETYPE, NLGEOM>(nod, coord, unode, dunode, 0.5, g, det, inv);
  // gdispderiv = matmul(totaldisp, gderiv) (:646); totaldisp = u + ddu, or ddu for UPDATELAG (:561-566)
  double gu[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
  for (int a = 0; a < NN; a++) {
    double gd[3];
    tet_node_gderiv<ETYPE>(a, xi, et, ze, &inv[0][0], gd);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const size_t o = (size_t)3 * (nod[a] - 1) + i;
      const double td = NLGEOM == 2 ? dunode[o] : unode[o] + dunode[o];
#pragma unroll
      for (int j = 0; j < 3; j++) gu[i][j] += td * gd[j];
    }
  }
  double de[6];
  small_strain(gu, de);
  double eth = 0.0;  // EPSTH(1:3), subtracted before the Green-Lagrange terms (:653)
  if constexpr (TH != 0) {
    eth = nl_thermal_point<NN>(th, m, mats ? emat[elem] - 1 : 0, [&](int j) { return nod[j]; },
                               [&](int j) { return c3_shape_func<ETYPE>(j, xi, et, ze); });
    de[0] -= eth; de[1] -= eth; de[2] -= eth;
  }
  if (NLGEOM == 1) {  // Green-Lagrange strain (:671-679)
#pragma unroll
    for (int c = 0; c < 3; c++) de[c] += 0.5 * (gu[0][c] * gu[0][c] + gu[1][c] * gu[1][c] + gu[2][c] * gu[2][c]);
    de[3] += gu[0][0] * gu[0][1] + gu[1][0] * gu[1][1] + gu[2][0] * gu[2][1];
    de[4] += gu[0][1] * gu[0][2] + gu[1][1] * gu[1][2] + gu[2][1] * gu[2][2];
    de[5] += gu[0][0] * gu[0][2] + gu[1][0] * gu[1][2] + gu[2][0] * gu[2][2];
  }
  // MatlMatrix with isEp: the elastic matrix (the call itself sets the latch for an elastoplastic material)
  double ds[6];
  if (G == 3) {  // StressUpdate: 2nd Piola-Kirchhoff stress from the total strain (:681-684)
    hyper_stress(nl_hyper_kind(m), m.pl, de, ds);
  } else if constexpr (nl_group_visco(G)) {  // StressUpdate -> UpdateViscoelastic under tincr /= 0, else matmul(D, dstrain)
    nl_visco_stress<NLGEOM>(m, de, hs, (size_t)NQ * elem + g, active, ds);
  } else {
    double D11, D12, D44;
    elastic_constants(m.E, m.nu, D11, D12, D44);
    iso_stress(D11, D12, D44, de, ds);
  }
  const size_t gp = (size_t)NQ * elem + g;
  double sg[6], eg[6];
  if (NLGEOM == 2) {  // :702-732
    double sb[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { sb[i] = active ? stress_bak[gp * 6 + i] : 0.0; eg[i] = (active ? strain_bak[gp * 6 + i] : 0.0) + de[i]; }
    const double r01 = 0.5 * (gu[0][1] - gu[1][0]), r12 = 0.5 * (gu[1][2] - gu[2][1]), r02 = 0.5 * (gu[0][2] - gu[2][0]);
    const double rot[3][3] = {{0.0, r01, r02}, {-r01, 0.0, r12}, {-r02, -r12, 0.0}};
    const double Sb[3][3] = {{sb[0], sb[3], sb[5]}, {sb[3], sb[1], sb[4]}, {sb[5], sb[4], sb[2]}};
    double dum[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double p = 0.0, q = 0.0;
#pragma unroll
        for (int l = 0; l < 3; l++) { p += rot[i][l] * Sb[l][j]; q += Sb[i][l] * rot[l][j]; }
        dum[i][j] = p - q;
      }
    sg[0] = sb[0] + fx_real_default(ds[0]) + dum[0][0];
    sg[1] = sb[1] + fx_real_default(ds[1]) + dum[1][1];
    sg[2] = sb[2] + fx_real_default(ds[2]) + dum[2][2];
    sg[3] = sb[3] + fx_real_default(ds[3]) + dum[0][1];
    sg[4] = sb[4] + fx_real_default(ds[4]) + dum[1][2];
    sg[5] = sb[5] + fx_real_default(ds[5]) + dum[2][0];
  } else {
#pragma unroll
    for (int i = 0; i < 6; i++) { sg[i] = ds[i]; eg[i] = de[i]; }
  }
  if constexpr (TH != 0) { eg[0] += eth; eg[1] += eth; eg[2] += eth; }  // the stored strain is the total one (:657, :683-694, :707)
  if constexpr (nl_group_creep(G)) nl_creep_stress(m, sg, hs, fstat, gp, active, active ? err : nullptr);  // NORTON behind the UPDATELAG stress
  if (G != 3 && m.plastic) {
    int32_t ist = active ? istat[gp] : 0;      // idle lanes read no state another workgroup may be writing
    double fs = active ? fstat[gp] : 0.0;
    nl_backward_euler<nl_group_yield(G)>(m, sg, active ? plstrain[gp] : 0.0, ist, fs, active ? err : nullptr);  // an idle lane's stress is no point's: it reports nothing
    if (active) { istat[gp] = ist; fstat[gp] = fs; }
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < 6; i++) { stress[gp * 6 + i] = sg[i]; strain[gp * 6 + i] = eg[i]; }
  }
  // ---- internal force of this point (:767-833): UPDATELAG takes the derivatives and the determinant at the end configuration
  double F[9];
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int d = 0; d < 3; d++) F[3 * c + d] = gu[c][d];
  if (NLGEOM == 2) nl_tet_config_jacobian<ETYPE, NLGEOM>(nod, coord, unode, dunode, 1.0, g, det, inv);
  const double wg = w * det;
#pragma unroll
  for (int a = 0; a < NN; a++) {
    const double h0[3] = {0.0, 0.0, 0.0};
    double gd[3], B[6][3], o[3];
    tet_node_gderiv<ETYPE>(a, xi, et, ze, &inv[0][0], gd);
    nl_node_B<NLGEOM>(gd, h0, F, B);
#pragma unroll
    for (int d = 0; d < 3; d++) {
      double s = 0.0;
#pragma unroll
      for (int p = 0; p < 6; p++) s += sg[p] * B[p][d];
      o[d] = s * wg;
#pragma unroll
      for (int sft = 1; sft < NQ; sft <<= 1) o[d] += __shfl_xor(o[d], sft, 64);
    }
    if (active && a % NQ == g) {
#pragma unroll
      for (int d = 0; d < 3; d++) {
        if (qf_out) qf_out[(size_t)elem * (3 * NN) + 3 * a + d] = o[d];
        else unsafeAtomicAdd(qforce + (size_t)3 * (nod[a] - 1) + d, o[d]);
      }
    }
  }
}
