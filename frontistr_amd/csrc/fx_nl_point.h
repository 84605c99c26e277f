// Point functions of the nonlinear element kernels: what does not depend on the element family a quadrature point
// belongs to.  The families (fx_nonlinear.h: 361 B-bar; fx_nonlinear_fbar.h: 361 F-bar; fx_nonlinear_tet.h: 341 / 342; fx_nonlinear_c3.h: 351 / 352 / 362) keep
// their own lane mappings, staging and their own text of the tangent and update sequences; shared are:
//
//   nl_point_matrix    material matrix of a point: MatlMatrix with its latch minus GEOMAT_C3, as STF_C3D8Bbar
//                      (static_LIB_C3D8.f90:90-101) and STF_C3 (static_LIB_3d.f90:108-119) call them
//   nl_backward_euler  the return mapping of Update_C3D8Bbar (static_LIB_C3D8.f90:446-455) and UPDATE_C3 (static_LIB_3d.f90:752-761)
//   nl_block_point     one point's share of the 3x3 block (a, b) of the tangent, BL0 (+ BL1) and the initial-stress matrix of
//                      STF_C3 (static_LIB_3d.f90:120-199)
//   nl_node_B          strain-displacement block of one node (B-bar correction and BL1 included)
// with MatlMatrix (calMatMatrix.f90:28-113), calElastoPlasticMatrix (Elastoplastic.f90:16-117), BackwardEuler (:351-558), the
// hardening laws and the table lookups underneath.  Hyperelastic points: fx_hyperelastic.h; Mohr-Coulomb / Drucker-Prager: fx_yield.h;
// viscoelastic points: fx_visco.h.
#pragma once
#include "fx_assemble.h"
#include "fx_hyperelastic.h"
#include "fx_yield.h"
#include "fx_visco.h"

// `real(x)` of a double-precision x without KIND: default real.  UPDATE_C3's UPDATELAG branch rounds the stress increment so
// (static_LIB_3d.f90:718); Update_C3D8Bbar does not.
__device__ __forceinline__ double fx_real_default(double x) { return (double)(float)x; }

// 1-D table lookups (GetTableData / GetTableGrad, ttable.f90:320-335, :221-235)
__device__ __forceinline__ double nl_table_value(const NlMat &m, double a) {
  const int n = m.ntab;
  const double *t = m.tab;
  if (a < t[1]) return t[0];
  if (a >= t[2 * (n - 1) + 1]) return t[2 * (n - 1)];
  for (int i = 0; i < n - 1; i++)
    if (a >= t[2 * i + 1] && a < t[2 * i + 3]) {
      const double lambda = (a - t[2 * i + 1]) / (t[2 * i + 3] - t[2 * i + 1]);
      return (1.0 - lambda) * t[2 * i] + lambda * t[2 * i + 2];
    }
  return t[2 * (n - 1)];
}
__device__ __forceinline__ double nl_table_grad(const NlMat &m, double a) {
  const int n = m.ntab;
  const double *t = m.tab;
  if (a < t[1]) return 0.0;
  if (a >= t[2 * (n - 1) + 1]) return 0.0;
  for (int i = 0; i < n - 1; i++)
    if (a >= t[2 * i + 1] && a < t[2 * i + 3]) return (t[2 * i + 2] - t[2 * i]) / (t[2 * i + 3] - t[2 * i + 1]);
  return 0.0;
}
// calCurrYield, Elastoplastic.f90:254-292
__device__ __forceinline__ double nl_curr_yield(const NlMat &m, double p) {
  switch (m.harden) {
    case 0: return m.pl[0] + m.pl[1] * p;
    case 1: return nl_table_value(m, p);
    case 2: return m.pl[1] * pow(m.pl[0] + p, m.pl[2]);
    case 3: return (p <= m.pl[0]) ? m.pl[1] : m.pl[1] * pow(p / m.pl[0], 1.0 / m.pl[2]);
  }
  return -1.0;
}
// calHardenCoeff, Elastoplastic.f90:175-220
__device__ __forceinline__ double nl_harden_coeff(const NlMat &m, double p) {
  switch (m.harden) {
    case 0: return m.pl[1];
    case 1: return nl_table_grad(m, p);
    case 2: return m.pl[1] * m.pl[2] * pow(m.pl[0] + p, m.pl[2] - 1.0);
    case 3: {
      const double ef = nl_curr_yield(m, p);
      return m.pl[1] * pow(ef / m.pl[1], 1.0 - m.pl[2]) / (m.pl[0] * m.pl[2]);
    }
  }
  return -1.0;
}

// BackwardEuler, Mises branch (Elastoplastic.f90:351-459, :557); Y != 0: the Mohr-Coulomb / Drucker-Prager branches of fx_yield.h, whose
// `stop` statements report through err
template <int Y = 0>
__device__ __forceinline__ void nl_backward_euler(const NlMat &m, double (&s)[6], double plstrain, int32_t &istat, double &fstat1,
                                                  int32_t *err = nullptr) {
  if constexpr (Y == 1) {
    yield_backward_euler(m.plastic, m.E, m.nu, m.pl[0], m.pl[1], m.pl[2], m.pl4, s, plstrain, istat, fstat1, err);
  } else {
    const double tol = 1.0e-3;
    const double J1 = (s[0] + s[1] + s[2]) / 3.0;
    double dv[6] = {s[0] - J1, s[1] - J1, s[2] - J1, s[3], s[4], s[5]};
    const double J2 = 0.5 * (dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]) + (dv[3] * dv[3] + dv[4] * dv[4] + dv[5] * dv[5]);
    const double yd = sqrt(3.0 * J2);
    double f = yd - nl_curr_yield(m, plstrain);
    if (fabs(f) < tol) { istat = 1; return; }
    if (f < 0.0) { istat = 0; return; }
    istat = 1;
    const double G = m.E / (2.0 * (1.0 + m.nu));
    double dlambda = 0.0;
    for (int i = 0; i < 5; i++) {
      const double H = nl_harden_coeff(m, plstrain + dlambda);
      dlambda = dlambda + f / (3.0 * G + H);
      if (dlambda < 0.0) { dlambda = 0.0; istat = 0; break; }
      f = yd - 3.0 * G * dlambda - nl_curr_yield(m, plstrain + dlambda);
      if (fabs(f) < tol * tol) break;
    }
    const double fac = 1.0 - 3.0 * dlambda * G / yd;
    s[0] = fac * dv[0] + J1; s[1] = fac * dv[1] + J1; s[2] = fac * dv[2] + J1;
    s[3] = fac * dv[3]; s[4] = fac * dv[4]; s[5] = fac * dv[5];
    fstat1 = plstrain + dlambda;
  }
}

// Thermal strain of one quadrature point of the update routines (Update_C3D8Bbar static_LIB_C3D8.f90:309-344, UPDATE_C3
// static_LIB_3d.f90:602-637, Update_C3D8Fbar static_LIB_Fbar.f90:487-522), the compile-time switch TH of the four update kernels:
// ttc = H . temperature, tt0 = H . last_temp for an elastoplastic element and H . initial condition for any other
// (fstr_Update.f90:92-102), EPSTH(1:3) = alp (ttc - ref_temp) - alp0 (tt0 - ref_temp) with MC_THEMOEXP at ttc and at tt0.  Where
// the material has an MC_ISOELASTIC table, m.E and m.nu become its values at ttc: MatlMatrix(..., ttc, isEp) and
// BackwardEuler(..., ttc) read them from there.  node(j): id of the element's node j (1-based), H(j): its shape function at the point.
template <int NN, class Node, class Shape>
__device__ __forceinline__ double nl_thermal_point(const ThermalDev &th, NlMat &m, int mid, Node &&node, Shape &&H) {
  const double *t0n = m.plastic ? th.temp0 : th.temp_init;
  double ttc = 0.0, tt0 = 0.0;
#pragma unroll
  for (int j = 0; j < NN; j++) {
    const double h = H(j);
    const int32_t nd = node(j) - 1;
    ttc += h * th.temp[nd];
    tt0 += h * t0n[nd];
  }
  double alp, alp0;
  thermal_coefficients(th, mid, ttc, tt0, alp, alp0, m.E, m.nu);
  return thermal_eps(alp, alp0, ttc, tt0, th.ref_temp);
}
// The tangent kernels' share of it (TH, launched only where a material has an MC_ISOELASTIC table): MatlMatrix's E, nu at
// tt = H . temperature (fstr_StiffMatrix.f90:72-73)
template <int NN, class Node, class Shape>
__device__ __forceinline__ void nl_thermal_matrix(const ThermalDev &th, NlMat &m, int mid, Node &&node, Shape &&H) {
  const int32_t *ix = th.tab_idx + 4 * mid;
  if (ix[3] < 1) return;
  double ttc = 0.0;
#pragma unroll
  for (int j = 0; j < NN; j++) ttc += H(j) * th.temp[node(j) - 1];
  double en[2];
  thermal_table<2>(th.tabs + ix[2], ix[3], ttc, en);
  m.E = en[0];
  m.nu = en[1];
}

// symmetric 6x6 in 21 entries, row-major upper triangle: index of (i,j), i<=j
__device__ __forceinline__ constexpr int sym21(int i, int j) { return (i <= j) ? (i * (13 - i)) / 2 + (j - i) : (j * (13 - j)) / 2 + (i - j); }

// material matrix of one quadrature point, as STF_C3D8Bbar (:90-101) and STF_C3 (static_LIB_3d.f90:108-119) use it: MatlMatrix with
// the latch, minus GEOMAT_C3 for the updated-Lagrange flag.  Y == 1: the flow vector of Mohr-Coulomb / Drucker-Prager (fx_yield.h);
// Y == 2: calViscoelasticMatrix (fx_visco.h), which MatlMatrix takes before it looks at the latch.  Y == 3: NORTON -- iso_creep
// (calMatMatrix.f90:100-107) while the latch is clear, with gauss%plstrain in `creep_dg`; the elastic matrix at dtime == 0, at an
// all-zero stress (creep.f90:40) and, as for every material but the viscoelastic one, once the latch is set.
template <int Y = 0>
__device__ __forceinline__ void nl_point_matrix(const NlMat &m, int latch, int flag, const double (&s)[6], int istat, double fstat1,
                                                double (&Dm)[21], int32_t *err = nullptr, double creep_dg = 0.0) {
  double D11, D12, D44;
  if constexpr (Y == 2) visco_constants(m, D11, D12, D44);
  else elastic_constants(m.E, m.nu, D11, D12, D44);
#pragma unroll
  for (int k = 0; k < 21; k++) Dm[k] = 0.0;
  Dm[sym21(0, 0)] = D11; Dm[sym21(1, 1)] = D11; Dm[sym21(2, 2)] = D11;
  Dm[sym21(0, 1)] = D12; Dm[sym21(0, 2)] = D12; Dm[sym21(1, 2)] = D12;
  Dm[sym21(3, 3)] = D44; Dm[sym21(4, 4)] = D44; Dm[sym21(5, 5)] = D44;
  if (m.plastic && !latch && istat != 0) {  // calElastoPlasticMatrix, Mises (:49-115)
    const double J1 = s[0] + s[1] + s[2];
    const double dv[6] = {s[0] - J1 / 3.0, s[1] - J1 / 3.0, s[2] - J1 / 3.0, s[3], s[4], s[5]};
    const double J2 = 0.5 * (dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]) + (dv[3] * dv[3] + dv[4] * dv[4] + dv[5] * dv[5]);
    double a[6];
    bool flow = true;
    if constexpr (Y == 1) {
      flow = yield_flow_vector(m.plastic, m.pl[2], dv, J2, a, err);
    } else {
      const double q = 2.0 * sqrt(J2), r3 = sqrt(3.0);
      a[0] = r3 * (dv[0] / q); a[1] = r3 * (dv[1] / q); a[2] = r3 * (dv[2] / q);
      a[3] = r3 * (2.0 * dv[3] / q); a[4] = r3 * (2.0 * dv[4] / q); a[5] = r3 * (2.0 * dv[5] / q);
    }
    if (flow) {
      double da[6];
      iso_stress(D11, D12, D44, a, da);
      double dum = 0.0;
#pragma unroll
      for (int i = 0; i < 6; i++) dum += da[i] * a[i];
      dum = nl_harden_coeff(m, fstat1) + dum;
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) Dm[sym21(i, j)] -= da[i] * da[j] / dum;
    }
  }
  if constexpr (Y == 3) {
    if (!latch && m.pl[2] != 0.0 && !(s[0] == 0.0 && s[1] == 0.0 && s[2] == 0.0 && s[3] == 0.0 && s[4] == 0.0 && s[5] == 0.0))
      norton_tangent(m, s, creep_dg, Dm);
  }
  if (flag == 2) {  // GEOMAT_C3
    Dm[sym21(0, 0)] -= 2.0 * s[0]; Dm[sym21(0, 3)] -= s[3]; Dm[sym21(0, 5)] -= s[5];
    Dm[sym21(1, 1)] -= 2.0 * s[1]; Dm[sym21(1, 3)] -= s[3]; Dm[sym21(1, 4)] -= s[4];
    Dm[sym21(2, 2)] -= 2.0 * s[2]; Dm[sym21(2, 4)] -= s[4]; Dm[sym21(2, 5)] -= s[5];
    Dm[sym21(3, 3)] -= 0.5 * (s[0] + s[1]); Dm[sym21(3, 4)] -= 0.5 * s[5]; Dm[sym21(3, 5)] -= 0.5 * s[4];
    Dm[sym21(4, 4)] -= 0.5 * (s[2] + s[1]); Dm[sym21(4, 5)] -= 0.5 * s[3];
    Dm[sym21(5, 5)] -= 0.5 * (s[0] + s[2]);
  }
}

// strain-displacement block of one node incl. the B-bar correction and, for the total-Lagrange flag, BL1
// (static_LIB_C3D8.f90:103-158, static_LIB_3d.f90:120-162): g = global derivatives of the node, h = (Bbar - g)/3 (zero for
// STF_C3), F = gdispderiv.
template <int NLGEOM>
__device__ __forceinline__ void nl_node_B(const double *g, const double *h, const double (&F)[9], double (&B)[6][3]) {
  node_B(g, h, B);
  if (NLGEOM == 1) {
#pragma unroll
    for (int c = 0; c < 3; c++) {  // F[3*c+d] = gdispderiv(c+1, d+1)
      B[0][c] += F[3 * c + 0] * g[0];
      B[1][c] += F[3 * c + 1] * g[1];
      B[2][c] += F[3 * c + 2] * g[2];
      B[3][c] += F[3 * c + 1] * g[0] + F[3 * c + 0] * g[1];
      B[4][c] += F[3 * c + 1] * g[2] + F[3 * c + 2] * g[1];
      B[5][c] += F[3 * c + 2] * g[0] + F[3 * c + 0] * g[2];
    }
  }
}

// Compile-time group G of the element kernels: 0 INFINITE, 1 TOTALLAG, 2 UPDATELAG -- the NLGEOM flag of an ELASTIC / Mises material --
// and 3: total-Lagrange kinematics with the hyperelastic point functions of fx_hyperelastic.h (the material kind, Mooney-Rivlin family
// or Arruda-Boyce, is a run-time branch on the element's NlMat).  `strain` (the points' stored strain) is read by group 3 only.
// Groups 4, 5, 6: the three flags again for a Mohr-Coulomb or Drucker-Prager material (fx_yield.h; which of the two is a run-time
// branch on NlMat::plastic).  The yield family is a compile-time parameter so that the instantiations 0..3 stay what they were:
// k_nl_stiffness<1> sits at 512 VGPRs with scratch and has no register to give to another branch.  NL_GROUPS (fx_internal.h) counts them.
// Groups 7, 8: INFINITE and TOTALLAG for a viscoelastic material (fx_visco.h), compile-time for the same reason; nl_group_yield
// names the point functions of a group: 0 ELASTIC / Mises, 1 Mohr-Coulomb / Drucker-Prager, 2 viscoelastic, 3 NORTON.
// Group 9: UPDATELAG for a NORTON material.
__host__ __device__ __forceinline__ constexpr int nl_group_flag(int G) { return G == 3 ? 1 : (G >= 7 ? G - 7 : (G >= 4 ? G - 4 : G)); }
__device__ __forceinline__ constexpr int nl_group_yield(int G) { return G == 9 ? 3 : (G >= 7 ? 2 : (G >= 4 ? 1 : 0)); }

// One quadrature point's share of the 3x3 block (a, b) of STF_C3's element matrix, added to K: Ba^T D Bb w with BL0 (+ BL1 for
// TOTALLAG, static_LIB_3d.f90:120-162) and, for NLGEOM != 0, the initial-stress matrix BN^T S BN (:170-199), which is
// (grad N_a . S grad N_b) on the block's diagonal.  ga, gb: global derivatives of the two nodes; Dl: the 21 entries of the point's
// material matrix; Sl: its stress (read for NLGEOM != 0); Fl: gdispderiv (read for TOTALLAG); w: weight * determinant.
template <int NLGEOM>
__device__ __forceinline__ void nl_block_point(const double *ga, const double *gb, const double *Dl, const double *Sl, const double *Fl,
                                               double w, double (&K)[9]) {
  const double h0[3] = {0.0, 0.0, 0.0};
  double F[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (NLGEOM == 1) {
#pragma unroll
    for (int i = 0; i < 9; i++) F[i] = Fl[i];
  }
  double Ba[6][3], Bb[6][3], DB[6][3];
  nl_node_B<NLGEOM>(ga, h0, F, Ba);
  nl_node_B<NLGEOM>(gb, h0, F, Bb);
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
#pragma unroll
      for (int p = 0; p < 6; p++) s += Dl[sym21(r, p)] * Bb[p][j];
      DB[r][j] = s;
    }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
#pragma unroll
      for (int p = 0; p < 6; p++) s += Ba[p][i] * DB[p][j];
      K[3 * i + j] += s * w;
    }
  if (NLGEOM != 0) {
    const double sb0 = Sl[0] * gb[0] + Sl[3] * gb[1] + Sl[5] * gb[2];
    const double sb1 = Sl[3] * gb[0] + Sl[1] * gb[1] + Sl[4] * gb[2];
    const double sb2 = Sl[5] * gb[0] + Sl[4] * gb[1] + Sl[2] * gb[2];
    const double geo = (ga[0] * sb0 + ga[1] * sb1 + ga[2] * sb2) * w;
    K[0] += geo; K[4] += geo; K[8] += geo;
  }
}

// fstr_UpdateState (fstr_Update.f90:296-345) for npt points, nq per element: plstrain = fstatus(1) (updateEPState) where the
// element's material is elastoplastic (isElastoplastic(pMaterial%mtype), :323-326), strain_bak / stress_bak = strain / stress
__global__ void k_nl_commit(int64_t npt, int nq, int plastic, const double *__restrict__ fstat, double *__restrict__ plstrain,
                            const double *__restrict__ stress, const double *__restrict__ strain, double *__restrict__ stress_bak,
                            double *__restrict__ strain_bak, const NlMat *__restrict__ mats, const int32_t *__restrict__ emat) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 6 * npt; i += (int64_t)gridDim.x * blockDim.x) {
    stress_bak[i] = stress[i];
    strain_bak[i] = strain[i];
    if (i < npt) {
      const int pl = mats ? mats[emat[i / nq] - 1].plastic : plastic;
      if (pl) plstrain[i] = fstat[i];
    }
  }
}
