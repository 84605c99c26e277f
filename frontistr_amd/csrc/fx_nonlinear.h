// Nonlinear (elastoplastic, updated/total Lagrange) C3D8 B-bar path of libfistr_hip: the steps either
// side of the linear solve inside fstr_Newton (fstr_solve_NonLinear.f90:29-167).
//
//   k_nl_stiffness   fstr_StiffMatrix.f90:58-207 -> STF_C3D8Bbar static_LIB_C3D8.f90:23-200
//                    (+ GEOMAT_C3 static_LIB_3d.f90:15-37, MatlMatrix calMatMatrix.f90:28-113,
//                    calElastoPlasticMatrix Elastoplastic.f90:16-117) + hecmw_mat_ass_elem scatter
//   k_nl_update      fstr_UpdateNewton fstr_Update.f90:25-293 -> Update_C3D8Bbar static_LIB_C3D8.f90:203-547
//                    + BackwardEuler Elastoplastic.f90:351-558 (Mises, isotropic hardening; Mohr-Coulomb and Drucker-Prager:
//                    fx_yield.h, groups 4..6 of the two element kernels)
//   k_nl_residual    fstr_Update_NDForce fstr_Residual.f90:23-71
//   fx_nl_commit     fstr_UpdateState fstr_Update.f90:296-345 (k_nl_commit, fx_nl_point.h)
// The tangent of one quadrature point, its return mapping and hardening laws and the groups G are fx_nl_point.h's, shared
// with the STF_C3 families (fx_nonlinear_tet.h, fx_nonlinear_c3.h); this file holds what is 361's own: hex8_gderiv, the lane
// mapping of the two kernels, the B-bar terms, k_nl_residual.
//
// Work decomposition: 8 lanes per element (8 elements per wave64).  A lane first acts as quadrature
// point LX = lane: Jacobian, global derivatives, material matrix, stress update and return mapping of
// that point -- each of these is computed once per element, not once per row as a node-parallel
// kernel would.  For the tangent the lanes then turn into the 8 node rows: the per-point data
// (24 derivatives, 21 material entries, 6 stresses, weight) is broadcast point by point with
// 8-wide shuffles (no LDS, no barrier) and lane a accumulates its 3x24 row block in registers, which
// it scatters with the same binary search + hardware fp64 atomics as the linear assembly kernel.
// The internal force is reduced over the 8 points with a shuffle butterfly and scattered by node.
//
// The reference's `integer :: flag = 0` latch in MatlMatrix (implicitly SAVEd; see oracle/fstr_nl_oracle.c)
// is state of the context: NlDev::latch is set by the first stress update of an elastoplastic material and
// from then on the tangent uses the elastic matrix, exactly as the reference does.
#pragma once
#include "fx_nl_point.h"

#define FXN_BLOCK 256
#define FXN_EPB (FXN_BLOCK / 8)

// getGlobalDeriv for the 8 corner nodes (element.f90:693-744, :772-818)
__device__ __forceinline__ void hex8_gderiv(const double (&ec)[8][3], double xi, double et, double ze, double &det,
                                            double (&gd)[8][3]) {
  double dN[8][3];
  hex8_shape_deriv(xi, et, ze, dN);
  double J[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 8; a++) s += ec[a][i] * dN[a][j];
      J[i][j] = s;
    }
  double inv[3][3];
  invert3(J, det, inv);
#pragma unroll
  for (int a = 0; a < 8; a++)
#pragma unroll
    for (int j = 0; j < 3; j++) gd[a][j] = dN[a][0] * inv[0][j] + dN[a][1] * inv[1][j] + dN[a][2] * inv[2][j];
}

__device__ __forceinline__ double bcast8(double v, int src) { return __shfl(v, src, 8); }

// TH: MatlMatrix with E, nu at the point's temperature (nl_thermal_matrix, fx_nl_point.h); th is read by TH = 1 alone.
template <int G, int TH = 0>
__global__ __launch_bounds__(FXN_BLOCK) void k_nl_stiffness(int32_t n_elem, const double *__restrict__ coord,
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
                                                            int kout_pos, const double *__restrict__ strain, ThermalDev th, NlHist hs) {
  constexpr int NLGEOM = nl_group_flag(G);
  // positions [e0, n_elem) of elem_list: elements of one NLGEOM group; atomic == 0: they are of one colour (no shared node),
  // scattered without atomics, see k_assemble_c3d8.  mats / emat: several sections, element e uses mats[emat[e] - 1].
  // Kout: element matrices out instead of the scatter, by element id (kout_pos == 0) or by position in elem_list.
  const int lane8 = threadIdx.x & 7;
  int32_t epos = e0 + blockIdx.x * FXN_EPB + (threadIdx.x >> 3);
  const bool active = epos < n_elem;
  if (!active) epos = n_elem - 1;  // keep the 8-lane group converged for the shuffles; results discarded
  const int32_t elem = elem_list ? elem_list[epos] : epos;
  if (mats) m = mats[emat[elem] - 1];
  int32_t nod[8];
  double gd[8][3], bbar[8][3], Dm[21], S[6], F[9], wg;
  // group 3: the 21 tangent entries of every point and the element's centroid derivatives wait in LDS (42 + 6 KB a workgroup), not
  // in registers, for the node-row loop -- the TOTALLAG instantiation, whose registers it shares otherwise, spills; with one wave per
  // SIMD either way the LDS costs no occupancy
  double *Dsh = nullptr, *Bsh = nullptr;
  if constexpr (G == 3) {
    __shared__ double dsh[FXN_EPB][8][21];
    __shared__ double bsh[FXN_EPB][24];
    Dsh = &dsh[threadIdx.x >> 3][0][0];
    Bsh = &bsh[threadIdx.x >> 3][0];
  }
  {
    double ec[8][3], ut[8][3];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      nod[j] = conn[(size_t)8 * elem + j];
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const size_t k = (size_t)3 * (nod[j] - 1) + d;
        ut[j][d] = unode[k] + dunode[k];
        ec[j][d] = coord[k];
        if (NLGEOM == 2) ec[j][d] += ut[j][d];
      }
    }
    double det;
    hex8_gderiv(ec, 0.0, 0.0, 0.0, det, bbar);  // dilatation at the centroid (:72-73)
    if (G == 3) {  // the same 24 numbers in the element's eight lanes: lane b keeps node b's
#pragma unroll
      for (int b = 0; b < 8; b++)
        if (b == lane8) { Bsh[3 * b] = bbar[b][0]; Bsh[3 * b + 1] = bbar[b][1]; Bsh[3 * b + 2] = bbar[b][2]; }
    }
    const double GP = 0.577350269189626;
    const double xi = (lane8 & 1) ? GP : -GP, et = (lane8 & 2) ? GP : -GP, ze = (lane8 & 4) ? GP : -GP;
    hex8_gderiv(ec, xi, et, ze, det, gd);
    wg = det;
#pragma unroll
    for (int i = 0; i < 6; i++) S[i] = stress[((size_t)8 * elem + lane8) * 6 + i];
    if (G == 3) {  // MatlMatrix of a hyperelastic point: from the stored strain (calMatMatrix.f90:81-86)
      double E[6];
#pragma unroll
      for (int i = 0; i < 6; i++) E[i] = strain[((size_t)8 * elem + lane8) * 6 + i];
      hyper_tangent(nl_hyper_kind(m), m.pl, E, Dm);
#pragma unroll
      for (int k = 0; k < 21; k++) Dsh[21 * lane8 + k] = Dm[k];
    } else {
      if constexpr (TH != 0)
        nl_thermal_matrix<8>(th, m, mats ? emat[elem] - 1 : 0, [&](int j) { return nod[j]; }, [&](int j) { return hex8_shape_func(j, xi, et, ze); });
      nl_point_matrix<nl_group_yield(G)>(m, latch, NLGEOM, S, m.plastic ? istat[(size_t)8 * elem + lane8] : 0, m.plastic ? fstat[(size_t)8 * elem + lane8] : 0.0, Dm, active ? err : nullptr, nl_group_creep(G) ? hs.plstrain[(size_t)8 * elem + lane8] : 0.0);
    }
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = 0.0;
    if (NLGEOM == 1) {  // gdispderiv = u . gderiv (:131)
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int d = 0; d < 3; d++) {
          double s = 0.0;
#pragma unroll
          for (int a = 0; a < 8; a++) s += ut[a][c] * gd[a][d];
          F[3 * c + d] = s;
        }
    }
  }
  // the LDS values only pass between the eight lanes of one element, which share a wave; the barrier is what makes the writes
  // visible to the reads in the language's terms (no wave-level fence is relied on), and it is safe: every lane reaches it, the idle
  // ones shadow the last element.  One barrier per workgroup against eight passes over 24 x 24 blocks: not measurable.
  if (G == 3) __syncthreads();
  // ---- lanes become node rows
  const int a = lane8;
  double K[8][9];
#pragma unroll
  for (int b = 0; b < 8; b++)
#pragma unroll
    for (int e = 0; e < 9; e++) K[b][e] = 0.0;
  for (int LX = 0; LX < 8; LX++) {
    double g[8][3], Dl[21], Sl[6], Fl[9];
#pragma unroll
    for (int b = 0; b < 8; b++)
#pragma unroll
      for (int d = 0; d < 3; d++) g[b][d] = bcast8(gd[b][d], LX);
#pragma unroll
    for (int k = 0; k < 21; k++) Dl[k] = G == 3 ? Dsh[21 * LX + k] : bcast8(Dm[k], LX);
    if (NLGEOM != 0) {
#pragma unroll
      for (int k = 0; k < 6; k++) Sl[k] = bcast8(S[k], LX);
    }
    if (NLGEOM == 1) {
#pragma unroll
      for (int k = 0; k < 9; k++) Fl[k] = bcast8(F[k], LX);
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++) Fl[k] = 0.0;
    }
    const double w = bcast8(wg, LX);
    double ga[3] = {0.0, 0.0, 0.0}, ha[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < 8; b++)
      if (b == a) {
#pragma unroll
        for (int d = 0; d < 3; d++) { ga[d] = g[b][d]; ha[d] = ((G == 3 ? Bsh[3 * b + d] : bbar[b][d]) - g[b][d]) / 3.0; }
      }
    double Ba[6][3];
    nl_node_B<NLGEOM>(ga, ha, Fl, Ba);
    double sa[3] = {0.0, 0.0, 0.0};  // S . grad N_a  (initial stress matrix :164-195)
    if (NLGEOM != 0) {
      sa[0] = Sl[0] * ga[0] + Sl[3] * ga[1] + Sl[5] * ga[2];
      sa[1] = Sl[3] * ga[0] + Sl[1] * ga[1] + Sl[4] * ga[2];
      sa[2] = Sl[5] * ga[0] + Sl[4] * ga[1] + Sl[2] * ga[2];
    }
#pragma unroll
    for (int b = 0; b < 8; b++) {
      double hb[3];
#pragma unroll
      for (int d = 0; d < 3; d++) hb[d] = ((G == 3 ? Bsh[3 * b + d] : bbar[b][d]) - g[b][d]) / 3.0;
      double Bb[6][3], DB[6][3];
      nl_node_B<NLGEOM>(g[b], hb, Fl, Bb);
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < 6; q++) s += Dl[sym21(r, q)] * Bb[q][j];
          DB[r][j] = s;
        }
      double geo = 0.0;
      if (NLGEOM != 0) geo = (sa[0] * g[b][0] + sa[1] * g[b][1] + sa[2] * g[b][2]) * w;
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < 6; q++) s += Ba[q][i] * DB[q][j];
          K[b][3 * i + j] += s * w;
        }
      if (NLGEOM != 0) { K[b][0] += geo; K[b][4] += geo; K[b][8] += geo; }
    }
  }
  if (!active) return;
  if (Kout) {
#pragma unroll
    for (int b = 0; b < 8; b++)
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Kout[(size_t)(kout_pos ? epos : elem) * 576 + (size_t)(3 * a + i) * 24 + 3 * b + j] = K[b][3 * i + j];
    return;
  }
  int32_t inod = 0;
#pragma unroll
  for (int b = 0; b < 8; b++)
    if (b == a) inod = nod[b];
#pragma unroll
  for (int b = 0; b < 8; b++) {  // hecmw_mat_add_node, hecmw_mat_ass.f90:72-134
    const int32_t jnod = nod[b];
    double *dst;
    if (inod == jnod) dst = D + (size_t)9 * (inod - 1);
    else if (jnod < inod) {
      const int32_t k = pos_map ? pos_map[(size_t)64 * elem + 8 * a + b] : item_search(itemL, indexL[inod - 1], indexL[inod], jnod);
      if (k < 0) { if (err) atomicExch(err, 2); continue; }
      dst = AL + (size_t)9 * k;
    } else {
      const int32_t k = pos_map ? pos_map[(size_t)64 * elem + 8 * a + b] : item_search(itemU, indexU[inod - 1], indexU[inod], jnod);
      if (k < 0) { if (err) atomicExch(err, 2); continue; }
      dst = AU + (size_t)9 * k;
    }
    if (!atomic) {
#pragma unroll
      for (int e = 0; e < 9; e++) dst[e] += K[b][e];
    } else {
#pragma unroll
      for (int e = 0; e < 9; e++) unsafeAtomicAdd(dst + e, K[b][e]);
    }
  }
}

// Update_C3D8Bbar + scatter of the internal force.  qf_out (tests): per-element qf[24] instead of the scatter.
// TH: the routine's thermal branch (nl_thermal_point, fx_nl_point.h); th is read by TH = 1 alone.
template <int G, int TH = 0>
__global__ __launch_bounds__(FXN_BLOCK) void k_nl_update(int32_t n_elem, const double *__restrict__ coord,
                                                         const int32_t *__restrict__ conn, const double *__restrict__ unode,
                                                         const double *__restrict__ dunode, NlMat m, double *__restrict__ stress,
                                                         double *__restrict__ strain, const double *__restrict__ stress_bak,
                                                         const double *__restrict__ strain_bak, const double *__restrict__ plstrain,
                                                         double *__restrict__ fstat, int32_t *__restrict__ istat,
                                                         double *__restrict__ qforce, double *__restrict__ qf_out,
                                                         const int32_t *__restrict__ elem_list, int32_t e0,
                                                         const NlMat *__restrict__ mats, const int32_t *__restrict__ emat,
                                                         int32_t *__restrict__ err, ThermalDev th, NlHist hs) {
  // positions [e0, n_elem) of elem_list: the elements of this group; mats / emat: several sections
  constexpr int NLGEOM = nl_group_flag(G);
  const int LX = threadIdx.x & 7;
  int32_t epos = e0 + blockIdx.x * FXN_EPB + (threadIdx.x >> 3);
  const bool active = epos < n_elem;
  if (!active) epos = n_elem - 1;
  const int32_t elem = elem_list ? elem_list[epos] : epos;
  if (mats) m = mats[emat[elem] - 1];
  int32_t nod[8];
  double ec[8][3], td[8][3], e1[8][3];  // integration configuration, displacement driving the strain, end configuration
#pragma unroll
  for (int j = 0; j < 8; j++) {
    nod[j] = conn[(size_t)8 * elem + j];
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const size_t k = (size_t)3 * (nod[j] - 1) + d;
      const double u = unode[k], du = dunode[k], x = coord[k];
      if (NLGEOM == 2) {  // :255-260
        ec[j][d] = (0.5 * du + u) + x;
        e1[j][d] = (du + u) + x;
        td[j][d] = du;
      } else {
        ec[j][d] = x;
        e1[j][d] = x;
        td[j][d] = u + du;
      }
    }
  }
  double det, gd[8][3], bbar[8][3];
  hex8_gderiv(ec, 0.0, 0.0, 0.0, det, bbar);
  double vol0 = 0.0;
  {
    double dd[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 8; a++) s += td[a][i] * bbar[a][i];
      dd[i] = s;
    }
    vol0 = (dd[0] + dd[1] + dd[2]) / 3.0;
  }
  const double GP = 0.577350269189626;
  const double xi = (LX & 1) ? GP : -GP, et = (LX & 2) ? GP : -GP, ze = (LX & 4) ? GP : -GP;
  hex8_gderiv(ec, xi, et, ze, det, gd);
  double g[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 8; a++) s += td[a][i] * gd[a][j];
      g[i][j] = s;
    }
  const double dvol = vol0 - (g[0][0] + g[1][1] + g[2][2]) / 3.0;
  double de[6];
  small_strain(g, de);
  de[0] += dvol; de[1] += dvol; de[2] += dvol;
  double eth = 0.0;  // EPSTH(1:3), subtracted before the Green-Lagrange terms (:359)
  if constexpr (TH != 0) {
    eth = nl_thermal_point<8>(th, m, mats ? emat[elem] - 1 : 0, [&](int j) { return nod[j]; },
                              [&](int j) { return hex8_shape_func(j, xi, et, ze); });
    de[0] -= eth; de[1] -= eth; de[2] -= eth;
  }
  if (NLGEOM == 1) {  // Green-Lagrange strain :378-388
#pragma unroll
    for (int c = 0; c < 3; c++) de[c] += 0.5 * (g[0][c] * g[0][c] + g[1][c] * g[1][c] + g[2][c] * g[2][c]);
    de[3] += g[0][0] * g[0][1] + g[1][0] * g[1][1] + g[2][0] * g[2][1];
    de[4] += g[0][1] * g[0][2] + g[1][1] * g[1][2] + g[2][1] * g[2][2];
    de[5] += g[0][0] * g[0][2] + g[1][0] * g[1][2] + g[2][0] * g[2][2];
  }
  double ds[6];
  if (G == 3) {  // StressUpdate: 2nd Piola-Kirchhoff stress from the total strain (:387-390)
    hyper_stress(nl_hyper_kind(m), m.pl, de, ds);
  } else if constexpr (nl_group_visco(G)) {  // StressUpdate -> UpdateViscoelastic under tincr /= 0, else matmul(D, dstrain)
    nl_visco_stress<NLGEOM>(m, de, hs, (size_t)8 * elem + LX, active, ds);
  } else {
    double D11, D12, D44;
    elastic_constants(m.E, m.nu, D11, D12, D44);
    iso_stress(D11, D12, D44, de, ds);
  }
  const size_t gp = (size_t)8 * elem + LX;
  double sg[6], eg[6];
  if (NLGEOM == 2) {  // :407-432
    double sb[6], eb[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { sb[i] = stress_bak[gp * 6 + i]; eb[i] = strain_bak[gp * 6 + i]; }
    const double r01 = 0.5 * (g[0][1] - g[1][0]), r12 = 0.5 * (g[1][2] - g[2][1]), r02 = 0.5 * (g[0][2] - g[2][0]);
    const double rot[3][3] = {{0.0, r01, r02}, {-r01, 0.0, r12}, {-r02, -r12, 0.0}};
    const double Sb[3][3] = {{sb[0], sb[3], sb[5]}, {sb[3], sb[1], sb[4]}, {sb[5], sb[4], sb[2]}};
    double dum[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double p = 0.0, q = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) { p += rot[i][k] * Sb[k][j]; q += Sb[i][k] * rot[k][j]; }
        dum[i][j] = p - q;
      }
    const double t3 = 3.0 * vol0;
    sg[0] = sb[0] + ds[0] + dum[0][0] - sb[0] * t3;
    sg[1] = sb[1] + ds[1] + dum[1][1] - sb[1] * t3;
    sg[2] = sb[2] + ds[2] + dum[2][2] - sb[2] * t3;
    sg[3] = sb[3] + ds[3] + dum[0][1] - sb[3] * t3;
    sg[4] = sb[4] + ds[4] + dum[1][2] - sb[4] * t3;
    sg[5] = sb[5] + ds[5] + dum[2][0] - sb[5] * t3;
#pragma unroll
    for (int i = 0; i < 6; i++) eg[i] = eb[i] + de[i];
  } else {
#pragma unroll
    for (int i = 0; i < 6; i++) { sg[i] = ds[i]; eg[i] = de[i]; }
  }
  if constexpr (TH != 0) { eg[0] += eth; eg[1] += eth; eg[2] += eth; }  // the stored strain is the total one (:363, :389-401, :412)
  if constexpr (nl_group_creep(G)) nl_creep_stress(m, sg, hs, fstat, gp, active, active ? err : nullptr);  // NORTON behind the UPDATELAG stress
  if (G != 3 && m.plastic) {
    int32_t ist = istat[gp];
    double fs = fstat[gp];
    nl_backward_euler<nl_group_yield(G)>(m, sg, plstrain[gp], ist, fs, active ? err : nullptr);  // idle lanes recompute the last element: they report nothing
    if (active) { istat[gp] = ist; fstat[gp] = fs; }
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < 6; i++) { stress[gp * 6 + i] = sg[i]; strain[gp * 6 + i] = eg[i]; }
  }
  // ---- internal force of this point (:451-545)
  double F[9];
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int d = 0; d < 3; d++) F[3 * c + d] = g[c][d];
  if (NLGEOM == 2) {
    hex8_gderiv(e1, 0.0, 0.0, 0.0, det, bbar);  // Bbar2 at the end configuration
    hex8_gderiv(e1, xi, et, ze, det, gd);
  }
  const double wg = det;
  double qf[24];
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const double hb[3] = {(bbar[b][0] - gd[b][0]) / 3.0, (bbar[b][1] - gd[b][1]) / 3.0, (bbar[b][2] - gd[b][2]) / 3.0};
    double Bb[6][3];
    nl_node_B<NLGEOM>(gd[b], hb, F, Bb);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 6; q++) s += sg[q] * Bb[q][j];
      qf[3 * b + j] = s * wg;
    }
  }
#pragma unroll
  for (int k = 0; k < 24; k++) {  // sum over the 8 quadrature points
    double v = qf[k];
    v += __shfl_xor(v, 1, 8);
    v += __shfl_xor(v, 2, 8);
    v += __shfl_xor(v, 4, 8);
    qf[k] = v;
  }
  if (!active) return;
  double mine[3] = {0.0, 0.0, 0.0};
  int32_t inod = 0;
#pragma unroll
  for (int b = 0; b < 8; b++)
    if (b == LX) { mine[0] = qf[3 * b]; mine[1] = qf[3 * b + 1]; mine[2] = qf[3 * b + 2]; inod = nod[b]; }
  if (qf_out) {
#pragma unroll
    for (int i = 0; i < 3; i++) qf_out[(size_t)elem * 24 + 3 * LX + i] = mine[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < 3; i++) unsafeAtomicAdd(qforce + (size_t)3 * (inod - 1) + i, mine[i]);
}

// fstr_Update_NDForce: B = GL - QFORCE, prescribed dofs cleared (fstr_Residual.f90:45-47, :100-133)
__global__ void k_nl_residual(int64_t n3, const double *__restrict__ GL, const double *__restrict__ Q,
                              const uint8_t *__restrict__ flag, double *__restrict__ B) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x)
    B[i] = (flag && flag[i]) ? 0.0 : GL[i] - Q[i];
}
