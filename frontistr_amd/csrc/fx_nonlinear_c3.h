// Nonlinear (total / updated Lagrange, Mises elastoplastic) path of the wedges TYPE=351, 352 and of the 20-node hexahedron
// TYPE=362: STF_C3 (static_LIB_3d.f90:47-205) with `u` present and UPDATE_C3 (:516-837) without temperatures -- with the
// tetrahedra of fx_nonlinear_tet.h the five types fstr_StiffMatrix.f90:134-144 and fstr_Update.f90:182-189 send through these
// two routines inside fstr_Newton.  Element data: fx_c3_element.h; staging (c3_stage) and lane mappings: fx_assemble_c3.h; the
// material point (MatlMatrix with its latch, GEOMAT_C3, BackwardEuler, hardening): fx_nl_point.h.
//
// k_nl_stiffness_c3 keeps k_assemble_c3's lane mapping (one lane per upper block a <= b: 21 / 120 / 210 lanes, 12 / 2 / 1
// elements per workgroup) and its staging, in the configuration STF_C3 takes the derivatives in: ecoord + u for UPDATELAG (:91),
// ecoord otherwise.  New per quadrature point, computed by the element's lanes q < NQ (strided: 351 has 2 points for 21 lanes,
// 362 has 27) and staged in LDS beside the derivatives: the material matrix of nl_point_matrix (21 doubles), the stress (6)
// and, for TOTALLAG, gdispderiv (9).  The block lanes then loop over the points -- rolled, as in the linear kernel: nine
// accumulators and the old values of two destination blocks are what a lane holds across the loop.
//
// LDS per element, bytes (NN nodes, NQ points): X 24 NN, Jq 80 NQ, G 24 NN NQ, D 168 NQ, S 48 NQ (NLGEOM != 0), F 72 NQ (TOTALLAG):
//   351 (12 elements):   144 +  160 +   288 +  336 +   96 +  144 =  1168 ->  14.0 KB per workgroup
//   352 ( 2 elements):   360 +  720 +  3240 + 1512 +  432 +  648 =  6912 ->  13.8 KB
//   362 ( 1 element ):   480 + 2160 + 12960 + 4536 + 1296 + 1944 = 23376 ->  23.4 KB (22.8 KB = 0.5 + 2.2 + 13.0 + 4.5 + 1.3 + 1.9)
// of the 160 KB of a CU: six one-element workgroups of 362 fit beside each other, so the registers (228 VGPRs, two waves per SIMD
// for TOTALLAG, three otherwise), not the LDS, bound the occupancy.
//
// k_nl_update_c3 works on k_update_c3's layout (8 / 32 / 128 lanes per element, 32 / 8 / 2 elements per workgroup).  The
// derivatives are staged at the configuration of the strain increment (ecoord + u + ddu / 2 for UPDATELAG, :563), lanes g < NQ
// compute strain and stress of their point, run BackwardEuler, write the state and leave the stress (TOTALLAG: and gdispderiv)
// in LDS; UPDATELAG then stages again at the end configuration ecoord + u + ddu (:767-833); lanes t < 3 NN sum the internal
// force of node t / 3, component t % 3 over the points in the reference's order.  LDS per element: X + Jq + G + S + F as above,
// 27 / 43 / 38 KB per workgroup.
#pragma once
#include "fx_assemble_c3.h"
#include "fx_nl_point.h"

// Arguments as k_nl_stiffness_tet.
// TH: MatlMatrix with E, nu at the point's temperature (nl_thermal_matrix, fx_nl_point.h); th is read by TH = 1 alone.
template <int ETYPE, int G, int TH = 0>
__global__ __launch_bounds__(C3El<ETYPE>::BS) void k_nl_stiffness_c3(int32_t n_elem, const double *__restrict__ coord,
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
  __shared__ double Xsh[EPB][NN][3];
  __shared__ double Jsh[EPB][NQ][10];
  __shared__ double Gsh[EPB][NQ][NN][3];
  __shared__ double Dsh[EPB][NQ][21];  // material matrix (MatlMatrix, minus GEOMAT_C3 for UPDATELAG), upper triangle
  __shared__ double Ssh[EPB][NQ][NS];  // stress (initial-stress term)
  __shared__ double Fsh[EPB][NQ][NF];  // gdispderiv = u . gderiv (TOTALLAG)
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
  c3_stage<ETYPE, LPE, NLGEOM == 2>(active, k, elem, coord, conn, Xsh[el], Jsh[el], Gsh[el], unode, dunode, 1.0);  // elem = ecoord + u (:91)
  if (active) {
    for (int q = k; q < NQ; q += LPE) {
      if (mats) m = mats[emat[elem] - 1];
      const size_t gp = (size_t)NQ * elem + q;
      double S[6], Dm[21];
#pragma unroll
      for (int i = 0; i < 6; i++) S[i] = stress[gp * 6 + i];
      if (G == 3) {  // MatlMatrix of a hyperelastic point: from the stored strain (calMatMatrix.f90:81-86)
        double E[6];
#pragma unroll
        for (int i = 0; i < 6; i++) E[i] = strain[gp * 6 + i];
        hyper_tangent(nl_hyper_kind(m), m.pl, E, Dm);
      } else {
        if constexpr (TH != 0) {
          double xi, et, ze, w;
          c3_gauss<ETYPE>(q, xi, et, ze, w);
          nl_thermal_matrix<NN>(th, m, mats ? emat[elem] - 1 : 0, [&](int j) { return conn[(size_t)NN * elem + j]; },
                                [&](int j) { return c3_shape_func<ETYPE>(j, xi, et, ze); });
        }
        // (inside `if (active)`: only lanes that own a real point get here, so err needs no `active ?` guard as in k_nl_stiffness)
        nl_point_matrix<nl_group_yield(G)>(m, latch, NLGEOM, S, m.plastic ? istat[gp] : 0, m.plastic ? fstat[gp] : 0.0, Dm, err, nl_group_creep(G) ? hs.plstrain[gp] : 0.0);
      }
#pragma unroll
      for (int i = 0; i < 21; i++) Dsh[el][q][i] = Dm[i];
      if (NLGEOM != 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) Ssh[el][q][i % NS] = S[i];
      }
      if (NLGEOM == 1) {  // gdispderiv = matmul(u, gderiv) (:136)
        double F[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int a = 0; a < NN; a++) {
          const int32_t nd = conn[(size_t)NN * elem + a];
          const double *g = Gsh[el][q][a];
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const size_t o = (size_t)3 * (nd - 1) + c;
            const double u = unode[o] + dunode[o];
#pragma unroll
            for (int d = 0; d < 3; d++) F[3 * c + d] += u * g[d];
          }
        }
#pragma unroll
        for (int i = 0; i < 9; i++) Fsh[el][q][i % NF] = F[i];
      }
    }
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
  // The body is nl_block_point's (fx_nl_point.h), written out: called from this rolled loop, in any of five shapes tried, the
  // function costs k_nl_stiffness_c3<352, 0> and <351, 4> a wave per SIMD ("What the nonlinear element kernels share")
#pragma unroll 1
  for (int q = 0; q < NQ; q++) {
    const double h0[3] = {0.0, 0.0, 0.0};
    const double *ga = Gsh[el][q][a], *gb = Gsh[el][q][b], *Dl = Dsh[el][q];
    const double w = Jsh[el][q][9];
    double F[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (NLGEOM == 1) {
#pragma unroll
      for (int i = 0; i < 9; i++) F[i] = Fsh[el][q][i % NF];
    }
    double Ba[6][3], Bb[6][3], DB[6][3];
    nl_node_B<NLGEOM>(ga, h0, F, Ba);  // BL0 (+ BL1 for TOTALLAG, :120-162)
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
    if (NLGEOM != 0) {  // initial-stress matrix BN^T S BN (:170-199): (grad N_a . S grad N_b) on the diagonal of the block
      const double *Sl = Ssh[el][q];
      const double sb0 = Sl[0 % NS] * gb[0] + Sl[3 % NS] * gb[1] + Sl[5 % NS] * gb[2];
      const double sb1 = Sl[3 % NS] * gb[0] + Sl[1 % NS] * gb[1] + Sl[4 % NS] * gb[2];
      const double sb2 = Sl[5 % NS] * gb[0] + Sl[4 % NS] * gb[1] + Sl[2 % NS] * gb[2];
      const double geo = (ga[0] * sb0 + ga[1] * sb1 + ga[2] * sb2) * w;
      K[0] += geo; K[4] += geo; K[8] += geo;
    }
  }
  sc.commit(K, Kout, (size_t)elem * (9 * NN * NN));
}

// UPDATE_C3 + scatter of the internal force.  Arguments as k_nl_update_tet; state arrays [elem][NQ][.].
// TH: the routine's thermal branch (nl_thermal_point, fx_nl_point.h); th is read by TH = 1 alone.
template <int ETYPE, int G, int TH = 0>
__global__ __launch_bounds__(C3El<ETYPE>::BS) void k_nl_update_c3(int32_t n_elem, const double *__restrict__ coord,
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
  constexpr int NN = C3El<ETYPE>::NN, NQ = C3El<ETYPE>::NQ, LPE = C3El<ETYPE>::ULPE, EPB = C3El<ETYPE>::UEPB;
  constexpr int NF = NLGEOM == 1 ? 9 : 1;
  __shared__ double Xsh[EPB][NN][3];
  __shared__ double Jsh[EPB][NQ][10];
  __shared__ double Gsh[EPB][NQ][NN][3];
  __shared__ double Ssh[EPB][NQ][6];   // stress at every point
  __shared__ double Fsh[EPB][NQ][NF];  // gdispderiv (TOTALLAG: BL1 of the internal force)
  const int el = threadIdx.x / LPE, k = threadIdx.x % LPE;
  const int64_t epos = (int64_t)e0 + (int64_t)blockIdx.x * EPB + el;
  const bool active = epos < n_elem;  // idle lanes read no state and write nothing
  const int32_t elem = !active ? 0 : (elem_list ? elem_list[epos] : (int32_t)epos);
  // derivatives at `(0.5 ddu + u) + ecoord` (:563) for UPDATELAG, else at the initial coordinates
  c3_stage<ETYPE, LPE, NLGEOM == 2>(active, k, elem, coord, conn, Xsh[el], Jsh[el], Gsh[el], unode, dunode, 0.5);
  if (active) {
    for (int g = k; g < NQ; g += LPE) {
      if (mats) m = mats[emat[elem] - 1];
      // gdispderiv = matmul(totaldisp, gderiv) (:646); totaldisp = u + ddu, or ddu for UPDATELAG (:561-566)
      double gu[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll 1
      for (int a = 0; a < NN; a++) {
        const int32_t nd = conn[(size_t)NN * elem + a];
        const double *gd = Gsh[el][g][a];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const size_t o = (size_t)3 * (nd - 1) + i;
          const double td = NLGEOM == 2 ? dunode[o] : unode[o] + dunode[o];
#pragma unroll
          for (int j = 0; j < 3; j++) gu[i][j] += td * gd[j];
        }
      }
      double de[6];
      small_strain(gu, de);
      double eth = 0.0;  // EPSTH(1:3), subtracted before the Green-Lagrange terms (:653)
      if constexpr (TH != 0) {
        double xi, et, ze, w;
        c3_gauss<ETYPE>(g, xi, et, ze, w);
        eth = nl_thermal_point<NN>(th, m, mats ? emat[elem] - 1 : 0, [&](int j) { return conn[(size_t)NN * elem + j]; },
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
        nl_visco_stress<NLGEOM>(m, de, hs, (size_t)NQ * elem + g, true, ds);
      } else {
        double D11, D12, D44;
        elastic_constants(m.E, m.nu, D11, D12, D44);
        iso_stress(D11, D12, D44, de, ds);
      }
      const size_t gp = (size_t)NQ * elem + g;
      double sg[6], eg[6];
      if (NLGEOM == 2) {  // :702-732; the stress increment is rounded as `real()` rounds it (:718)
        double sb[6];
#pragma unroll
        for (int i = 0; i < 6; i++) { sb[i] = stress_bak[gp * 6 + i]; eg[i] = strain_bak[gp * 6 + i] + de[i]; }
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
      if constexpr (nl_group_creep(G)) nl_creep_stress(m, sg, hs, fstat, gp, true, err);  // NORTON behind the UPDATELAG stress
      if (G != 3 && m.plastic) {
        int32_t ist = istat[gp];
        double fs = fstat[gp];
        nl_backward_euler<nl_group_yield(G)>(m, sg, plstrain[gp], ist, fs, err);  // inside `if (active)`: real points only, err unguarded
        istat[gp] = ist;
        fstat[gp] = fs;
      }
#pragma unroll
      for (int i = 0; i < 6; i++) { stress[gp * 6 + i] = sg[i]; strain[gp * 6 + i] = eg[i]; Ssh[el][g][i] = sg[i]; }
      if (NLGEOM == 1) {
#pragma unroll
        for (int i = 0; i < 9; i++) Fsh[el][g][i % NF] = gu[i / 3][i % 3];
      }
    }
  }
  __syncthreads();
  // internal force (:767-833): UPDATELAG takes the derivatives and the determinant at the end configuration `(ddu + u) + ecoord` (:564)
  if (NLGEOM == 2) c3_stage<ETYPE, LPE, true>(active, k, elem, coord, conn, Xsh[el], Jsh[el], Gsh[el], unode, dunode, 1.0);
  if (!active) return;
  for (int t = k; t < 3 * NN; t += LPE) {
    const int a = t / 3, d = t % 3;
    double f = 0.0;
#pragma unroll 1
    for (int g = 0; g < NQ; g++) {
      const double h0[3] = {0.0, 0.0, 0.0};
      const double *sg = Ssh[el][g];
      double F[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, B[6][3], o[3];
      if (NLGEOM == 1) {
#pragma unroll
        for (int i = 0; i < 9; i++) F[i] = Fsh[el][g][i % NF];
      }
      nl_node_B<NLGEOM>(Gsh[el][g][a], h0, F, B);
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double s = 0.0;
#pragma unroll
        for (int p = 0; p < 6; p++) s += sg[p] * B[p][j];
        o[j] = s;
      }
      f += (d == 0 ? o[0] : (d == 1 ? o[1] : o[2])) * Jsh[el][g][9];
    }
    if (qf_out) qf_out[(size_t)elem * (3 * NN) + t] = f;
    else unsafeAtomicAdd(qforce + (size_t)3 * (conn[(size_t)NN * elem + a] - 1) + d, f);
  }
}
