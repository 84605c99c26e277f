// Nonlinear C3D8 F-bar path of libfistr_hip (!SECTION, FORM361=FBAR; fx_elem_group::elemopt 4): the 361 kernels of fx_nonlinear.h with
// the B-bar terms replaced by the volume averages of fistr1/src/lib/static_LIB_Fbar.f90.
//
//   k_nl_stiffness_fbar   STF_C3D8Fbar    static_LIB_Fbar.f90:26-336, INFINITE and TOTALLAG branches
//   k_nl_update_fbar      Update_C3D8Fbar static_LIB_Fbar.f90:341-769, INFINITE and TOTALLAG branches
// The UPDATELAG branch is not restated: Update_C3D8Fbar builds `rot` there (:600-602) from the local array Fbar, which only the
// TOTALLAG branch assigns (:556), so the reference defines no result to be equal to; fx_nl_init_groups refuses such a group.
//
// The material of a quadrature point is fx_nl_point.h's as in every other family (nl_point_matrix, hyper_tangent, nl_backward_euler,
// the latch, the error word); the groups G are 0, 1, 3, 4, 5 of nl_group_flag.  What is new per element is the averaging over
// the eight points (:82-122, :418-457):
//   V0 = sum wg, jacob_ave = sum jacob wg / V0, Jratio(LX) = jacob_ave^(1/3) jacob(LX)^(-1/3) with jacob = det(I + gdispderiv),
//   gderiv1_ave = sum jacob wg gderiv1 / (V0 jacob_ave), gderiv1 the global derivatives in the end configuration (elem1),
//   gderiv2_ave(3a+p, 3b+q) = sum jacob wg (gderiv1(a,p) gderiv1(b,q) - gderiv1(b,p) gderiv1(a,q)) / (V0 jacob_ave).
// With the INFINITE flag jacob = 1 and gderiv1 = gderiv: the element is the B-bar one with the centroid derivatives replaced by
// gderiv1_ave.  V0, jacob_ave and gderiv1_ave are 8-lane shuffle butterflies over the points.  gderiv2_ave is never stored: its
// block (a, b) is antisymmetric in (p, q), three numbers, and it enters the tangent only as sum_LX (sff wg / 3) gderiv2_ave (:323,
// :325), so node row a accumulates its 8 x 3 numbers in a pass over the points and adds them once with the sum of sff wg; the
// -gderiv1_ave(a,p) gderiv1_ave(b,q) / 3 beside it (:323) is added the same way.
//
// Work decomposition as fx_nonlinear.h: 8 lanes per element, a lane is first quadrature point LX, then node row a.  The per-point
// data of the node-row loop (two sets of 24 derivatives, 21 material entries, stress, Fbar, weights) waits in LDS, 6.7 KB per
// element at TOTALLAG, which is why a workgroup is one wave of 8 elements: a node row takes its 3 x 24 block in two halves of four
// node columns, so that the loop holds 36 entries of the block and one node pair's operands in registers and nothing in scratch
// (gderiv2_ave's accumulators have a second pass of their own).  The element stride is padded by two
// doubles so that the eight elements of a wave, which read the same offset, fall on different banks.
// The reference's two `stop` statements (:114-122, :449-457) set the error word: FX_FERR_VOLUME, FX_FERR_JACOB.
#pragma once
#include "fx_nonlinear.h"

#define FXF_BLOCK 64
#define FXF_EPB (FXF_BLOCK / 8)
#define FX_FERR_VOLUME 6  // error word: `too small element volume`
#define FX_FERR_JACOB 7   //             `too small average jacob`

__device__ __forceinline__ double fbar_sum8(double v) {  // over the eight lanes of an element, the same value in each
  v += __shfl_xor(v, 1, 8);
  v += __shfl_xor(v, 2, 8);
  v += __shfl_xor(v, 4, 8);
  return v;
}

// The averages of one element from its lanes' point values: w = wg, jw = jacob wg, g1 = gderiv1 of the point.  Out: Jr = what
// multiplies jacob(LX)^(-1/3) to Jratio(LX), g1 = gderiv1_ave (all lanes), inv = 1 / (V0 jacob_ave).  The reference's two `stop`
// statements raise the error word; the arithmetic goes on (inf or NaN: no address depends on it).
__device__ __forceinline__ void fbar_averages(double w, double jw, double (&g1)[8][3], double &Jr, double &inv, int32_t *err) {
  const double V0 = fbar_sum8(w);
  double jave = fbar_sum8(jw);
#pragma unroll
  for (int b = 0; b < 8; b++)
#pragma unroll
    for (int d = 0; d < 3; d++) g1[b][d] = fbar_sum8(jw * g1[b][d]);
  if (!(fabs(V0) > 1.0e-12)) yield_raise(err, FX_FERR_VOLUME);
  else if (fabs(jave) < 1.0e-12) yield_raise(err, FX_FERR_JACOB);
  jave = jave / V0;
  Jr = pow(jave, 1.0 / 3.0);
  inv = 1.0 / (V0 * jave);
#pragma unroll
  for (int b = 0; b < 8; b++)
#pragma unroll
    for (int d = 0; d < 3; d++) g1[b][d] = g1[b][d] / (V0 * jave);
}

// Determinant33 (utilities.f90) of I + g
__device__ __forceinline__ double fbar_jacob(const double (&g)[3][3]) {
  const double a = 1.0 + g[0][0], e = 1.0 + g[1][1], i = 1.0 + g[2][2];
  return a * e * i + g[0][1] * g[1][2] * g[2][0] + g[0][2] * g[1][0] * g[2][1] - g[0][2] * e * g[2][0] - g[0][1] * g[1][0] * i -
         a * g[1][2] * g[2][1];
}

// Green-Lagrange strain of Fbar = Jr (I + g) (:207-212, :559-564) and Fbar itself, row-major
__device__ __forceinline__ void fbar_strain(double Jr, const double (&g)[3][3], double (&Fb)[9], double (&e)[6]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Fb[3 * i + j] = Jr * ((i == j ? 1.0 : 0.0) + g[i][j]);
  e[0] = 0.5 * (Fb[0] * Fb[0] + Fb[3] * Fb[3] + Fb[6] * Fb[6] - 1.0);
  e[1] = 0.5 * (Fb[1] * Fb[1] + Fb[4] * Fb[4] + Fb[7] * Fb[7] - 1.0);
  e[2] = 0.5 * (Fb[2] * Fb[2] + Fb[5] * Fb[5] + Fb[8] * Fb[8] - 1.0);
  e[3] = Fb[0] * Fb[1] + Fb[3] * Fb[4] + Fb[6] * Fb[7];
  e[4] = Fb[1] * Fb[2] + Fb[4] * Fb[5] + Fb[7] * Fb[8];
  e[5] = Fb[2] * Fb[0] + Fb[5] * Fb[3] + Fb[8] * Fb[6];
}

// BL of one node (:151-228, :661-731).  INFINITE: BL0 with the dilatational rows moved to Z = (gderiv1_ave - gderiv) / 3.
// TOTALLAG: Jratio^2 (BL0 + BL1) + BL2, BL2(r, :) = c(r) Z with c = (2 e1 + 1, 2 e2 + 1, 2 e3 + 1, 2 e4, 2 e5, 2 e6) of the point's
// F-bar strain and Z = (gderiv1_ave - gderiv1) / 3.  g: the node's gderiv (reference configuration), F = gdispderiv, J2 = Jratio^2.
template <int NLGEOM>
__device__ __forceinline__ void fbar_node_B(const double *g, const double *Z, const double (&F)[9], double J2, const double (&c)[6],
                                            double (&B)[6][3]) {
  if (NLGEOM == 0) {
    node_B(g, Z, B);
  } else {
    const double h0[3] = {0.0, 0.0, 0.0};
    nl_node_B<1>(g, h0, F, B);
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int j = 0; j < 3; j++) B[r][j] = J2 * B[r][j] + c[r] * Z[j];
  }
}

// doubles of one element in LDS: per point gderiv (24), the material matrix (21), and for TOTALLAG gderiv1 (24) and PT scalars;
// gderiv1_ave (24); two of padding (see the head of the file)
#define FXF_PT 35  // per point at TOTALLAG: 0 wg, 1 Jratio, 2 jacob wg / (V0 jacob_ave), 3 sff, 4..9 stress, 10..18 gdispderiv, 19..27 Fbar S, 28 tr(Fbar S Fbar^T), 29..34 c of BL2
template <int NLGEOM>
__device__ __forceinline__ constexpr int fbar_lds_doubles() { return NLGEOM == 1 ? 8 * (24 + 21 + 24 + FXF_PT) + 24 + 2 : 8 * (24 + 21 + 1) + 24 + 2; }

// TH: MatlMatrix with E, nu at the point's temperature (nl_thermal_matrix, fx_nl_point.h); th is read by TH = 1 alone.
template <int G, int TH = 0>
__global__ __launch_bounds__(FXF_BLOCK) void k_nl_stiffness_fbar(
    int32_t n_elem, const double *__restrict__ coord, const int32_t *__restrict__ conn, const double *__restrict__ unode,
    const double *__restrict__ dunode, NlMat m, int latch, const double *__restrict__ stress, const double *__restrict__ fstat,
    const int32_t *__restrict__ istat, const int32_t *__restrict__ indexL, const int32_t *__restrict__ itemL,
    const int32_t *__restrict__ indexU, const int32_t *__restrict__ itemU, double *__restrict__ D, double *__restrict__ AL,
    double *__restrict__ AU, double *__restrict__ Kout, int32_t *__restrict__ err, const int32_t *__restrict__ elem_list, int32_t e0,
    const int32_t *__restrict__ pos_map, int atomic, const NlMat *__restrict__ mats, const int32_t *__restrict__ emat, int kout_pos,
    const double *__restrict__ strain, ThermalDev th, NlHist hs) {
  // arguments and element lists as k_nl_stiffness
  constexpr int NLGEOM = nl_group_flag(G);
  static_assert(NLGEOM != 2, "F-bar: INFINITE and TOTALLAG only");
  constexpr int NSH = fbar_lds_doubles<NLGEOM>();
  __shared__ double sh[FXF_EPB][NSH];
  const int lane8 = threadIdx.x & 7;
  int32_t epos = e0 + blockIdx.x * FXF_EPB + (threadIdx.x >> 3);
  const bool active = epos < n_elem;
  if (!active) epos = n_elem - 1;  // keep the 8-lane group converged for the shuffles; results discarded
  const int32_t elem = elem_list ? elem_list[epos] : epos;
  if (mats) m = mats[emat[elem] - 1];
  double *const gsh = &sh[threadIdx.x >> 3][0];  // [8][24] gderiv
  double *const dsh = gsh + 8 * 24;              // [8][21] material matrix
  double *const wsh = dsh + 8 * 21;              // INFINITE: [8] wg; TOTALLAG: [8][24] gderiv1, then [8][FXF_PT]
  double *const ash = wsh + (NLGEOM == 1 ? 8 * (24 + FXF_PT) : 8);  // [24] gderiv1_ave
  {  // ---- lane = quadrature point LX
    double ec[8][3], ut[8][3];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int32_t nod = conn[(size_t)8 * elem + j];
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const size_t k = (size_t)3 * (nod - 1) + d;
        ut[j][d] = unode[k] + dunode[k];
        ec[j][d] = coord[k];
      }
    }
    const double GP = 0.577350269189626;
    const double xi = (lane8 & 1) ? GP : -GP, et = (lane8 & 2) ? GP : -GP, ze = (lane8 & 4) ? GP : -GP;
    double gd[8][3], g1[8][3], wg, jacob = 1.0;
    hex8_gderiv(ec, xi, et, ze, wg, gd);
    double g[3][3];
    if (NLGEOM == 1) {
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int d = 0; d < 3; d++) {  // gdispderiv = u . gderiv (:95)
          double s = 0.0;
#pragma unroll
          for (int a = 0; a < 8; a++) s += ut[a][c] * gd[a][d];
          g[c][d] = s;
        }
      jacob = fbar_jacob(g);
#pragma unroll
      for (int j = 0; j < 8; j++)
#pragma unroll
        for (int d = 0; d < 3; d++) ec[j][d] += ut[j][d];  // elem1
      double det1;
      hex8_gderiv(ec, xi, et, ze, det1, g1);
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++)
#pragma unroll
        for (int d = 0; d < 3; d++) g1[j][d] = gd[j][d];
    }
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
      for (int d = 0; d < 3; d++) {
        gsh[24 * lane8 + 3 * j + d] = gd[j][d];
        if (NLGEOM == 1) wsh[24 * lane8 + 3 * j + d] = g1[j][d];
      }
    double Jr, inv;
    fbar_averages(wg, jacob * wg, g1, Jr, inv, active ? err : nullptr);  // g1 is gderiv1_ave from here
#pragma unroll
    for (int b = 0; b < 8; b++)
      if (b == lane8) { ash[3 * b] = g1[b][0]; ash[3 * b + 1] = g1[b][1]; ash[3 * b + 2] = g1[b][2]; }
    double Dm[21], S[6];
#pragma unroll
    for (int i = 0; i < 6; i++) S[i] = stress[((size_t)8 * elem + lane8) * 6 + i];
    if (G == 3) {  // MatlMatrix of a hyperelastic point: from the stored strain (calMatMatrix.f90:81-86)
      double E[6];
#pragma unroll
      for (int i = 0; i < 6; i++) E[i] = strain[((size_t)8 * elem + lane8) * 6 + i];
      hyper_tangent(nl_hyper_kind(m), m.pl, E, Dm);
    } else {
      if constexpr (TH != 0)
        nl_thermal_matrix<8>(th, m, mats ? emat[elem] - 1 : 0, [&](int j) { return conn[(size_t)8 * elem + j]; },
                             [&](int j) { return hex8_shape_func(j, xi, et, ze); });
      nl_point_matrix<nl_group_yield(G)>(m, latch, NLGEOM, S, m.plastic ? istat[(size_t)8 * elem + lane8] : 0,
                                         m.plastic ? fstat[(size_t)8 * elem + lane8] : 0.0, Dm, active ? err : nullptr, nl_group_creep(G) ? hs.plstrain[(size_t)8 * elem + lane8] : 0.0);
    }
#pragma unroll
    for (int k = 0; k < 21; k++) dsh[21 * lane8 + k] = Dm[k];
    if (NLGEOM == 1) {
      double *const P = wsh + 8 * 24 + FXF_PT * lane8;
      const double Jl = Jr * pow(jacob, -1.0 / 3.0);  // Jratio(LX) (:97, :117)
      double Fb[9], e[6];
      fbar_strain(Jl, g, Fb, e);
      P[0] = wg;
      P[1] = Jl;
      P[2] = jacob * wg * inv;
      P[3] = S[0] * e[0] + S[1] * e[1] + S[2] * e[2] + S[3] * e[3] + S[4] * e[4] + S[5] * e[5];  // sff (:257)
#pragma unroll
      for (int i = 0; i < 6; i++) P[4 + i] = S[i];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int d = 0; d < 3; d++) P[10 + 3 * c + d] = g[c][d];
      double tr = 0.0;
#pragma unroll
      for (int i = 0; i < 3; i++) {  // FS = Fbar S (:305-313)
        const double f0 = Fb[3 * i], f1 = Fb[3 * i + 1], f2 = Fb[3 * i + 2];
        const double s0 = f0 * S[0] + f1 * S[3] + f2 * S[5], s1 = f0 * S[3] + f1 * S[1] + f2 * S[4], s2 = f0 * S[5] + f1 * S[4] + f2 * S[2];
        P[19 + 3 * i] = s0; P[19 + 3 * i + 1] = s1; P[19 + 3 * i + 2] = s2;
        tr += s0 * f0 + s1 * f1 + s2 * f2;
      }
      P[28] = tr;
      P[29] = 2.0 * e[0] + 1.0; P[30] = 2.0 * e[1] + 1.0; P[31] = 2.0 * e[2] + 1.0;  // c of BL2 (:217-222)
      P[32] = 2.0 * e[3]; P[33] = 2.0 * e[4]; P[34] = 2.0 * e[5];
    } else {
      wsh[lane8] = wg;
    }
  }
  // the LDS values pass between the eight lanes of one element, which share the workgroup's one wave; the barrier is what makes the
  // writes visible to the reads in the language's terms, and every lane reaches it (the idle ones shadow the last element)
  __syncthreads();
  // ---- lanes become node rows; the row block in two halves of four node columns, so that 36 and not 72 entries are held at a time
  const int a = lane8;
  const double va[3] = {ash[3 * a], ash[3 * a + 1], ash[3 * a + 2]};
  const int32_t inod = conn[(size_t)8 * elem + a];
#pragma unroll 1
  for (int b0 = 0; b0 < 8; b0 += 4) {
    double K[4][9];
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
      for (int e = 0; e < 9; e++) K[b][e] = 0.0;
    double ssum = 0.0;  // sum over the points of sff wg
#pragma unroll 1
    for (int LX = 0; LX < 8; LX++) {
      const double *const gp = gsh + 24 * LX, *const Dl = dsh + 21 * LX;
      const double ga[3] = {gp[3 * a], gp[3 * a + 1], gp[3 * a + 2]};
      double Fl[9], cr[6], Sl[6], FS[9], w, J2 = 1.0, Jl = 1.0, sff = 0.0, tr = 0.0;
      double g1a[3] = {ga[0], ga[1], ga[2]};
      const double *g1p = gp;
      if (NLGEOM == 1) {
        const double *const P = wsh + 8 * 24 + FXF_PT * LX;
        g1p = wsh + 24 * LX;
        w = P[0]; Jl = P[1]; sff = P[3]; tr = P[28];
        J2 = Jl * Jl;
#pragma unroll
        for (int i = 0; i < 6; i++) { Sl[i] = P[4 + i]; cr[i] = P[29 + i]; }
#pragma unroll
        for (int i = 0; i < 9; i++) { Fl[i] = P[10 + i]; FS[i] = P[19 + i]; }
        g1a[0] = g1p[3 * a]; g1a[1] = g1p[3 * a + 1]; g1a[2] = g1p[3 * a + 2];
        ssum += sff * w;
      } else {
        w = wsh[LX];
#pragma unroll
        for (int i = 0; i < 9; i++) Fl[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) cr[i] = 0.0;
      }
      const double Za[3] = {(va[0] - g1a[0]) / 3.0, (va[1] - g1a[1]) / 3.0, (va[2] - g1a[2]) / 3.0};
      double Ba[6][3];
      fbar_node_B<NLGEOM>(ga, Za, Fl, J2, cr, Ba);
      double sa[3] = {0.0, 0.0, 0.0}, Ga[3] = {0.0, 0.0, 0.0};  // Jratio^2 S grad N_a; GFS of node a = Jratio FS grad N_a (:316)
      if (NLGEOM == 1) {
        sa[0] = J2 * (Sl[0] * ga[0] + Sl[3] * ga[1] + Sl[5] * ga[2]);
        sa[1] = J2 * (Sl[3] * ga[0] + Sl[1] * ga[1] + Sl[4] * ga[2]);
        sa[2] = J2 * (Sl[5] * ga[0] + Sl[4] * ga[1] + Sl[2] * ga[2]);
#pragma unroll
        for (int i = 0; i < 3; i++) Ga[i] = Jl * (FS[3 * i] * ga[0] + FS[3 * i + 1] * ga[1] + FS[3 * i + 2] * ga[2]);
      }
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int bb = b0 + b;
        const double gb[3] = {gp[3 * bb], gp[3 * bb + 1], gp[3 * bb + 2]};
        const double g1b[3] = {g1p[3 * bb], g1p[3 * bb + 1], g1p[3 * bb + 2]};
        const double Zb[3] = {(ash[3 * bb] - g1b[0]) / 3.0, (ash[3 * bb + 1] - g1b[1]) / 3.0, (ash[3 * bb + 2] - g1b[2]) / 3.0};
        double Bb[6][3], DB[6][3];
        fbar_node_B<NLGEOM>(gb, Zb, Fl, J2, cr, Bb);
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
          for (int j = 0; j < 3; j++) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 6; q++) s += Dl[sym21(r, q)] * Bb[q][j];
            DB[r][j] = s;
          }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 6; q++) s += Ba[q][i] * DB[q][j];
            K[b][3 * i + j] += s * w;
          }
        if (NLGEOM == 1) {
          // initial stress matrix (1), BN^T Smat BN (:265-302), BN(3d+i, c) = Jratio gderiv(d) delta(i,c) + Fbar(i,d) Z(c):
          //   Jratio^2 (grad N_a . S grad N_b) delta(p,q) + GFSa(p) Zb(q) + Za(p) GFSb(q) + tr(Fbar S Fbar^T) Za(p) Zb(q)
          // and (2), ddFS (:314-330), without its gderiv2_ave and gderiv1_ave terms (added after the loop):
          //   sff (Za(p) Zb(q) + gderiv1(a,q) gderiv1(b,p) / 3) + Za(p) GFSb(q) + Zb(q) GFSa(p)
          double Gb[3];
#pragma unroll
          for (int i = 0; i < 3; i++) Gb[i] = Jl * (FS[3 * i] * gb[0] + FS[3 * i + 1] * gb[1] + FS[3 * i + 2] * gb[2]);
          const double geo = (sa[0] * gb[0] + sa[1] * gb[1] + sa[2] * gb[2]) * w;
          K[b][0] += geo; K[b][4] += geo; K[b][8] += geo;
#pragma unroll
          for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = 0; q < 3; q++) {
              const double zz = Za[p] * Zb[q], gz = Za[p] * Gb[q] + Zb[q] * Ga[p];
              K[b][3 * p + q] += ((gz + tr * zz) + (sff * (zz + g1a[q] * g1b[p] / 3.0) + gz)) * w;
            }
        }
      }
    }
    if (NLGEOM == 1) {  // sum_LX sff wg (gderiv2_ave(3a+p, 3b+q) - gderiv1_ave(a,p) gderiv1_ave(b,q)) / 3 (:323, :325-326)
      // a second pass over the points for the row's share of gderiv2_ave: its accumulators stay out of the loop above
      double A2[4][3];  // gderiv2_ave(3a+p, 3b+q) for (p, q) = (0,1), (0,2), (1,2)
#pragma unroll
      for (int b = 0; b < 4; b++) A2[b][0] = A2[b][1] = A2[b][2] = 0.0;
#pragma unroll 1
      for (int LX = 0; LX < 8; LX++) {
        const double *const g1p = wsh + 24 * LX;
        const double jw = wsh[8 * 24 + FXF_PT * LX + 2];
        const double g1a[3] = {g1p[3 * a], g1p[3 * a + 1], g1p[3 * a + 2]};
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const int bb = b0 + b;
          const double g1b[3] = {g1p[3 * bb], g1p[3 * bb + 1], g1p[3 * bb + 2]};
          A2[b][0] += jw * (g1a[0] * g1b[1] - g1b[0] * g1a[1]);
          A2[b][1] += jw * (g1a[0] * g1b[2] - g1b[0] * g1a[2]);
          A2[b][2] += jw * (g1a[1] * g1b[2] - g1b[1] * g1a[2]);
        }
      }
      const double s3 = ssum / 3.0;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int bb = b0 + b;
        const double vb[3] = {ash[3 * bb], ash[3 * bb + 1], ash[3 * bb + 2]};
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
          for (int q = 0; q < 3; q++) K[b][3 * p + q] -= s3 * va[p] * vb[q];
        K[b][1] += s3 * A2[b][0]; K[b][3] -= s3 * A2[b][0];
        K[b][2] += s3 * A2[b][1]; K[b][6] -= s3 * A2[b][1];
        K[b][5] += s3 * A2[b][2]; K[b][7] -= s3 * A2[b][2];
      }
    }
    if (!active) continue;
    if (Kout) {
#pragma unroll
      for (int b = 0; b < 4; b++)
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++)
            Kout[(size_t)(kout_pos ? epos : elem) * 576 + (size_t)(3 * a + i) * 24 + 3 * (b0 + b) + j] = K[b][3 * i + j];
      continue;
    }
#pragma unroll
    for (int b = 0; b < 4; b++) {  // hecmw_mat_add_node, hecmw_mat_ass.f90:72-134: the scatter of k_nl_stiffness
      const int bb = b0 + b;
      const int32_t jnod = conn[(size_t)8 * elem + bb];  // the node ids are read again, not kept across the loops above
      double *dst;
      if (inod == jnod) dst = D + (size_t)9 * (inod - 1);
      else if (jnod < inod) {
        const int32_t k = pos_map ? pos_map[(size_t)64 * elem + 8 * a + bb] : item_search(itemL, indexL[inod - 1], indexL[inod], jnod);
        if (k < 0) { if (err) atomicExch(err, 2); continue; }
        dst = AL + (size_t)9 * k;
      } else {
        const int32_t k = pos_map ? pos_map[(size_t)64 * elem + 8 * a + bb] : item_search(itemU, indexU[inod - 1], indexU[inod], jnod);
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
}

// Update_C3D8Fbar + scatter of the internal force; arguments as k_nl_update.  All of it is per point, in registers: no LDS.
// TH: the routine's thermal branch (nl_thermal_point, fx_nl_point.h); th is read by TH = 1 alone.
template <int G, int TH = 0>
__global__ __launch_bounds__(FXN_BLOCK) void k_nl_update_fbar(
    int32_t n_elem, const double *__restrict__ coord, const int32_t *__restrict__ conn, const double *__restrict__ unode,
    const double *__restrict__ dunode, NlMat m, double *__restrict__ stress, double *__restrict__ strain,
    const double *__restrict__ stress_bak, const double *__restrict__ strain_bak, const double *__restrict__ plstrain,
    double *__restrict__ fstat, int32_t *__restrict__ istat, double *__restrict__ qforce, double *__restrict__ qf_out,
    const int32_t *__restrict__ elem_list, int32_t e0, const NlMat *__restrict__ mats, const int32_t *__restrict__ emat,
    int32_t *__restrict__ err, ThermalDev th, NlHist hs) {
  constexpr int NLGEOM = nl_group_flag(G);
  static_assert(NLGEOM != 2, "F-bar: INFINITE and TOTALLAG only");
  const int LX = threadIdx.x & 7;
  int32_t epos = e0 + blockIdx.x * FXN_EPB + (threadIdx.x >> 3);
  const bool active = epos < n_elem;
  if (!active) epos = n_elem - 1;
  const int32_t elem = elem_list ? elem_list[epos] : epos;
  if (mats) m = mats[emat[elem] - 1];
  int32_t nod[8];
  double ec[8][3], td[8][3];  // reference configuration (elem0 = elem), totaldisp
#pragma unroll
  for (int j = 0; j < 8; j++) {
    nod[j] = conn[(size_t)8 * elem + j];
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const size_t k = (size_t)3 * (nod[j] - 1) + d;
      ec[j][d] = coord[k];
      td[j][d] = unode[k] + dunode[k];
    }
  }
  const double GP = 0.577350269189626;
  const double xi = (LX & 1) ? GP : -GP, et = (LX & 2) ? GP : -GP, ze = (LX & 4) ? GP : -GP;
  double gd[8][3], g1[8][3], gave[8][3], wg, jacob = 1.0;
  hex8_gderiv(ec, xi, et, ze, wg, gd);
  double g[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {  // gdispderiv (:434, :474)
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 8; a++) s += td[a][i] * gd[a][j];
      g[i][j] = s;
    }
  if (NLGEOM == 1) {
    jacob = fbar_jacob(g);
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
      for (int d = 0; d < 3; d++) ec[j][d] = (td[j][d]) + ec[j][d];  // elem1 (:404)
    double det1;
    hex8_gderiv(ec, xi, et, ze, det1, g1);
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
      for (int d = 0; d < 3; d++) g1[j][d] = gd[j][d];
  }
#pragma unroll
  for (int j = 0; j < 8; j++)
#pragma unroll
    for (int d = 0; d < 3; d++) gave[j][d] = g1[j][d];
  double Jr, inv;
  fbar_averages(wg, jacob * wg, gave, Jr, inv, active ? err : nullptr);
  double de[6], Fl[9], cr[6], J2 = 1.0, eth = 0.0;
  // EPSTH(1:3): subtracted from the strain of either branch where the routine does it (:542, :565) -- in the TOTALLAG branch
  // before the strain enters B2 of the internal force (:720-725)
  if constexpr (TH != 0)
    eth = nl_thermal_point<8>(th, m, mats ? emat[elem] - 1 : 0, [&](int j) { return nod[j]; },
                              [&](int j) { return hex8_shape_func(j, xi, et, ze); });
  if (NLGEOM == 0) {  // :532-541
    double dvol = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 8; a++) s += td[a][i] * gave[a][i];
      dvol += s;
    }
    dvol = (dvol - (g[0][0] + g[1][1] + g[2][2])) / 3.0;
    small_strain(g, de);
    de[0] += dvol; de[1] += dvol; de[2] += dvol;
    if constexpr (TH != 0) { de[0] -= eth; de[1] -= eth; de[2] -= eth; }
#pragma unroll
    for (int i = 0; i < 9; i++) Fl[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) cr[i] = 0.0;
  } else {  // :556-564
    const double Jl = Jr * pow(jacob, -1.0 / 3.0);
    double Fb[9];
    fbar_strain(Jl, g, Fb, de);
    if constexpr (TH != 0) { de[0] -= eth; de[1] -= eth; de[2] -= eth; }
    J2 = Jl * Jl;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int d = 0; d < 3; d++) Fl[3 * c + d] = g[c][d];
    cr[0] = 2.0 * de[0] + 1.0; cr[1] = 2.0 * de[1] + 1.0; cr[2] = 2.0 * de[2] + 1.0;
    cr[3] = 2.0 * de[3]; cr[4] = 2.0 * de[4]; cr[5] = 2.0 * de[5];
  }
  double sg[6];
  if (G == 3) {  // StressUpdate: 2nd Piola-Kirchhoff stress from the total strain (:567-570)
    hyper_stress(nl_hyper_kind(m), m.pl, de, sg);
  } else if constexpr (nl_group_visco(G)) {  // StressUpdate -> UpdateViscoelastic under tincr /= 0, else matmul(D, dstrain)
    nl_visco_stress<NLGEOM>(m, de, hs, (size_t)8 * elem + LX, active, sg);
  } else {
    double D11, D12, D44;
    elastic_constants(m.E, m.nu, D11, D12, D44);
    iso_stress(D11, D12, D44, de, sg);
  }
  const size_t gp = (size_t)8 * elem + LX;
  if (G != 3 && m.plastic) {  // :646-655
    int32_t ist = istat[gp];
    double fs = fstat[gp];
    nl_backward_euler<nl_group_yield(G)>(m, sg, plstrain[gp], ist, fs, active ? err : nullptr);  // idle lanes recompute the last element: they report nothing
    if (active) { istat[gp] = ist; fstat[gp] = fs; }
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < 6; i++) { stress[gp * 6 + i] = sg[i]; strain[gp * 6 + i] = TH != 0 && i < 3 ? de[i] + eth : de[i]; }
  }
  // ---- internal force of this point (:661-765); WG is taken before gderiv1 is formed (:674): the reference configuration's
  double qf[24];
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const double Zb[3] = {(gave[b][0] - g1[b][0]) / 3.0, (gave[b][1] - g1[b][1]) / 3.0, (gave[b][2] - g1[b][2]) / 3.0};
    double Bb[6][3];
    fbar_node_B<NLGEOM>(gd[b], Zb, Fl, J2, cr, Bb);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 6; q++) s += sg[q] * Bb[q][j];
      qf[3 * b + j] = s * wg;
    }
  }
#pragma unroll
  for (int k = 0; k < 24; k++) qf[k] = fbar_sum8(qf[k]);  // sum over the 8 quadrature points
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
