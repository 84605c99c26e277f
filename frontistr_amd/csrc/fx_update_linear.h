// Stress update of a LINEAR static analysis on the device: fstr_UpdateNewton's element loop
// (fistr1/src/analysis/static/fstr_Update.f90:73-264) for TYPE=361 elements with isotropic ELASTIC materials, small strain:
//   ELEMOPT361 IC    UpdateST_C3D8IC  static_LIB_3dIC.f90:220-455
//              BBAR  Update_C3D8Bbar  static_LIB_C3D8.f90:203-547 (nlgeom_flag INFINITE)
//              FI    UPDATE_C3        static_LIB_3d.f90:516-837   (nlgeom_flag INFINITE)
// strain / stress at the 8 quadrature points of every element and the internal force QFORCE from the total displacement.
//
// Work decomposition: 8 lanes per element, lane g = quadrature point g (its Jacobian, strain and stress live in that lane).
// The incompatible-mode element needs the element's 9 internal dofs alpha = -Kaa^-1 (Kad u): the reference builds the whole 33x33
// matrix [Kdd Kda; Kad Kaa] for that; here Kad u = sum_g wg Ba_g^T D (B_g u) and Kaa = sum_g wg Ba_g^T D Ba_g are summed over the 8
// lanes of the element with an xor butterfly (54 values), every lane solves the 9x9 system (Cholesky, as the assembly kernel),
// strain_g = B_g u + Ba_g alpha, and the internal force [Kdd Kda][u; alpha] = sum_g wg B_g^T sigma_g is reduced the same way; lane a
// adds node a's three entries to QFORCE (hardware fp64 atomics: up to 8 elements share a node).  Same result as the
// reference's matrix products to rounding (the parity tests hold 1e-11 of the largest entry).  Included once by fistr_hip.hip.
#pragma once

#define FXU_BS 256
#define FXU_EPB (FXU_BS / 8)

__device__ __forceinline__ double sum8(double v) {  // over the 8 lanes of an element (lanes 8k .. 8k+7 of the wave)
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

// TH (fx_thermal.h): 0 no temperature (the kernel as it always was); 1 the routines' thermal branches -- stored strain = total
// strain, stress = D (strain - EPSTH), and IC's qf less its TLOAD_C3D8IC vector (3dIC.f90:337-342); 2 the thermal load vector
// alone (TLOAD_C3D8IC / TLOAD_C3D8Bbar / TLOAD_C3): no displacement read, nothing stored, qforce += sum_g wg B^T D EPSTH.
template <int ELEMOPT, int TH = 0>
__global__ __launch_bounds__(FXU_BS) void k_update_c3d8_linear(int32_t n_elem, const double *__restrict__ coord,
                                                              const int32_t *__restrict__ conn, double D11, double D12, double D44,
                                                              const int32_t *__restrict__ elem_mat,
                                                              const double *__restrict__ mat_tab, const double *__restrict__ disp,
                                                              double *__restrict__ strain, double *__restrict__ stress,
                                                              double *__restrict__ qforce, int32_t *__restrict__ err,
                                                              ThermalDev th) {
  const int el = threadIdx.x >> 3, g = threadIdx.x & 7;
  const int64_t e_raw = (int64_t)blockIdx.x * FXU_EPB + el;
  const bool active = e_raw < n_elem;
  const int32_t elem = active ? (int32_t)e_raw : n_elem - 1;  // idle lanes shadow the last element (uniform shuffles), write nothing
  const double GP = 0.577350269189626;
  if (elem_mat) {
    const int32_t mid = elem_mat[elem] - 1;
    D11 = mat_tab[3 * mid]; D12 = mat_tab[3 * mid + 1]; D44 = mat_tab[3 * mid + 2];
  }
  const double alp = TH ? th.alpha[elem_mat ? elem_mat[elem] - 1 : 0] : 0.0;
  int32_t nod[8];
  double ec[8][3], ue[8][3];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    nod[j] = conn[(size_t)8 * elem + j];
#pragma unroll
    for (int d = 0; d < 3; d++) {
      ec[j][d] = coord[(size_t)3 * (nod[j] - 1) + d];
      ue[j][d] = TH == 2 ? 0.0 : disp[(size_t)3 * (nod[j] - 1) + d];
    }
  }
  const double xi = (g & 1) ? GP : -GP, et = (g & 2) ? GP : -GP, ze = (g & 4) ? GP : -GP;
  double eth[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // EPSTH at this point; TLOAD_C3D8Bbar takes the centroid's temperatures (C3D8.f90:607-608, :688)
  if (TH) {
    const bool centre = TH == 2 && ELEMOPT == 2;
    double tc = 0.0, t0 = 0.0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const double h = centre ? 0.125 : hex8_shape_func(j, xi, et, ze);
      tc += h * th.temp[nod[j] - 1];
      t0 += h * th.temp0[nod[j] - 1];
    }
    if (TH == 2 && th.tab_idx) {  // tables (the nonlinear loop's load, the only caller with any): the coefficients and D at the POINT's temperatures (C3D8.f90:652-674)
      double pc = tc, p0 = t0, E, nu, a1, a0;
      if (centre) {
        pc = p0 = 0.0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const double h = hex8_shape_func(j, xi, et, ze);
          pc += h * th.temp[nod[j] - 1];
          p0 += h * th.temp0[nod[j] - 1];
        }
      }
      if (thermal_coefficients(th, elem_mat ? elem_mat[elem] - 1 : 0, pc, p0, a1, a0, E, nu)) elastic_constants(E, nu, D11, D12, D44);
      eth[0] = eth[1] = eth[2] = thermal_eps(a1, a0, tc, t0, th.ref_temp);
    } else {
      eth[0] = eth[1] = eth[2] = thermal_eps(alp, tc, t0, th.ref_temp);
    }
  }
  double det, inv[3][3], gd[11][3];
  double c0[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // IC: det0 * inverse Jacobian at the centre (3dIC.f90:268-270)
  double bbar[8][3];                                     // B-bar: global derivatives at the centroid (C3D8.f90:271-272)
  double vol0 = 0.0;
  if (ELEMOPT == 1 || ELEMOPT == 2) {
    hex8_global_deriv(ec, 0.0, 0.0, 0.0, det, inv, gd);
    if (ELEMOPT == 1) {
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) c0[i][j] = inv[i][j] * det;
    } else {
      double tr = 0.0;
#pragma unroll
      for (int a = 0; a < 8; a++)
#pragma unroll
        for (int d = 0; d < 3; d++) { bbar[a][d] = gd[a][d]; tr += ue[a][d] * gd[a][d]; }
      vol0 = tr / 3.0;
    }
  }
  hex8_global_deriv(ec, xi, et, ze, det, inv, gd);  // this lane's quadrature point
  const double wg = det;                             // unit weights (quadrature.f90:221)
  double gu[3][3];                                   // gdispderiv = matmul(totaldisp, gderiv)
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 8; a++) s += ue[a][i] * gd[a][j];
      gu[i][j] = s;
    }
  double eps[6];
  {
    const double dvol = (ELEMOPT == 2) ? vol0 - (gu[0][0] + gu[1][1] + gu[2][2]) / 3.0 : 0.0;
    small_strain(gu, eps);
    eps[0] += dvol; eps[1] += dvol; eps[2] += dvol;
  }
  auto stress_of = [&](const double *e, double *s) { iso_stress(D11, D12, D44, e, s); };
  double ic[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // TH, IC: Ba Kaa^-1 fa, the strain of the condensed thermal mode load
  if (ELEMOPT == 1) {
    // incompatible modes: derivatives of mode m at this point (3dIC.f90:296-298), B of the three modes, alpha
#pragma unroll
    for (int m = 0; m < 3; m++) {
      const double x = (m == 0) ? xi : ((m == 1) ? et : ze);
#pragma unroll
      for (int d = 0; d < 3; d++) gd[8 + m][d] = -2.0 * x * c0[m][d] / det;
    }
    double sc[6];
    stress_of(eps, sc);  // D B u: the compatible part
    double f[9], Kaa[45];
    // Ba^T s for a 6-vector s: column (m, d) of Ba has entries from node_B's pattern
    auto BaT = [&](int m, const double *s, double *out) {
      const double *q = gd[8 + m];
      out[0] = q[0] * s[0] + q[1] * s[3] + q[2] * s[5];
      out[1] = q[1] * s[1] + q[0] * s[3] + q[2] * s[4];
      out[2] = q[2] * s[2] + q[1] * s[4] + q[0] * s[5];
    };
#pragma unroll
    for (int m = 0; m < 3; m++) {
      double o[3];
      BaT(m, sc, o);
#pragma unroll
      for (int d = 0; d < 3; d++) f[3 * m + d] = o[d] * wg;
    }
    // Kaa (symmetric 9x9, lower triangle row-major: (i, j <= i) at i (i + 1) / 2 + j): column j = (m, d): D * Ba e_j, then Ba^T
#pragma unroll
    for (int mj = 0; mj < 3; mj++)
#pragma unroll
      for (int dj = 0; dj < 3; dj++) {
        const double *q = gd[8 + mj];
        double e[6] = {0, 0, 0, 0, 0, 0}, s[6];
        if (dj == 0) { e[0] = q[0]; e[3] = q[1]; e[5] = q[2]; }
        if (dj == 1) { e[1] = q[1]; e[3] = q[0]; e[4] = q[2]; }
        if (dj == 2) { e[2] = q[2]; e[4] = q[1]; e[5] = q[0]; }
        stress_of(e, s);
        const int j = 3 * mj + dj;
#pragma unroll
        for (int mi = 0; mi < 3; mi++) {
          double o[3];
          BaT(mi, s, o);
#pragma unroll
          for (int di = 0; di < 3; di++) {
            const int i = 3 * mi + di;
            if (i >= j) Kaa[i * (i + 1) / 2 + j] = o[di] * wg;
          }
        }
      }
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = sum8(f[k]);
#pragma unroll
    for (int k = 0; k < 45; k++) Kaa[k] = sum8(Kaa[k]);
    // Cholesky of Kaa in place (lower), alpha = -Kaa^-1 f
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 9; k++) {
      double d = Kaa[k * (k + 1) / 2 + k];
#pragma unroll
      for (int j = 0; j < k; j++) d -= Kaa[k * (k + 1) / 2 + j] * Kaa[k * (k + 1) / 2 + j];
      if (!(d > 1.0e-35)) { bad = true; d = 1.0; }
      const double lkk = sqrt(d), il = 1.0 / lkk;
      Kaa[k * (k + 1) / 2 + k] = il;  // keep the reciprocal on the diagonal
#pragma unroll
      for (int i = k + 1; i < 9; i++) {
        double v = Kaa[i * (i + 1) / 2 + k];
#pragma unroll
        for (int j = 0; j < k; j++) v -= Kaa[i * (i + 1) / 2 + j] * Kaa[k * (k + 1) / 2 + j];
        Kaa[i * (i + 1) / 2 + k] = v * il;
      }
    }
    if (bad && active && g == 0 && err) atomicExch(err, 1);
    auto kaa_solve = [&](double *v9) {  // v9 <- Kaa^-1 v9: L y = v9, then L^T x = y
#pragma unroll
      for (int q = 0; q < 9; q++) {
        double v = v9[q];
#pragma unroll
        for (int j = 0; j < q; j++) v -= Kaa[q * (q + 1) / 2 + j] * v9[j];
        v9[q] = v * Kaa[q * (q + 1) / 2 + q];
      }
#pragma unroll
      for (int q = 8; q >= 0; q--) {
        double v = v9[q];
#pragma unroll
        for (int j = q + 1; j < 9; j++) v -= Kaa[j * (j + 1) / 2 + q] * v9[j];
        v9[q] = v * Kaa[q * (q + 1) / 2 + q];
      }
    };
    double al[9];
#pragma unroll
    for (int q = 0; q < 9; q++) al[q] = -f[q];
    kaa_solve(al);
    // strain += Ba alpha (3dIC.f90:433)
#pragma unroll
    for (int m = 0; m < 3; m++) {
      const double *q = gd[8 + m], *a3 = al + 3 * m;
      eps[0] += q[0] * a3[0]; eps[1] += q[1] * a3[1]; eps[2] += q[2] * a3[2];
      eps[3] += q[1] * a3[0] + q[0] * a3[1];
      eps[4] += q[2] * a3[1] + q[1] * a3[2];
      eps[5] += q[2] * a3[0] + q[0] * a3[2];
    }
    if (TH) {
      // TLOAD_C3D8IC condensed: vect = fd - Kda Kaa^-1 fa with fa = sum_g wg Ba^T D EPSTH (3dIC.f90:611-623).  Kda y is
      // sum_g wg B^T D (Ba y), so the vector is the internal force of the strain EPSTH - Ba y: eth becomes that strain.
      double st[6], fa[9];
      stress_of(eth, st);
#pragma unroll
      for (int m = 0; m < 3; m++) {
        double o[3];
        BaT(m, st, o);
#pragma unroll
        for (int d = 0; d < 3; d++) fa[3 * m + d] = sum8(o[d] * wg);
      }
      kaa_solve(fa);
#pragma unroll
      for (int m = 0; m < 3; m++) {
        const double *q = gd[8 + m], *a3 = fa + 3 * m;
        ic[0] += q[0] * a3[0]; ic[1] += q[1] * a3[1]; ic[2] += q[2] * a3[2];
        ic[3] += q[1] * a3[0] + q[0] * a3[1];
        ic[4] += q[2] * a3[1] + q[1] * a3[2];
        ic[5] += q[2] * a3[0] + q[0] * a3[2];
      }
    }
  }
  double sg[6];
  // the stored stress in the written-out form (iso_stress_fixed), so that a temperature that causes no thermal strain gives
  // the bits of the kernel without one
  auto stored_stress_of = [&](const double *e, double *s) {
    iso_stress_fixed(D11, D12, D44, e, s);
  };
  if (TH) {  // stress = D (strain - EPSTH); the stored strain is the total one (dstrain + EPSTH, static_LIB_3d.f90:653-658)
    double em[6];
#pragma unroll
    for (int k = 0; k < 6; k++) em[k] = TH == 2 ? eth[k] : eps[k] - eth[k];
    stored_stress_of(em, sg);
  } else {
    stored_stress_of(eps, sg);
  }
  if (active && TH != 2) {
    double *se = strain + (size_t)48 * elem + 6 * g, *ss = stress + (size_t)48 * elem + 6 * g;
#pragma unroll
    for (int k = 0; k < 6; k++) { se[k] = eps[k]; ss[k] = sg[k]; }
  }
  if (TH && ELEMOPT == 1) {  // the force comes from the stress of (strain - EPSTH + Ba y), the load vector from that of (EPSTH - Ba y)
    double em[6];
#pragma unroll
    for (int k = 0; k < 6; k++) em[k] = TH == 2 ? eth[k] - ic[k] : eps[k] - eth[k] + ic[k];
    stress_of(em, sg);
  }
  // internal force: qf_a = sum_g wg B_a^T sigma_g  (B-bar: with the dilatational correction of C3D8.f90:458-481)
  double mine[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int a = 0; a < 8; a++) {
    double h[3] = {0.0, 0.0, 0.0};
    if (ELEMOPT == 2) {
#pragma unroll
      for (int d = 0; d < 3; d++) h[d] = (bbar[a][d] - gd[a][d]) / 3.0;
    }
    const double *q = gd[a];
    const double tr = sg[0] + sg[1] + sg[2];
    double o[3];
    o[0] = q[0] * sg[0] + q[1] * sg[3] + q[2] * sg[5] + h[0] * tr;
    o[1] = q[1] * sg[1] + q[0] * sg[3] + q[2] * sg[4] + h[1] * tr;
    o[2] = q[2] * sg[2] + q[1] * sg[4] + q[0] * sg[5] + h[2] * tr;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const double s = sum8(o[d] * wg);
      if (g == a) mine[d] = s;
    }
  }
  if (active) {
    int32_t mynode = nod[0];
#pragma unroll
    for (int a = 1; a < 8; a++)
      if (g == a) mynode = nod[a];
#pragma unroll
    for (int d = 0; d < 3; d++) unsafeAtomicAdd(qforce + (size_t)3 * (mynode - 1) + d, mine[d]);
  }
}

// One group's update kernel: 361 (elemopt 1..3) k_update_c3d8_linear, 341 / 342 k_update_tet, 351 / 352 / 362 k_update_c3.
// TH = 0: no temperature; 1: the thermal branch of the update; 2: the thermal load vector added to d_q (fx_thermal.h).
template <int TH>
static void launch_update_linear_th(fx_context *c, int32_t etype, int elemopt, int32_t ne, const double *d_coord, const int32_t *d_conn,
                                    double D11, double D12, double D44, const int32_t *d_emat, const double *d_mtab,
                                    const double *d_disp, double *d_strain, double *d_stress, double *d_q, int32_t *d_err,
                                    const ThermalDev &th) {
  if (with_c3_type(etype, [&](auto t) {
        constexpr int ET = decltype(t)::value;
        using El = C3El<ET>;
        const dim3 grid((unsigned)((ne + El::UEPB - 1) / El::UEPB)), blk(El::BS);
        if constexpr (El::TET)
          hipLaunchKernelGGL((k_update_tet<ET, TH>), grid, blk, 0, c->stream, ne, d_coord, d_conn, D11, D12, D44, d_emat, d_mtab, d_disp,
                             d_strain, d_stress, d_q, th);
        else
          hipLaunchKernelGGL((k_update_c3<ET, TH>), grid, blk, 0, c->stream, ne, d_coord, d_conn, D11, D12, D44, d_emat, d_mtab, d_disp,
                             d_strain, d_stress, d_q, th);
      }))
    return;
  const auto kern = elemopt == 1 ? k_update_c3d8_linear<1, TH> : (elemopt == 2 ? k_update_c3d8_linear<2, TH> : k_update_c3d8_linear<3, TH>);
  hipLaunchKernelGGL(kern, dim3((unsigned)((ne + FXU_EPB - 1) / FXU_EPB)), dim3(FXU_BS), 0, c->stream, ne, d_coord, d_conn, D11, D12, D44,
                     d_emat, d_mtab, d_disp, d_strain, d_stress, d_q, d_err, th);
}

// The caller's temperatures and expansion coefficients on the device.  `who` has checked the view (thermal_view_ok).
static int upload_thermal(fx_context *c, DevScratch &tmp, int32_t n_node, int32_t n_mat, const fx_thermal_view *tv, ThermalDev &td) {
  double *d_t = nullptr, *d_t0 = nullptr, *d_al = nullptr;
  if (tmp.alloc(&d_t, (size_t)n_node) || tmp.alloc(&d_t0, (size_t)n_node) || tmp.alloc(&d_al, (size_t)n_mat)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(d_t, tv->temp, (size_t)n_node * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_t0, tv->temp0, (size_t)n_node * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_al, tv->alpha, (size_t)n_mat * 8, hipMemcpyHostToDevice, c->stream));
  td = ThermalDev{d_t, d_t0, d_al, tv->ref_temp};
  return 0;
}
static int thermal_view_ok(const char *who, const fx_thermal_view *tv) {
  if (!tv) return fx_fail(who, FX_ERROR_RUNTIME, "thermal view missing");
  if (!tv->temp || !tv->temp0) return fx_fail(who, FX_ERROR_RUNTIME, "temperature array missing");
  if (!tv->alpha) return fx_fail(who, FX_ERROR_RUNTIME, "expansion coefficients missing");
  return 0;
}
