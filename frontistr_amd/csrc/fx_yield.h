// Mohr-Coulomb and Drucker-Prager material point (!PLASTIC, YIELD=MOHR-COULOMB | DRUCKER-PRAGER) of the nonlinear element kernels:
// Elastoplastic.f90 restated for yield types 1 and 2 as it is written -- calYieldFunc :297-348, the yield-type branches of
// BackwardEuler :461-558 and of calElastoPlasticMatrix :69-117 -- with eigen3 of lib/utilities/utilities.f90:107-201.
//
// Material constants (fstr_ctrl_material.f90:451-469): c = M_PLCONST1, H = M_PLCONST2 (linear hardening, the card forces the hardening
// digit to 0), M_PLCONST3 = the friction angle phi in radians (Mohr-Coulomb) or eta (Drucker-Prager), M_PLCONST4 = xi (Drucker-Prager).
//
// Where the reference disagrees with itself it is followed, each place cited below:
//   * calYieldFunc (:313, :344) takes J1 as the TRACE of the stress in `eta*J1`; the Drucker-Prager return (:402, :550, :555) takes
//     J1 as the MEAN stress in `fai*(J1-K*fai*dlambda)`.
//   * calYieldFunc's Mohr-Coulomb f (:340-341) is half of the principal-stress f the return iterates on (:506-509).
//   * The Mohr-Coulomb return sets stress components below 1e-10 in magnitude to zero before the eigen-solve (:476-478).
//   * The tests |f| < tol (:386), f < 0 (:389) and, inside the returns, |f| < tol (:510, Mohr-Coulomb) and |f| < tol*tol (:551,
//     Drucker-Prager) are absolute, tol = 1e-3, whatever the stress unit; the returns run MAXITER = 5 iterations (:486, :532).
//   * `dlambda < 0` (:495-499, :540-544) resets dlambda AND istat, and the stress is still rebuilt from the trial one.
//   * The hardening coefficient inside both returns is taken at the plastic strain of the sub-step's start (:488-490, :534-536).
//   * calElastoPlasticMatrix's Mohr-Coulomb branch: | |sin 3 theta| - 1 | < 1e-8 gives C1 = 0, C2 = sqrt 3, C3 = 0 (:80-83).
//   * maxloc / minloc (:481-482) take the first of tied principal stresses; the middle index mm is 1, then 2 if the maximum or
//     minimum is at 1, then 3 if either is at 2 (:483-485).
//
// The reference's `stop` statements cannot trap on the device: each sets the kernels' error word (FX_YERR_*), the kernel completes
// and the host entry point returns FX_ERROR_RUNTIME with the reference's text.  `Math error in return mapping` (:496, :541) guards
// `cos(fai)==0` / `dum==0` inside a branch those values cannot enter (the product tested just before is then 0, not < 0); it is
// restated all the same, and every fx_nl_init* refuses such constants.
//
// Registers: eigen3's three rotations are instantiated for their compile-time (ip, iq), and the maximum / minimum / middle principal
// stress are picked and updated with selects -- no array is indexed by a run-time value, so none is placed in scratch for that.
#pragma once
#include "fx_eigen3.h"  // yield_raise, yield_eigen3 and FX_YERR_JACOBI (5): shared with the nodal stress output

#define FX_MAT_MOHR 4     // fx_material_view::plastic: YIELD=MOHR-COULOMB,  plconst = c, H, phi [rad]
#define FX_MAT_DRUCKER 5  //                            YIELD=DRUCKER-PRAGER, plconst = c, H, eta; plconst4 = xi

#define FX_YERR_MOHR 3    // error word: `Math Error in Mohr-Coulomb calculation`
#define FX_YERR_RETURN 4  //             `Math error in return mapping`

// J3 of the deviator as BackwardEuler :467-471, cal_equivalent_stress :147-151 and calElastoPlasticMatrix :74-78 write it
__device__ __forceinline__ double yield_j3(const double (&d)[6]) {
  return d[0] * d[1] * d[2] + 2.0 * d[3] * d[4] * d[5] - d[5] * d[1] * d[5] - d[3] * d[3] * d[2] - d[0] * d[4] * d[4];
}

// sin 3 theta -> theta as calYieldFunc :336-339 and BackwardEuler :472-475 do; false: the reference stops
__device__ __forceinline__ bool yield_lode(double J2, double J3, double &sita, int32_t *err) {
  sita = -3.0 * sqrt(3.0) * J3 / (2.0 * pow(J2, 1.5));
  if (fabs(fabs(sita) - 1.0) < 1.0e-8) sita = copysign(1.0, sita);
  if (fabs(sita) > 1.0) { yield_raise(err, FX_YERR_MOHR); return false; }
  sita = asin(sita) / 3.0;
  return true;
}

// BackwardEuler for yield types 1 and 2 (Elastoplastic.f90:351-400, :461-560).  kind: FX_MAT_MOHR or FX_MAT_DRUCKER;
// c, H, p3, p4 = M_PLCONST1..4; s: trial stress in, returned stress out.
__device__ __forceinline__ void yield_backward_euler(int kind, double E, double nu, double c, double H, double p3, double p4, double (&s)[6],
                                                     double plstrain, int32_t &istat, double &fstat1, int32_t *err) {
  const double tol = 1.0e-3;
  // ---- calYieldFunc :313-345 (J1 is the trace here)
  double f;
  {
    const double J1 = s[0] + s[1] + s[2];
    const double d[6] = {s[0] - J1 / 3.0, s[1] - J1 / 3.0, s[2] - J1 / 3.0, s[3], s[4], s[5]};
    const double J2 = 0.5 * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
    const double eqvs = c + H * plstrain;  // calCurrYield, linear hardening
    if (kind == FX_MAT_MOHR) {
      // :331-335 orders the products of J3 differently from the other three places
      const double J3 = d[0] * d[1] * d[2] + 2.0 * d[3] * d[4] * d[5] - d[1] * d[5] * d[5] - d[2] * d[3] * d[3] - d[0] * d[4] * d[4];
      double sita;
      if (!yield_lode(J2, J3, sita, err)) return;
      f = (cos(sita) - sin(sita) * sin(p3) / sqrt(3.0)) * sqrt(J2) + J1 * sin(p3) / 3.0 - eqvs * cos(p3);
    } else {
      f = sqrt(J2) + p3 * J1 - eqvs * p4;
    }
  }
  if (fabs(f) < tol) { istat = 1; return; }
  if (f < 0.0) { istat = 0; return; }
  istat = 1;
  double J1 = (s[0] + s[1] + s[2]) / 3.0;  // :402, the mean stress from here on
  double d[6] = {s[0] - J1, s[1] - J1, s[2] - J1, s[3], s[4], s[5]};
  const double J2 = 0.5 * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  const double G = E / (2.0 * (1.0 + nu));
  const double K = E / (3.0 * (1.0 - 2.0 * nu));
  double dlambda = 0.0, pstrain = plstrain;
  if (kind == FX_MAT_MOHR) {
    // (cal_equivalent_stress :145-157 is called too, with M_PLCONST1 read as the angle; its value is overwritten before use and its
    //  stop condition is the one calYieldFunc has passed)
    double sita;
    if (!yield_lode(J2, yield_j3(d), sita, err)) return;
    const double sf = sin(p3), cf = cos(p3), ss = sin(sita);
#pragma unroll
    for (int i = 0; i < 6; i++)
      if (fabs(s[i]) < 1.0e-10) s[i] = 0.0;  // :476-478
    double prn[3], pr[3][3];
    yield_eigen3(s, prn, pr, err);
    // maxloc / minloc: the first of ties (:481-482); mm :483-485
    int maxp = 0, minp = 0;
    double smax = prn[0], smin = prn[0];
    if (prn[1] > smax) { maxp = 1; smax = prn[1]; }
    if (prn[2] > smax) { maxp = 2; smax = prn[2]; }
    if (prn[1] < smin) { minp = 1; smin = prn[1]; }
    if (prn[2] < smin) { minp = 2; smin = prn[2]; }
    int mm = 0;
    if (maxp == 0 || minp == 0) mm = 1;
    if (maxp == 1 || minp == 1) mm = 2;
    const double stiff = 4.0 * G * (1.0 + sf * ss / 3.0) + 4.0 * K * sf * ss;
    for (int i = 0; i < 5; i++) {
      const double dd = stiff + 4.0 * H * cf * cf;
      dlambda = dlambda + f / dd;
      if (2.0 * dlambda * cf < 0.0) {
        if (cf == 0.0) yield_raise(err, FX_YERR_RETURN);
        dlambda = 0.0;
        istat = 0;
        break;
      }
      const double yd = c + H * (pstrain + 2.0 * dlambda * cf);
      f = smax - smin + (smax + smin) * sf - stiff * dlambda - 2.0 * yd * cf;
      if (fabs(f) < tol) break;
    }
    pstrain = pstrain + 2.0 * dlambda * cf;
    const double umax = (2.0 * G * (1.0 + sf / 3.0) + 2.0 * K * sf) * dlambda;
    const double umin = (2.0 * G * (1.0 - sf / 3.0) - 2.0 * K * sf) * dlambda;
    const double umid = (4.0 * G / 3.0 - 2.0 * K) * sf * dlambda;
#pragma unroll
    for (int k = 0; k < 3; k++) prn[k] = k == maxp ? prn[k] - umax : prn[k];  // :513-517, in the reference's order
#pragma unroll
    for (int k = 0; k < 3; k++) prn[k] = k == minp ? prn[k] + umin : prn[k];
#pragma unroll
    for (int k = 0; k < 3; k++) prn[k] = k == mm ? prn[k] + umid : prn[k];
    // matmul(matmul(prnprj, diag(prnstre)), transpose(prnprj)) :519-528
    double mt[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) mt[i][j] = pr[i][j] * prn[j];
#define FX_YIELD_MAT(i, j) (mt[i][0] * pr[j][0] + mt[i][1] * pr[j][1] + mt[i][2] * pr[j][2])
    s[0] = FX_YIELD_MAT(0, 0); s[1] = FX_YIELD_MAT(1, 1); s[2] = FX_YIELD_MAT(2, 2);
    s[3] = FX_YIELD_MAT(0, 1); s[4] = FX_YIELD_MAT(1, 2); s[5] = FX_YIELD_MAT(2, 0);
#undef FX_YIELD_MAT
  } else {
    const double yd = sqrt(J2);  // cal_equivalent_stress :158-159
    for (int i = 0; i < 5; i++) {
      const double dd = G + K * p3 * p3 + H * p4 * p4;
      dlambda = dlambda + f / dd;
      if (p4 * dlambda < 0.0) {
        if (p4 == 0.0) yield_raise(err, FX_YERR_RETURN);
        dlambda = 0.0;
        istat = 0;
        break;
      }
      f = c + H * (pstrain + p4 * dlambda);
      f = yd - G * dlambda + p3 * (J1 - K * p3 * dlambda) - p4 * f;
      if (fabs(f) < tol * tol) break;
    }
    pstrain = pstrain + p4 * dlambda;
    const double fac = 1.0 - G * dlambda / yd;
    J1 = J1 - K * p3 * dlambda;
    s[0] = fac * d[0] + J1; s[1] = fac * d[1] + J1; s[2] = fac * d[2] + J1;
    s[3] = fac * d[3]; s[4] = fac * d[4]; s[5] = fac * d[5];
  }
  fstat1 = pstrain;
}

// The flow vector `a` of calElastoPlasticMatrix for yield types 1 and 2 (:59-62, :72-108).  dv, J2: the deviator and its second
// invariant as :49-54 form them.  false: the reference stops (the caller leaves the matrix elastic).
__device__ __forceinline__ bool yield_flow_vector(int kind, double p3, const double (&dv)[6], double J2, double (&a)[6], int32_t *err) {
  const double q = 2.0 * sqrt(J2);
  const double dj2[6] = {dv[0] / q, dv[1] / q, dv[2] / q, 2.0 * dv[3] / q, 2.0 * dv[4] / q, 2.0 * dv[5] / q};
  if (kind == FX_MAT_DRUCKER) {
    a[0] = p3 * 1.0 + dj2[0]; a[1] = p3 * 1.0 + dj2[1]; a[2] = p3 * 1.0 + dj2[2];
    a[3] = p3 * 0.0 + dj2[3]; a[4] = p3 * 0.0 + dj2[4]; a[5] = p3 * 0.0 + dj2[5];
    return true;
  }
  double C1, C2, C3;
  double sita = -3.0 * sqrt(3.0) * yield_j3(dv) / (2.0 * pow(J2, 1.5));
  if (fabs(fabs(sita) - 1.0) < 1.0e-8) {
    C1 = 0.0; C2 = sqrt(3.0); C3 = 0.0;
  } else {
    if (fabs(sita) > 1.0) { yield_raise(err, FX_YERR_MOHR); return false; }
    sita = asin(sita) / 3.0;
    const double sf = sin(p3);
    C2 = cos(sita) * (1.0 * tan(sita) * tan(3.0 * sita) + sf * (tan(3.0 * sita) - tan(sita) / sqrt(3.0)));
    C1 = sf / 3.0;
    C3 = sqrt(3.0) * sin(sita) + cos(sita) * sf / (2.0 * J2 * cos(3.0 * sita));
  }
  const double dj3[6] = {dv[1] * dv[2] - dv[4] * dv[4] + J2 / 3.0, dv[0] * dv[2] - dv[5] * dv[5] + J2 / 3.0,
                         dv[0] * dv[1] - dv[3] * dv[3] + J2 / 3.0, 2.0 * (dv[4] * dv[5] - dv[2] * dv[3]),
                         2.0 * (dv[3] * dv[5] - dv[0] * dv[4]), 2.0 * (dv[3] * dv[4] - dv[1] * dv[5])};
#pragma unroll
  for (int i = 0; i < 6; i++) a[i] = C1 * (i < 3 ? 1.0 : 0.0) + C2 * dj2[i] + C3 * dj3[i];
  return true;
}
