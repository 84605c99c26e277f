// Viscoelastic material points (mtype VISCOELASTIC, card !VISCOELASTIC: one Prony row (g_n, tau_n) per term) of the nonlinear element
// kernels, restated from lib/physics/Viscoelastic.f90 as written:
//
//   visco_constants   calViscoelasticMatrix (:91-178): the isotropic tangent with G scaled by gfac; the elastic matrix at dt == 0
//   nl_visco_stress   UpdateViscoelastic (:182-277) as the update routines call it (UPDATE_C3 static_LIB_3d.f90:655-696,
//                     Update_C3D8Bbar static_LIB_C3D8.f90:361-403, Update_C3D8Fbar static_LIB_Fbar.f90:544-583): the stress from the
//                     strain handed in and the point's history; the elastic product at tincr == 0
//   k_nl_commit_visco updateViscoElasticState (:280-300), which fstr_UpdateState runs under tincr > 0 (fstr_Update.f90:333-337)
//
// NORTON creep (creep.f90) follows further down: norton_tangent, norton_update, group 9.
//
// Groups 7 (INFINITE) and 8 (TOTALLAG) of the element kernels; the card reaches no other flag (fstr_ctrl_material.f90:277-279).
// MatlMatrix tests isViscoelastic before its saved flag (calMatMatrix.f90:51): the latch never changes this tangent, and this
// material never sets it.
//
// What depends on the material and the time increment alone is formed once per fx_nl_set_time on the host (nl_apply_time /
// nl_visco_factors, fx_nonlinear_host.h) exactly as the routines form it per point -- dtau = dt / tau_n, exp_n = dexp(-dtau), dq_n = g_n hvisc(dtau,
// exp_n) with hvisc's series branch below 1e-4, mu_0 = 1 - sum g_n, gfac = sum dq_n + mu_0 in the routine's order -- and travels in
// the element's NlMat: pl[0] = mu_0, pl[1] = gfac, pl[2] = dt, tab = nrow rows (exp_n, dq_n), ntab = nrow.
//
// History of a point: fstatus(1 : 12 nrow + 6) -- per term 6 old and 6 new components of q_n, then the 6 components of the deviatoric
// strain of the last committed state.  On the device it is component-major over ALL points of the context, hist[k * stride + p]
// (stride = points of the context, p = the point's flat index), so the lanes of a wave, which are consecutive points, read and
// write consecutive doubles for every component k.  The update reads old slots and writes new ones: repeating it gives the same bits.
#pragma once
#include "fx_assemble.h"

#define FX_MAT_VISCO 7   // fx_material_view::plastic: VISCOELASTIC, tab / ntab = the Prony rows (g, tau)
#define FX_MAT_NORTON 8  //                            NORTON (card !CREEP), plconst = A, n, m

#define FX_CERR_CREEP 8   // error word: the creep iteration of update_iso_creep did not end (see norton_update)
#define FX_CREEP_CAP 100  // its bound on the device; the reference's loop has none

// A part's block of the history of the time-dependent materials (null in a context without one) and the stride between
// components; plstrain: the part's block of gauss%plstrain, which update_iso_creep writes and iso_creep reads (the update kernels
// take the array read-only for the return mappings, the tangent kernels not at all)
struct NlHist {
  double *h;
  int64_t stride;
  double *plstrain;
};

__host__ __device__ __forceinline__ constexpr bool nl_group_visco(int G) { return G == 7 || G == 8; }
__host__ __device__ __forceinline__ constexpr bool nl_group_creep(int G) { return G == 9; }

// hvisc (Viscoelastic.f90:16-31): H(x) = (1 - exp(-x)) / x
__host__ __device__ __forceinline__ double visco_hvisc(double x, double expx) {
  if (x < 1.0e-4) return 1.0 - 0.5 * x * (1.0 - x / 3.0 * (1.0 - 0.25 * x * (1.0 - 0.2 * x)));
  return (1.0 - expx) / x;
}

// calViscoelasticMatrix: D11, D12, D44 of the isotropic matrix it fills (:163-175)
__device__ __forceinline__ void visco_constants(const NlMat &m, double &D11, double &D12, double &D44) {
  if (m.pl[2] == 0.0) {  // `if( dt==0.d0 )` (:108): calElasticMatrix
    elastic_constants(m.E, m.nu, D11, D12, D44);
    return;
  }
  const double G = m.E / (2.0 * (1.0 + m.nu));
  const double K = m.E / (3.0 * (1.0 - 2.0 * m.nu));
  const double Gg = G * m.pl[1];
  const double Kg = K - 0.6666666666666666 * Gg;
  D12 = Kg;
  D11 = Kg + 2.0 * Gg;
  D44 = Gg;
}

// Stress of a viscoelastic point from the strain eps the update routine hands to StressUpdate; p: the point's index in hs, written
// only where `write` (idle lanes shadow a real point).  INFINITE: `stress = real(stress)` (static_LIB_3d.f90:665,
// static_LIB_C3D8.f90:371, static_LIB_Fbar.f90:552), a rounding to default real that the TOTALLAG branch does not have.
template <int NLGEOM>
__device__ __forceinline__ void nl_visco_stress(const NlMat &m, const double (&eps)[6], const NlHist &hs, size_t p, bool write,
                                                double (&sig)[6]) {
  if (m.pl[2] == 0.0) {  // tincr == 0: matmul(D, dstrain) with the elastic D
    double D11, D12, D44;
    elastic_constants(m.E, m.nu, D11, D12, D44);
    iso_stress(D11, D12, D44, eps, sig);
    return;
  }
  const double G = m.E / (2.0 * (1.0 + m.nu));
  const double K = m.E / (3.0 * (1.0 - 2.0 * m.nu));
  const double theta = (eps[0] + eps[1] + eps[2]) / 3.0;
  const double dev[6] = {eps[0] - theta, eps[1] - theta, eps[2] - theta, eps[3] * 0.5, eps[4] * 0.5, eps[5] * 0.5};
  const int nrow = m.ntab;
  double *h = hs.h + p;
  double en[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    en[i] = h[(int64_t)(12 * nrow + i) * hs.stride];
    sig[i] = 0.0;
  }
  for (int n = 0; n < nrow; n++) {
    const double exp_n = m.tab[2 * n], dq_n = m.tab[2 * n + 1];
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const double q = exp_n * h[(int64_t)(12 * n + i) * hs.stride] + dq_n * (dev[i] - en[i]);
      if (write) h[(int64_t)(12 * n + 6 + i) * hs.stride] = q;
      sig[i] = sig[i] + q;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) sig[i] = 2.0 * G * (m.pl[0] * dev[i] + sig[i]);
  const double Kth = K * theta * 3.0;
  sig[0] = sig[0] + Kth; sig[1] = sig[1] + Kth; sig[2] = sig[2] + Kth;
  if (NLGEOM == 0) {
#pragma unroll
    for (int i = 0; i < 6; i++) sig[i] = (double)(float)sig[i];
  }
}

// ---- NORTON creep (lib/physics/creep.f90), group 9: UPDATELAG, the card's default flag (fstr_ctrl_material.f90:502-504).
// The factor of the law that depends on the material and the time alone is formed once per fx_nl_set_time on the host
// (nl_apply_time) as iso_creep (:66) and update_iso_creep (:165) form it per point:
//   aa = A ((ttime + dtime)**(m + 1) - ttime**(m + 1)) / (m + 1)
// and travels in the element's NlMat: pl[0] = aa, pl[1] = n, pl[2] = dtime.  History: gauss%plstrain = dg of the last update (written
// by the update itself, not by the commit), fstatus(1) = eqvs (the context's fstat array and component 0 of the history),
// fstatus(2) += plstrain at a commit under tincr > 0 (updateViscoState :210-215; component 1 of the history).

// position of (i, j), i <= j, among the 21 entries of a symmetric 6x6 (sym21 of fx_nl_point.h)
__device__ __forceinline__ constexpr int norton_at(int i, int j) { return (i * (13 - i)) / 2 + (j - i); }

// iso_creep (:17-113) past its calElasticMatrix: the terms added to the 21 entries of the elastic matrix.  The caller has tested
// `dtime==0.d0 .or. all(stress==0.d0)` (:40).
__device__ __forceinline__ void norton_tangent(const NlMat &m, const double (&stress)[6], double plstrain, double (&Dm)[21]) {
  const double xxn = m.pl[1], aa = m.pl[0];
  const double G = 0.5 * m.E / (1.0 + m.nu);
  double stri[6];
#pragma unroll
  for (int i = 0; i < 6; i++) stri[i] = stress[i];
  const double p = -(stri[0] + stri[1] + stri[2]) / 3.0;
  stri[0] += p; stri[1] += p; stri[2] += p;
  const double dstri = sqrt(1.5 * (stri[0] * stri[0] + stri[1] * stri[1] + stri[2] * stri[2] +
                                   2.0 * (stri[3] * stri[3] + stri[4] * stri[4] + stri[5] * stri[5])));
#pragma unroll
  for (int i = 0; i < 6; i++) stri[i] = stri[i] / dstri;
  double eqvs = dstri;
  if (eqvs < 1.0e-10) eqvs = 1.0e-10;
  const double f = aa * pow(eqvs, xxn);
  const double df = xxn * f / eqvs;
  double c3 = 6.0 * G * G;
  const double c4 = c3 * plstrain / (dstri + 3.0 * G * plstrain);
  c3 = c4 - c3 * df / (3.0 * G * df + 1.0);
  const double c5 = c4 / 3.0;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = i; j < 6; j++) Dm[norton_at(i, j)] += c3 * stri[i] * stri[j];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    Dm[norton_at(i, i)] -= c4;
#pragma unroll
    for (int j = i; j < 3; j++) Dm[norton_at(i, j)] += c5;
  }
#pragma unroll
  for (int i = 3; i < 6; i++) Dm[norton_at(i, i)] -= c4 / 2.0;
}

// update_iso_creep (:117-207): relaxes the stress in place, dg -> plstrain, eqvs -> fstatus(1).  The reference's iteration on dg has
// no bound (`do ... if((ddg<dg*1.d-6).or.(ddg<1.d-12)) exit`, a signed test: a negative ddg exits): a purely hydrostatic non-zero
// stress gives dstri = 0, df = 0/0, and it spins.  Here it ends after FX_CREEP_CAP passes or at a dg that is not finite; the point
// then keeps its trial stress and the error word is set (FX_CERR_CREEP).  false: that happened.
__device__ __forceinline__ bool norton_update(const NlMat &m, double (&stress)[6], double &plstrain, double &fstat1, int32_t *err) {
  const double xxn = m.pl[1], aa = m.pl[0];
  const double G = 0.5 * m.E / (1.0 + m.nu);
  double stri[6];
#pragma unroll
  for (int i = 0; i < 6; i++) stri[i] = stress[i];
  const double p = -(stri[0] + stri[1] + stri[2]) / 3.0;
  stri[0] += p; stri[1] += p; stri[2] += p;
  const double dstri = sqrt(1.5 * (stri[0] * stri[0] + stri[1] * stri[1] + stri[2] * stri[2] +
                                   2.0 * (stri[3] * stri[3] + stri[4] * stri[4] + stri[5] * stri[5])));
  double dg = 0.0, eqvs = 0.0;
  bool done = false;
  for (int it = 0; it < FX_CREEP_CAP; it++) {
    eqvs = dstri - 3.0 * G * dg;
    const double f = aa * pow(eqvs, xxn);
    const double df = xxn * f / eqvs;
    const double ddg = (f - dg) / (3.0 * G * df + 1.0);
    dg = dg + ddg;
    if (!(fabs(dg) <= 1.79769313486231570e308)) break;  // NaN or infinite
    if (ddg < dg * 1.0e-6 || ddg < 1.0e-12) { done = true; break; }
  }
  if (!done) {
    if (err) atomicCAS(err, 0, FX_CERR_CREEP);
    return false;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) stri[i] = stri[i] - 3.0 * G * dg * stri[i] / dstri;
  stress[0] = stri[0] - p; stress[1] = stri[1] - p; stress[2] = stri[2] - p;
  stress[3] = stri[3]; stress[4] = stri[4]; stress[5] = stri[5];
  plstrain = dg;
  fstat1 = eqvs;
  return true;
}

// The NORTON branch behind the UPDATELAG stress of the update routines (static_LIB_3d.f90:736-746, static_LIB_C3D8.f90:433-442):
// `tincr /= 0 .AND. any(stress /= 0)`, then StressUpdate -> update_iso_creep; fstat: the point's entry of the context's array
__device__ __forceinline__ void nl_creep_stress(const NlMat &m, double (&sg)[6], const NlHist &hs, double *fstat, size_t p, bool write,
                                                int32_t *err) {
  if (m.pl[2] == 0.0) return;
  if (sg[0] == 0.0 && sg[1] == 0.0 && sg[2] == 0.0 && sg[3] == 0.0 && sg[4] == 0.0 && sg[5] == 0.0) return;
  double dg = 0.0, eqvs = 0.0;
  if (!norton_update(m, sg, dg, eqvs, err) || !write) return;
  hs.plstrain[p] = dg;
  fstat[p] = eqvs;
  hs.h[p] = eqvs;
}

// fstatus(1) of the NORTON points between the context's fstat array and component 0 of the history, after a transfer into either
__global__ void k_nl_creep_fstat(int64_t npt, int nq, NlMat m, const NlMat *__restrict__ mats, const int32_t *__restrict__ emat,
                                 double *__restrict__ fstat, NlHist hs, int to_fstat) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npt; p += (int64_t)gridDim.x * blockDim.x) {
    if (mats) m = mats[emat[p / nq] - 1];
    if (!nl_group_creep(m.group)) continue;
    if (to_fstat) fstat[p] = hs.h[p];
    else hs.h[p] = fstat[p];
  }
}

// updateViscoElasticState / updateViscoState for the npt points of one part (nq per element): new q -> old q and the deviator of
// gauss%strain; fstatus(2) += plstrain
__global__ void k_nl_commit_visco(int64_t npt, int nq, NlMat m, const NlMat *__restrict__ mats, const int32_t *__restrict__ emat,
                                  const double *__restrict__ strain, NlHist hs) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npt; p += (int64_t)gridDim.x * blockDim.x) {
    if (mats) m = mats[emat[p / nq] - 1];
    if (nl_group_creep(m.group)) hs.h[hs.stride + p] = hs.h[hs.stride + p] + hs.plstrain[p];
    if (!nl_group_visco(m.group)) continue;
    const int nrow = m.ntab;
    double *h = hs.h + p;
    for (int n = 0; n < nrow; n++)
#pragma unroll
      for (int i = 0; i < 6; i++) h[(int64_t)(12 * n + i) * hs.stride] = h[(int64_t)(12 * n + 6 + i) * hs.stride];
    double e[6];
#pragma unroll
    for (int i = 0; i < 6; i++) e[i] = strain[p * 6 + i];
    const double thetan = (e[0] + e[1] + e[2]) / 3.0;
#pragma unroll
    for (int i = 0; i < 3; i++) h[(int64_t)(12 * nrow + i) * hs.stride] = e[i] - thetan;
#pragma unroll
    for (int i = 3; i < 6; i++) h[(int64_t)(12 * nrow + i) * hs.stride] = e[i] * 0.5;
  }
}
