// The arithmetic of eigen3 (utilities.f90:107-201), written once and compiled twice by fx_eigen3.h, which sets FX_EIGEN3_NAME (the
// prefix of the two functions) and FX_EIGEN3_FP (empty, or the pragma that keeps products and sums apart).  No include guard.
// one rotation of eigen3's sweep (utilities.f90:150-193) for the compile-time pair (IP, IQ), 0-based
template <int IP, int IQ>
__device__ __forceinline__ void FX_EIGEN3_NAME(jacobi_rotate)(double (&b)[3], double (&ev)[3], double (&pr)[3][3]) {
  FX_EIGEN3_FP
  constexpr int IR = 3 - IP - IQ;
  constexpr int PQ = yield_od(IP, IQ);
  constexpr int RP = IR < IP ? yield_od(IR, IP) : yield_od(IP, IR);
  constexpr int RQ = IR < IQ ? yield_od(IR, IQ) : yield_od(IQ, IR);
  const double od = 100.0 * fabs(b[PQ]);
  if ((od + fabs(ev[IP]) != fabs(ev[IP])) && (od + fabs(ev[IQ]) != fabs(ev[IQ]))) {
    const double hd = ev[IQ] - ev[IP];
    double t;
    if (fabs(hd) + od == fabs(hd)) {
      t = b[PQ] / hd;
    } else {
      const double theta = 0.5 * hd / b[PQ];
      t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
      if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(1.0 + t * t);
    const double s = t * c;
    const double tau = s / (1.0 + c);
    double h = t * b[PQ];
    ev[IP] = ev[IP] - h;
    ev[IQ] = ev[IQ] + h;
    double g = b[RP];
    h = b[RQ];
    b[RP] = g - s * (h + g * tau);
    b[RQ] = h + s * (g - h * tau);
#pragma unroll
    for (int ir = 0; ir < 3; ir++) {
      g = pr[ir][IP];
      h = pr[ir][IQ];
      pr[ir][IP] = g - s * (h + g * tau);
      pr[ir][IQ] = h + s * (g - h * tau);
    }
  }
  b[PQ] = 0.0;
}

// eigen3, utilities.f90:107-201: Jacobi iteration on the tensor (11, 22, 33, 12, 23, 31); pr holds the principal vectors as columns
__device__ __forceinline__ void FX_EIGEN3_NAME(eigen3)(const double (&tensor)[6], double (&ev)[3], double (&pr)[3][3], int32_t *err) {
  FX_EIGEN3_FP
  double b[3] = {tensor[3], tensor[5], tensor[4]};  // btens(1,2), btens(1,3), btens(2,3): only the upper triangle is read
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) pr[i][j] = i == j ? 1.0 : 0.0;
    ev[i] = tensor[i];
  }
  for (int is = 0; is < 50; is++) {
    const double fsum = fabs(b[0]) + fabs(b[1]) + fabs(b[2]);
    if (fsum < 1.0e-10) return;
    FX_EIGEN3_NAME(jacobi_rotate)<0, 1>(b, ev, pr);
    FX_EIGEN3_NAME(jacobi_rotate)<0, 2>(b, ev, pr);
    FX_EIGEN3_NAME(jacobi_rotate)<1, 2>(b, ev, pr);
  }
  yield_raise(err, FX_YERR_JACOBI);  // :200
}
