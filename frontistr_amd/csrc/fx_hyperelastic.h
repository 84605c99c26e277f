// Hyperelastic material point of the total-Lagrange path: Neo-Hooke / Mooney-Rivlin and Arruda-Boyce, Hyperelastic.f90 (cderiv :14-132,
// calElasticMooneyRivlin :221-247, calUpdateElasticMooneyRivlin :252-286, calElasticArrudaBoyce :138-172,
// calUpdateElasticArrudaBoyce :176-216) with mat_c2d (calMatMatrix.f90:154-197).
//
// The reference fills dibdc(3,3,3) and d2ibdc2(3,3,3,3,3) -- 270 doubles -- and contracts them with the material constants.  Both
// materials are functions W(I1b, I2b, J) of the reduced invariants, so every entry of those arrays is a combination of six tensors
// built from delta, C and C^-1, and what differs between the materials is five scalars:
//
//   PK_ij        = a1 dI1b_ij + a2 dI2b_ij + g3 dJ_ij                                       stress = 2 PK
//   cijkl / 4    = a1 d2I1b + a2 d2I2b + b11 dI1b (x) dI1b + g33 dJ (x) dJ + g3 d2J
//
//   Mooney-Rivlin (Neo-Hooke: C01 = 0)   a1 = C10, a2 = C01, b11 = 0, g33 = 2 / D1, g3 = 2 (J - 1) / D1
//   Arruda-Boyce                         a1 = mu (1/2 + I1b / (10 lm^2) + ...), b11 = mu (1 / (10 lm^2) + ...), a2 = 0,
//                                        g33 = (1 + 1 / J^2) / D, g3 = (J - 1 / J) / D
//
// With Ci = C^-1, B = inv1 delta - C, H = inv3 (Ci (x) Ci - Ci (.) Ci), (Ci (.) Ci)_ijkl = (Ci_ik Ci_jl + Ci_il Ci_jk) / 2,
// sym(x, y) = x (x) y + y (x) x, I4 the symmetric identity and inv33 = inv3^(-1/3), cderiv's arrays are
//
//   dI1b  = -inv33^4 inv1 inv3 / 3 Ci + inv33 delta
//   dI2b  = -2 inv33^5 inv2 inv3 / 3 Ci + inv33^2 B
//   dJ    = inv3 / (2 sqrt(inv3)) Ci
//   d2I1b = 4/9 inv33^7 inv1 inv3^2 Ci (x) Ci - inv33^4 / 3 inv3 sym(delta, Ci) - inv33^4 / 3 inv1 H
//   d2I2b = 10/9 inv33^8 inv2 inv3^2 Ci (x) Ci - 2/3 inv33^5 inv3 sym(B, Ci) - 2/3 inv33^5 inv2 H + inv33^2 (delta (x) delta - I4)
//   d2J   = -inv3^2 / (4 inv3^1.5) Ci (x) Ci + H / (2 sqrt(inv3))
//
// so the 6x6 tangent is six scalar coefficients times six symmetric 6x6 patterns of the Voigt vectors of delta, C and Ci: a point
// holds C and Ci (12 doubles), the invariants and the coefficients while it writes the 21 entries, no array of derivatives.
// Strain and stress are in the reference's order (11, 22, 33, 12, 23, 31) with engineering shear strains: C_12 = strain(4).
#pragma once

#define FX_MAT_MOONEY 2  // fx_material_view::plastic: NEOHOOKE / MOONEYRIVLIN, plconst = C10, C01, D1
#define FX_MAT_ARRUDA 3  //                            ARRUDABOYCE, plconst = mu, lambda_m, D

// kind of the hyperelastic material of group 3 (NlMat::harden holds it there)
__device__ __forceinline__ int nl_hyper_kind(const NlMat &m) { return m.harden; }

// Voigt position of the tensor component (i, j)
__device__ __forceinline__ constexpr int hy_v(int i, int j) { return i == j ? i : (i + j == 1 ? 3 : (i + j == 3 ? 4 : 5)); }

struct HyperPoint {
  double c[6], ci[6];  // C and its inverse, Voigt
  double inv1, inv2, inv3, inv33, inv3b;
  double a1, a2, b11, g33, g3;
};

// cderiv :41-72, :99-101 and the scalar factors of the two materials.  kind: FX_MAT_MOONEY or FX_MAT_ARRUDA; k = PLCONST1..3.
__device__ __forceinline__ void hyper_point(int kind, const double (&k)[3], const double (&e)[6], HyperPoint &h) {
  double(&c)[6] = h.c;
  c[0] = e[0] * 2.0 + 1.0; c[1] = e[1] * 2.0 + 1.0; c[2] = e[2] * 2.0 + 1.0;
  c[3] = e[3]; c[4] = e[4]; c[5] = e[5];
  h.inv1 = c[0] + c[1] + c[2];
  h.inv2 = c[1] * c[2] + c[0] * c[2] + c[0] * c[1] - c[4] * c[4] - c[5] * c[5] - c[3] * c[3];
  h.inv3 = c[0] * c[1] * c[2] + c[3] * c[4] * c[5] + c[5] * c[3] * c[4] - c[5] * c[1] * c[5] - c[3] * c[3] * c[2] - c[0] * c[4] * c[4];
  h.inv33 = pow(h.inv3, -1.0 / 3.0);
  h.ci[0] = (c[1] * c[2] - c[4] * c[4]) / h.inv3;
  h.ci[1] = (c[0] * c[2] - c[5] * c[5]) / h.inv3;
  h.ci[2] = (c[0] * c[1] - c[3] * c[3]) / h.inv3;
  h.ci[3] = (c[5] * c[4] - c[3] * c[2]) / h.inv3;
  h.ci[5] = (c[3] * c[4] - c[1] * c[5]) / h.inv3;
  h.ci[4] = (c[3] * c[5] - c[0] * c[4]) / h.inv3;
  h.inv3b = sqrt(h.inv3);
  if (kind == FX_MAT_ARRUDA) {  // calElasticArrudaBoyce :157-168, calUpdateElasticArrudaBoyce :201-205
    const double x = h.inv1 * h.inv33;  // inv1b
    const double l2 = k[1] * k[1], l4 = l2 * l2, l6 = l4 * l2, l8 = l4 * l4;
    const double x2 = x * x, x3 = x2 * x, x4 = x2 * x2;
    h.b11 = k[0] * (1.0 / (10.0 * l2) + 66.0 * x / (1050.0 * l4) + 228.0 * x2 / (7000.0 * l6) + 10380.0 * x3 / (673750.0 * l8));
    h.a1 = k[0] * (0.5 + x / (10.0 * l2) + 33.0 * x2 / (1050.0 * l4) + 76.0 * x3 / (7000.0 * l6) + 2595.0 * x4 / (673750.0 * l8));
    h.a2 = 0.0;
    h.g33 = (1.0 + 1.0 / (h.inv3b * h.inv3b)) / k[2];
    h.g3 = (h.inv3b - 1.0 / h.inv3b) / k[2];
  } else {  // calElasticMooneyRivlin :240-243, calUpdateElasticMooneyRivlin :274-275
    h.a1 = k[0];
    h.a2 = k[1];
    h.b11 = 0.0;
    h.g33 = 2.0 / k[2];
    h.g3 = 2.0 * (h.inv3b - 1.0) / k[2];
  }
}

// 2nd Piola-Kirchhoff stress of a point from its Green-Lagrange strain (StressUpdate, calMatMatrix.f90:126-129)
__device__ __forceinline__ void hyper_stress(int kind, const double (&k)[3], const double (&e)[6], double (&s)[6]) {
  HyperPoint h;
  hyper_point(kind, k, e, h);
  const double i2 = h.inv33 * h.inv33, i4 = i2 * i2, i5 = i4 * h.inv33;
  // PK = pc Ci + pd delta + pb C
  const double pc = h.a1 * (-i4 * h.inv1 * h.inv3 / 3.0) + h.a2 * (-2.0 * i5 * h.inv2 * h.inv3 / 3.0) + h.g3 * (h.inv3 / (2.0 * h.inv3b));
  const double pd = h.a1 * h.inv33 + h.a2 * i2 * h.inv1;
  const double pb = -h.a2 * i2;
#pragma unroll
  for (int i = 0; i < 6; i++) s[i] = 2.0 * (pc * h.ci[i] + (i < 3 ? pd : 0.0) + pb * h.c[i]);
}

// Tangent of a point from its stored Green-Lagrange strain (MatlMatrix :81-86 + mat_c2d), the 21 entries of sym21
__device__ __forceinline__ void hyper_tangent(int kind, const double (&k)[3], const double (&e)[6], double (&Dm)[21]) {
  HyperPoint h;
  hyper_point(kind, k, e, h);
  const double i2 = h.inv33 * h.inv33, i4 = i2 * i2, i5 = i4 * h.inv33, i7 = i5 * i2, i8 = i4 * i4;
  const double p = -i4 * h.inv1 * h.inv3 / 3.0, q = h.inv33;  // dI1b = p Ci + q delta
  const double kH = -h.a1 * (i4 / 3.0 * h.inv1) - h.a2 * (2.0 / 3.0 * i5 * h.inv2) + h.g3 / (2.0 * h.inv3b);
  const double kCC = h.a1 * (4.0 / 9.0 * i7 * h.inv1 * h.inv3 * h.inv3) + h.a2 * (10.0 / 9.0 * i8 * h.inv2 * h.inv3 * h.inv3) + h.b11 * p * p +
                     h.g33 * (h.inv3 / 4.0) - h.g3 * (h.inv3 * h.inv3 / (4.0 * h.inv3 * h.inv3b)) + kH * h.inv3;
  const double kO = -kH * h.inv3;
  const double kdc = -h.a1 * (i4 / 3.0 * h.inv3) + h.b11 * p * q - h.a2 * (2.0 / 3.0 * i5 * h.inv3) * h.inv1;
  const double kcc = h.a2 * (2.0 / 3.0 * i5 * h.inv3);
  const double kdd = h.a2 * i2 + h.b11 * q * q;
  const double kI = -h.a2 * i2;
  constexpr int vi[6] = {0, 1, 2, 0, 1, 2}, vj[6] = {0, 1, 2, 1, 2, 0};  // (i, j) of a Voigt position
#pragma unroll
  for (int I = 0; I < 6; I++)
#pragma unroll
    for (int J = I; J < 6; J++) {
      const int i = vi[I], j = vj[I], m = vi[J], n = vj[J];
      const double o = 0.5 * (h.ci[hy_v(i, m)] * h.ci[hy_v(j, n)] + h.ci[hy_v(i, n)] * h.ci[hy_v(j, m)]);
      const double dI = I < 3 ? 1.0 : 0.0, dJ = J < 3 ? 1.0 : 0.0;
      double t = kCC * h.ci[I] * h.ci[J] + kO * o + kdc * (dI * h.ci[J] + h.ci[I] * dJ) + kcc * (h.c[I] * h.ci[J] + h.ci[I] * h.c[J]) +
                 kdd * dI * dJ;
      if (I == J) t += kI * (I < 3 ? 1.0 : 0.5);
      Dm[(I * (13 - I)) / 2 + (J - I)] = 4.0 * t;
    }
}
