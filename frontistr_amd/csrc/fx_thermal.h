// Thermal strain of a linear static analysis (!TEMPERATURE, !REFTEMP, !INITIAL CONDITION TYPE=TEMPERATURE): what the element
// kernels need to know about a temperature.  One constant isotropic expansion coefficient per material (M_EXAPNSION; no
// MC_THEMOEXP table, no MC_ORTHOEXP), so alp == alp0 in
//   EPSTH(1:3) = alp (TEMPC - ref_temp) - alp0 (TEMP0 - ref_temp),  TEMPC = H . TT,  TEMP0 = H . T0
// (static_LIB_3d.f90:459-498, :604-637; static_LIB_C3D8.f90:311-344, :607-691; static_LIB_3dIC.f90:383-429, :535-601).
//
// The kernels themselves are the linear update kernels with a compile-time switch TH (fx_update_linear.h, fx_assemble_tet.h,
// fx_assemble_c3.h): TH = 1 is the thermal branch of UpdateST_C3D8IC / Update_C3D8Bbar / UPDATE_C3, TH = 2 is TLOAD_C3D8IC /
// TLOAD_C3D8Bbar / TLOAD_C3 -- the same lanes (one per quadrature point, one per node component for the sum), the same staging,
// and for the IC element the same factor of the mode block: the load vector sum_g wg B^T D EPSTH is the internal force of the
// strain EPSTH, which is what those kernels already sum.  It is added to the 3 NP vector with fp64 atomics, as QFORCE is.
// This header holds the shape functions (the update kernels needed only their derivatives); the host entry points
// fx_thermal_load_groups and fx_update_groups_linear_thermal are in fx_assemble_groups.h.
#pragma once
#include "fx_c3_element.h"

// device pointers: node temperatures now and in the reference state (n_node each), expansion coefficient per material
struct ThermalDev {
  const double *temp, *temp0, *alpha;
  double ref_temp;
  // The nonlinear loop alone (fx_nl_set_thermal; null in a linear static analysis).  tabs: the temperature tables of all materials
  // in one array; tab_idx[4 m ..]: offset and rows of material m's MC_THEMOEXP table (rows alpha, T), offset and rows of its
  // MC_ISOELASTIC table (rows E, nu, T); rows = 0: no table, the constant holds.  temp_init: the initial condition, the TEMP0 of
  // an element whose material is not elastoplastic (fstr_Update.f90:93-99); temp0 is then last_temp.
  const double *tabs = nullptr;
  const int32_t *tab_idx = nullptr;
  const double *temp_init = nullptr;
};

// (two rounded products, never one product fused into the subtraction: equal temperatures give exactly zero)
__device__ __forceinline__ double thermal_eps(double alp, double tempc, double temp0, double ref_temp) {
#pragma clang fp contract(off)
  const double now = alp * (tempc - ref_temp), then = alp * (temp0 - ref_temp);
  return now - then;
}
// the same with each temperature's own coefficient: MC_THEMOEXP fetched at TEMPC and at TEMP0 (static_LIB_3d.f90:610-636)
__device__ __forceinline__ double thermal_eps(double alp, double alp0, double tempc, double temp0, double ref_temp) {
#pragma clang fp contract(off)
  const double now = alp * (tempc - ref_temp), then = alp0 * (temp0 - ref_temp);
  return now - then;
}

// fetch_TableData on a table with one dependency (ttable.f90:282-354): n rows of NV values and the temperature, ascending.  Below
// the first row the first row, at or above the last row the last, in between the blend of rows i and i + 1 for T_i <= a < T_i+1.
template <int NV>
__device__ __forceinline__ void thermal_table(const double *t, int n, double a, double (&out)[NV]) {
  constexpr int NC = NV + 1;
  const double *last = t + (size_t)NC * (n - 1);
#pragma unroll
  for (int v = 0; v < NV; v++) out[v] = last[v];
  if (n == 1 || a >= last[NV]) return;
  if (a < t[NV]) {
#pragma unroll
    for (int v = 0; v < NV; v++) out[v] = t[v];
    return;
  }
  for (int i = 0; i < n - 1; i++) {
    const double *r0 = t + (size_t)NC * i, *r1 = r0 + NC;
    if (a >= r0[NV] && a < r1[NV]) {
      const double lambda = (a - r0[NV]) / (r1[NV] - r0[NV]);
#pragma unroll
      for (int v = 0; v < NV; v++) out[v] = (1.0 - lambda) * r0[v] + lambda * r1[v];
      return;
    }
  }
}
// What a point of material `mid` (0-based) takes from the temperature: alp at TEMPC, alp0 at TEMP0 and, where the material has an
// MC_ISOELASTIC table, E and nu at TEMPC (MatlMatrix's temperature argument, calElasticMatrix).  Without tables: the constant
// coefficient twice, E and nu untouched.  Returns whether E and nu were replaced.
__device__ __forceinline__ bool thermal_coefficients(const ThermalDev &th, int mid, double tempc, double temp0, double &alp, double &alp0,
                                                     double &E, double &nu) {
  alp = alp0 = th.alpha[mid];
  if (!th.tab_idx) return false;
  const int32_t *ix = th.tab_idx + 4 * mid;
  if (ix[1] > 0) {
    double o[1];
    thermal_table<1>(th.tabs + ix[0], ix[1], tempc, o);
    alp = o[0];
    thermal_table<1>(th.tabs + ix[0], ix[1], temp0, o);
    alp0 = o[0];
  }
  if (ix[3] < 1) return false;
  double en[2];
  thermal_table<2>(th.tabs + ix[2], ix[3], tempc, en);
  E = en[0];
  nu = en[1];
  return true;
}

// ShapeFunc_hex8n (hex8n.f90), node order of TYPE=361
__host__ __device__ __forceinline__ double hex8_shape_func(int n, double xi, double et, double ze) {
  const double sx = ((n & 3) == 1 || (n & 3) == 2) ? 1.0 : -1.0, sy = (n & 2) ? 1.0 : -1.0, sz = (n & 4) ? 1.0 : -1.0;
  return 0.125 * (1.0 + sx * xi) * (1.0 + sy * et) * (1.0 + sz * ze);
}

// shape function of node n (getShapeFunc): ShapeFunc_tet4n, tet10n, prism6n, prism15n, hex20n in the node order of c3_shape_deriv
template <int ETYPE>
__host__ __device__ __forceinline__ double c3_shape_func(int n, double xi, double et, double ze) {
  if (ETYPE == 341) {
    return n == 0 ? 1.0 - xi - et - ze : (n == 1 ? xi : (n == 2 ? et : ze));
  } else if (ETYPE == 342) {
    const double a = 1.0 - xi - et - ze;
    switch (n) {
      case 0: return (2.0 * a - 1.0) * a;
      case 1: return xi * (2.0 * xi - 1.0);
      case 2: return et * (2.0 * et - 1.0);
      case 3: return ze * (2.0 * ze - 1.0);
      case 4: return 4.0 * xi * a;
      case 5: return 4.0 * xi * et;
      case 6: return 4.0 * et * a;
      case 7: return 4.0 * ze * a;
      case 8: return 4.0 * xi * ze;
      default: return 4.0 * et * ze;
    }
  } else if (ETYPE == 351) {
    const double a = 1.0 - xi - et, s = n < 3 ? -1.0 : 1.0;
    const int i = n % 3;
    return 0.5 * (i == 0 ? a : (i == 1 ? xi : et)) * (1.0 + s * ze);
  } else if (ETYPE == 352) {
    const double a = 1.0 - xi - et;
    if (n < 6) {
      const double s = n < 3 ? -1.0 : 1.0, L = n % 3 == 0 ? a : (n % 3 == 1 ? xi : et);
      return 0.5 * L * (1.0 + s * ze) * (2.0 * L - 2.0 + s * ze);
    }
    if (n < 12) {
      const double s = n < 9 ? -1.0 : 1.0;
      const int i = (n - 6) % 3;
      return 2.0 * (i == 0 ? xi * a : (i == 1 ? xi * et : et * a)) * (1.0 + s * ze);
    }
    return (n == 12 ? a : (n == 13 ? xi : et)) * (1.0 - ze * ze);
  } else {
    if (n < 8) {
      const int c = n & 3;
      const double sx = (c == 1 || c == 2) ? 1.0 : -1.0, sy = c >= 2 ? 1.0 : -1.0, sz = n >= 4 ? 1.0 : -1.0;
      return -0.125 * (1.0 + sx * xi) * (1.0 + sy * et) * (1.0 + sz * ze) * (2.0 - sx * xi - sy * et - sz * ze);
    }
    if (n < 16) {
      const int c = (n - 8) & 3;
      const double Z = 1.0 + (n >= 12 ? 1.0 : -1.0) * ze;
      if ((c & 1) == 0) return 0.25 * (1.0 - xi * xi) * (1.0 + (c == 2 ? 1.0 : -1.0) * et) * Z;
      return 0.25 * (1.0 + (c == 1 ? 1.0 : -1.0) * xi) * (1.0 - et * et) * Z;
    }
    const int c = n - 16;
    const double sx = (c == 1 || c == 2) ? 1.0 : -1.0, sy = c >= 2 ? 1.0 : -1.0;
    return 0.25 * (1.0 + sx * xi) * (1.0 + sy * et) * (1.0 - ze * ze);
  }
}
