// Nodal and element stress output: fstr_NodalStress3D (fistr1/src/analysis/static/fstr_NodalStress.f90:13-272) for TYPE=341, 342,
// 351, 352, 361 and 362 in any mix of groups, with NodalStress_INV3 (:337-481), inverse_func (:714-748), get_mises (:483-499),
// make_principal (:889-980), NodalStress_C3 / ElementStress_C3 (static_LIB_3d.f90:840-913) and get_principal (utilities.f90:362-406)
// over eigen3 (fx_eigen3.h).  Included by fistr_hip.hip after fx_nonlinear_host.h.
//
// The rules, as the reference writes them:
//   element values  ESTRAIN / ESTRESS = (sum over ALL quadrature points in point order) / their number
//   341, 351        every node of the element gets that mean
//   361             vertex i = sum_j inv(i, j) * point j, j ascending; inv = inverse of func(i, j) = shape function j at point i
//   342             the same with the 4-node functions at the four points; nodes 5..10 = half-sums of vertex pairs
//   352             points 1, 2, 3, 7, 8, 9 with the 6-node wedge functions; nodes 7..15 = half-sums
//   362             points 1, 3, 7, 9, 19, 21, 25, 27 with the 8-node functions; nodes 9..20 = half-sums
//   nodes           the nodal values of every element that names the node are added in ascending element position (the groups one
//                   after the other: the reference's loop order), a node named twice by one element twice, and divided by their
//                   number; a node that no element names keeps zeros; then MISES / EMISES and, on request, the principal values
// The inverses are made once on the host by inverse_func's own algorithm (Gauss-Jordan without pivoting, divide then eliminate)
// from the project's point coordinates and shape functions and reach the kernels as a by-value argument.
//
// Launches: one k_nodal_element<ETYPE> per group (means to ESTRAIN / ESTRESS, one 12-double record per vertex -- or, 341 / 351,
// per element -- to a scratch array), one k_nodal_node over (node, strain | stress) that walks the node's list of record pairs
// (a, b): value = record a, or (record a + record b) / 2 for a mid-edge node, and k_nodal_tensor_post over the elements for
// EMISES and the element principal values.  The list is CSR by node, in the reference's order of addition: no atomics, and the
// result does not depend on the workgroup size or on the run.  Products and sums are kept apart (no contraction), as the
// reference's compilers leave them.
#pragma once
#include "fx_eigen3.h"

struct NodalInv { double a[64]; };  // inv(i, j) at a[i * NS + j], NS = vertices = selected points of the type

template <int ETYPE>
struct NodalEl {
  static constexpr int NQ = c3_facts(ETYPE).nq;
  static constexpr int NV = ETYPE == 341 || ETYPE == 351 ? 1 : (ETYPE == 342 ? 4 : (ETYPE == 352 ? 6 : 8));  // records per element
  static constexpr bool MEAN = ETYPE == 341 || ETYPE == 351;  // the record is the element mean
  static constexpr int BS = ETYPE == 362 ? 128 : 256;         // workgroup size: 12 lanes per element, EPB elements' points in LDS
  static constexpr int EPB = BS / 12;                         // 21 (16 KB of LDS at 361), 362: 10 (26 KB)
  // 0-based quadrature point of selected point j (fstr_NodalStress.f90:84, :95)
  __host__ __device__ static constexpr int sel(int j) {
    return ETYPE == 352 ? (j < 3 ? j : j + 3) : (ETYPE == 362 ? ((j & 1) * 2 + ((j >> 1) & 1) * 6 + (j >> 2) * 18) : j);
  }
};
static int nodal_records(int32_t etype) {  // NodalEl<etype>::NV; 0: not a type the device knows
  if (c3_facts(etype).nn == 0) return 0;
  return etype == 341 || etype == 351 ? 1 : (etype == 342 ? 4 : (etype == 352 ? 6 : 8));
}

// strain, stress: this group's [elem][point][6]; estrain, estress: its [elem][6]; rec: its records, [record][strain | stress][6]
template <int ETYPE>
__global__ __launch_bounds__(NodalEl<ETYPE>::BS) void k_nodal_element(int32_t n_elem, const double *__restrict__ strain,
                                                                       const double *__restrict__ stress, NodalInv inv,
                                                                       double *__restrict__ estrain, double *__restrict__ estress,
                                                                       double *__restrict__ rec) {
#pragma clang fp contract(off)
  using T = NodalEl<ETYPE>;
  constexpr int NQ = T::NQ, NV = T::NV, EPB = T::EPB, BS = T::BS;
  __shared__ double pts[2][EPB * NQ * 6];
  const int64_t e0 = (int64_t)blockIdx.x * EPB;
  const int ne = (int)(n_elem - e0 < EPB ? n_elem - e0 : EPB);
  const int cnt = ne * NQ * 6;
  const size_t base = (size_t)e0 * NQ * 6;
  for (int i = threadIdx.x; i < cnt; i += BS) {
    pts[0][i] = strain[base + i];
    pts[1][i] = stress[base + i];
  }
  __syncthreads();
  const int h = threadIdx.x >= EPB * 6 ? 1 : 0, t = threadIdx.x - h * EPB * 6, e = t / 6, k = t - 6 * e;
  if (threadIdx.x >= EPB * 12 || e >= ne) return;
  const double *p = pts[h] + e * NQ * 6 + k;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < NQ; q++) s = s + p[q * 6];
  s = s / (double)NQ;
  (h ? estress : estrain)[(size_t)(e0 + e) * 6 + k] = s;
  double *r = rec + ((size_t)(e0 + e) * NV * 2 + h) * 6 + k;
  if (T::MEAN) {
    r[0] = s;
  } else {
#pragma unroll
    for (int v = 0; v < NV; v++) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < NV; j++) a = a + inv.a[v * NV + j] * p[T::sel(j) * 6];
      r[(size_t)v * 12] = a;
    }
  }
}

// get_mises (fstr_NodalStress.f90:483-499)
__device__ __forceinline__ double nodal_mises(const double (&s)[6]) {
#pragma clang fp contract(off)
  const double ps = (s[0] + s[1] + s[2]) / 3.0;
  const double a = s[0] - ps, b = s[1] - ps, c = s[2] - ps;
  const double sm = 0.5 * (a * a + b * b + c * c) + s[3] * s[3] + s[4] * s[4] + s[5] * s[5];
  return sqrt(3.0 * sm);
}

// get_principal (utilities.f90:362-406): eigen3, the three conditional swaps, princmatrix(i, j) = princnormal(i, j) * eigval(j).
// pval: [3]; pvec: [vector j][component i].  Either may be null.
__device__ __forceinline__ void nodal_principal(const double (&t)[6], double *pval, double *pvec, int32_t *err) {
#pragma clang fp contract(off)
  double ev[3], pr[3][3];
  exact_eigen3(t, ev, pr, err);
#define FX_NODAL_SWAP(A, B)                                                   \
  if (ev[A] < ev[B]) {                                                        \
    const double ts = ev[A]; ev[A] = ev[B]; ev[B] = ts;                       \
    _Pragma("unroll") for (int i = 0; i < 3; i++) { const double tv = pr[i][A]; pr[i][A] = pr[i][B]; pr[i][B] = tv; } \
  }
  FX_NODAL_SWAP(0, 1)
  FX_NODAL_SWAP(0, 2)
  FX_NODAL_SWAP(1, 2)
#undef FX_NODAL_SWAP
  if (pval) { pval[0] = ev[0]; pval[1] = ev[1]; pval[2] = ev[2]; }
  if (pvec) {
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int i = 0; i < 3; i++) pvec[3 * j + i] = pr[i][j] * ev[j];
  }
}

#define FX_NODAL_BS 256  // workgroup size of k_nodal_node and k_nodal_tensor_post

// What one half (strain: h = 0, stress: h = 1) of the node kernel writes: tensor [n][6], mises [n] (stress only), principal
// values [n][3] and vectors [n][3][3]; null = not asked for
struct NodalHalfOut { double *tensor, *mises, *pval, *pvec; };

// One lane per (node, half); blockIdx.y is the half, so a wave never diverges over it.
__global__ __launch_bounds__(FX_NODAL_BS) void k_nodal_node(int32_t n_node, const int32_t *__restrict__ row, const int2 *__restrict__ ent,
                                                             const double *__restrict__ rec, NodalHalfOut o0, NodalHalfOut o1,
                                                             int32_t *__restrict__ err) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * FX_NODAL_BS + threadIdx.x;
  if (i >= n_node) return;
  const int h = blockIdx.y;
  const NodalHalfOut o = h ? o1 : o0;
  const int32_t b = row[i], e = row[i + 1];
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int32_t t = b; t < e; t++) {
    const int2 ab = ent[t];
    const double2 *ra = reinterpret_cast<const double2 *>(rec + ((size_t)ab.x * 2 + h) * 6);
    const double2 a0 = ra[0], a1 = ra[1], a2 = ra[2];
    double v[6] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y};
    if (ab.y != ab.x) {  // a mid-edge node: the half-sum of two vertices (fstr_NodalStress.f90:370-387, :402-428, :444-479)
      const double2 *rb = reinterpret_cast<const double2 *>(rec + ((size_t)ab.y * 2 + h) * 6);
      const double2 b0 = rb[0], b1 = rb[1], b2 = rb[2];
      const double w[6] = {b0.x, b0.y, b1.x, b1.y, b2.x, b2.y};
#pragma unroll
      for (int k = 0; k < 6; k++) v[k] = (v[k] + w[k]) / 2.0;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] = acc[k] + v[k];
  }
  if (e > b) {
    const double n = (double)(e - b);
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] = acc[k] / n;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) o.tensor[(size_t)i * 6 + k] = acc[k];
  if (o.mises) o.mises[i] = nodal_mises(acc);
  if (o.pval || o.pvec) nodal_principal(acc, o.pval ? o.pval + (size_t)i * 3 : nullptr, o.pvec ? o.pvec + (size_t)i * 9 : nullptr, err);
}

// EMISES and the principal values of tensors already in memory (the elements')
__global__ __launch_bounds__(FX_NODAL_BS) void k_nodal_tensor_post(int64_t n, NodalHalfOut o, int32_t *__restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * FX_NODAL_BS + threadIdx.x;
  if (i >= n) return;
  double t[6];
#pragma unroll
  for (int k = 0; k < 6; k++) t[k] = o.tensor[(size_t)i * 6 + k];
  if (o.mises) o.mises[i] = nodal_mises(t);
  if (o.pval || o.pvec) nodal_principal(t, o.pval ? o.pval + (size_t)i * 3 : nullptr, o.pvec ? o.pvec + (size_t)i * 9 : nullptr, err);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// inverse_func (fstr_NodalStress.f90:714-748) as written; a: n x n row-major, destroyed
static void nodal_inverse_func(int n, double *a, double *inv) {
#pragma clang fp contract(off)
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) inv[i * n + j] = i == j ? 1.0 : 0.0;
  for (int i = 0; i < n; i++) {
    double buf = 1.0 / a[i * n + i];
    for (int j = 0; j < n; j++) {
      a[i * n + j] = a[i * n + j] * buf;
      inv[i * n + j] = inv[i * n + j] * buf;
    }
    for (int j = 0; j < n; j++) {
      if (i == j) continue;
      buf = a[j * n + i];
      for (int k = 0; k < n; k++) {
        a[j * n + k] = a[j * n + k] - a[i * n + k] * buf;
        inv[j * n + k] = inv[j * n + k] - inv[i * n + k] * buf;
      }
    }
  }
}
// func(i, j) = shape function j of the vertex element (hex8n, tet4n, prism6n) at selected point i of the type's own rule
template <int ETYPE>
static NodalInv nodal_make_inv() {
  using T = NodalEl<ETYPE>;
  NodalInv r = {};
  constexpr int n = T::NV;
  double a[64];
  for (int i = 0; i < n; i++) {
    double xi, et, ze, w;
    if (ETYPE == 361) {
      const double GP = 0.577350269189626;  // quadrature.f90:83-91
      xi = (i & 1) ? GP : -GP; et = (i & 2) ? GP : -GP; ze = (i & 4) ? GP : -GP;
    } else {
      c3_gauss<ETYPE>(T::sel(i), xi, et, ze, w);
    }
    for (int j = 0; j < n; j++)
      a[i * n + j] = ETYPE == 342 ? c3_shape_func<341>(j, xi, et, ze) : (ETYPE == 352 ? c3_shape_func<351>(j, xi, et, ze) : hex8_shape_func(j, xi, et, ze));
  }
  nodal_inverse_func(n, a, r.a);
  return r;
}
static const NodalInv &nodal_inv(int32_t etype) {
  static const NodalInv i361 = nodal_make_inv<361>(), i342 = nodal_make_inv<342>(), i352 = nodal_make_inv<352>(), i362 = nodal_make_inv<362>(),
                        none = {};
  return etype == 361 ? i361 : (etype == 342 ? i342 : (etype == 352 ? i352 : (etype == 362 ? i362 : none)));
}
// for tests: the inverse the kernels of `etype` take, n x n row-major (n = 8, 4, 6, 8 at 361, 342, 352, 362; else 0)
extern "C" int fx_nodal_inverse(int32_t etype, double *inv, int32_t *n) {
  const int nv = etype == 341 || etype == 351 ? 0 : nodal_records(etype);
  if (n) *n = nv;
  if (inv && nv) memcpy(inv, nodal_inv(etype).a, sizeof(double) * nv * nv);
  return nv || etype == 341 || etype == 351 ? 0 : fx_fail("fx_nodal_inverse", FX_ERROR_UNSUPPORTED, "element type %d", (int)etype);
}

// the vertex pairs of the mid-edge nodes, 0-based, in node order (fstr_NodalStress.f90:370-387, :402-428, :444-479)
static const int8_t NODAL_PAIRS_342[6][2] = {{0, 1}, {1, 2}, {2, 0}, {0, 3}, {1, 3}, {2, 3}};
static const int8_t NODAL_PAIRS_352[9][2] = {{0, 1}, {1, 2}, {2, 0}, {3, 4}, {4, 5}, {5, 3}, {0, 3}, {1, 4}, {2, 5}};
static const int8_t NODAL_PAIRS_362[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
// records (a, b) of local node j of an element whose first record is r
static inline void nodal_entry(int32_t etype, int64_t r, int j, int32_t &a, int32_t &b) {
  const int nv = nodal_records(etype);
  if (nv == 1) { a = b = (int32_t)r; return; }
  if (j < nv) { a = b = (int32_t)(r + j); return; }
  const int8_t *p = etype == 342 ? NODAL_PAIRS_342[j - 4] : (etype == 352 ? NODAL_PAIRS_352[j - 6] : NODAL_PAIRS_362[j - 8]);
  a = (int32_t)(r + p[0]); b = (int32_t)(r + p[1]);
}

struct NodalPartIn {  // one group: its type and size, its connectivity on the host, its point arrays on the device
  int32_t etype, n_elem;
  const int32_t *conn;
  const double *d_strain, *d_stress;
};

static void nodal_list_free(NodalList &L) {
  dev_free(L.row); dev_free(L.ent);
  const int64_t builds = L.builds;
  L = NodalList();
  L.builds = builds;
}
static void nodal_free(fx_context *c) {
  nodal_list_free(c->nodal_list);
  nodal_list_free(c->nodal_list_nl);
  NodalStage &s = c->nodal_stage;
  dev_free(s.dev); dev_free(s.rec); dev_free(s.err);
  if (s.host) (void)hipHostFree(s.host);
  s = NodalStage();
}

// checksum of what the list depends on: n_node and every group's type, size and connectivity (FNV-1a per chunk, chunks in order)
static uint64_t nodal_key(int32_t n_node, const std::vector<NodalPartIn> &parts) {
  uint64_t key = fnv_mix(1469598103934665603ull, (uint64_t)n_node);
  for (const NodalPartIn &p : parts) {
    key = fnv_mix(fnv_mix(key, (uint64_t)p.etype), (uint64_t)p.n_elem);
    const int64_t nw = (int64_t)c3_nodes(p.etype) * p.n_elem;
    const int nchunk = 64;
    uint64_t part[nchunk];
    parallel_for(nchunk, [&](int64_t a, int64_t b) {
      for (int64_t q = a; q < b; q++) {
        uint64_t h = 1469598103934665603ull;
        for (int64_t i = nw * q / nchunk; i < nw * (q + 1) / nchunk; i++) h = (h ^ (uint32_t)p.conn[i]) * 1099511628211ull;
        part[q] = h;
      }
    });
    for (int q = 0; q < nchunk; q++) key = fnv_mix(key, part[q]);
  }
  return key | 1;
}

// The node -> (record a, record b) list in CSR form, entries of a node in ascending element position of the concatenated groups
// and, inside one element, ascending local node: the reference's order of addition.  key == 0: build unconditionally.
static int nodal_ensure_list(fx_context *c, const char *who, NodalList &L, uint64_t key, int32_t n_node, const std::vector<NodalPartIn> &parts) {
  if (key && L.key == key && L.row) return 0;
  std::vector<int32_t> row((size_t)n_node + 1, 0);
  int64_t n_ent = 0, n_rec = 0, n_elem = 0;
  for (size_t g = 0; g < parts.size(); g++) {
    const NodalPartIn &p = parts[g];
    const int nn = c3_nodes(p.etype);
    for (int64_t i = 0; i < (int64_t)nn * p.n_elem; i++) {
      const int32_t v = p.conn[i];
      if (v < 1 || v > n_node)
        return fx_fail(who, FX_ERROR_RUNTIME, "group %d, element %d: node id out of range", (int)g + 1, (int)(i / nn) + 1);
      row[v]++;
    }
    n_ent += (int64_t)nn * p.n_elem;
    n_rec += (int64_t)nodal_records(p.etype) * p.n_elem;
    n_elem += p.n_elem;
  }
  if (n_ent > INT32_MAX || n_rec > INT32_MAX) return fx_fail(who, FX_ERROR_UNSUPPORTED, "more than 2^31 - 1 element nodes");
  for (int32_t i = 0; i < n_node; i++) row[i + 1] += row[i];
  std::vector<int2> ent((size_t)std::max<int64_t>(n_ent, 1));
  {
    std::vector<int32_t> at(row.begin(), row.end() - 1);
    int64_t r = 0;
    for (const NodalPartIn &p : parts) {
      const int nn = c3_nodes(p.etype), nv = nodal_records(p.etype);
      for (int64_t e = 0; e < p.n_elem; e++, r += nv)
        for (int j = 0; j < nn; j++) {
          int2 ab;
          nodal_entry(p.etype, r, j, ab.x, ab.y);
          ent[(size_t)at[p.conn[(size_t)nn * e + j] - 1]++] = ab;
        }
    }
  }
  nodal_list_free(L);
  if (dev_alloc(&L.row, row.size()) || dev_alloc(&L.ent, ent.size())) { nodal_list_free(L); return FX_ERROR_RUNTIME; }
  HIP_TRY(hipMemcpy(L.row, row.data(), row.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(L.ent, ent.data(), ent.size() * sizeof(int2), hipMemcpyHostToDevice));
  L.key = key; L.n_node = n_node; L.n_elem = n_elem; L.n_rec = n_rec; L.n_ent = n_ent;
  L.builds++;
  return 0;
}

// doubles of the result block for these sizes and flags, and where each array starts (-1: not asked for).  Order: STRAIN, STRESS,
// MISES, ESTRAIN, ESTRESS, EMISES, then the eight principal arrays in the order of make_principal's flag bits.
struct NodalLayout { int64_t at[14]; int64_t total; };
static NodalLayout nodal_layout(int64_t N, int64_t E, int flags) {
  NodalLayout l;
  const int64_t size[14] = {6 * N, 6 * N, N, 6 * E, 6 * E, E, 3 * N, 9 * N, 3 * N, 9 * N, 3 * E, 9 * E, 3 * E, 9 * E};
  int64_t t = 0;
  for (int k = 0; k < 14; k++) {
    const bool on = k < 6 || (flags >> (k - 6) & 1);
    l.at[k] = on ? t : -1;
    if (on) t += (size[k] + 1) & ~(int64_t)1;  // every array starts at a multiple of 16 bytes
  }
  l.total = t;
  return l;
}

template <int ETYPE>
static void nodal_launch_element(fx_context *c, const NodalPartIn &p, double *estrain, double *estress, double *rec) {
  using T = NodalEl<ETYPE>;
  const int grid = (int)((p.n_elem + T::EPB - 1) / T::EPB);
  hipLaunchKernelGGL(k_nodal_element<ETYPE>, dim3(grid), dim3(T::BS), 0, c->stream, p.n_elem, p.d_strain, p.d_stress, nodal_inv(ETYPE), estrain,
                     estress, rec);
}

// The pass itself on device-resident point arrays; the result in the context's pinned staging.
static int nodal_run(fx_context *c, const char *who, const NodalList &L, const std::vector<NodalPartIn> &parts, int flags, fx_nodal_result *out,
                     float *ms_kernel) {
  NodalStage &s = c->nodal_stage;
  const int64_t N = L.n_node, E = L.n_elem;
  const NodalLayout lay = nodal_layout(N, E, flags);
  if (s.cap < (size_t)lay.total) {
    dev_free(s.dev);
    if (s.host) (void)hipHostFree(s.host);
    s.host = nullptr; s.cap = 0;
    if (dev_alloc(&s.dev, (size_t)lay.total)) return FX_ERROR_RUNTIME;
    if (hipHostMalloc((void **)&s.host, (size_t)lay.total * 8, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fx_fail(who, FX_ERROR_RUNTIME, "cannot pin the host staging");
    }
    s.cap = (size_t)lay.total;
  }
  if (s.rec_cap < (size_t)L.n_rec * 12) {
    dev_free(s.rec); s.rec_cap = 0;
    if (dev_alloc(&s.rec, (size_t)std::max<int64_t>(L.n_rec, 1) * 12)) return FX_ERROR_RUNTIME;
    s.rec_cap = (size_t)L.n_rec * 12;
  }
  if (!s.err && dev_alloc(&s.err, 1)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemsetAsync(s.err, 0, 4, c->stream));
  auto arr = [&](int k) { return lay.at[k] < 0 ? (double *)nullptr : s.dev + lay.at[k]; };
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  int64_t e_at = 0, r_at = 0;
  for (const NodalPartIn &p : parts) {
    if (p.n_elem < 1) continue;
    double *es = arr(3) + 6 * e_at, *et = arr(4) + 6 * e_at, *rec = s.rec + 12 * r_at;
    with_solid_type(p.etype, [&](auto t) { nodal_launch_element<decltype(t)::value>(c, p, es, et, rec); });
    e_at += p.n_elem;
    r_at += (int64_t)nodal_records(p.etype) * p.n_elem;
  }
  const NodalHalfOut n0 = {arr(0), nullptr, arr(8), arr(9)}, n1 = {arr(1), arr(2), arr(6), arr(7)};
  hipLaunchKernelGGL(k_nodal_node, dim3((unsigned)((N + FX_NODAL_BS - 1) / FX_NODAL_BS), 2), dim3(FX_NODAL_BS), 0, c->stream, (int32_t)N, L.row,
                     L.ent, s.rec, n0, n1, s.err);
  if (E > 0) {
    const unsigned grid = (unsigned)((E + FX_NODAL_BS - 1) / FX_NODAL_BS);
    const NodalHalfOut e1 = {arr(4), arr(5), arr(10), arr(11)}, e0 = {arr(3), nullptr, arr(12), arr(13)};
    hipLaunchKernelGGL(k_nodal_tensor_post, dim3(grid), dim3(FX_NODAL_BS), 0, c->stream, E, e1, s.err);
    if (flags & 0xC0) hipLaunchKernelGGL(k_nodal_tensor_post, dim3(grid), dim3(FX_NODAL_BS), 0, c->stream, E, e0, s.err);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  int32_t herr = 0;
  HIP_TRY(hipMemcpyAsync(s.host, s.dev, (size_t)lay.total * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&herr, s.err, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  if (ms_kernel) *ms_kernel = ms;
  if (int rc = assembly_error(herr)) return rc;  // eigen3's `stop`
  auto harr = [&](int k) { return lay.at[k] < 0 ? (const double *)nullptr : s.host + lay.at[k]; };
  fx_nodal_result r;
  r.n_node = (int32_t)N; r.n_elem = (int32_t)E;
  r.strain = harr(0); r.stress = harr(1); r.mises = harr(2); r.estrain = harr(3); r.estress = harr(4); r.emises = harr(5);
  r.pstress = harr(6); r.pstress_vect = harr(7); r.pstrain = harr(8); r.pstrain_vect = harr(9);
  r.epstress = harr(10); r.epstress_vect = harr(11); r.epstrain = harr(12); r.epstrain_vect = harr(13);
  *out = r;
  return 0;
}

extern "C" int fx_nodal_stress_groups(fx_context *c, int32_t n_node, int32_t n_group, const fx_elem_group *groups, const double *strain,
                                      const double *stress, int32_t flags, fx_nodal_result *out, float *ms_kernel) {
  const char *who = "fx_nodal_stress_groups";
  if (!c || !out) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  if (int rc = check_group_types(who, n_group, groups, "361, 341, 342, 351, 352, 362")) return rc;
  if (n_node < 1 || !strain || !stress) return fx_fail(who, FX_ERROR_RUNTIME, "empty mesh or missing point arrays");
  if (flags < 0 || flags > 255) return fx_fail(who, FX_ERROR_RUNTIME, "flags outside 0..255");
  std::vector<NodalPartIn> parts;
  size_t total = 0;
  for (int32_t g = 0; g < n_group; g++) {
    const fx_elem_group &G = groups[g];
    if (G.n_elem < 0 || (G.n_elem > 0 && !G.conn)) return fx_fail(who, FX_ERROR_RUNTIME, "group %d: connectivity missing", (int)g + 1);
    parts.push_back({G.etype, G.n_elem, G.conn, nullptr, nullptr});
    total += (size_t)6 * c3_points(G.etype) * (size_t)G.n_elem;
  }
  if (total == 0) return fx_fail(who, FX_ERROR_RUNTIME, "empty mesh");
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = nodal_ensure_list(c, who, c->nodal_list, nodal_key(n_node, parts), n_node, parts)) return rc;
  DevScratch tmp;
  double *d_strain = nullptr, *d_stress = nullptr;
  if (tmp.alloc(&d_strain, total) || tmp.alloc(&d_stress, total)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(d_strain, strain, total * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_stress, stress, total * 8, hipMemcpyHostToDevice, c->stream));
  size_t at = 0;
  for (NodalPartIn &p : parts) {
    p.d_strain = d_strain + at; p.d_stress = d_stress + at;
    at += (size_t)6 * c3_points(p.etype) * (size_t)p.n_elem;
  }
  return nodal_run(c, who, c->nodal_list, parts, flags, out, ms_kernel);
}

extern "C" int fx_nl_nodal_stress(fx_context *c, int32_t flags, fx_nodal_result *out, float *ms_kernel) {
  const char *who = "fx_nl_nodal_stress";
  if (!c || !out) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  NL_READY("fx_nl_nodal_stress");
  if (flags < 0 || flags > 255) return fx_fail(who, FX_ERROR_RUNTIME, "flags outside 0..255");
  NlDev &n = c->nl;
  std::vector<NodalPartIn> parts;
  for (const NlPart &p : n.parts) parts.push_back({p.etype, p.n_elem, nullptr, n.st.strain + 6 * p.pt_off, n.st.stress + 6 * p.pt_off});
  if (!c->nodal_list_nl.row) {  // once per fx_nl_init*: the connectivity lives on the device, the list is made on the host
    std::vector<std::vector<int32_t>> conn, emat;
    if (int rc = nl_parts_to_host(n, false, conn, emat)) return rc;
    for (size_t g = 0; g < parts.size(); g++) parts[g].conn = conn[g].data();
    if (int rc = nodal_ensure_list(c, who, c->nodal_list_nl, 0, c->A.NP, parts)) return rc;
  }
  return nodal_run(c, who, c->nodal_list_nl, parts, flags, out, ms_kernel);
}

// out[0] lists built for fx_nodal_stress_groups on this context, [1] for fx_nl_nodal_stress, [2] entries and [3] records of the
// list last used by fx_nodal_stress_groups, [4] workgroup size of the node kernel, [5..10] elements per workgroup of the element
// kernel of 341, 342, 351, 352, 361, 362
extern "C" int fx_nodal_get_stats(fx_context *c, int64_t out[12]) {
  if (!c || !out) return fx_fail("fx_nodal_get_stats", FX_ERROR_RUNTIME, "null argument");
  out[0] = c->nodal_list.builds; out[1] = c->nodal_list_nl.builds; out[2] = c->nodal_list.n_ent; out[3] = c->nodal_list.n_rec;
  out[4] = FX_NODAL_BS;
  out[5] = NodalEl<341>::EPB; out[6] = NodalEl<342>::EPB; out[7] = NodalEl<351>::EPB; out[8] = NodalEl<352>::EPB;
  out[9] = NodalEl<361>::EPB; out[10] = NodalEl<362>::EPB; out[11] = 0;
  return 0;
}
