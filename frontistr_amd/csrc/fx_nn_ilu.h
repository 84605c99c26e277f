// Block ILU(0) (PRECOND = 10) for NDOF = 4, 5, 6 on the generic-block path (included from fx_nn_host.h).
//
//   hecmw_precond_BILU_44_setup / FORM_ILU0_44 / _apply  hecmw1/src/solver/precond/44/hecmw_precond_BILU_44.f90:34-173, :201-437
//   hecmw_precond_BILU_66_setup / FORM_ILU0_66 / _apply  precond/66/hecmw_precond_BILU_66.f90:33-238, :267-589
//   hecmw_precond_BILU_nn_setup / FORM_ILU0_nn / _apply  precond/nn/hecmw_precond_BILU_nn.f90:34-168, :196-333 (NDOF = 5)
//
// The three modules compute the same thing (DESIGN.md §8 lists the differences that do not change a bit):
//   Dlu_i = LU of the sigma-scaled diagonal block (ILU1a: reciprocal pivots, no pivoting) -- k_nn_lu.  The Schur update of
//           the diagonal block never runs (row i is in neither of its own IW1 / IW2 lists), so Dlu depends on D only.
//   for i, for k in L(i) ascending, for j in U(k) with (i, j) in the pattern of row i:  A_ij -= A_ik (Dlu_k^-1 A_kj)
//           (ILU1b: column by column, the same triangular solves as the apply, then row-times-column sums in index order).
//   apply: forward over rows 1..N   z_i = Dlu_i^-1 (z_i - sum_{L(i), ascending} A_ij z_j)
//          backward over rows N..1  z_i = z_i - Dlu_i^-1 (sum_{U(i), descending} A_ij z_j); halo columns multiply ZP(halo) = 0.
// Device form: rows grouped by dependency level of the natural-order lower pattern, 64-row slices, level by level; the
// factor runs one launch per level on device copies of the caller's CSR blocks, the factors are then gathered into the
// entry-major sliced layouts (NnBell) that the sweeps stream.  The sweeps are one persistent launch per apply
// (k_nn_tri_dataflow), or one launch per level (k_nn_ilu_rows: FX_DATAFLOW=0, and after a dataflow sweep timed out).
#pragma once

// One update A_ij -= A_ik (Dlu_k^-1 A_kj) of a destination block held in a[] (ILU1b44 / ILU1b66 / ILU1bNN).  Both factor
// kernels call exactly this, in the same order per destination; both match the reference to 1e-12 (tests/test_gpu_nn_ilu.py).
template <int ND>
__device__ __forceinline__ void nn_ilu_update(double *a, const double *aik, const double *__restrict__ dk,
                                              const double *__restrict__ akj) {
#pragma unroll
  for (int col = 0; col < ND; col++) {
    double x[ND];
#pragma unroll
    for (int r = 0; r < ND; r++) x[r] = akj[r * ND + col];
    nn_lusolve<ND, false>(dk, x);
#pragma unroll
    for (int r = 0; r < ND; r++) {
      double s = aik[r * ND] * x[0];
#pragma unroll
      for (int q = 1; q < ND; q++) s = s + aik[r * ND + q] * x[q];
      a[r * ND + col] = a[r * ND + col] - s;
    }
  }
}

// One level, one thread per row: the reference's loop as written (rows with more than 32 L + U blocks).
template <int ND>
__global__ __launch_bounds__(128) void k_nn_ilu0_factor_level(int32_t slot0, int32_t slot1, const int32_t *__restrict__ slot_row,
                                                              int32_t N, const int32_t *__restrict__ indexL,
                                                              const int32_t *__restrict__ itemL, const int32_t *__restrict__ indexU,
                                                              const int32_t *__restrict__ itemU, const double *__restrict__ Dlu,
                                                              double *__restrict__ AL, double *__restrict__ AU) {
  constexpr int NN = ND * ND;
  const int32_t s = slot0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= slot1) return;
  const int32_t i = slot_row[s];
  if (i < 0) return;
  const int32_t iL0 = indexL[i], iL1 = indexL[i + 1], iU0 = indexU[i], iU1 = indexU[i + 1];
  for (int32_t kk = iL0; kk < iL1; kk++) {
    const int32_t k = itemL[kk] - 1;
    double aik[NN];
#pragma unroll
    for (int e = 0; e < NN; e++) aik[e] = AL[(size_t)NN * kk + e];
    for (int32_t jj = indexU[k]; jj < indexU[k + 1]; jj++) {
      const int32_t j = itemU[jj] - 1;
      if (j >= N) continue;  // halo columns only feed halo columns, which multiply ZP(halo) = 0 in the apply
      const int32_t pos = j < i ? item_find(itemL, iL0, iL1, j + 1) : item_find(itemU, iU0, iU1, j + 1);
      if (pos < 0) continue;  // not in the pattern of row i (j == i never is: see the header)
      double *dst = (j < i ? AL : AU) + (size_t)NN * pos;
      double a[NN];
#pragma unroll
      for (int e = 0; e < NN; e++) a[e] = dst[e];
      nn_ilu_update<ND>(a, aik, Dlu + (size_t)NN * k, AU + (size_t)NN * jj);
#pragma unroll
      for (int e = 0; e < NN; e++) dst[e] = a[e];
    }
  }
}

// The same level with 32 lanes per row (k_ilu0_factor_level32's scheme): lane t owns destination block t of row i (its nl
// lower, then nu upper blocks; nl + nu <= 32) in registers and walks k over L(i) in ascending order; the (i, k) block of a
// step is the owner lane's current value, taken by shuffle.  Every destination receives its updates in the reference's order.
template <int ND>
__global__ __launch_bounds__(256) void k_nn_ilu0_factor_level32(int32_t slot0, int32_t slot1, const int32_t *__restrict__ slot_row,
                                                                int32_t N, const int32_t *__restrict__ indexL,
                                                                const int32_t *__restrict__ itemL,
                                                                const int32_t *__restrict__ indexU,
                                                                const int32_t *__restrict__ itemU, const double *__restrict__ Dlu,
                                                                double *__restrict__ AL, double *__restrict__ AU) {
  constexpr int NN = ND * ND;
  const int t = threadIdx.x & 31;
  const int32_t s = slot0 + blockIdx.x * 8 + (threadIdx.x >> 5);
  if (s >= slot1) return;  // uniform over the 32-lane group
  const int32_t i = slot_row[s];
  if (i < 0) return;
  const int32_t iL0 = indexL[i], nl = indexL[i + 1] - iL0, iU0 = indexU[i], nu = indexU[i + 1] - iU0;
  const bool active = t < nl + nu;
  int32_t jt = -1;
  double *ptr = nullptr;
  if (active) {
    if (t < nl) { jt = itemL[iL0 + t] - 1; ptr = AL + (size_t)NN * (iL0 + t); }
    else { jt = itemU[iU0 + (t - nl)] - 1; ptr = AU + (size_t)NN * (iU0 + (t - nl)); }
  }
  double a[NN];
#pragma unroll
  for (int e = 0; e < NN; e++) a[e] = active ? ptr[e] : 0.0;
  for (int q = 0; q < nl; q++) {
    const int32_t k = itemL[iL0 + q] - 1;
    double aik[NN];
#pragma unroll
    for (int e = 0; e < NN; e++) aik[e] = __shfl(a[e], q, 32);
    if (active && jt > k && jt < N) {
      const int32_t pos = item_find(itemU, indexU[k], indexU[k + 1], jt + 1);
      if (pos >= 0) nn_ilu_update<ND>(a, aik, Dlu + (size_t)NN * k, AU + (size_t)NN * pos);
    }
  }
  if (active) {
#pragma unroll
    for (int e = 0; e < NN; e++) ptr[e] = a[e];
  }
}

// factor blocks -> sweep layout: entry (slice, k, lane) takes block src[(base + k) * 64 + lane] of csr (-1: padding, zeros)
template <int ND>
__global__ __launch_bounds__(256) void k_nn_bell_gather(int32_t nslices, const int64_t *__restrict__ slice_ptr,
                                                        const int32_t *__restrict__ src, const double *__restrict__ csr,
                                                        double *__restrict__ val) {
  constexpr int NN = ND * ND;
  const int lane = threadIdx.x & 63;
  const int32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= nslices) return;
  const int64_t base = slice_ptr[s], w = slice_ptr[s + 1] - base;
  for (int64_t k = 0; k < w; k++) {
    const int32_t j = src[(base + k) * 64 + lane];
#pragma unroll
    for (int q = 0; q < NN; q++) val[nn_pos(NN, base + k, q, lane)] = j >= 0 ? csr[(size_t)NN * j + q] : 0.0;
  }
}

// One level of the sweeps (the fallback of k_nn_tri_dataflow, and FX_DATAFLOW=0), one thread per row of a slice, the row's blocks in layout order (L ascending, U descending).
// FWD: z_i = Dlu_i^-1 (z_i - sum A_ij z_j), the sums run down from z_i as the reference's SW(ii) = SW(ii) - ... does;
// backward: z_i = z_i - Dlu_i^-1 (sum A_ij z_j).  Slices [s0, s1) are one level: mutually independent.
template <int ND, bool FWD>
__global__ __launch_bounds__(64) void k_nn_ilu_rows(int32_t s0, int32_t s1, const int64_t *__restrict__ slice_ptr,
                                                     const int32_t *__restrict__ slot_row, const int32_t *__restrict__ col,
                                                     const double *__restrict__ val, double *z, const double *__restrict__ dlu,
                                                     const int32_t *__restrict__ gate, int32_t gate_val) {
  if (gate && *gate != gate_val) return;  // device-resident Krylov state
  const int lane = threadIdx.x & 63;
  const int32_t s = s0 + blockIdx.x;  // one slice per workgroup: a level of a few slices still spreads over as many CUs
  if (s >= s1) return;
  const int32_t row = slot_row[(size_t)s * 64 + lane];
  const int64_t base = slice_ptr[s];
  const int w = (int)(slice_ptr[s + 1] - base);
  double acc[ND];
#pragma unroll
  for (int d = 0; d < ND; d++) acc[d] = (FWD && row >= 0) ? z[(size_t)ND * row + d] : 0.0;
  for (int k = 0; k < w; k++) {
    const int32_t cidx = col[(base + k) * 64 + lane];
    const double *v = val + (size_t)(base + k) * (ND * ND) * 64;
    double a[ND * ND], xv[ND];
#pragma unroll
    for (int j = 0; j < (ND * ND) / 2; j++) {
      const fx_d2 wd = __builtin_nontemporal_load((const fx_d2 *)(v + (size_t)2 * j * 64) + lane);
      a[2 * j] = wd.x;
      a[2 * j + 1] = wd.y;
    }
    if ((ND * ND) & 1) a[ND * ND - 1] = __builtin_nontemporal_load(v + (size_t)(ND * ND - 1) * 64 + lane);
#pragma unroll
    for (int e = 0; e < ND; e++) xv[e] = z[(size_t)ND * cidx + e];
#pragma unroll
    for (int d = 0; d < ND; d++)
#pragma unroll
      for (int e = 0; e < ND; e++) acc[d] = FWD ? acc[d] - a[d * ND + e] * xv[e] : acc[d] + a[d * ND + e] * xv[e];
  }
  if (row < 0) return;
  nn_lusolve<ND, false>(dlu + (size_t)ND * ND * row, acc);
#pragma unroll
  for (int d = 0; d < ND; d++) z[(size_t)ND * row + d] = FWD ? acc[d] : z[(size_t)ND * row + d] - acc[d];
}

// The same sweeps as ONE persistent launch per apply (the hand-off protocol of k_tri_dataflow): workgroup w (one wave) owns
// slices w, w + G, ...; it walks them upwards in the forward sweep and downwards in the backward sweep.  A row's entries are
// published in zf (forward) / zb (backward) with agent-scope stores over FX_DF_SENTINEL tags (k_df_fill), and a gather waits,
// boundedly, until its producer has published.  A slice waits only for slices earlier in its sweep's order (L(i) lies in
// lower levels, U(i) in higher ones: nn_ilu_symbolic checks this), so with all G workgroups resident the first unfinished
// slice can always run; G is clamped to the occupancy bound.  Every row sums its blocks in the order k_nn_ilu_rows does, with
// the same operands (a padding block names the row itself, whose value both forms read as the one the per-level form sees),
// so both forms give the same bits.  A wait that runs out (FX_DF_TIMEOUT_TICKS, or nsleep < 0: the FX_DEBUG_DF_FAIL hook)
// raises *err and the launch drains without waiting; the host then redoes the work with per-level launches.
template <int ND, bool FWD>
__device__ __forceinline__ void nn_df_slice(int32_t s, const int64_t *__restrict__ slice_ptr, const int32_t *__restrict__ slot_row,
                                            const int32_t *__restrict__ col, const double *__restrict__ val,
                                            const double *__restrict__ dlu, const double *r, double *zf, double *zb, double *z,
                                            int32_t *__restrict__ err, bool &dead) {
  const int lane = threadIdx.x & 63;
  const int32_t row = slot_row[(size_t)s * 64 + lane];
  const int64_t base = slice_ptr[s];
  const int w = (int)(slice_ptr[s + 1] - base);
  const double *src = FWD ? zf : zb;  // the vector this sweep produces and gathers
  double own[ND];  // the value the per-level form holds in z for this row while it sums: r (forward) / the forward result
#pragma unroll
  for (int d = 0; d < ND; d++) own[d] = row < 0 ? 0.0 : FWD ? r[(size_t)ND * row + d] : df_load(zf + (size_t)ND * row + d);
  double acc[ND];
#pragma unroll
  for (int d = 0; d < ND; d++) acc[d] = FWD ? own[d] : 0.0;
  for (int k = 0; k < w; k++) {
    const int32_t cidx = col[(base + k) * 64 + lane];
    const double *v = val + (size_t)(base + k) * (ND * ND) * 64;
    double a[ND * ND], xv[ND];
#pragma unroll
    for (int j = 0; j < (ND * ND) / 2; j++) {
      const fx_d2 wd = __builtin_nontemporal_load((const fx_d2 *)(v + (size_t)2 * j * 64) + lane);
      a[2 * j] = wd.x;
      a[2 * j + 1] = wd.y;
    }
    if ((ND * ND) & 1) a[ND * ND - 1] = __builtin_nontemporal_load(v + (size_t)(ND * ND - 1) * 64 + lane);
    const bool need = row >= 0 && cidx != row;
    bool miss = false;
#pragma unroll
    for (int e = 0; e < ND; e++) {
      xv[e] = need ? df_load(src + (size_t)ND * cidx + e) : own[e];
      miss |= need && __double_as_longlong(xv[e]) == FX_DF_SENTINEL;
    }
    unsigned long long t0 = 0;
    for (unsigned spins = 1; __any(miss) && !dead; spins++) {  // bounded wait for the producer of this block's column
      if (miss) {
        miss = false;
#pragma unroll
        for (int e = 0; e < ND; e++) {
          xv[e] = df_load(src + (size_t)ND * cidx + e);
          miss |= __double_as_longlong(xv[e]) == FX_DF_SENTINEL;
        }
      }
      if ((spins & 255u) == 0u) {
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        if (t0 == 0) t0 = now;
        const int e = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (e != 0 || now - t0 > FX_DF_TIMEOUT_TICKS) {
          if (e == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          dead = true;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < ND; d++)
#pragma unroll
      for (int e = 0; e < ND; e++) acc[d] = FWD ? acc[d] - a[d * ND + e] * xv[e] : acc[d] + a[d * ND + e] * xv[e];
  }
  if (row < 0) return;
  nn_lusolve<ND, false>(dlu + (size_t)ND * ND * row, acc);
#pragma unroll
  for (int d = 0; d < ND; d++) {
    if (FWD) {
      df_store(zf + (size_t)ND * row + d, acc[d]);
    } else {
      const double x = own[d] - acc[d];
      df_store(zb + (size_t)ND * row + d, x);
      z[(size_t)ND * row + d] = x;
    }
  }
}

template <int ND>
__global__ __launch_bounds__(64) void k_nn_tri_dataflow(int32_t nslices, const int64_t *__restrict__ Lptr, const int32_t *__restrict__ slot_row,
                                                        const int32_t *__restrict__ Lcol, const double *__restrict__ Lval,
                                                        const int64_t *__restrict__ Uptr, const int32_t *__restrict__ Ucol,
                                                        const double *__restrict__ Uval, const double *__restrict__ dlu, const double *r,
                                                        double *zf, double *zb, double *z, const int32_t *__restrict__ gate,
                                                        int32_t gate_val, int32_t *__restrict__ err, int nsleep) {
  if (gate && *gate != gate_val) return;  // device-resident Krylov state
  if (nsleep < 0) {  // test hook (FX_DEBUG_DF_FAIL): a launch whose bounded wait ran out at once -- nothing usable written, err raised
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  bool dead = false;
  for (int32_t s = blockIdx.x; s < nslices; s += gridDim.x)
    nn_df_slice<ND, true>(s, Lptr, slot_row, Lcol, Lval, dlu, r, zf, zb, z, err, dead);
  const int32_t mine = nslices > (int32_t)blockIdx.x ? (nslices - 1 - (int32_t)blockIdx.x) / (int32_t)gridDim.x : -1;
  for (int32_t s = (int32_t)blockIdx.x + mine * (int32_t)gridDim.x; mine >= 0 && s >= 0; s -= gridDim.x)
    nn_df_slice<ND, false>(s, Uptr, slot_row, Ucol, Uval, dlu, r, zf, zb, z, err, dead);
}

// SCALING=YES: the device copies of the caller's off-diagonal blocks scaled as the SpMV layout is (k_nn_scale_bell), rows 0..N-1
template <int ND>
__global__ __launch_bounds__(128) void k_nn_scale_csr(int32_t N, const int32_t *__restrict__ index, const int32_t *__restrict__ item, double *__restrict__ A,
                               const double *__restrict__ scale) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int32_t j = index[i]; j < index[i + 1]; j++) {
    const int32_t c = item[j] - 1;
#pragma unroll
    for (int d = 0; d < ND; d++)
#pragma unroll
      for (int e = 0; e < ND; e++) {
        double &x = A[(size_t)ND * ND * j + d * ND + e];
        x = (x * scale[(size_t)ND * i + d]) * scale[(size_t)ND * c + e];
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
#define NN_ILU_DISPATCH(nd, ...)                                                                                \
  switch (nd) {                                                                                                 \
    case 4: { constexpr int ND = 4; __VA_ARGS__; } break;                                                       \
    case 5: { constexpr int ND = 5; __VA_ARGS__; } break;                                                       \
    case 6: { constexpr int ND = 6; __VA_ARGS__; } break;                                                       \
    default: g_fx_error = "block ILU(0) on the generic-block path needs NDOF 4, 5 or 6"; return FX_ERROR_INCONS_PC;  \
  }

// Sliced layout of the rows `rows` (slot -> row or -1) whose blocks fill(slot, out) lists as CSR indices: structure on the
// host, values gathered on the device from a CSR block array by k_nn_bell_gather.  src: device, nblocks_padded * 64.
template <class Fill>
static int nn_bell_build_idx(NnBell &b, int nd2, const std::vector<int32_t> &rows, int32_t **src, Fill fill) {
  nn_bell_free(b);
  dev_free(*src);
  b.nslots = (int32_t)rows.size();
  b.nslices = b.nslots / 64;
  std::vector<int64_t> sp((size_t)b.nslices + 1, 0);
  parallel_for(b.nslices, [&](int64_t s0, int64_t s1) {
    std::vector<std::pair<int32_t, int32_t>> tmp;
    for (int64_t s = s0; s < s1; s++) {
      size_t w = 0;
      for (int l = 0; l < 64; l++) {
        tmp.clear();
        if (rows[(size_t)s * 64 + l] >= 0) fill((int64_t)s * 64 + l, tmp);
        w = std::max(w, tmp.size());
      }
      sp[s + 1] = (int64_t)w;
    }
  });
  for (int32_t s = 0; s < b.nslices; s++) sp[s + 1] += sp[s];
  b.nblocks_padded = sp[b.nslices];
  const size_t ne = (size_t)std::max<int64_t>(b.nblocks_padded, 1) * 64;
  std::vector<int32_t> col(ne, 0), idx(ne, -1);
  parallel_for(b.nslices, [&](int64_t s0, int64_t s1) {
    std::vector<std::pair<int32_t, int32_t>> tmp;  // (column row id, CSR index)
    for (int64_t s = s0; s < s1; s++)
      for (int l = 0; l < 64; l++) {
        tmp.clear();
        if (rows[(size_t)s * 64 + l] >= 0) fill((int64_t)s * 64 + l, tmp);
        for (size_t k = 0; k < tmp.size(); k++) {
          col[(size_t)(sp[s] + k) * 64 + l] = tmp[k].first;
          idx[(size_t)(sp[s] + k) * 64 + l] = tmp[k].second;
        }
        // padding blocks of a row (value 0) name the row itself: the dataflow sweep then never waits on them and multiplies
        // the value the per-level sweep multiplies (k_nn_tri_dataflow)
        if (rows[(size_t)s * 64 + l] >= 0)
          for (int64_t k = (int64_t)tmp.size(); k < sp[s + 1] - sp[s]; k++) col[(size_t)(sp[s] + k) * 64 + l] = rows[(size_t)s * 64 + l];
      }
  });
  if (dev_alloc(&b.slice_ptr, sp.size()) || dev_alloc(&b.slot_row, std::max<size_t>(rows.size(), 1)) || dev_alloc(&b.col, ne) ||
      dev_alloc(src, ne) || dev_alloc(&b.val, ne * nd2))
    return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpy(b.slice_ptr, sp.data(), sp.size() * 8, hipMemcpyHostToDevice));
  if (!rows.empty()) HIP_TRY(hipMemcpy(b.slot_row, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b.col, col.data(), ne * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(*src, idx.data(), ne * 4, hipMemcpyHostToDevice));
  return 0;
}

// Levels of the natural-order lower pattern and the level-ordered layouts of L (ascending columns, BILU_nn.f90:107) and U
// (descending, :138, halo columns dropped); the CSR profile goes up for the factor kernels.
static int nn_ilu_symbolic(fx_context *c) {
  NnDev *n = nn_of(c);
  const int32_t N = n->N, NP = n->NP;
  const int32_t *iL = n->h_indexL.data(), *jL = n->h_itemL.data(), *iU = n->h_indexU.data(), *jU = n->h_itemU.data();
  std::vector<int32_t> level((size_t)std::max(N, 1), 0);
  int32_t nlev = 0;
  n->ilu_max_row_blocks = 0;
  for (int32_t i = 0; i < N; i++) {  // every k in L(i) is < i
    int32_t l = 0;
    for (int32_t j = iL[i]; j < iL[i + 1]; j++) l = std::max(l, level[jL[j] - 1]);
    level[i] = l + 1;
    nlev = std::max(nlev, l + 1);
    n->ilu_max_row_blocks = std::max(n->ilu_max_row_blocks, (iL[i + 1] - iL[i]) + (iU[i + 1] - iU[i]));
  }
  std::vector<int32_t> cnt((size_t)nlev + 2, 0);
  for (int32_t i = 0; i < N; i++) cnt[level[i]]++;
  std::vector<int32_t> start((size_t)nlev + 2, 0);  // first slot of level l at start[l], levels padded to whole slices
  for (int32_t l = 1; l <= nlev; l++) start[l + 1] = start[l] + (cnt[l] + 63) / 64 * 64;
  std::vector<int32_t> rows((size_t)start[nlev + 1], -1), fillpos(start.begin(), start.end());
  for (int32_t i = 0; i < N; i++) rows[fillpos[level[i]]++] = i;  // natural order inside a level
  n->ncolor = nlev;
  n->color_slice.assign((size_t)nlev + 1, 0);
  for (int32_t l = 1; l <= nlev; l++) n->color_slice[l] = start[l + 1] / 64;
  auto fillL = [&](int64_t slot, std::vector<std::pair<int32_t, int32_t>> &e) {
    const int32_t r = rows[slot];
    for (int32_t j = iL[r]; j < iL[r + 1]; j++) e.push_back({jL[j] - 1, j});
  };
  auto fillU = [&](int64_t slot, std::vector<std::pair<int32_t, int32_t>> &e) {
    const int32_t r = rows[slot];
    for (int32_t j = iU[r + 1] - 1; j >= iU[r]; j--)
      if (jU[j] <= N) e.push_back({jU[j] - 1, j});
  };
  for (int32_t i = 0; i < N; i++)  // the backward sweeps need every U column in a higher level (a structurally symmetric profile)
    for (int32_t j = iU[i]; j < iU[i + 1]; j++)
      if (jU[j] <= N && level[jU[j] - 1] <= level[i]) {
        g_fx_error = "block ILU(0): the profile is not structurally symmetric (an upper block lies in a lower or equal level)";
        return FX_ERROR_UNSUPPORTED;
      }
  const int nd2 = n->ndof * n->ndof;
  if (nn_bell_build_idx(n->L, nd2, rows, &n->ilu_srcL, fillL) || nn_bell_build_idx(n->U, nd2, rows, &n->ilu_srcU, fillU))
    return FX_ERROR_RUNTIME;
  const size_t npl = n->h_itemL.size(), npu = n->h_itemU.size();
  dev_free(n->ilu_iL); dev_free(n->ilu_jL); dev_free(n->ilu_iU); dev_free(n->ilu_jU);
  if (dev_alloc(&n->ilu_iL, (size_t)NP + 1) || dev_alloc(&n->ilu_iU, (size_t)NP + 1) || dev_alloc(&n->ilu_jL, std::max<size_t>(npl, 1)) ||
      dev_alloc(&n->ilu_jU, std::max<size_t>(npu, 1)))
    return FX_ERROR_RUNTIME;
  {  // private sweep vectors of the dataflow form (whole 16-byte words for k_df_fill), and its co-residency bound
    const size_t len = ((size_t)n->ndof * std::max(NP, 1) + 1) / 2 * 2;
    dev_free(n->ilu_zf); dev_free(n->ilu_zb);
    if (dev_alloc(&n->ilu_zf, len) || dev_alloc(&n->ilu_zb, len)) return FX_ERROR_RUNTIME;
    n->ilu_zlen = len;
    int pc = 64;
    auto occ = [&](auto kernel) {
      int b = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kernel, 64, 0) != hipSuccess) b = 1;
      pc = std::min(pc, b);
    };
    occ(k_nn_tri_dataflow<4>); occ(k_nn_tri_dataflow<5>); occ(k_nn_tri_dataflow<6>);
    (void)hipGetLastError();
    n->ilu_df_grid_max = std::max(1, c->n_cu * std::max(1, std::min(pc, 8)));
  }
  HIP_TRY(hipMemcpy(n->ilu_iL, iL, ((size_t)NP + 1) * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(n->ilu_iU, iU, ((size_t)NP + 1) * 4, hipMemcpyHostToDevice));
  if (npl) HIP_TRY(hipMemcpy(n->ilu_jL, jL, npl * 4, hipMemcpyHostToDevice));
  if (npu) HIP_TRY(hipMemcpy(n->ilu_jU, jU, npu * 4, hipMemcpyHostToDevice));
  n->ilu_symbolic = true;
  return 0;
}

// FORM_ILU0: the caller's off-diagonal blocks (scaled when the solve scales: they are what the reference factors then),
// Dlu = k_nn_lu of the sigma-scaled D (already in n->alu), one factor launch per level, then the layouts' values.
static int nn_ilu_numeric(fx_context *c, bool scaled) {
  NnDev *n = nn_of(c);
  const int nd = n->ndof, nd2 = nd * nd;
  const size_t npl = n->h_itemL.size(), npu = n->h_itemU.size();
  if (!n->cur_AL || !n->cur_AU) { g_fx_error = "block ILU(0) set-up: the caller's AL / AU are not available"; return FX_ERROR_RUNTIME; }
  // the CSR copies live for the set-up only: the sweeps stream the layouts
  dev_free(n->ilu_AL); dev_free(n->ilu_AU);
  if (dev_alloc(&n->ilu_AL, (size_t)nd2 * std::max<size_t>(npl, 1)) || dev_alloc(&n->ilu_AU, (size_t)nd2 * std::max<size_t>(npu, 1)))
    return FX_ERROR_RUNTIME;
  if (npl) HIP_TRY(hipMemcpyAsync(n->ilu_AL, n->cur_AL, npl * nd2 * 8, hipMemcpyHostToDevice, c->stream));
  if (npu) HIP_TRY(hipMemcpyAsync(n->ilu_AU, n->cur_AU, npu * nd2 * 8, hipMemcpyHostToDevice, c->stream));
  if (scaled && n->N > 0) {
    NN_ILU_DISPATCH(nd, hipLaunchKernelGGL((k_nn_scale_csr<ND>), dim3((n->N + 127) / 128), dim3(128), 0, c->stream, n->N, n->ilu_iL,
                                           n->ilu_jL, n->ilu_AL, n->scale);
                    hipLaunchKernelGGL((k_nn_scale_csr<ND>), dim3((n->N + 127) / 128), dim3(128), 0, c->stream, n->N, n->ilu_iU,
                                       n->ilu_jU, n->ilu_AU, n->scale))
  }
  n->ilu_factor_lanes = n->ilu_max_row_blocks <= 32 ? 32 : 1;
  for (int l = 1; l < n->ncolor; l++) {  // level 1 rows have no lower blocks
    const int32_t s0 = n->color_slice[l] * 64, s1 = n->color_slice[l + 1] * 64;
    if (n->ilu_factor_lanes == 32) {
      NN_ILU_DISPATCH(nd, hipLaunchKernelGGL((k_nn_ilu0_factor_level32<ND>), dim3((s1 - s0 + 7) / 8), dim3(256), 0, c->stream, s0, s1,
                                             n->L.slot_row, n->N, n->ilu_iL, n->ilu_jL, n->ilu_iU, n->ilu_jU, n->alu, n->ilu_AL,
                                             n->ilu_AU))
    } else {
      NN_ILU_DISPATCH(nd, hipLaunchKernelGGL((k_nn_ilu0_factor_level<ND>), dim3((s1 - s0 + 127) / 128), dim3(128), 0, c->stream, s0,
                                             s1, n->L.slot_row, n->N, n->ilu_iL, n->ilu_jL, n->ilu_iU, n->ilu_jU, n->alu, n->ilu_AL,
                                             n->ilu_AU))
    }
  }
  if (n->L.nslices > 0) {
    NN_ILU_DISPATCH(nd, hipLaunchKernelGGL((k_nn_bell_gather<ND>), dim3((n->L.nslices + 3) / 4), dim3(256), 0, c->stream, n->L.nslices,
                                           n->L.slice_ptr, n->ilu_srcL, n->ilu_AL, n->L.val);
                    hipLaunchKernelGGL((k_nn_bell_gather<ND>), dim3((n->U.nslices + 3) / 4), dim3(256), 0, c->stream, n->U.nslices,
                                       n->U.slice_ptr, n->ilu_srcU, n->ilu_AU, n->U.val))
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  dev_free(n->ilu_AL); dev_free(n->ilu_AU);
  return 0;
}

// A dataflow sweep of this context gave up (its bounded wait ran out): the context now sweeps with per-level launches for
// good, and the caller redoes its work.  Called after every host-visible synchronisation of a path that ran a block ILU(0) apply.
static bool nn_df_take_error(fx_context *c) {
  NnDev *n = nn_of(c);
  if (n->precond_kind != 10) return false;
  int32_t e = 0;
  if (hipMemcpy(&e, c->df_err, 4, hipMemcpyDeviceToHost) != hipSuccess || e == 0) return false;
  (void)hipMemset(c->df_err, 0, 4);
  c->df_mode = 0;
  c->df_fallbacks++;
  n->ilu_df_fallbacks++;
  return true;
}

// z <- M^-1 z in place (hecmw_precond_BILU_nn_apply): one persistent dataflow launch (FX_DATAFLOW >= 1, the default), or
// per-level launches, forward over ascending levels, backward over descending ones.  Both give the same bits.
static int nn_ilu_sweeps(fx_context *c, double *zp, const int32_t *gate, int32_t gate_val) {
  NnDev *n = nn_of(c);
  if (c->df_mode >= 1 && n->L.nslices > 0) {
    hipLaunchKernelGGL(k_df_fill, dim3(grid_for((int64_t)(n->ilu_zlen / 2), 256, 2048)), dim3(256), 0, c->stream,
                       (int64_t)(n->ilu_zlen / 2), (fx_u4 *)n->ilu_zf, (fx_u4 *)n->ilu_zb);
    const int grid = std::min(n->L.nslices, c->df_grid > 0 ? std::min(c->df_grid, n->ilu_df_grid_max) : std::min(c->n_cu, n->ilu_df_grid_max));
    n->ilu_df_grid_last = grid;
    NN_ILU_DISPATCH(n->ndof, hipLaunchKernelGGL((k_nn_tri_dataflow<ND>), dim3(grid), dim3(64), 0, c->stream, n->L.nslices, n->L.slice_ptr,
                                                n->L.slot_row, n->L.col, n->L.val, n->U.slice_ptr, n->U.col, n->U.val, n->alu, zp,
                                                n->ilu_zf, n->ilu_zb, zp, gate, gate_val, c->df_err, c->dbg_df_fail ? -1 : 0))
    HIP_TRY(hipGetLastError());
    return 0;
  }
  for (int l = 0; l < n->ncolor; l++) {
    const int32_t s0 = n->color_slice[l], s1 = n->color_slice[l + 1];
    if (s1 > s0)
      NN_ILU_DISPATCH(n->ndof, hipLaunchKernelGGL((k_nn_ilu_rows<ND, true>), dim3(s1 - s0), dim3(64), 0, c->stream, s0, s1,
                                                  n->L.slice_ptr, n->L.slot_row, n->L.col, n->L.val, zp, n->alu, gate, gate_val))
  }
  for (int l = n->ncolor - 1; l >= 0; l--) {
    const int32_t s0 = n->color_slice[l], s1 = n->color_slice[l + 1];
    if (s1 > s0)
      NN_ILU_DISPATCH(n->ndof, hipLaunchKernelGGL((k_nn_ilu_rows<ND, false>), dim3(s1 - s0), dim3(64), 0, c->stream, s0, s1,
                                                  n->U.slice_ptr, n->U.slot_row, n->U.col, n->U.val, zp, n->alu, gate, gate_val))
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
