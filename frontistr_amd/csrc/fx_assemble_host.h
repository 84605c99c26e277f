// Host helpers of the assembly side (included at the end of fistr_hip.hip); the linear entry points are in fx_assemble_groups.h.
#pragma once
#include <cstdarg>

// hecmw_mat_con (hecmw_mat_con.f90:23-268): CRS block profile from element connectivity.
// Node -> element incidence by counting sort (host threads, relaxed atomic counters: the order of a node's elements does
// not matter, its neighbour set is sorted afterwards), then per node the sorted unique set of the nodes of its elements,
// split into lower / upper; rows are independent => one contiguous chunk of nodes per host thread, each keeping the lists
// of its rows back to back.  The two-call protocol (count, then fill) would build all of that twice; the first call keeps
// the chunks (~ (NPL + NPU + NP) ints) for the second, which then only splits them.
struct MatConCache {
  const int32_t *conn = nullptr;
  int32_t NP = 0, n_elem = 0, nn = 0;
  std::vector<int64_t> cstart;             // chunk c holds the rows of nodes cstart[c] + 1 .. cstart[c + 1] (1-based)
  std::vector<std::vector<int32_t>> rows;  // per chunk: sorted unique neighbour ids (1-based, itself included) of its nodes, back to back
  std::vector<int32_t> rlen;               // per node (index 1..NP): length of its list
  void clear() {
    conn = nullptr;
    std::vector<int64_t>().swap(cstart);
    std::vector<std::vector<int32_t>>().swap(rows);
    std::vector<int32_t>().swap(rlen);
  }
  template <class F>
  void for_chunks(F f) const {  // f(chunk) on one host thread per chunk
    std::vector<std::thread> th;
    for (size_t c = 0; c + 1 < cstart.size(); c++) th.emplace_back([=] { f((int)c); });
    for (auto &t : th) t.join();
  }
};
static thread_local MatConCache g_matcon;  // per calling thread: the count and the fill call of one profile come from the same thread; concurrent callers (one thread per subdomain) do not share it

extern "C" int fx_mat_con(int32_t NP, int32_t n_elem, int32_t nn, const int32_t *conn, int32_t *indexL, int32_t *indexU,
                          int32_t *itemL, int32_t *itemU) {
  MatConCache &mc = g_matcon;
  const bool fill = itemL && itemU;
  if (!(fill && mc.conn == conn && mc.NP == NP && mc.n_elem == n_elem && mc.nn == nn && !mc.rlen.empty())) {
    mc.clear();
    PhaseTimer pt("mat_con");
    const int64_t tot = (int64_t)n_elem * nn;
    std::vector<int64_t> ptr((size_t)NP + 2, 0);
    {
      std::vector<int32_t> deg((size_t)NP + 2, 0);
      int bad = 0;
      parallel_for(tot, [&](int64_t a, int64_t b) {
        for (int64_t k = a; k < b; k++) {
          const int32_t v = conn[k];
          if (v < 1 || v > NP) { __atomic_store_n(&bad, 1, __ATOMIC_RELAXED); return; }
          __atomic_fetch_add(&deg[v + 1], 1, __ATOMIC_RELAXED);
        }
      });
      if (bad) { g_fx_error = "fx_mat_con: node id out of range"; return FX_ERROR_RUNTIME; }
      for (int32_t i = 1; i <= NP + 1; i++) ptr[i] = ptr[i - 1] + deg[i];
    }
    pt.lap("count");
    std::vector<int32_t> inc((size_t)tot);
    {
      std::vector<int64_t> pos(ptr.begin(), ptr.end());
      parallel_for(n_elem, [&](int64_t a, int64_t b) {
        for (int64_t e = a; e < b; e++)
          for (int j = 0; j < nn; j++) inc[__atomic_fetch_add(&pos[conn[(size_t)e * nn + j]], 1, __ATOMIC_RELAXED)] = (int32_t)e;
      });
    }
    pt.lap("incidence");
    const int nt = (int)std::min<int64_t>(nthreads_host(), std::max<int64_t>(1, NP / 4096));
    mc.cstart.resize((size_t)nt + 1);
    for (int c = 0; c <= nt; c++) mc.cstart[c] = (int64_t)NP * c / nt;
    mc.rows.assign((size_t)nt, std::vector<int32_t>());
    mc.rlen.assign((size_t)NP + 1, 0);
    mc.for_chunks([&](int c) {
      std::vector<int32_t> &out = mc.rows[c];
      const int64_t a = mc.cstart[c], b = mc.cstart[c + 1];
      out.reserve((size_t)((ptr[b + 1] - ptr[a + 1]) * 7 / 2 + 64));  // a hex8 node: 8 elements x 8 nodes -> 27 neighbours
      std::vector<int32_t> buf;
      for (int64_t i = a + 1; i <= b; i++) {
        buf.clear();
        for (int64_t q = ptr[i]; q < ptr[i + 1]; q++) {
          const int32_t *en = conn + (size_t)inc[q] * nn;
          buf.insert(buf.end(), en, en + nn);
        }
        std::sort(buf.begin(), buf.end());
        buf.erase(std::unique(buf.begin(), buf.end()), buf.end());
        mc.rlen[i] = (int32_t)buf.size();
        out.insert(out.end(), buf.begin(), buf.end());
      }
    });
    mc.conn = conn; mc.NP = NP; mc.n_elem = n_elem; mc.nn = nn;
    pt.lap("row lists");
  }
  PhaseTimer pt2(fill ? "mat_con fill" : "mat_con index");
  if (!fill) {
    std::vector<int32_t> nl((size_t)NP + 1, 0), nu((size_t)NP + 1, 0);
    mc.for_chunks([&](int c) {
      const int32_t *r = mc.rows[c].data();
      for (int64_t i = mc.cstart[c] + 1; i <= mc.cstart[c + 1]; i++) {
        int32_t l = 0, u = 0;
        for (int32_t k = 0; k < mc.rlen[i]; k++) { l += (r[k] < i); u += (r[k] > i); }
        nl[i] = l; nu[i] = u;
        r += mc.rlen[i];
      }
    });
    indexL[0] = 0; indexU[0] = 0;
    int64_t cl = 0, cu = 0;
    for (int32_t i = 1; i <= NP; i++) {
      cl += nl[i]; cu += nu[i];
      if (cl > INT32_MAX || cu > INT32_MAX) { g_fx_error = "fx_mat_con: profile exceeds int32 (kint=4)"; mc.clear(); return FX_ERROR_RUNTIME; }
      indexL[i] = (int32_t)cl; indexU[i] = (int32_t)cu;
    }
    pt2.lap("indexL / indexU");
    return 0;  // the lists stay for the fill call
  }
  mc.for_chunks([&](int c) {
    const int32_t *r = mc.rows[c].data();
    for (int64_t i = mc.cstart[c] + 1; i <= mc.cstart[c + 1]; i++) {
      int32_t *pl = itemL + indexL[i - 1], *pu = itemU + indexU[i - 1];
      for (int32_t k = 0; k < mc.rlen[i]; k++) {
        const int32_t v = r[k];
        if (v < i) *pl++ = v;
        else if (v > i) *pu++ = v;
      }
      r += mc.rlen[i];
    }
  });
  pt2.lap("itemL / itemU");
  mc.clear();
  return 0;
}

// Host only: the ordering of the multicolour SSOR (hecmw_precond_SSOR_33.f90:102-111 -> hecmw_matrix_ordering_CM.f90:16-178,
// hecmw_matrix_ordering_MC.f90:15-72) as the library computes it: perm (new -> old, 1-based, N entries) and COLORindex(0:ncolor).
extern "C" int fx_ssor_ordering(int32_t N, const int32_t *indexL, const int32_t *itemL, const int32_t *indexU, const int32_t *itemU,
                                int32_t ncolor_in, int32_t *perm, int32_t *colorindex, int32_t colorindex_cap, int32_t *ncolor) {
  if (N < 1 || ncolor_in < 1) { g_fx_error = "fx_ssor_ordering: N and ncolor_in must be >= 1"; return FX_ERROR_RUNTIME; }
  fxo::Graph g = fxo::build_graph(N, indexL, itemL, indexU, itemU);
  std::vector<int32_t> seq = fxo::rcm_sequence(g), p0, cidx;
  fxo::multicolor(g, seq, ncolor_in, p0, cidx);
  *ncolor = (int32_t)cidx.size() - 1;
  if ((int32_t)cidx.size() > colorindex_cap) { g_fx_error = "fx_ssor_ordering: colorindex too small"; return FX_ERROR_RUNTIME; }
  for (int32_t i = 0; i < N; i++) perm[i] = p0[i] + 1;
  std::copy(cidx.begin(), cidx.end(), colorindex);
  return 0;
}

extern "C" int fx_color_elements(int32_t NP, int32_t n_elem, int32_t nn, const int32_t *conn, int32_t *order, int32_t *offsets,
                                 int32_t *ncolor) {
  for (int64_t k = 0; k < (int64_t)n_elem * nn; k++)
    if (conn[k] < 1 || conn[k] > NP) { g_fx_error = "fx_color_elements: node id out of range"; return FX_ERROR_RUNTIME; }
  std::vector<int32_t> ord, off;
  *ncolor = 0;
  for (int k = 0; k < 65; k++) offsets[k] = 0;
  if (!fxo::color_elements(n_elem, nn, conn, NP, ord, off)) return 0;
  *ncolor = (int32_t)off.size() - 1;
  std::copy(ord.begin(), ord.end(), order);
  for (size_t k = 0; k < off.size(); k++) offsets[k] = off[k];
  for (size_t k = off.size(); k < 65; k++) offsets[k] = off.back();
  return 0;
}

// Colour the elements of a mesh once (fx_order.cpp: color_elements) and keep the grouped element list on the device; the
// stiffness kernels then scatter colour by colour without atomics.  FX_ASM_ATOMIC=1 keeps the single-launch atomic scatter.
static void elem_colors_free(ElemColors &ec) {
  dev_free(ec.order);
  dev_free(ec.pos);
  dev_free(ec.dup);
  ec = ElemColors();
}
// f(C3Tag<ETYPE>()) for the element type given at run time: the five STF_C3 types (with_c3_type), or those and 361
// (with_solid_type).  false: not one of them, f is not called.
template <int ETYPE>
struct C3Tag {
  static constexpr int value = ETYPE;
};
template <class F>
static bool with_c3_type(int32_t etype, F &&f) {
  switch (etype) {
    case 341: f(C3Tag<341>()); return true;
    case 342: f(C3Tag<342>()); return true;
    case 351: f(C3Tag<351>()); return true;
    case 352: f(C3Tag<352>()); return true;
    case 362: f(C3Tag<362>()); return true;
    default: return false;
  }
}
template <class F>
static bool with_solid_type(int32_t etype, F &&f) {
  if (etype != 361) return with_c3_type(etype, f);
  f(C3Tag<361>());
  return true;
}
// f(std::integral_constant<int, MM>()) for the node count of a face: 3, 4, 6 or 8.  false: none of them, f is not called.
template <class F>
static bool with_face_nodes(int mm, F &&f) {
  switch (mm) {
    case 3: f(std::integral_constant<int, 3>()); return true;
    case 4: f(std::integral_constant<int, 4>()); return true;
    case 6: f(std::integral_constant<int, 6>()); return true;
    case 8: f(std::integral_constant<int, 8>()); return true;
    default: return false;
  }
}
// nodes and quadrature points per element of the types the device knows (C3_TABLE); 0: none of them
static int c3_nodes(int32_t etype) { return c3_facts(etype).nn; }
static int c3_points(int32_t etype) { return c3_facts(etype).nq; }
// the types of fx_assemble_c3 / fx_update_c3_linear / fx_element_stiffness_c3: what STF_C3 / UPDATE_C3 serve (361 has its own entries)
static bool c3_linear_type(int32_t etype) { return etype != 361 && c3_nodes(etype) != 0; }
#define FX_C3_UNSUPPORTED "element type not supported on the device (341, 342, 351, 352, 362; 361 through "

// g_fx_error = "<who>: <formatted text>"; returns code
static thread_local char g_fail_msg[240];
static int fx_fail(const char *who, int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  const int n = snprintf(g_fail_msg, sizeof g_fail_msg, "%s: ", who);
  vsnprintf(g_fail_msg + n, sizeof g_fail_msg - (size_t)n, fmt, ap);
  va_end(ap);
  g_fx_error = g_fail_msg;
  return code;
}
// what the stiffness kernels report through their error word
static int assembly_error(int32_t herr) {
  if (herr == 1) { g_fx_error = "PIVOT ERROR in the incompatible-mode condensation (calInverse)"; return FX_ERROR_RUNTIME; }
  if (herr == 2) { g_fx_error = "###ERROR### : cannot find connectivity (element not covered by the profile)"; return FX_ERROR_RUNTIME; }
  // the `stop` statements of the Mohr-Coulomb / Drucker-Prager material point (FX_YERR_*, fx_yield.h)
  if (herr == 3) { g_fx_error = "Math Error in Mohr-Coulomb calculation (|sin 3 theta| > 1, Elastoplastic.f90:85, :338, :474)"; return FX_ERROR_RUNTIME; }
  if (herr == 4) { g_fx_error = "Math error in return mapping (Elastoplastic.f90:496, :541)"; return FX_ERROR_RUNTIME; }
  if (herr == 5) { g_fx_error = "Jacobi iteration unable to converge (eigen3, utilities.f90:200)"; return FX_ERROR_RUNTIME; }
  // the `stop` statements of the F-bar hexahedron (FX_FERR_*, fx_nonlinear_fbar.h)
  if (herr == 6) { g_fx_error = "Error in Update_C3D8Fbar: too small element volume (static_LIB_Fbar.f90:121, :456)"; return FX_ERROR_RUNTIME; }
  if (herr == 7) { g_fx_error = "Error in Update_C3D8Fbar: too small average jacob (static_LIB_Fbar.f90:115, :450)"; return FX_ERROR_RUNTIME; }
  // the creep iteration of a NORTON point (FX_CERR_CREEP, fx_visco.h)
  if (herr == 8) { g_fx_error = "creep: the iteration of update_iso_creep on the consistency parameter did not end within 100 passes or left the finite numbers (creep.f90:185-195; the reference's loop has no bound)"; return FX_ERROR_RUNTIME; }
  return 0;
}
// hecmw_mat_clear (fstr_StiffMatrix.f90:40)
static int mat_clear(fx_context *c) {
  DevCSR &A = c->A;
  HIP_TRY(hipMemsetAsync(A.D, 0, (size_t)9 * A.NP * 8, c->stream));
  HIP_TRY(hipMemsetAsync(A.AL, 0, (size_t)9 * A.NPL * 8, c->stream));
  HIP_TRY(hipMemsetAsync(A.AU, 0, (size_t)9 * A.NPU * 8, c->stream));
  return 0;
}

// k_scatter_map over n elements (or faces) of nn nodes -- a face's 3, 4, 6, 8, an element's 4, 6, 8, 10, 15, 20 -- into pos, for the
// profile given
static void launch_scatter_map(fx_context *c, int nn, int32_t n, const int32_t *d_conn, const int32_t *indexL, const int32_t *itemL,
                               const int32_t *indexU, const int32_t *itemU, int32_t *pos) {
  const dim3 grid((unsigned)(((int64_t)nn * nn * n + 255) / 256)), bs(256);
  switch (nn) {
    case 3: hipLaunchKernelGGL((k_scatter_map<3>), grid, bs, 0, c->stream, n, d_conn, indexL, itemL, indexU, itemU, pos); break;
    case 4: hipLaunchKernelGGL((k_scatter_map<4>), grid, bs, 0, c->stream, n, d_conn, indexL, itemL, indexU, itemU, pos); break;
    case 6: hipLaunchKernelGGL((k_scatter_map<6>), grid, bs, 0, c->stream, n, d_conn, indexL, itemL, indexU, itemU, pos); break;
    case 8: hipLaunchKernelGGL((k_scatter_map<8>), grid, bs, 0, c->stream, n, d_conn, indexL, itemL, indexU, itemU, pos); break;
    case 10: hipLaunchKernelGGL((k_scatter_map<10>), grid, bs, 0, c->stream, n, d_conn, indexL, itemL, indexU, itemU, pos); break;
    case 15: hipLaunchKernelGGL((k_scatter_map<15>), grid, bs, 0, c->stream, n, d_conn, indexL, itemL, indexU, itemU, pos); break;
    case 20: hipLaunchKernelGGL((k_scatter_map<20>), grid, bs, 0, c->stream, n, d_conn, indexL, itemL, indexU, itemU, pos); break;
  }
}
// the position map of k_scatter_map for the resident profile and the device connectivity d_conn of the elements of type etype
// (FX_ASM_MAP=0: search every time); without first-write flags
static int ensure_scatter_map(fx_context *c, ElemColors &ec, int32_t n_elem, const int32_t *d_conn, int32_t etype) {
  static const bool off = getenv("FX_ASM_MAP") && atoi(getenv("FX_ASM_MAP")) == 0;
  if (off || ec.pos || ec.offsets.empty()) return 0;
  const int nn = c3_nodes(etype);
  const int64_t nmap = (int64_t)nn * nn * n_elem;
  if (dev_alloc(&ec.pos, (size_t)nmap)) { (void)hipGetLastError(); ec.pos = nullptr; return 0; }  // no memory: keep searching
  const DevCSR &A = c->A;
  ec.first_write = false;
  launch_scatter_map(c, nn, n_elem, d_conn, A.indexL, A.itemL, A.indexU, A.itemU, ec.pos);
  HIP_TRY(hipGetLastError());
  return 0;
}

// First-write flags (FX_ASM_FIRST=0: off) in the position maps of element groups that are launched one after another, each
// colour by colour: which contribution to a block comes first in that order.  An element's colour is "colours of the groups
// before its own + its colour" (k_elem_colors), k_scatter_first_min runs over every group's map into one set of per-block
// minima, then k_scatter_first_flag over every group's map.  The flags are set only where every group is coloured, has its map
// and no collapsed element; *covered: they are set and no block of the profile is left without a contribution, so the
// matrix needs no clearing.
struct FirstWriteGroup {
  ElemColors *ec;
  const int32_t *d_conn;
};
static int build_first_write(fx_context *c, const std::vector<FirstWriteGroup> &groups, bool *covered) {
  static const bool no_first = getenv("FX_ASM_FIRST") && atoi(getenv("FX_ASM_FIRST")) == 0;
  const DevCSR &A = c->A;
  *covered = false;
  if (groups.empty()) return 0;
  std::vector<int32_t> offs;  // every group's colour offsets, back to back
  for (const FirstWriteGroup &g : groups) {
    g.ec->first_write = false;
    if (!g.ec->pos || g.ec->offsets.empty() || g.ec->dup_nodes) return 0;
    offs.insert(offs.end(), g.ec->offsets.begin(), g.ec->offsets.end());
  }
  if (no_first) return 0;
  DevScratch tmp;
  int32_t *d_offs = nullptr, *minD = nullptr, *minL = nullptr, *minU = nullptr;
  unsigned long long *cnt = nullptr;
  std::vector<int32_t *> ecol(groups.size(), nullptr);
  bool mem = !(tmp.alloc(&d_offs, offs.size()) || tmp.alloc(&minD, (size_t)A.NP) || tmp.alloc(&minL, (size_t)std::max(A.NPL, 1)) ||
               tmp.alloc(&minU, (size_t)std::max(A.NPU, 1)) || tmp.alloc(&cnt, 1));
  for (size_t g = 0; g < groups.size() && mem; g++) mem = !tmp.alloc(&ecol[g], (size_t)groups[g].ec->n_elem);
  if (!mem) { (void)hipGetLastError(); return 0; }  // no memory for the temporaries: read-modify-write everywhere, cleared matrix
  HIP_TRY(hipMemcpyAsync(d_offs, offs.data(), offs.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(minD, 0x7F, (size_t)A.NP * 4, c->stream));  // FXA_NO_COLOR = 0x7F7F7F7F: above every colour
  HIP_TRY(hipMemsetAsync(minL, 0x7F, (size_t)std::max(A.NPL, 1) * 4, c->stream));
  HIP_TRY(hipMemsetAsync(minU, 0x7F, (size_t)std::max(A.NPU, 1) * 4, c->stream));
  HIP_TRY(hipMemsetAsync(cnt, 0, 8, c->stream));
  const dim3 b(256);
  for (int pass = 0; pass < 2; pass++) {  // the minima over all groups, then the flags
    const int32_t *go = d_offs;
    int32_t base = 0;
    for (size_t g = 0; g < groups.size(); g++) {
      const ElemColors &ec = *groups[g].ec;
      const int32_t ne = ec.n_elem, ncolor = (int32_t)ec.offsets.size() - 1;
      const int nn = c3_nodes(ec.etype);
      const dim3 gr((unsigned)(((int64_t)nn * nn * ne + 255) / 256));
      with_solid_type(ec.etype, [&](auto t) {
        constexpr int NN = C3El<decltype(t)::value>::NN;
        if (pass == 0) {
          hipLaunchKernelGGL(k_elem_colors, dim3((unsigned)((ne + 255) / 256)), b, 0, c->stream, ne, (const int32_t *)ec.order, go, ncolor,
                             base, ecol[g]);
          hipLaunchKernelGGL((k_scatter_first_min<NN>), gr, b, 0, c->stream, ne, groups[g].d_conn, (const int32_t *)ec.pos,
                             (const int32_t *)ecol[g], minD, minL, minU);
        } else {
          hipLaunchKernelGGL((k_scatter_first_flag<NN>), gr, b, 0, c->stream, ne, groups[g].d_conn, ec.pos, (const int32_t *)ecol[g],
                             (const int32_t *)minD, (const int32_t *)minL, (const int32_t *)minU);
        }
      });
      base += ncolor;
      go += ncolor + 1;
    }
  }
  hipLaunchKernelGGL(k_count_uncovered, dim3(1024), b, 0, c->stream, (int64_t)A.NP, (const int32_t *)minD, cnt);
  if (A.NPL > 0) hipLaunchKernelGGL(k_count_uncovered, dim3(1024), b, 0, c->stream, (int64_t)A.NPL, (const int32_t *)minL, cnt);
  if (A.NPU > 0) hipLaunchKernelGGL(k_count_uncovered, dim3(1024), b, 0, c->stream, (int64_t)A.NPU, (const int32_t *)minU, cnt);
  unsigned long long uncovered = 1;
  HIP_TRY(hipMemcpyAsync(&uncovered, cnt, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // also: `offs` is a host temporary
  HIP_TRY(hipGetLastError());
  *covered = (uncovered == 0);  // a block nobody writes would keep what it held: then the matrix is cleared as before (the flags are harmless)
  for (const FirstWriteGroup &g : groups) g.ec->first_write = *covered;
  return 0;
}
// Moves the elements that name a node twice out of the colour lists (order, off) into their own list (dups, dup_off), colour by
// colour, each list keeping the colour order; an empty dup_off: there are none.  k_add_elem_blocks adds them after the colours.
static bool names_a_node_twice(const int32_t *en, int nn = 8) {
  for (int x = 0; x < nn; x++)
    for (int y = x + 1; y < nn; y++)
      if (en[x] == en[y]) return true;
  return false;
}
static void split_collapsed(const int32_t *conn, std::vector<int32_t> &order, std::vector<int32_t> &off, std::vector<int32_t> &dups,
                            std::vector<int32_t> &dup_off) {
  std::vector<int32_t> keep, koff(1, 0);
  dups.clear();
  dup_off.assign(1, 0);
  keep.reserve(order.size());
  for (size_t k = 0; k + 1 < off.size(); k++) {
    for (int32_t q = off[k]; q < off[k + 1]; q++)
      (names_a_node_twice(conn + (size_t)8 * order[q]) ? dups : keep).push_back(order[q]);
    koff.push_back((int32_t)keep.size());
    dup_off.push_back((int32_t)dups.size());
  }
  order.swap(keep);
  off.swap(koff);
  if (dups.empty()) dup_off.clear();
}
// nn nodes per element of type etype (361: 8; 341: 4; 342: 10; 351: 6; 352: 15; 362: 20).  The colouring and the map are cached per (connectivity, type).
static int ensure_elem_colors(fx_context *c, ElemColors &ec, int32_t n_elem, const int32_t *conn, int32_t NP, int nn = 8,
                              int32_t etype = 361) {
  static const bool force_atomic = getenv("FX_ASM_ATOMIC") && atoi(getenv("FX_ASM_ATOMIC")) != 0;
  if (force_atomic || n_elem < 1) { elem_colors_free(ec); return 0; }
  // checksum of the connectivity: per-chunk FNV-1a, chunks combined in order
  const int64_t nw = (int64_t)nn * n_elem;
  const int nchunk = 64;
  uint64_t part[nchunk];
  bool bad[nchunk], dup[nchunk];
  parallel_for(nchunk, [&](int64_t a, int64_t b) {
    for (int64_t q = a; q < b; q++) {
      uint64_t h = 1469598103934665603ull;
      bool oob = false;
      for (int64_t i = nw * q / nchunk; i < nw * (q + 1) / nchunk; i++) {
        h = (h ^ (uint32_t)conn[i]) * 1099511628211ull;
        oob |= (conn[i] < 1 || conn[i] > NP);
      }
      bool dp = false;  // an element that names a node twice (a collapsed hexahedron): two of its nn^2 blocks coincide
      for (int64_t e = (int64_t)n_elem * q / nchunk; e < (int64_t)n_elem * (q + 1) / nchunk; e++)
        for (int x = 0; x < nn; x++)
          for (int y = x + 1; y < nn; y++) dp |= (conn[nn * e + x] == conn[nn * e + y]);
      part[q] = h; bad[q] = oob; dup[q] = dp;
    }
  });
  uint64_t key = 1469598103934665603ull;
  for (int q = 0; q < nchunk; q++) {
    if (bad[q]) { g_fx_error = "element connectivity: node id out of range"; return FX_ERROR_RUNTIME; }
    key = (key ^ part[q]) * 1099511628211ull;
  }
  if (ec.order && ec.n_elem == n_elem && ec.key == key && ec.etype == etype && !ec.offsets.empty()) return 0;
  elem_colors_free(ec);
  std::vector<int32_t> order, off, dups, dup_off;
  if (!fxo::color_elements(n_elem, nn, conn, NP, order, off)) return 0;  // a node in more than 64 elements: atomics
  ec.dup_nodes = false;
  for (int q = 0; q < nchunk; q++) ec.dup_nodes |= dup[q];
  if (ec.dup_nodes && nn != 8) { g_fx_error = "element connectivity: an element names a node twice"; return FX_ERROR_RUNTIME; }
  if (ec.dup_nodes) split_collapsed(conn, order, off, dups, dup_off);
  if (dev_alloc(&ec.order, std::max<size_t>(order.size(), 1)) || (!dups.empty() && dev_alloc(&ec.dup, dups.size())))
    return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(ec.order, order.data(), order.size() * 4, hipMemcpyHostToDevice, c->stream));
  if (!dups.empty()) HIP_TRY(hipMemcpyAsync(ec.dup, dups.data(), dups.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  ec.n_elem = n_elem; ec.key = key; ec.etype = etype; ec.offsets = off; ec.dup_off = dup_off;
  return 0;
}

// launch(grid, e0, e1) for every non-empty range [off[k], off[k + 1]) of an element list -- one launch per colour -- with
// epb elements per workgroup; one_range: a single launch over [off.front(), off.back()).
template <class L>
static void for_colour_ranges(const std::vector<int32_t> &off, bool one_range, int epb, L &&launch) {
  for (size_t k = 0; k + 1 < off.size(); k++) {
    const int32_t e0 = one_range ? off.front() : off[k], e1 = one_range ? off.back() : off[k + 1];
    if (e1 > e0) launch(dim3((unsigned)((e1 - e0 + epb - 1) / epb)), e0, e1);
    if (one_range) break;
  }
}
// One linear stiffness kernel (k_assemble_c3d8, k_assemble_tet, k_assemble_c3: epb elements per workgroup of bs lanes) over a mesh:
// colour by colour through the position map, or -- not coloured, or element matrices out (Kout) -- all elements in one launch.
using AssembleKernel = void (*)(int32_t, const double *, const int32_t *, double, double, double, const int32_t *, const int32_t *,
                                const int32_t *, const int32_t *, double *, double *, double *, double *, int32_t *, const int32_t *,
                                const double *, const int32_t *, int32_t, const int32_t *);
static void launch_coloured(fx_context *c, AssembleKernel kern, int epb, int bs, int32_t n_elem, const double *coord, const int32_t *conn,
                            double D11, double D12, double D44, double *Kout, int32_t *err, const int32_t *elem_mat, const double *mat_tab,
                            const ElemColors *ec) {
  const DevCSR &A = c->A;
  const bool coloured = ec && !ec->offsets.empty() && !Kout;
  const int32_t *list = coloured ? ec->order : nullptr, *pos = coloured ? ec->pos : nullptr;
  for_colour_ranges(coloured ? ec->offsets : std::vector<int32_t>{0, n_elem}, false, epb, [&](dim3 grid, int32_t e0, int32_t e1) {
    hipLaunchKernelGGL(kern, grid, dim3(bs), 0, c->stream, e1, coord, conn, D11, D12, D44, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL,
                       A.AU, Kout, err, elem_mat, mat_tab, list, e0, pos);
  });
}

// TYPE=361 (elemopt 1 IC, 2 B-bar, 3 FI) through k_assemble_c3d8, 341 / 342 through k_assemble_tet, 351 / 352 / 362 through
// k_assemble_c3 (elemopt unused).  dup_k: room for the element matrices of the collapsed hexahedra of ec.
static void launch_assemble(fx_context *c, int32_t etype, int elemopt, int32_t n_elem, const double *coord, const int32_t *conn, double D11,
                            double D12, double D44, double *Kout, int32_t *err, const int32_t *elem_mat, const double *mat_tab,
                            const ElemColors *ec, double *dup_k = nullptr) {
  if (with_c3_type(etype, [&](auto t) {
        using El = C3El<decltype(t)::value>;
        AssembleKernel kern;
        if constexpr (El::TET) kern = k_assemble_tet<decltype(t)::value>;
        else kern = k_assemble_c3<decltype(t)::value>;
        launch_coloured(c, kern, El::EPB, El::BS, n_elem, coord, conn, D11, D12, D44, Kout, err, elem_mat, mat_tab, ec);
      }))
    return;
  const AssembleKernel kern = elemopt == 1 ? k_assemble_c3d8<1> : (elemopt == 2 ? k_assemble_c3d8<2> : k_assemble_c3d8<3>);
  const int epb = elemopt == 1 ? FXA_EPB(1) : FXA_EPB(3), bs = elemopt == 1 ? FXA_BS(1) : FXA_BS(3);
  launch_coloured(c, kern, epb, bs, n_elem, coord, conn, D11, D12, D44, Kout, err, elem_mat, mat_tab, ec);
  if (Kout || !ec || ec->dup_off.empty()) return;
  // collapsed elements: element matrices (dup_k, by position), then added colour by colour
  const DevCSR &A = c->A;
  const int32_t nd = ec->dup_off.back();
  hipLaunchKernelGGL(kern, dim3((nd + epb - 1) / epb), dim3(bs), 0, c->stream, nd, coord, conn, D11, D12, D44, A.indexL, A.itemL, A.indexU,
                     A.itemU, A.D, A.AL, A.AU, dup_k, err, elem_mat, mat_tab, (const int32_t *)ec->dup, 0, (const int32_t *)nullptr);
  for_colour_ranges(ec->dup_off, false, 64, [&](dim3 grid, int32_t p0, int32_t p1) {
    hipLaunchKernelGGL(k_add_elem_blocks, grid, dim3(64), 0, c->stream, p0, p1, (const int32_t *)ec->dup, (const double *)dup_k, conn,
                       (const int32_t *)ec->pos, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL, A.AU, err);
  });
}

// hecmw_mat_ass_bc (hecmw_mat_ass.f90:292-429) for n_bc prescribed dofs whose lists (node, dof, value) are on the device: column
// times value moved to B, row and column zeroed, unit diagonal, B = value.  d_flag (3*NP bytes) and d_bcv (3*NP doubles) are
// cleared and then hold the marks and values of the listed dofs; with n_bc == 0 that is all.
static int bc_eliminate(fx_context *c, int32_t n_bc, const int32_t *d_node, const int32_t *d_dof, const double *d_val, uint8_t *d_flag,
                        double *d_bcv) {
  DevCSR &A = c->A;
  HIP_TRY(hipMemsetAsync(d_flag, 0, (size_t)3 * A.NP, c->stream));
  HIP_TRY(hipMemsetAsync(d_bcv, 0, (size_t)3 * A.NP * 8, c->stream));
  if (n_bc < 1) return 0;
  hipLaunchKernelGGL(k_bc_mark, dim3((n_bc + 255) / 256), dim3(256), 0, c->stream, n_bc, d_node, d_dof, d_val, d_flag, d_bcv);
  const dim3 g((A.NP + 255) / 256);
  hipLaunchKernelGGL((k_bc_apply<1>), g, dim3(256), 0, c->stream, A.NP, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL, A.AU, A.B,
                     d_flag, d_bcv);
  hipLaunchKernelGGL((k_bc_apply<2>), g, dim3(256), 0, c->stream, A.NP, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL, A.AU, A.B,
                     d_flag, d_bcv);
  HIP_TRY(hipGetLastError());
  return 0;
}

// `load` (or zero) becomes B, then hecmw_mat_ass_bc (hecmw_mat_ass.f90:292) for the listed dofs: once per assembly, after the last
// element group.  The temporaries live in the caller's scratch until its synchronize.
static int load_and_bc(fx_context *c, DevScratch &tmp, const char *who, const double *load, int32_t n_bc, const int32_t *bc_node,
                       const int32_t *bc_dof, const double *bc_val) {
  DevCSR &A = c->A;
  double *d_bcv = nullptr, *d_val = nullptr;
  int32_t *d_node = nullptr, *d_dof = nullptr;
  uint8_t *d_flag = nullptr;
  if (load) HIP_TRY(hipMemcpyAsync(A.B, load, (size_t)3 * A.NP * 8, hipMemcpyHostToDevice, c->stream));
  else HIP_TRY(hipMemsetAsync(A.B, 0, (size_t)3 * A.NP * 8, c->stream));
  if (n_bc > 0) {
    if (tmp.alloc(&d_flag, (size_t)3 * A.NP) || tmp.alloc(&d_bcv, (size_t)3 * A.NP) || tmp.alloc(&d_node, (size_t)n_bc) ||
        tmp.alloc(&d_dof, (size_t)n_bc) || tmp.alloc(&d_val, (size_t)n_bc))
      return FX_ERROR_RUNTIME;
    for (int32_t k = 0; k < n_bc; k++)
      if (bc_node[k] < 1 || bc_node[k] > A.NP) return fx_fail(who, FX_ERROR_RUNTIME, "BC node id out of range");
    HIP_TRY(hipMemcpyAsync(d_node, bc_node, (size_t)n_bc * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_dof, bc_dof, (size_t)n_bc * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_val, bc_val, (size_t)n_bc * 8, hipMemcpyHostToDevice, c->stream));
    if (bc_eliminate(c, n_bc, d_node, d_dof, d_val, d_flag, d_bcv)) return FX_ERROR_RUNTIME;
  }
  return 0;
}

// One element's stiffness through the device kernel (tests): etype 361 with elemopt 1..3, or an STF_C3 type.
static int element_stiffness(fx_context *c, int32_t etype, int elemopt, const double *ecoord, double E, double nu, double *stiff) {
  HIP_TRY(hipSetDevice(c->device));
  const int nn = c3_nodes(etype), w = 3 * nn;
  DevScratch tmp;
  double *d_coord = nullptr, *d_k = nullptr;
  int32_t *d_conn = nullptr, *d_err = nullptr;
  if (tmp.alloc(&d_coord, (size_t)w) || tmp.alloc(&d_conn, (size_t)nn) || tmp.alloc(&d_k, (size_t)w * w) || tmp.alloc(&d_err, 1))
    return FX_ERROR_RUNTIME;
  const int32_t conn[20] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20};
  HIP_TRY(hipMemcpy(d_coord, ecoord, (size_t)w * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_conn, conn, (size_t)nn * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_err, 0, 4));
  double D11, D12, D44;
  elastic_constants(E, nu, D11, D12, D44);
  launch_assemble(c, etype, elemopt, 1, d_coord, d_conn, D11, D12, D44, d_k, d_err, nullptr, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(stiff, d_k, (size_t)w * w * 8, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int fx_element_stiffness_c3d8(fx_context *c, int elemopt, const double *ecoord, double E, double nu, double *stiff) {
  if (!c || !ecoord || !stiff) { g_fx_error = "fx_element_stiffness_c3d8: null argument"; return FX_ERROR_RUNTIME; }
  if (elemopt < 1 || elemopt > 3) { g_fx_error = "fx_element_stiffness_c3d8: elemopt must be 1, 2 or 3"; return FX_ERROR_UNSUPPORTED; }
  return element_stiffness(c, 361, elemopt, ecoord, E, nu, stiff);
}

extern "C" int fx_element_stiffness_c3(fx_context *c, int32_t etype, const double *ecoord, double E, double nu, double *stiff) {
  if (!c || !ecoord || !stiff) { g_fx_error = "fx_element_stiffness_c3: null argument"; return FX_ERROR_RUNTIME; }
  if (!c3_linear_type(etype)) { g_fx_error = "fx_element_stiffness_c3: etype must be 341, 342, 351, 352 or 362"; return FX_ERROR_UNSUPPORTED; }
  return element_stiffness(c, etype, 0, ecoord, E, nu, stiff);
}
