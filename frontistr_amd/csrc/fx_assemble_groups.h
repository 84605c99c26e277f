// A mesh of several solid element types: fx_assemble_groups, fx_update_groups_linear (included by fistr_hip.hip after
// fx_assemble_host.h and fx_update_linear.h).  fstr_StiffMatrix.f90:43-212 and fstr_Update.f90:73-264 loop over
// hecMESH%elem_type_item; a group here is one entry of that loop.  The element kernels are those of the single-type entry points.
//
// Scatter: every group keeps its own colouring (ElemColors, as the single-type calls) and the groups run one after another,
// colour after colour, on one stream: no two elements of a launch share a node, launches are ordered, so there are no atomics and
// the sums are bitwise reproducible.  The first-write flags (fx_assemble.h) must know the first contribution to a block in the
// launch order of ALL groups: build_first_write (fx_assemble_host.h) takes every group's map.  A block that no element of the
// first group touches is then stored by the first later group that does, and the matrix needs no clearing.
#pragma once

static uint64_t fnv_mix(uint64_t h, uint64_t v) { return (h ^ v) * 1099511628211ull; }

// Position maps of all groups and, where every group allows it, their first-write flags in the global launch order.
// d_conn[g]: group g's connectivity on the device.
static int ensure_group_maps(fx_context *c, int32_t n_group, const fx_elem_group *groups, const std::vector<const int32_t *> &d_conn) {
  AsmGroups &ag = c->asm_groups;
  uint64_t sig = 1469598103934665603ull;
  bool have_all = true;
  for (int32_t g = 0; g < n_group; g++) {
    const ElemColors &ec = ag.ec[g];
    if (groups[g].n_elem < 1) continue;
    sig = fnv_mix(fnv_mix(fnv_mix(sig, ec.key), (uint64_t)ec.etype), (uint64_t)ec.n_elem);
    have_all &= ec.pos != nullptr;
  }
  sig = fnv_mix(sig, (uint64_t)n_group) | 1;
  if (have_all && ag.flag_sig == sig) return 0;
  ag.flag_sig = 0;
  ag.first_write = false;
  std::vector<FirstWriteGroup> fw;
  for (int32_t g = 0; g < n_group; g++) {  // maps made for another set of groups may carry that set's flags: made again, without
    dev_free(ag.ec[g].pos);
    ag.ec[g].first_write = false;
    if (groups[g].n_elem < 1) continue;
    if (ensure_scatter_map(c, ag.ec[g], groups[g].n_elem, d_conn[g], groups[g].etype)) return FX_ERROR_RUNTIME;
    fw.push_back({&ag.ec[g], d_conn[g]});
  }
  // atomics (not coloured), collapsed hexahedra or no map (FX_ASM_MAP=0, no memory) in a group: no flags anywhere
  if (build_first_write(c, fw, &ag.first_write)) return FX_ERROR_RUNTIME;
  ag.flag_sig = sig;
  return 0;
}

static const char SOLID_TYPES_ASCENDING[] = "341, 342, 351, 352, 361, 362";  // the types served, as the heat and load entry points spell them
// What every entry point over element groups refuses before anything is uploaded, in two halves.  The first: unknown types
// (FX_ERROR_UNSUPPORTED; `served` is the entry point's own spelling of the list) and, where asked, the elemopt of 361.
static int check_group_types(const char *who, int32_t n_group, const fx_elem_group *groups, const char *served, bool linear_elemopt = false) {
  if (n_group < 1 || !groups) return fx_fail(who, FX_ERROR_RUNTIME, "n_group must be >= 1");
  for (int32_t g = 0; g < n_group; g++) {
    if (c3_nodes(groups[g].etype) == 0)
      return fx_fail(who, FX_ERROR_UNSUPPORTED, "group %d: element type %d not supported on the device (%s)", (int)g + 1,
                     (int)groups[g].etype, served);
    if (linear_elemopt && groups[g].etype == 361 && (groups[g].elemopt < 1 || groups[g].elemopt > 3))
      return fx_fail(who, FX_ERROR_UNSUPPORTED, "group %d: elemopt must be 1 (IC), 2 (B-bar) or 3 (FI)", (int)g + 1);
  }
  return 0;
}
// The second: per group the arguments, material ids, node ids and degenerate elements (FX_ERROR_RUNTIME), each named with its group
// and element (1-based).  collapsed_361: a 361 element may name a node twice (collapsed hexahedra are assembled).
static int check_group_elements(const char *who, int32_t n_node, int32_t n_group, const fx_elem_group *groups, int32_t n_mat, bool collapsed_361) {
  for (int32_t g = 0; g < n_group; g++) {
    const fx_elem_group &G = groups[g];
    if (G.n_elem < 0 || (G.n_elem > 0 && !G.conn)) return fx_fail(who, FX_ERROR_RUNTIME, "group %d: connectivity missing", (int)g + 1);
    if (n_mat > 1 && G.n_elem > 0 && !G.elem_mat) return fx_fail(who, FX_ERROR_RUNTIME, "group %d: several materials need elem_mat", (int)g + 1);
    const int nn = c3_nodes(G.etype);
    const bool may_repeat = collapsed_361 && G.etype == 361;
    const int32_t *conn = G.conn, *emat = G.elem_mat;
    int32_t bad_mat = INT32_MAX, bad_node = INT32_MAX, dup = INT32_MAX;  // lowest offending element (0-based) of each kind
    parallel_for(G.n_elem, [=, &bad_mat, &bad_node, &dup](int64_t a, int64_t b) {  // (what the loop reads, by value: it stays in registers)
      int32_t bm = INT32_MAX, bn = INT32_MAX, dp = INT32_MAX;
      for (int64_t e = a; e < b && bm == INT32_MAX && bn == INT32_MAX && dp == INT32_MAX; e++) {
        const int32_t *en = conn + (size_t)nn * e;
        if (emat && (emat[e] < 1 || emat[e] > n_mat)) bm = (int32_t)e;
        for (int x = 0; x < nn; x++)
          if (en[x] < 1 || en[x] > n_node) bn = (int32_t)e;
        if (bn == INT32_MAX && !may_repeat && names_a_node_twice(en, nn)) dp = (int32_t)e;
      }
      __atomic_fetch_min(&bad_mat, bm, __ATOMIC_RELAXED);
      __atomic_fetch_min(&bad_node, bn, __ATOMIC_RELAXED);
      __atomic_fetch_min(&dup, dp, __ATOMIC_RELAXED);
    });
    if (bad_mat != INT32_MAX) return fx_fail(who, FX_ERROR_RUNTIME, "group %d, element %d: material id out of range", (int)g + 1, (int)bad_mat + 1);
    if (bad_node != INT32_MAX) return fx_fail(who, FX_ERROR_RUNTIME, "group %d, element %d: node id out of range", (int)g + 1, (int)bad_node + 1);
    if (dup != INT32_MAX)
      return fx_fail(who, FX_ERROR_RUNTIME, "group %d (TYPE=%d), element %d names a node twice (a degenerate element)", (int)g + 1,
                         (int)G.etype, (int)dup + 1);
  }
  return 0;
}
// The linear entry points, fx_dload_groups and the nonlinear set-up (nl_init_driver, which names what it serves of 361 itself).
static int check_groups(const char *who, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                        int32_t n_mat, bool have_mats, bool nonlinear = false) {
  if (int rc = check_group_types(who, n_group, groups, "361, 341, 342, 351, 352, 362", !nonlinear)) return rc;
  if (n_node < 1 || !coord) return fx_fail(who, FX_ERROR_RUNTIME, "empty mesh");
  if (n_mat < 1 || !have_mats) return fx_fail(who, FX_ERROR_RUNTIME, "materials missing");
  return check_group_elements(who, n_node, n_group, groups, n_mat, true);
}
// Entry k (0-based) of the list `name` (dflux, film, radiate, dload) names a group and an element of it.
static int check_list_entry(const char *who, const char *name, int32_t k, int32_t group, int32_t elem, int32_t n_group,
                            const fx_elem_group *groups) {
  if (group < 0 || group >= n_group) return fx_fail(who, FX_ERROR_RUNTIME, "%s, entry %d: group out of range", name, (int)k + 1);
  if (elem < 0 || elem >= groups[group].n_elem)
    return fx_fail(who, FX_ERROR_RUNTIME, "%s, entry %d: element %d is not in group %d", name, (int)k + 1, (int)elem, (int)group + 1);
  return 0;
}

// Every group's connectivity and material ids on the device (null: an empty group, no elem_mat), on the context's stream.
static int upload_group_conn(fx_context *c, DevScratch &tmp, int32_t n_group, const fx_elem_group *groups, std::vector<const int32_t *> &conn,
                             std::vector<const int32_t *> &emat) {
  conn.assign((size_t)n_group, nullptr);
  emat.assign((size_t)n_group, nullptr);
  for (int32_t g = 0; g < n_group; g++) {
    const fx_elem_group &G = groups[g];
    if (G.n_elem < 1) continue;
    const size_t nw = (size_t)c3_nodes(G.etype) * G.n_elem;
    int32_t *d_conn = nullptr, *d_emat = nullptr;
    if (tmp.alloc(&d_conn, nw)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpyAsync(d_conn, G.conn, nw * 4, hipMemcpyHostToDevice, c->stream));
    conn[g] = d_conn;
    if (G.elem_mat) {
      if (tmp.alloc(&d_emat, (size_t)G.n_elem)) return FX_ERROR_RUNTIME;
      HIP_TRY(hipMemcpyAsync(d_emat, G.elem_mat, (size_t)G.n_elem * 4, hipMemcpyHostToDevice, c->stream));
      emat[g] = d_emat;
    }
  }
  return 0;
}

// The (D11, D12, D44) table of the materials on the device, every group's connectivity and material ids.
struct GroupUploads {
  std::vector<const int32_t *> conn, emat;
  const double *mtab = nullptr;            // null when no group has elem_mat
  double D11 = 0.0, D12 = 0.0, D44 = 0.0;  // material 1: what a group without elem_mat takes
  std::vector<double> tab;                 // host copy of mtab: lives until the caller's synchronize
};
static int upload_groups(fx_context *c, DevScratch &tmp, int32_t n_group, const fx_elem_group *groups, int32_t n_mat, const double *E,
                         const double *nu, GroupUploads &up) {
  up.tab.resize((size_t)3 * n_mat);
  for (int32_t k = 0; k < n_mat; k++) elastic_constants(E[k], nu[k], up.tab[3 * k], up.tab[3 * k + 1], up.tab[3 * k + 2]);
  up.D11 = up.tab[0]; up.D12 = up.tab[1]; up.D44 = up.tab[2];
  bool by_element = false;  // some group selects its materials per element: the table goes to the device
  for (int32_t g = 0; g < n_group; g++) by_element |= groups[g].n_elem > 0 && groups[g].elem_mat;
  if (by_element) {
    double *d_mtab = nullptr;
    if (tmp.alloc(&d_mtab, up.tab.size())) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpyAsync(d_mtab, up.tab.data(), up.tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    up.mtab = d_mtab;
  }
  return upload_group_conn(c, tmp, n_group, groups, up.conn, up.emat);
}

// The assembly of every linear entry point; `who` is the entry point called.  All groups into the resident matrix, group after
// group, colour after colour; first-write (no clearing) where every group is coloured, mapped, free of collapsed elements and
// the groups cover the profile, otherwise the matrix is cleared once.
static int assemble_groups_driver(const char *who, fx_context *c, int32_t n_node, const double *coord, int32_t n_group,
                                  const fx_elem_group *groups, int32_t n_mat, const double *E, const double *nu, const double *load,
                                  int32_t n_bc, const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val, float *ms_assemble) {
  PhaseTimer pt("assemble");
  if (int rc = check_groups(who, n_node, coord, n_group, groups, n_mat, E && nu)) return rc;
  pt.lap("check_groups");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->have_profile) return fx_fail(who, FX_ERROR_RUNTIME, "upload the profile first (fx_upload FX_UP_PROFILE)");
  if (n_node != c->A.NP) return fx_fail(who, FX_ERROR_RUNTIME, "mesh/profile size mismatch");
  AsmGroups &ag = c->asm_groups;
  DevScratch tmp;
  GroupUploads up;
  double *d_coord = nullptr;
  int32_t *d_err = nullptr;
  if (tmp.alloc(&d_coord, (size_t)3 * n_node) || tmp.alloc(&d_err, 1)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(d_coord, coord, (size_t)3 * n_node * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(d_err, 0, 4, c->stream));
  if (int rc = upload_groups(c, tmp, n_group, groups, n_mat, E, nu, up)) return rc;
  // one cache entry per group, by position: a group whose connectivity and type are those of the last call keeps its colours
  for (size_t g = (size_t)n_group; g < ag.ec.size(); g++) elem_colors_free(ag.ec[g]);
  if (ag.ec.size() != (size_t)n_group) { ag.ec.resize((size_t)n_group); ag.flag_sig = 0; }
  for (int32_t g = 0; g < n_group; g++) {
    const fx_elem_group &G = groups[g];
    if (G.n_elem < 1) { elem_colors_free(ag.ec[g]); continue; }
    if (ensure_elem_colors(c, ag.ec[g], G.n_elem, G.conn, n_node, c3_nodes(G.etype), G.etype)) return FX_ERROR_RUNTIME;
  }
  if (ensure_group_maps(c, n_group, groups, up.conn)) return FX_ERROR_RUNTIME;
  std::vector<double *> d_dupk((size_t)n_group, nullptr);  // element matrices of the collapsed hexahedra
  for (int32_t g = 0; g < n_group; g++)
    if (!ag.ec[g].dup_off.empty() && tmp.alloc(&d_dupk[g], (size_t)576 * ag.ec[g].dup_off.back())) return FX_ERROR_RUNTIME;
  pt.lap("uploads, colours, maps");
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  if (!ag.first_write && mat_clear(c)) return FX_ERROR_RUNTIME;  // once
  for (int32_t g = 0; g < n_group; g++) {
    const fx_elem_group &G = groups[g];
    if (G.n_elem < 1) continue;
    launch_assemble(c, G.etype, G.elemopt, G.n_elem, d_coord, up.conn[g], up.D11, up.D12, up.D44, nullptr, d_err, up.emat[g],
                    up.emat[g] ? up.mtab : nullptr, &ag.ec[g], d_dupk[g]);
  }
  HIP_TRY(hipGetLastError());
  if (int rc = load_and_bc(c, tmp, who, load, n_bc, bc_node, bc_dof, bc_val)) return rc;
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  int32_t herr = 0;  // the streaming (BELL) layouts re-gather these values on next use (ensure_solver)
  HIP_TRY(hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  pt.lap("kernels");
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  if (ms_assemble) *ms_assemble = ms;
  if (int rc = assembly_error(herr)) return rc;
  c->have_values = true;
  c->bell_valid = false;  // the preconditioner is refreshed by the flags / recycle policy of the next solve, not here
  return 0;
}

extern "C" int fx_assemble_groups(fx_context *c, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                                  int32_t n_mat, const double *E, const double *nu, const double *load, int32_t n_bc,
                                  const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val, float *ms_assemble) {
  if (!c) return fx_fail("fx_assemble_groups", FX_ERROR_RUNTIME, "null argument");
  return assemble_groups_driver("fx_assemble_groups", c, n_node, coord, n_group, groups, n_mat, E, nu, load, n_bc, bc_node, bc_dof,
                                bc_val, ms_assemble);
}

// The single-type entry points: one group.
extern "C" int fx_assemble_c3d8(fx_context *c, const fx_mesh_view *mesh, double E, double nu, int elemopt, const double *load,
                                int32_t n_bc, const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val,
                                float *ms_assemble) {
  if (!c || !mesh) return fx_fail("fx_assemble_c3d8", FX_ERROR_RUNTIME, "null argument");
  const fx_elem_group G = {361, elemopt, mesh->n_elem, mesh->conn, nullptr};
  return assemble_groups_driver("fx_assemble_c3d8", c, mesh->n_node, mesh->coord, 1, &G, 1, &E, &nu, load, n_bc, bc_node, bc_dof, bc_val,
                                ms_assemble);
}

extern "C" int fx_assemble_c3d8_sections(fx_context *c, const fx_mesh_view *mesh, int32_t n_mat, const double *E, const double *nu,
                                         const int32_t *elem_mat, int elemopt, const double *load, int32_t n_bc,
                                         const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val,
                                         float *ms_assemble) {
  const char *who = "fx_assemble_c3d8_sections";
  if (!c || !mesh) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  if (!elem_mat) return fx_fail(who, FX_ERROR_RUNTIME, "materials missing");
  const fx_elem_group G = {361, elemopt, mesh->n_elem, mesh->conn, elem_mat};
  return assemble_groups_driver(who, c, mesh->n_node, mesh->coord, 1, &G, n_mat, E, nu, load, n_bc, bc_node, bc_dof, bc_val, ms_assemble);
}

// tetrahedra, wedges, 20-node hexahedra (TYPE=341, 342, 351, 352, 362)
extern "C" int fx_assemble_c3(fx_context *c, const fx_mesh_view *mesh, int32_t etype, int32_t n_mat, const double *E,
                              const double *nu, const int32_t *elem_mat, const double *load, int32_t n_bc, const int32_t *bc_node,
                              const int32_t *bc_dof, const double *bc_val, float *ms_assemble) {
  const char *who = "fx_assemble_c3";
  if (!c || !mesh) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  if (!c3_linear_type(etype)) return fx_fail(who, FX_ERROR_UNSUPPORTED, FX_C3_UNSUPPORTED "fx_assemble_c3d8)");
  const fx_elem_group G = {etype, 0, mesh->n_elem, mesh->conn, elem_mat};
  return assemble_groups_driver(who, c, mesh->n_node, mesh->coord, 1, &G, n_mat, E, nu, load, n_bc, bc_node, bc_dof, bc_val, ms_assemble);
}

// ---- stress update and thermal load -----------------------------------------------------------------------------------------
static void upd_stage_wait(UpdStage &st) {
  if (st.maker.joinable()) st.maker.join();
}
static int upd_stage_make(UpdStage *st, int device, size_t doubles) {  // (re)allocates both arrays; on the calling thread
  if (hipSetDevice(device) != hipSuccess) return 1;
  if (st->strain) (void)hipHostFree(st->strain);
  if (st->stress) (void)hipHostFree(st->stress);
  st->strain = st->stress = nullptr;
  st->cap = 0;
  if (hipHostMalloc((void **)&st->strain, doubles * 8, hipHostMallocDefault) != hipSuccess) return 1;
  if (hipHostMalloc((void **)&st->stress, doubles * 8, hipHostMallocDefault) != hipSuccess) return 1;
  st->cap = doubles;
  return 0;
}
// fx_destroy: joins the helper thread, frees the pinned arrays
static void upd_stage_free(fx_context *c) {
  UpdStage &st = c->upd_stage;
  upd_stage_wait(st);
  if (st.strain) (void)hipHostFree(st.strain);
  if (st.stress) (void)hipHostFree(st.stress);
  st.strain = st.stress = nullptr;
  st.cap = 0;
}
// Optional: start pinning the staging of an update with `doubles` of strain (and of stress) on a helper thread and return at
// once (a caller that knows a stress update will follow the solve -- the fistr1 binding after fstr_StiffMatrix -- hides the 0.3 s).
static int upd_stage_prepare(fx_context *c, size_t doubles) {
  UpdStage *st = &c->upd_stage;
  upd_stage_wait(*st);
  if (doubles == 0 || st->cap >= doubles) return 0;
  const int device = c->device;
  st->make_err = 0;
  st->maker = std::thread([st, device, doubles] { st->make_err = upd_stage_make(st, device, doubles); });
  return 0;
}
static size_t groups_stage_doubles(int32_t n_group, const fx_elem_group *groups) {
  size_t tot = 0;
  for (int32_t g = 0; g < n_group; g++) tot += (size_t)6 * c3_points(groups[g].etype) * (size_t)std::max(groups[g].n_elem, 0);
  return tot;
}

extern "C" int fx_update_c3d8_linear_prepare(fx_context *c, int32_t n_elem) {
  if (!c || n_elem < 1) return fx_fail("fx_update_c3d8_linear_prepare", FX_ERROR_RUNTIME, "bad argument");
  return upd_stage_prepare(c, (size_t)48 * n_elem);
}
extern "C" int fx_update_groups_linear_prepare(fx_context *c, int32_t n_group, const fx_elem_group *groups) {
  if (!c || n_group < 1 || !groups) return fx_fail("fx_update_groups_linear_prepare", FX_ERROR_RUNTIME, "bad argument");
  return upd_stage_prepare(c, groups_stage_doubles(n_group, groups));
}

// fstr_UpdateNewton of a linear static analysis over element groups (see the header of fx_update_linear.h), and the thermal load
// of fstr_ass_load.f90:287-428, which is the update kernels with TH = 2.  coord, disp, E, nu: host.
//   TH = 0 / 1 (without / with `thermal`): strain[g], stress[g] = group g's [n_elem][nq][6] in the context's pinned staging
//     (valid until the next update or prepare on this context, or fx_destroy); q = qforce (3 * n_node, caller's, may be NULL).
//   TH = 2: q = the caller's load vector, to which every element's TLOAD vector is added -- only when everything succeeded; no
//     displacement, no staging.  Elements that share a node add with fp64 atomics: reproducible to rounding, not bit for bit.
// 361 (elemopt 1..3, 8 points) runs k_update_c3d8_linear, 341 / 342 (1 / 4 points) k_update_tet, 351 / 352 / 362 (2 / 9 / 27
// points) k_update_c3, group after group on one stream.
template <int TH>
static int update_groups_driver(const char *who, fx_context *c, int32_t n_node, const double *coord, int32_t n_group,
                                const fx_elem_group *groups, int32_t n_mat, const double *E, const double *nu,
                                const fx_thermal_view *thermal, const double *disp, const double **strain, const double **stress,
                                double *q, float *ms_kernel) {
  if (int rc = check_groups(who, n_node, coord, n_group, groups, n_mat, E && nu)) return rc;
  if (TH)
    if (int rc = thermal_view_ok(who, thermal)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t total = groups_stage_doubles(n_group, groups), nq3 = (size_t)3 * n_node;
  if (total == 0 && TH < 2) return fx_fail(who, FX_ERROR_RUNTIME, "empty mesh");
  PhaseTimer pt("update linear");
  UpdStage &st = c->upd_stage;
  DevScratch tmp;
  GroupUploads up;
  ThermalDev td{nullptr, nullptr, nullptr, 0.0};
  double *d_coord = nullptr, *d_disp = nullptr, *d_q = nullptr, *d_strain = nullptr, *d_stress = nullptr;
  int32_t *d_err = nullptr;
  if (tmp.alloc(&d_coord, nq3) || tmp.alloc(&d_q, nq3) || tmp.alloc(&d_err, 1)) return FX_ERROR_RUNTIME;
  if (TH < 2 && (tmp.alloc(&d_disp, nq3) || tmp.alloc(&d_strain, total) || tmp.alloc(&d_stress, total))) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(d_coord, coord, nq3 * 8, hipMemcpyHostToDevice, c->stream));
  if (TH < 2) {
    HIP_TRY(hipMemcpyAsync(d_disp, disp, nq3 * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_q, 0, nq3 * 8, c->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(d_q, q, nq3 * 8, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(hipMemsetAsync(d_err, 0, 4, c->stream));
  if (int rc = upload_groups(c, tmp, n_group, groups, n_mat, E, nu, up)) return rc;
  if (TH && upload_thermal(c, tmp, n_node, n_mat, thermal, td)) return FX_ERROR_RUNTIME;
  if (pt.on) HIP_TRY(hipStreamSynchronize(c->stream));
  pt.lap("device buffers + uploads");
  if (TH < 2) {
    upd_stage_wait(st);
    if (st.make_err || st.cap < total) {
      st.make_err = 0;
      if (upd_stage_make(&st, c->device, total)) { (void)hipGetLastError(); return fx_fail(who, FX_ERROR_RUNTIME, "cannot pin the host staging"); }
    }
    pt.lap("pinned staging");
  }
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  size_t at = 0;  // group g's results start at `at` doubles, in the device arrays and in the staging
  for (int32_t g = 0; g < n_group; g++) {
    const fx_elem_group &G = groups[g];
    if (G.n_elem < 1) continue;
    launch_update_linear_th<TH>(c, G.etype, G.elemopt, G.n_elem, d_coord, up.conn[g], up.D11, up.D12, up.D44, up.emat[g],
                                up.emat[g] ? up.mtab : nullptr, d_disp, TH < 2 ? d_strain + at : nullptr,
                                TH < 2 ? d_stress + at : nullptr, d_q, d_err, td);
    at += (size_t)6 * c3_points(G.etype) * G.n_elem;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  int32_t herr = 0;
  std::vector<double> out(TH == 2 ? nq3 : 0);  // the caller's load vector changes only when everything went well
  if (TH < 2) {
    HIP_TRY(hipMemcpyAsync(st.strain, d_strain, total * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(st.stress, d_stress, total * 8, hipMemcpyDeviceToHost, c->stream));
    if (q) HIP_TRY(hipMemcpyAsync(q, d_q, nq3 * 8, hipMemcpyDeviceToHost, c->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(out.data(), d_q, nq3 * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  pt.lap("kernel + downloads");
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  if (ms_kernel) *ms_kernel = ms;
  if (herr)
    return fx_fail(who, FX_ERROR_RUNTIME, "PIVOT ERROR in the incompatible-mode block of an element (%s, calInverse)",
                   TH == 2 ? "TLOAD_C3D8IC" : "UpdateST_C3D8IC");
  if (TH == 2) memcpy(q, out.data(), nq3 * 8);
  at = 0;
  for (int32_t g = 0; g < n_group && TH < 2; g++) {
    if (strain) strain[g] = st.strain + at;
    if (stress) stress[g] = st.stress + at;
    at += (size_t)6 * c3_points(groups[g].etype) * (size_t)groups[g].n_elem;
  }
  return 0;
}

extern "C" int fx_update_groups_linear(fx_context *c, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                                       int32_t n_mat, const double *E, const double *nu, const double *disp, const double **strain,
                                       const double **stress, double *qforce, float *ms_kernel) {
  const char *who = "fx_update_groups_linear";
  if (!c || !disp) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  return update_groups_driver<0>(who, c, n_node, coord, n_group, groups, n_mat, E, nu, nullptr, disp, strain, stress, qforce, ms_kernel);
}

// the same with the routines' thermal branches (fx_thermal.h)
extern "C" int fx_update_groups_linear_thermal(fx_context *c, int32_t n_node, const double *coord, int32_t n_group,
                                               const fx_elem_group *groups, int32_t n_mat, const double *E, const double *nu,
                                               const fx_thermal_view *thermal, const double *disp, const double **strain,
                                               const double **stress, double *qforce, float *ms_kernel) {
  const char *who = "fx_update_groups_linear_thermal";
  if (!c || !disp) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  return update_groups_driver<1>(who, c, n_node, coord, n_group, groups, n_mat, E, nu, thermal, disp, strain, stress, qforce, ms_kernel);
}

extern "C" int fx_thermal_load_groups(fx_context *c, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                                      int32_t n_mat, const double *E, const double *nu, const fx_thermal_view *thermal,
                                      double *load_inout, float *ms_kernel) {
  const char *who = "fx_thermal_load_groups";
  if (!c || !load_inout) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  return update_groups_driver<2>(who, c, n_node, coord, n_group, groups, n_mat, E, nu, thermal, nullptr, nullptr, nullptr, load_inout,
                                 ms_kernel);
}

// The single-type entry points: one group.
extern "C" int fx_update_c3d8_linear(fx_context *c, const fx_mesh_view *mesh, int32_t n_mat, const double *E, const double *nu,
                                     const int32_t *elem_mat, int elemopt, const double *disp, const double **strain,
                                     const double **stress, double *qforce, float *ms_kernel) {
  const char *who = "fx_update_c3d8_linear";
  if (!c || !mesh || !disp) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  const fx_elem_group G = {361, elemopt, mesh->n_elem, mesh->conn, elem_mat};
  return update_groups_driver<0>(who, c, mesh->n_node, mesh->coord, 1, &G, n_mat, E, nu, nullptr, disp, strain, stress, qforce, ms_kernel);
}

extern "C" int fx_update_c3_linear(fx_context *c, const fx_mesh_view *mesh, int32_t etype, int32_t n_mat, const double *E,
                                   const double *nu, const int32_t *elem_mat, const double *disp, const double **strain,
                                   const double **stress, double *qforce, float *ms_kernel) {
  const char *who = "fx_update_c3_linear";
  if (!c || !mesh || !disp) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  if (!c3_linear_type(etype)) return fx_fail(who, FX_ERROR_UNSUPPORTED, FX_C3_UNSUPPORTED "fx_update_c3d8_linear)");
  const fx_elem_group G = {etype, 0, mesh->n_elem, mesh->conn, elem_mat};
  return update_groups_driver<0>(who, c, mesh->n_node, mesh->coord, 1, &G, n_mat, E, nu, nullptr, disp, strain, stress, qforce, ms_kernel);
}
