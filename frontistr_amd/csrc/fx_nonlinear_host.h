// Host entry points of the nonlinear path (included at the end of fistr_hip.hip): the steps of
// fstr_Newton (fstr_solve_NonLinear.f90:29-167) either side of the linear solve, on resident state.
#pragma once

static void nl_thermal_free(NlDev::Thermal &t) {
  dev_free(t.temp); dev_free(t.last_temp); dev_free(t.temp_init); dev_free(t.last_temp_bk);
  dev_free(t.alpha); dev_free(t.tabs); dev_free(t.tab_idx); dev_free(t.mtab); dev_free(t.xc);
  t = NlDev::Thermal();
}
// The kernels' view of the context's thermal data (all null while thermal is off: the TH = 0 instantiations do not read it)
static ThermalDev nl_thermal_dev(const NlDev &n) {
  const NlDev::Thermal &t = n.th;
  ThermalDev d{t.temp, t.last_temp, t.alpha, t.ref_temp};
  d.tabs = t.tabs;
  d.tab_idx = t.any_tab ? t.tab_idx : nullptr;
  d.temp_init = t.temp_init;
  return d;
}

static void nl_free(fx_context *c) {
  NlDev &n = c->nl;
  dev_free(n.tab); dev_free(n.coord);
  for (NlPart &p : n.parts) {
    dev_free(p.conn); dev_free(p.emat);
    elem_colors_free(p.colors);
  }
  for (NlPartState *s : {&n.st, &n.bk})
    for_each_point_array([](size_t, auto *&a) { dev_free(a); return 0; }, *s);
  dev_free(n.unode); dev_free(n.dunode); dev_free(n.qforce); dev_free(n.GL);
  dev_free(n.bc_flag); dev_free(n.bc_val); dev_free(n.bc_node); dev_free(n.bc_dof); dev_free(n.bc_v); dev_free(n.err);
  dev_free(n.mats); dev_free(n.hist); dev_free(n.hist_bk);
  for (double *t : n.tabs) { double *q = t; dev_free(q); }
  nl_thermal_free(n.th);
  nl_dload_free(n);
  nodal_list_free(c->nodal_list_nl);  // fx_nodal_stress.h: the list of fx_nl_nodal_stress belongs to this connectivity
  n = NlDev();
}

// What the device loop serves of one material; everything else is refused by name
static int nl_check_material(const char *who, const fx_material_view *mat) {
  if (mat->plastic == FX_MAT_MOONEY || mat->plastic == FX_MAT_ARRUDA) {  // E, nu, harden, tab are not read
    if (mat->nlgeom != 1)
      return fx_fail(who, FX_ERROR_UNSUPPORTED,
                     "a hyperelastic material needs nlgeom = 1 (TOTALLAG): under UPDATELAG (CAUCHY) the reference multiplies the "
                     "hyperelastic tangent with the strain increment, a different algorithm that is not on the device");
    if (mat->plconst[2] == 0.0)
      return fx_fail(who, FX_ERROR_UNSUPPORTED, "hyperelastic material with plconst[2] = 0: cannot deal with incompressible material");
    if (mat->plastic == FX_MAT_ARRUDA && mat->plconst[1] == 0.0)
      return fx_fail(who, FX_ERROR_UNSUPPORTED, "Arruda-Boyce material with plconst[1] = 0 (locking stretch lambda_m)");
    return 0;
  }
  if (mat->plastic == FX_MAT_VISCO) {  // harden, plconst are not read; tab / ntab: the Prony rows (g, tau)
    if (mat->nlgeom != 0 && mat->nlgeom != 1)
      return fx_fail(who, FX_ERROR_UNSUPPORTED,
                     "a viscoelastic material has nlgeom 0 (INFINITE) or 1 (TOTALLAG): the card reaches no other flag "
                     "(fstr_ctrl_material.f90:277-279), and UPDATELAG is not on the device");
    if (mat->ntab < 1 || !mat->tab) return fx_fail(who, FX_ERROR_RUNTIME, "a viscoelastic material needs at least one Prony row (g, tau)");
    for (int32_t r = 0; r < mat->ntab; r++)
      if (mat->tab[2 * r + 1] == 0.0)
        return fx_fail(who, FX_ERROR_UNSUPPORTED, "viscoelastic material: Prony row %d has tau = 0 (dt / tau is formed for every row)", (int)r + 1);
    return 0;
  }
  if (mat->plastic == FX_MAT_NORTON) {  // harden, tab are not read; plconst = A, n, m
    // TOTALLAG (KIRCHHOFF): the update routines hand StressUpdate the point's STORED stress and never D . strain
    // (static_LIB_3d.f90:685-692), so a point that starts a VISCO step at zero stress divides 0 by 0 in update_iso_creep's loop,
    // which has no exit then; INFINITE is not reachable from the card and has no NORTON branch at all
    if (!(mat->plconst[2] > -1.0))
      return fx_fail(who, FX_ERROR_UNSUPPORTED, "NORTON material with m = %g: the law divides by m + 1 and takes time**(m + 1) (creep.f90:66), m must be above -1",
                     mat->plconst[2]);
    if (mat->nlgeom != 2)
      return fx_fail(who, FX_ERROR_UNSUPPORTED,
                     "a NORTON material needs nlgeom = 2 (UPDATELAG, the default of !CREEP): under TOTALLAG the reference relaxes the "
                     "stored stress instead of the trial one, which defines no usable result, and INFINITE has no creep branch");
    return 0;
  }
  if (mat->plastic < 0 || mat->plastic > FX_MAT_DRUCKER)
    return fx_fail(who, FX_ERROR_UNSUPPORTED,
                   "material kind %d: 0 ELASTIC, 1 Mises, 2 Neo-Hooke / Mooney-Rivlin, 3 Arruda-Boyce, 4 Mohr-Coulomb, 5 Drucker-Prager, "
                   "7 viscoelastic, 8 NORTON", (int)mat->plastic);
  if (mat->plastic == FX_MAT_MOHR || mat->plastic == FX_MAT_DRUCKER) {  // fstr_ctrl_material.f90:451-469: linear hardening, no table
    if (mat->harden != 0 || mat->nlgeom < 0 || mat->nlgeom > 2)
      return fx_fail(who, FX_ERROR_UNSUPPORTED,
                     "a Mohr-Coulomb / Drucker-Prager material has harden = 0 (the card forces linear hardening) and nlgeom 0, 1 or 2");
    // the constants at which BackwardEuler would stop with `Math error in return mapping` (Elastoplastic.f90:496, :541)
    if (mat->plastic == FX_MAT_MOHR && cos(mat->plconst[2]) == 0.0)
      return fx_fail(who, FX_ERROR_UNSUPPORTED, "Mohr-Coulomb material with cos(phi) = 0 (plconst[2] is the friction angle in radians)");
    if (mat->plastic == FX_MAT_DRUCKER && mat->plconst4 == 0.0)
      return fx_fail(who, FX_ERROR_UNSUPPORTED, "Drucker-Prager material with xi = 0 (plconst4)");
    return 0;
  }
  if (mat->harden < 0 || mat->harden > 3 || mat->nlgeom < 0 || mat->nlgeom > 2)
    return fx_fail(who, FX_ERROR_UNSUPPORTED, "only Mises yield with BILINEAR/MULTILINEAR/SWIFT/RAMBERG-OSGOOD hardening is on the hot path");
  if (mat->plastic && mat->harden == 1 && (mat->ntab < 1 || !mat->tab)) return fx_fail(who, FX_ERROR_RUNTIME, "MULTILINEAR hardening needs a table");
  return 0;
}

// nl_check_material for every material, and the refusal of an elastoplastic beside a hyperelastic one, over the whole context
static int nl_check_materials(const char *who, int32_t n_mat, const fx_material_view *mats) {
  for (int32_t k = 0; k < n_mat; k++)
    if (int e = nl_check_material(who, &mats[k])) return e;
  // MatlMatrix's saved flag (calMatMatrix.f90:39-62): after the first plastic update EVERY material goes to calElasticMatrix, which
  // for a hyperelastic one reads a Young's modulus and a Poisson's ratio that were never set
  bool mises = false, hyper = false, yield = false, creep = false;
  for (int32_t k = 0; k < n_mat; k++) {
    creep |= mats[k].plastic == FX_MAT_NORTON;
    mises |= mats[k].plastic == 1;
    hyper |= mats[k].plastic == FX_MAT_MOONEY || mats[k].plastic == FX_MAT_ARRUDA;
    yield |= mats[k].plastic == FX_MAT_MOHR || mats[k].plastic == FX_MAT_DRUCKER;
  }
  if (mises && hyper)
    return fx_fail(who, FX_ERROR_UNSUPPORTED,
                   "a Mises and a hyperelastic material in one context: after the first plastic update the reference takes the elastic "
                   "matrix of every material, which a hyperelastic one does not define");
  if (creep && hyper)
    return fx_fail(who, FX_ERROR_UNSUPPORTED,
                   "a NORTON and a hyperelastic material in one context: the first stress update of a NORTON element sets MatlMatrix's "
                   "saved flag (static_LIB_3d.f90:595), after which the reference takes the elastic matrix of every material, which a "
                   "hyperelastic one does not define");
  if (yield && hyper)
    return fx_fail(who, FX_ERROR_UNSUPPORTED,
                   "a Mohr-Coulomb / Drucker-Prager and a hyperelastic material in one context: after the first plastic update the "
                   "reference takes the elastic matrix of every material, which a hyperelastic one does not define");
  return 0;
}

// One element group as the caller holds it (checked): what a part is made from
struct NlPartIn {
  int32_t etype, n_elem;
  const int32_t *conn, *elem_mat;  // elem_mat: null with one material
  bool fbar = false;               // 361: F-bar (elemopt 4), not B-bar
};

// The factors of a viscoelastic material that depend on it and the time increment alone, as calViscoelasticMatrix (:143-161) and
// UpdateViscoelastic (:249-265) form them per point: rows (exp_n, dq_n) into `rows`, mu_0 -> pl[0], gfac -> pl[1], dt -> pl[2]
static void nl_visco_factors(const std::vector<double> &prony, double dt, NlMat &m, std::vector<double> &rows) {
  const size_t nrow = prony.size() / 2;
  rows.assign(2 * nrow, 0.0);
  double mu_0 = 0.0, gfac = 0.0;
  for (size_t r = 0; r < nrow; r++) {
    const double mu_n = prony[2 * r], dtau = dt / prony[2 * r + 1], exp_n = exp(-dtau);
    const double dq_n = mu_n * visco_hvisc(dtau, exp_n);
    gfac = gfac + dq_n;
    mu_0 = mu_0 + mu_n;
    rows[2 * r] = exp_n;
    rows[2 * r + 1] = dq_n;
  }
  mu_0 = 1.0 - mu_0;
  gfac = gfac + mu_0;
  m.pl[0] = mu_0; m.pl[1] = gfac; m.pl[2] = dt;
}
// The time of the coming sub-step into the context and the materials the kernels take (`who`: the entry point called).  A NORTON
// material forms ttime**(m + 1): a negative time or increment is refused before anything changes, with the reason, instead of
// travelling to every point as a NaN that the creep iteration's error word would report afterwards.
static int nl_apply_time(fx_context *c, const char *who, double time, double tincr) {
  NlDev &n = c->nl;
  if (n.has_creep && !(time >= 0.0 && tincr >= 0.0))
    return fx_fail(who, FX_ERROR_RUNTIME, "time %g, tincr %g: a NORTON material takes powers of the time (creep.f90:66), both must be >= 0 and finite",
                   time, tincr);
  n.time = time; n.tincr = tincr;
  if (n.hist_w == 0) return 0;
  std::vector<std::vector<double>> tables((size_t)n.n_mat);  // alive until the one synchronisation below
  bool copied = false;
  for (int32_t k = 0; k < n.n_mat; k++) {
    if (n.prony[k].empty()) continue;
    std::vector<double> &rows = tables[k];
    if (nl_group_creep(n.h_mats[k].group)) {  // creep.f90:66, :165
      const double A = n.prony[k][0], xm = n.prony[k][2];
      n.h_mats[k].pl[0] = A * (pow(time + tincr, xm + 1.0) - pow(time, xm + 1.0)) / (xm + 1.0);
      n.h_mats[k].pl[1] = n.prony[k][1];
      n.h_mats[k].pl[2] = tincr;
      continue;
    }
    nl_visco_factors(n.prony[k], tincr, n.h_mats[k], rows);
    HIP_TRY(hipMemcpyAsync(n.tabs[k], rows.data(), rows.size() * 8, hipMemcpyHostToDevice, c->stream));
    copied = true;
  }
  n.mat = n.h_mats[0];
  if (n.mats) HIP_TRY(hipMemcpyAsync(n.mats, n.h_mats.data(), (size_t)n.n_mat * sizeof(NlMat), hipMemcpyHostToDevice, c->stream));
  if (copied || n.mats) HIP_TRY(hipStreamSynchronize(c->stream));  // with one NORTON material everything travels by value
  return 0;
}

static int nl_alloc_point_arrays(NlPartState &s, size_t npt) {
  return for_each_point_array([&](size_t b, auto *&a) { return dev_alloc(&a, npt * b / sizeof(*a)); }, s);
}

// Element lists of one part: grouped by the NLGEOM flag of the element's material, hyperelastic ones apart (one kernel instantiation
// per group), inside a group colour by colour (fx_order.cpp: color_elements) for the atomic-free scatter
static int nl_part_lists(fx_context *c, NlPart &p, const NlPartIn &in, int32_t n_node) {
  const NlDev &n = c->nl;
  const int nn = p.nn;
  static const bool force_atomic = getenv("FX_ASM_ATOMIC") && atoi(getenv("FX_ASM_ATOMIC")) != 0;
  std::vector<int32_t> order, off;
  const bool coloured = !force_atomic && fxo::color_elements(in.n_elem, nn, in.conn, n_node, order, off);
  if (!coloured) {
    order.resize((size_t)in.n_elem);
    for (int32_t e = 0; e < in.n_elem; e++) order[e] = e;
    off = {0, in.n_elem};
  }
  p.scatter_atomic = !coloured;
  // coloured: the elements that name a node twice go to their own list (colors.dup, dup_off), as in the linear assembly
  std::vector<int32_t> grouped, dups;
  grouped.reserve((size_t)in.n_elem);
  for (int g = 0; g < NL_GROUPS; g++) {
    p.grp_off[g].clear();
    p.dup_off[g].clear();
    std::vector<int32_t> doff(1, (int32_t)dups.size());
    bool any = false;
    for (size_t k = 0; k + 1 < off.size(); k++) {
      const size_t before = grouped.size();
      for (int32_t q = off[k]; q < off[k + 1]; q++) {
        const int32_t e = order[q];
        const int group = n.h_mats[in.elem_mat ? in.elem_mat[e] - 1 : 0].group;
        if (group == g) (coloured && names_a_node_twice(in.conn + (size_t)nn * e, nn) ? dups : grouped).push_back(e);
      }
      doff.push_back((int32_t)dups.size());
      if (grouped.size() > before || any) {
        if (!any) p.grp_off[g].push_back((int32_t)before);
        any = true;
        p.grp_off[g].push_back((int32_t)grouped.size());
      }
    }
    if (doff.back() > doff.front()) p.dup_off[g] = doff;
  }
  p.n_dup = (int32_t)dups.size();
  if (dev_alloc(&p.colors.order, std::max<size_t>(grouped.size(), 1)) || (p.n_dup > 0 && dev_alloc(&p.colors.dup, dups.size())))
    return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(p.colors.order, grouped.data(), grouped.size() * 4, hipMemcpyHostToDevice, c->stream));
  if (p.n_dup > 0) HIP_TRY(hipMemcpyAsync(p.colors.dup, dups.data(), dups.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // grouped and dups are host temporaries
  p.colors.n_elem = in.n_elem;
  p.colors.etype = p.etype;
  p.colors.offsets = {0, in.n_elem};       // marks the lists as built (ensure_scatter_map)
  return 0;
}

// The context for checked parts (none empty) and checked materials (nl_init_driver)
static int nl_init_parts(fx_context *c, int32_t n_node, const double *coord, const std::vector<NlPartIn> &in, int32_t n_mat,
                         const fx_material_view *mats) {
  nl_free(c);
  NlDev &n = c->nl;
  n.n_mat = n_mat;
  n.parts.resize(in.size());
  for (size_t i = 0; i < in.size(); i++) {
    NlPart &p = n.parts[i];
    p.etype = in[i].etype; p.nn = c3_nodes(p.etype); p.nq = c3_points(p.etype);
    p.fbar = p.etype == 361 && in[i].fbar;
    n.has_fbar |= p.fbar;
    p.n_elem = in[i].n_elem;
    p.elem_off = n.n_elem; p.pt_off = n.n_pt; p.k_off = n.n_k; p.qf_off = n.n_qf;
    if ((int64_t)n.n_elem + p.n_elem > INT32_MAX) { g_fx_error = "fx_nl_init: more than 2^31 - 1 elements"; return FX_ERROR_RUNTIME; }
    n.n_elem += p.n_elem;
    n.n_pt += (int64_t)p.nq * p.n_elem;
    n.n_k += (size_t)(3 * p.nn) * (3 * p.nn) * p.n_elem;
    n.n_qf += (size_t)3 * p.nn * p.n_elem;
  }
  const size_t np3 = (size_t)3 * c->A.NP, npt = (size_t)n.n_pt;
  if (dev_alloc(&n.coord, np3) || nl_alloc_point_arrays(n.st, npt) || dev_alloc(&n.unode, np3) || dev_alloc(&n.dunode, np3) ||
      dev_alloc(&n.qforce, np3) || dev_alloc(&n.GL, np3) || dev_alloc(&n.bc_flag, np3) || dev_alloc(&n.bc_val, np3) ||
      dev_alloc(&n.err, 1))
    return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(n.coord, coord, np3 * 8, hipMemcpyHostToDevice, c->stream));
  for (size_t i = 0; i < in.size(); i++) {
    NlPart &p = n.parts[i];
    const size_t ncn = (size_t)p.nn * p.n_elem;
    if (dev_alloc(&p.conn, ncn)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpyAsync(p.conn, in[i].conn, ncn * 4, hipMemcpyHostToDevice, c->stream));
  }
  // materials: one NlMat per section, hardening tables on the device
  n.h_mats.resize((size_t)n_mat);
  n.prony.assign((size_t)n_mat, std::vector<double>());
  for (int32_t k = 0; k < n_mat; k++) {
    const fx_material_view &mv = mats[k];
    double *tab = nullptr;
    if (dev_alloc(&tab, (size_t)2 * std::max(mv.ntab, 1))) return FX_ERROR_RUNTIME;
    n.tabs.push_back(tab);
    if (mv.ntab > 0) HIP_TRY(hipMemcpyAsync(tab, mv.tab, (size_t)2 * mv.ntab * 8, hipMemcpyHostToDevice, c->stream));
    NlMat &m = n.h_mats[k];
    m.E = mv.E; m.nu = mv.nu;
    for (int i = 0; i < 3; i++) m.pl[i] = mv.plconst[i];
    m.plastic = mv.plastic == 1 ? 1 : 0; m.harden = mv.harden; m.group = mv.nlgeom; m.ntab = mv.ntab;
    m.pl4 = 0.0;
    if (mv.plastic == FX_MAT_MOONEY || mv.plastic == FX_MAT_ARRUDA) { m.harden = mv.plastic; m.group = 3; m.ntab = 0; }  // group 3: no history, no latch
    if (mv.plastic == FX_MAT_MOHR || mv.plastic == FX_MAT_DRUCKER) {  // groups 4..6: plastic in every piece of history, its own point functions
      m.plastic = mv.plastic; m.harden = 0; m.group = 4 + mv.nlgeom; m.ntab = 0; m.pl4 = mv.plconst4;
      n.has_yield = true;
    }
    if (mv.plastic == FX_MAT_VISCO) {  // groups 7, 8: its own tangent and stress, fstatus(1 : 12 nrow + 6) in n.hist, no latch
      m.plastic = 0; m.harden = 0; m.group = 7 + mv.nlgeom;
      n.prony[k].assign(mv.tab, mv.tab + (size_t)2 * mv.ntab);
      n.hist_w = std::max(n.hist_w, 12 * mv.ntab + 6);
    }
    if (mv.plastic == FX_MAT_NORTON) {  // group 9: plstrain, fstatus(1), fstatus(2); sets the latch
      m.plastic = 0; m.harden = 0; m.group = 9; m.ntab = 0;
      n.prony[k].assign(mv.plconst, mv.plconst + 3);
      n.hist_w = std::max(n.hist_w, 2);
      n.has_creep = true;
    }
    m.tab = tab;
  }
  if (n.hist_w > 0) {
    if (dev_alloc(&n.hist, (size_t)n.hist_w * npt)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemsetAsync(n.hist, 0, (size_t)n.hist_w * npt * 8, c->stream));
    if (int rc = nl_apply_time(c, "fx_nl_init", 0.0, 0.0)) return rc;  // the device tables hold (exp_n, dq_n), not the card's rows
  }
  n.mat = n.h_mats[0];
  n.tab = nullptr;
  if (n_mat > 1) {
    if (dev_alloc(&n.mats, (size_t)n_mat)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpyAsync(n.mats, n.h_mats.data(), (size_t)n_mat * sizeof(NlMat), hipMemcpyHostToDevice, c->stream));
    for (size_t i = 0; i < in.size(); i++) {
      NlPart &p = n.parts[i];
      if (dev_alloc(&p.emat, (size_t)p.n_elem)) return FX_ERROR_RUNTIME;
      HIP_TRY(hipMemcpyAsync(p.emat, in[i].elem_mat, (size_t)p.n_elem * 4, hipMemcpyHostToDevice, c->stream));
    }
  }
  bool flags = true;  // STF_C3 parts only, all coloured: k_nl_stiffness<G> (361) does not read first-write flags
  for (size_t i = 0; i < in.size(); i++) {
    if (int rc = nl_part_lists(c, n.parts[i], in[i], n_node)) return rc;
    flags &= n.parts[i].etype != 361 && !n.parts[i].scatter_atomic;
  }
  std::vector<FirstWriteGroup> fw;
  for (NlPart &p : n.parts) {
    if (flags) {
      // first-write flags in the order of the launches (part after part, group after group, colour after colour): the boundaries
      // of all the launches are the `colours` the flags are made for (none of the elements is in colors.dup: they were refused)
      p.colors.offsets.assign(1, 0);
      for (int g = 0; g < NL_GROUPS; g++)
        for (size_t k = 1; k < p.grp_off[g].size(); k++)
          if (p.grp_off[g][k] > p.colors.offsets.back()) p.colors.offsets.push_back(p.grp_off[g][k]);
    }
    if (ensure_scatter_map(c, p.colors, p.n_elem, p.conn, p.etype)) return FX_ERROR_RUNTIME;
    fw.push_back({&p.colors, p.conn});
  }
  // otherwise unflagged maps in every part and the matrix is cleared once: never both uncleared and unflagged
  if (flags && build_first_write(c, fw, &n.first_write)) return FX_ERROR_RUNTIME;
  if (for_each_point_array([&](size_t b, void *a) { HIP_TRY(hipMemsetAsync(a, 0, npt * b, c->stream)); return 0; }, n.st))
    return FX_ERROR_RUNTIME;
  for (double *p : {n.unode, n.dunode, n.qforce, n.GL, n.bc_val}) HIP_TRY(hipMemsetAsync(p, 0, np3 * 8, c->stream));
  HIP_TRY(hipMemsetAsync(n.bc_flag, 0, np3, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  n.latch = 0;
  n.ready = true;
  return 0;
}

// The one set-up of the nonlinear context, for every fx_nl_init* entry point (`who`: the one called).  fstr_solid / tGaussStatus
// set-up (fstr_setup.f90:325-400, fstr_init_gauss mechgauss.f90:37-71) over the groups of fstr_StiffMatrix's and fstr_Update's
// loops over hecMESH%elem_type_item: zero state, zero displacement.  Everything is refused before nl_init_parts frees the
// context that is there.
static int nl_init_driver(fx_context *c, const char *who, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                          int32_t n_mat, const fx_material_view *mats) {
  if (int rc = check_groups(who, n_node, coord, n_group, groups, n_mat, mats != nullptr, true)) return rc;
  for (int32_t g = 0; g < n_group; g++) {
    const fx_elem_group &G = groups[g];
    if (G.etype != 361) continue;
    if (G.elemopt != 2 && G.elemopt != 4)
      return fx_fail(who, FX_ERROR_UNSUPPORTED,
                     "group %d: elemopt %d of TYPE=361; the nonlinear loop serves 361 with elemopt 2 (B-bar) and 4 (F-bar) only", (int)g + 1,
                     (int)G.elemopt);
    if (G.elemopt != 4) continue;
    // Update_C3D8Fbar's UPDATELAG branch reads a local array it never assigned (static_LIB_Fbar.f90:600-602): nothing to be equal to
    for (int32_t e = 0; e < G.n_elem; e++)
      if (mats[n_mat > 1 ? G.elem_mat[e] - 1 : 0].nlgeom == 2)
        return fx_fail(who, FX_ERROR_UNSUPPORTED,
                       "group %d: an F-bar element (elemopt 4) with an UPDATELAG material (nlgeom 2), element %d; F-bar is served for "
                       "INFINITE and TOTALLAG", (int)g + 1, (int)e + 1);
  }
  if (!c->have_profile) return fx_fail(who, FX_ERROR_RUNTIME, "upload the profile first (fx_upload FX_UP_PROFILE)");
  if (n_node != c->A.NP) return fx_fail(who, FX_ERROR_RUNTIME, "mesh/profile size mismatch");
  if (int e = nl_check_materials(who, n_mat, mats)) return e;
  std::vector<NlPartIn> in;
  for (int32_t g = 0; g < n_group; g++)
    if (groups[g].n_elem > 0)
      in.push_back({groups[g].etype, groups[g].n_elem, groups[g].conn, n_mat > 1 ? groups[g].elem_mat : nullptr,
                    groups[g].etype == 361 && groups[g].elemopt == 4});
  if (in.empty()) return fx_fail(who, FX_ERROR_RUNTIME, "empty mesh");
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = nl_init_parts(c, n_node, coord, in, n_mat, mats)) return rc;
  // lists that name a group (fx_nl_set_dload) do so by the caller's position, empty groups counted
  int32_t part = 0;
  for (int32_t g = 0; g < n_group; g++) {
    c->nl.group_part.push_back(groups[g].n_elem > 0 ? part++ : -1);
    c->nl.group_etype.push_back(groups[g].etype);
  }
  return 0;
}
// The single-type entry points: the mesh as one group (361: B-bar).  With one material elem_mat is not read, whatever it holds.
static int nl_init_mesh(fx_context *c, const char *who, const fx_mesh_view *mesh, int32_t etype, int32_t n_mat,
                        const fx_material_view *mats, const int32_t *elem_mat) {
  if (!c || !mesh) return fx_fail(who, FX_ERROR_RUNTIME, "null argument");
  const fx_elem_group g = {etype, 2, mesh->n_elem, mesh->conn, n_mat > 1 ? elem_mat : nullptr};
  return nl_init_driver(c, who, mesh->n_node, mesh->coord, 1, &g, n_mat, mats);
}

extern "C" int fx_nl_init(fx_context *c, const fx_mesh_view *mesh, const fx_material_view *mat) {
  return nl_init_mesh(c, "fx_nl_init", mesh, 361, 1, mat, nullptr);
}

// Several sections (hecMESH%section_ID -> fstrSOLID%materials, fstr_setup.f90:325-400): elem_mat[e] in 1..n_mat.  The materials may
// carry different NLGEOM flags (an elastic TOTALLAG part next to an elastoplastic UPDATELAG part).
extern "C" int fx_nl_init_sections(fx_context *c, const fx_mesh_view *mesh, int32_t n_mat, const fx_material_view *mats,
                                   const int32_t *elem_mat) {
  return nl_init_mesh(c, "fx_nl_init_sections", mesh, 361, n_mat, mats, elem_mat);
}

// The same context for a mesh of tetrahedra, etype 341 or 342 (STF_C3 / UPDATE_C3, fx_nonlinear_tet.h): n_mat materials,
// elem_mat[e] in 1..n_mat (may be NULL with one material).  Every other fx_nl_* entry point works on either context.
extern "C" int fx_nl_init_c3(fx_context *c, const fx_mesh_view *mesh, int32_t etype, int32_t n_mat, const fx_material_view *mats,
                             const int32_t *elem_mat) {
  if (etype != 341 && etype != 342)
    return fx_fail("fx_nl_init_c3", FX_ERROR_UNSUPPORTED, "the nonlinear loop covers TYPE=341 and 342 (361 through fx_nl_init / fx_nl_init_sections)");
  return nl_init_mesh(c, "fx_nl_init_c3", mesh, etype, n_mat, mats, elem_mat);
}

// The same for any of the five types STF_C3 / UPDATE_C3 serve: 341, 342 (fx_nonlinear_tet.h), 351, 352, 362 (fx_nonlinear_c3.h).
// fx_mesh_view carries no nodes-per-element, so the caller states it: nn_elem is the row length of mesh->conn, and a type whose
// node count it is not is refused before anything reads the connectivity.
extern "C" int fx_nl_init_type(fx_context *c, const fx_mesh_view *mesh, int32_t etype, int32_t nn_elem, int32_t n_mat,
                               const fx_material_view *mats, const int32_t *elem_mat) {
  if (!c3_linear_type(etype))
    return fx_fail("fx_nl_init_type", FX_ERROR_UNSUPPORTED,
                   "TYPE=%d: the STF_C3 nonlinear loop covers 341, 342, 351, 352 and 362 (361 through fx_nl_init / fx_nl_init_sections)", (int)etype);
  if (nn_elem != c3_nodes(etype))
    return fx_fail("fx_nl_init_type", FX_ERROR_UNSUPPORTED, "TYPE=%d has %d nodes per element, the connectivity has %d", (int)etype,
                   c3_nodes(etype), (int)nn_elem);
  return nl_init_mesh(c, "fx_nl_init_type", mesh, etype, n_mat, mats, elem_mat);
}

// The same context for a mesh of several solid element types.  One material table serves all groups.  A 361 group is B-bar
// (elemopt 2) or F-bar (elemopt 4, fx_nonlinear_fbar.h: INFINITE and TOTALLAG materials only); part g launches the family its
// elemopt names, everything else of a part -- lists, colours, history, outputs -- is the same for both.
extern "C" int fx_nl_init_groups(fx_context *c, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                                 int32_t n_mat, const fx_material_view *mats) {
  if (!c) return fx_fail("fx_nl_init_groups", FX_ERROR_RUNTIME, "null argument");
  return nl_init_driver(c, "fx_nl_init_groups", n_node, coord, n_group, groups, n_mat, mats);
}

// The connectivity of the resident parts (and, with_emat, their material ids) back on the host: fx_nl_set_dload and fx_nl_nodal_stress
// resolve their lists there.
static int nl_parts_to_host(const NlDev &n, bool with_emat, std::vector<std::vector<int32_t>> &conn, std::vector<std::vector<int32_t>> &emat) {
  conn.assign(n.parts.size(), {});
  emat.assign(n.parts.size(), {});
  for (size_t g = 0; g < n.parts.size(); g++) {
    const NlPart &p = n.parts[g];
    conn[g].resize((size_t)p.nn * p.n_elem);
    if (!conn[g].empty()) HIP_TRY(hipMemcpy(conn[g].data(), p.conn, conn[g].size() * 4, hipMemcpyDeviceToHost));
    if (with_emat && p.emat && p.n_elem > 0) {
      emat[g].resize((size_t)p.n_elem);
      HIP_TRY(hipMemcpy(emat[g].data(), p.emat, emat[g].size() * 4, hipMemcpyDeviceToHost));
    }
  }
  return 0;
}

#define NL_READY(name)                                                                              \
  HIP_TRY(hipSetDevice(c->device));                                                                 \
  if (!c->nl.ready) { g_fx_error = name ": call fx_nl_init first"; return FX_ERROR_RUNTIME; }

// f(std::integral_constant<int, G>()) for every group G of the element kernels, in order
template <class F, int... G>
static void for_each_nl_group(F &&f, std::integer_sequence<int, G...>) {
  (f(std::integral_constant<int, G>()), ...);
}
template <class F>
static void for_each_nl_group(F &&f) {
  for_each_nl_group(f, std::make_integer_sequence<int, NL_GROUPS>());
}
// The element kernel of one type and group: k_nl_* of 361 (B-bar), k_nl_*_tet for the tetrahedra, k_nl_*_c3 for 351 / 352 / 362.
// The three tangents take the same arguments but for one int of 361's, the three updates the same arguments.
// TH: the thermal variant (fx_nl_set_thermal).  The update kernels take it whenever thermal is on, the tangent kernels only where a
// material has an elastic table; a context without thermal strain launches the TH = 0 instantiations, the kernels it always had.
template <int ETYPE, int G, bool UPDATE, int TH>
static constexpr auto nl_c3_kernel() {
  if constexpr (UPDATE) {
    if constexpr (ETYPE == 361) return k_nl_update<G, TH>;
    else if constexpr (C3El<ETYPE>::TET) return k_nl_update_tet<ETYPE, G, TH>;
    else return k_nl_update_c3<ETYPE, G, TH>;
  } else {
    if constexpr (ETYPE == 361) return k_nl_stiffness<G, TH>;
    else if constexpr (C3El<ETYPE>::TET) return k_nl_stiffness_tet<ETYPE, G, TH>;
    else return k_nl_stiffness_c3<ETYPE, G, TH>;
  }
}
// The groups the F-bar kernels are instantiated for: no UPDATELAG (nl_init_driver refuses it, so such a list is empty)
static constexpr bool nl_fbar_group(int G) { return nl_group_flag(G) != 2; }
// The groups that have thermal variants (TH = 1): fx_nl_set_thermal refuses a context with a viscoelastic or NORTON material, so
// groups 7..9 are instantiated without them
static constexpr bool nl_thermal_group(int G) { return !nl_group_visco(G) && !nl_group_creep(G); }
// What one group of a part launches: the kernel of its type (null: nothing to launch), elements per workgroup and workgroup size.
// An F-bar part takes the F-bar kernels, which have the arguments of 361's and, for the tangent, a workgroup of their own.
template <int ETYPE, int G, bool UPDATE, int TH>
struct NlKernel {
  decltype(nl_c3_kernel<ETYPE, G, UPDATE, TH>()) kern = nl_c3_kernel<ETYPE, G, UPDATE, TH>();
  int epb = ETYPE != 361 ? (UPDATE ? C3El<ETYPE>::UEPB : C3El<ETYPE>::EPB) : FXN_EPB;
  int block = ETYPE != 361 ? C3El<ETYPE>::BS : FXN_BLOCK;
  explicit NlKernel(const NlPart &p) {
    if constexpr (ETYPE == 361) {
      if (!p.fbar) return;
      if constexpr (!nl_fbar_group(G)) kern = nullptr;
      else if constexpr (UPDATE) kern = k_nl_update_fbar<G, TH>;
      else { kern = k_nl_stiffness_fbar<G, TH>; epb = FXF_EPB; block = FXF_BLOCK; }
    }
  }
};
// A part's block of the viscoelastic history
static NlHist nl_part_hist(const NlDev &n, const NlPart &p) {
  return NlHist{n.hist ? n.hist + p.pt_off : nullptr, n.n_pt, n.st.plstrain + p.pt_off};
}
// A part's block of the per-point arrays
static NlPartState nl_part_state(const NlDev &n, const NlPart &p) {
  NlPartState s = n.st;
  for_each_point_array([&](size_t b, auto *&a) { a += (int64_t)(b / sizeof(*a)) * p.pt_off; return 0; }, s);
  return s;
}
template <int ETYPE>
static constexpr size_t NL_KE = (size_t)(3 * C3El<ETYPE>::NN) * (3 * C3El<ETYPE>::NN);  // doubles of one element matrix
// The tangent of one group of a part of any of the six types.  Kout: the part's block of the element matrices, or null (scatter);
// dup_k (361, scatter): room for the element matrices of the part's collapsed elements
template <int ETYPE, int G, int TH>
static void nl_launch_stiffness_group(fx_context *c, const NlPart &p, double *Kout, double *dup_k) {
  NlDev &n = c->nl;
  const DevCSR &A = c->A;
  const NlPartState s = nl_part_state(n, p);
  const NlKernel<ETYPE, G, false, TH> k(p);
  if (!k.kern) return;
  const ThermalDev th = nl_thermal_dev(n);
  auto launch = [&](dim3 grid, int32_t e0, int32_t e1, double *K, const int32_t *list, const int32_t *pos, int atomic, int k_by_pos) {
    auto go = [&](auto... tail) {
      hipLaunchKernelGGL(k.kern, grid, dim3(k.block), 0, c->stream, e1, n.coord, p.conn, n.unode, n.dunode, n.mat, n.latch, s.stress,
                         s.fstat, s.istat, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL, A.AU, K, n.err, list, e0, pos, atomic,
                         (const NlMat *)n.mats, (const int32_t *)p.emat, tail...);
    };
    if constexpr (ETYPE == 361) go(k_by_pos, (const double *)s.strain, th, nl_part_hist(n, p));  // 361's own argument: K by position in the list
    else go((const double *)s.strain, th, nl_part_hist(n, p));
  };
  // element matrices out, or atomics: the group's colours in one launch
  for_colour_ranges(p.grp_off[G], Kout || p.scatter_atomic, k.epb, [&](dim3 grid, int32_t e0, int32_t e1) {
    launch(grid, e0, e1, Kout, p.colors.order, p.colors.pos, p.scatter_atomic ? 1 : 0, 0);
  });
  if constexpr (ETYPE == 361) {  // the collapsed elements of the group: only 361 has them, the other types refuse them at init
    // their element matrices (into Kout by element id, or dup_k by position in colors.dup), then -- for the scatter -- added colour
    // by colour (k_add_elem_blocks)
    const std::vector<int32_t> &doff = p.dup_off[G];
    if (doff.empty()) return;
    const int32_t d0 = doff.front(), d1 = doff.back();
    launch(dim3((d1 - d0 + k.epb - 1) / k.epb), d0, d1, Kout ? Kout : dup_k, p.colors.dup, nullptr, 0, Kout ? 0 : 1);
    if (Kout) return;
    for_colour_ranges(doff, false, 64, [&](dim3 grid, int32_t p0, int32_t p1) {
      hipLaunchKernelGGL(k_add_elem_blocks, grid, dim3(64), 0, c->stream, p0, p1, (const int32_t *)p.colors.dup, (const double *)dup_k,
                         (const int32_t *)p.conn, (const int32_t *)p.colors.pos, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL, A.AU, n.err);
    });
  }
}
// The stress update of one group of a part of any of the six types
template <int ETYPE, int G, int TH>
static void nl_launch_update_group(fx_context *c, const NlPart &p, double *qf_out) {
  NlDev &n = c->nl;
  const NlPartState s = nl_part_state(n, p);
  const NlKernel<ETYPE, G, true, TH> k(p);
  if (!k.kern) return;
  const ThermalDev th = nl_thermal_dev(n);
  auto launch = [&](const int32_t *list, int32_t e0, int32_t e1) {
    hipLaunchKernelGGL(k.kern, dim3((unsigned)((e1 - e0 + k.epb - 1) / k.epb)), dim3(k.block), 0, c->stream, e1, n.coord, p.conn, n.unode,
                       n.dunode, n.mat, s.stress, s.strain, s.stress_bak, s.strain_bak, s.plstrain, s.fstat, s.istat, n.qforce, qf_out,
                       list, e0, (const NlMat *)n.mats, (const int32_t *)p.emat, n.err, th, nl_part_hist(n, p));
  };
  const std::vector<int32_t> &off = p.grp_off[G];
  // a group that holds every element of the part is walked in the elements' own order (contiguous history arrays); the internal
  // force is scattered with atomics either way
  if (!off.empty() && off.back() > off.front())
    launch((off.front() == 0 && off.back() == p.n_elem) ? nullptr : p.colors.order, off.front(), off.back());
  if constexpr (ETYPE == 361) {  // the collapsed elements of the group
    const std::vector<int32_t> &doff = p.dup_off[G];
    if (!doff.empty()) launch(p.colors.dup, doff.front(), doff.back());
  }
}
// Part after part, NLGEOM group after group, colour after colour on one stream: one kernel instantiation per type and group present
static int nl_launch_stiffness(fx_context *c, double *Kout) {  // Kout: the element matrices of all parts one after the other, or null
  DevScratch tmp;
  double *dup_k = nullptr;
  size_t n_dup = 0;
  for (const NlPart &p : c->nl.parts) n_dup += (size_t)p.n_dup;
  if (!Kout && n_dup > 0 && tmp.alloc(&dup_k, NL_KE<361> * n_dup)) return FX_ERROR_RUNTIME;
  size_t dup_at = 0;  // collapsed elements of the parts before this one (361 parts alone have any)
  for (const NlPart &p : c->nl.parts) {
    with_solid_type(p.etype, [&](auto t) {
      for_each_nl_group([&](auto g) {
        constexpr int ET = decltype(t)::value, G = decltype(g)::value;
        double *const K = Kout ? Kout + p.k_off : nullptr, *const dk = dup_k ? dup_k + NL_KE<361> * dup_at : nullptr;
        if constexpr (nl_thermal_group(G)) {
          if (c->nl.th.on && c->nl.th.elastic_tab) { nl_launch_stiffness_group<ET, G, 1>(c, p, K, dk); return; }
        }
        nl_launch_stiffness_group<ET, G, 0>(c, p, K, dk);
      });
    });
    dup_at += (size_t)p.n_dup;
  }
  if (dup_k) HIP_TRY(hipStreamSynchronize(c->stream));  // dup_k is freed on return
  return 0;
}
static void nl_launch_update(fx_context *c, double *qf_out) {  // qf_out: the element forces of all parts one after the other, or null
  for (const NlPart &p : c->nl.parts)
    with_solid_type(p.etype, [&](auto t) {
      for_each_nl_group([&](auto g) {
        constexpr int ET = decltype(t)::value, G = decltype(g)::value;
        if constexpr (nl_thermal_group(G)) {
          if (c->nl.th.on) { nl_launch_update_group<ET, G, 1>(c, p, qf_out ? qf_out + p.qf_off : nullptr); return; }
        }
        nl_launch_update_group<ET, G, 0>(c, p, qf_out ? qf_out + p.qf_off : nullptr);
      });
    });
}
// The stress update of a context with a Mohr-Coulomb / Drucker-Prager or NORTON section or an F-bar part reports the reference's `stop`
// statements through the error word: cleared before the launches, read after them (one 4-byte copy; other contexts skip both).
static int nl_update_err_clear(fx_context *c) {
  if (c->nl.has_yield || c->nl.has_fbar || c->nl.has_creep) HIP_TRY(hipMemsetAsync(c->nl.err, 0, 4, c->stream));
  return 0;
}
static int nl_update_err_check(fx_context *c) {
  if (!c->nl.has_yield && !c->nl.has_fbar && !c->nl.has_creep) return 0;
  int32_t herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, c->nl.err, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return assembly_error(herr);
}
// fstr_UpdateNewton's element loop for the three update entry points: error word, launches (`launched`, if given, is recorded
// behind them), the reference's `stop`s, and MatlMatrix's saved flag -- an update that stopped sets no latch.
static int nl_run_update(fx_context *c, double *qf_out, hipEvent_t launched = nullptr) {
  if (nl_update_err_clear(c)) return FX_ERROR_RUNTIME;
  nl_launch_update(c, qf_out);
  HIP_TRY(hipGetLastError());
  if (launched) HIP_TRY(hipEventRecord(launched, c->stream));
  if (int rc = nl_update_err_check(c)) return rc;
  // MatlMatrix(..., isEp=1) has now been called (calMatMatrix.f90:43-45); the flag is the process's, whichever section set it
  // (the update routines set isEp for a NORTON element too, whatever tincr is: static_LIB_3d.f90:595)
  for (const NlMat &m : c->nl.h_mats) if (m.plastic || nl_group_creep(m.group)) c->nl.latch = 1;
  return 0;
}

// fstr_StiffMatrix + fstr_AddBC (fstr_StiffMatrix.f90:18-212, fstr_AddBC.f90:17-190): tangent of the current
// state (u = unode + dunode) into the resident D/AL/AU, then Dirichlet elimination with the given increments
// against the resident right-hand side.  The prescribed dofs are remembered for fx_nl_update.
extern "C" int fx_nl_stiffness(fx_context *c, int32_t n_bc, const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val,
                               float *ms_assemble) {
  NL_READY("fx_nl_stiffness");
  NlDev &n = c->nl;
  DevCSR &A = c->A;
  for (int32_t k = 0; k < n_bc; k++)
    if (bc_node[k] < 1 || bc_node[k] > A.NP) { g_fx_error = "fx_nl_stiffness: BC node id out of range"; return FX_ERROR_RUNTIME; }
  HIP_TRY(hipMemsetAsync(n.err, 0, 4, c->stream));
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  // first-write scatter (parts of the STF_C3 types only): every block is stored before it is added to, no clearing
  if (!n.first_write && mat_clear(c)) return FX_ERROR_RUNTIME;
  if (nl_launch_stiffness(c, nullptr)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipGetLastError());
  n.n_bc = n_bc;
  if (n_bc > 0) {
    if (n_bc > n.bc_cap) {
      dev_free(n.bc_node); dev_free(n.bc_dof); dev_free(n.bc_v);
      if (dev_alloc(&n.bc_node, (size_t)n_bc) || dev_alloc(&n.bc_dof, (size_t)n_bc) || dev_alloc(&n.bc_v, (size_t)n_bc)) return FX_ERROR_RUNTIME;
      n.bc_cap = n_bc;
    }
    HIP_TRY(hipMemcpyAsync(n.bc_node, bc_node, (size_t)n_bc * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(n.bc_dof, bc_dof, (size_t)n_bc * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(n.bc_v, bc_val, (size_t)n_bc * 8, hipMemcpyHostToDevice, c->stream));
  }
  if (bc_eliminate(c, n_bc, n.bc_node, n.bc_dof, n.bc_v, n.bc_flag, n.bc_val)) return FX_ERROR_RUNTIME;  // no dof: the flags are cleared
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  int32_t herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, n.err, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (ms_assemble) HIP_TRY(hipEventElapsedTime(ms_assemble, c->ev0, c->ev1));
  if (int rc = assembly_error(herr)) return rc;
  c->have_values = true;
  c->bell_valid = false;   // the preconditioner is refreshed by the flags / recycle policy of the next solve, not here
  return 0;
}

static int nl_dot(fx_context *c, const double *x, const double *y, double *out) {  // hecmw_InnerProduct_R over the internal dofs
  if (c->max_partials < 4096 + 8) {
    dev_free(c->partials);
    if (dev_alloc(&c->partials, (size_t)(4096 + 8) * 3)) return FX_ERROR_RUNTIME;
    c->max_partials = 4096 + 8;
  }
  const int64_t len = (int64_t)3 * c->A.N;
  const int np = grid_for(len, FX_BLOCK, 2048);
  hipLaunchKernelGGL(k_dot, dim3(np), dim3(FX_BLOCK), 0, c->stream, len, x, y, c->partials, (const int32_t *)nullptr, 0);
  HIP_TRY(hipGetLastError());
  double tmp;
  return host_sum(c, np, 0, out, &tmp);
}

static int nl_halo_natural(fx_context *c, double *v) {  // hecmw_update_3_R on a vector in the reference numbering
  if (!multi_rank(c)) return 0;
  if (ensure_solver(c)) return FX_ERROR_RUNTIME;
  if (to_slots(c, v, c->W[6]) || halo_update(c, c->W[6]) || from_slots(c, c->W[6], v)) return FX_ERROR_RUNTIME;
  return 0;
}

// The thermal load of fstr_ass_load.f90:287-428 added to the resident right-hand side: the TLOAD vector of every element on the
// current configuration node + unode (:316-320) with TEMP0 = last_temp whatever the material (:307), through the thermal-load
// kernels of the linear path (fx_thermal.h, TH = 2).  Every 361 part is B-bar here, F-bar included (:391-398).  The kernels take
// the elastic matrix of the material's E, nu (or of its table at the point): a hyperelastic material, which has neither, adds nothing.
static int nl_thermal_load(fx_context *c) {
  NlDev &n = c->nl;
  const size_t np3 = (size_t)3 * c->A.NP;
  double *xc = n.th.xc;
  HIP_TRY(hipMemcpyAsync(xc, n.coord, np3 * 8, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_axpy_plain, dim3(grid_for((int64_t)np3)), dim3(256), 0, c->stream, (int64_t)np3, 1.0, n.unode, xc);
  const ThermalDev th = nl_thermal_dev(n);
  for (const NlPart &p : n.parts)
    launch_update_linear_th<2>(c, p.etype, 2, p.n_elem, xc, p.conn, n.th.D0[0], n.th.D0[1], n.th.D0[2], p.emat, p.emat ? n.th.mtab : nullptr, nullptr,
                               nullptr, nullptr, c->A.B, n.err, th);
  HIP_TRY(hipGetLastError());
  return 0;  // (on the context's stream: fx_nl_begin_substep synchronises)
}

// Start of a substep (fstr_Newton :63-68, fstr_ass_load.f90:64-91,:273): dunode = 0, GL = load at the end of the
// increment (host, 3*NP, may be NULL = no nodal load), B = GL - QFORCE.
extern "C" int fx_nl_begin_substep(fx_context *c, const double *GL) {
  NL_READY("fx_nl_begin_substep");
  NlDev &n = c->nl;
  const size_t np3 = (size_t)3 * c->A.NP;
  HIP_TRY(hipMemsetAsync(n.dunode, 0, np3 * 8, c->stream));
  if (GL) HIP_TRY(hipMemcpyAsync(n.GL, GL, np3 * 8, hipMemcpyHostToDevice, c->stream));
  else HIP_TRY(hipMemsetAsync(n.GL, 0, np3 * 8, c->stream));
  if (n.dl.on)  // GL = nodal load + factor DLOAD (fstr_ass_load.f90:138-257)
    if (int rc = nl_dload_rebuild(c, true)) return rc;
  hipLaunchKernelGGL(k_nl_residual, dim3(grid_for((int64_t)np3)), dim3(256), 0, c->stream, (int64_t)np3, n.GL, n.qforce,
                     (const uint8_t *)nullptr, c->A.B);
  HIP_TRY(hipGetLastError());
  if (n.th.on)
    if (int rc = nl_thermal_load(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// After the solve (fstr_Newton :92-122): dunode += X, fstr_UpdateNewton, fstr_Update_NDForce, and the four
// norms of the convergence test: out = {|B|^2, |X|^2, |QFORCE|^2, |dunode|^2} over the internal dofs.
extern "C" int fx_nl_update(fx_context *c, double out[4], float *ms_update) {
  NL_READY("fx_nl_update");
  NlDev &n = c->nl;
  const int64_t np3 = (int64_t)3 * c->A.NP;
  hipLaunchKernelGGL(k_axpy_plain, dim3(grid_for(np3)), dim3(256), 0, c->stream, np3, 1.0, c->A.X, n.dunode);
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  HIP_TRY(hipMemsetAsync(n.qforce, 0, (size_t)np3 * 8, c->stream));
  if (int rc = nl_run_update(c, nullptr, c->ev1)) return rc;
  if (nl_halo_natural(c, n.qforce)) return FX_ERROR_RUNTIME;
  if (n.dl.on && n.dl.follow)  // fstr_ass_load again on node + unode + dunode (fstr_solve_NonLinear.f90:103)
    if (int rc = nl_dload_rebuild(c, false)) return rc;
  hipLaunchKernelGGL(k_nl_residual, dim3(grid_for(np3)), dim3(256), 0, c->stream, np3, n.GL, n.qforce, n.bc_flag, c->A.B);
  HIP_TRY(hipGetLastError());
  if (nl_halo_natural(c, c->A.B)) return FX_ERROR_RUNTIME;
  if (out) {
    if (nl_dot(c, c->A.B, c->A.B, out + 0) || nl_dot(c, c->A.X, c->A.X, out + 1) || nl_dot(c, n.qforce, n.qforce, out + 2) ||
        nl_dot(c, n.dunode, n.dunode, out + 3))
      return FX_ERROR_RUNTIME;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (ms_update) HIP_TRY(hipEventElapsedTime(ms_update, c->ev0, c->ev1));
  return 0;
}

// ---- the same two steps for a caller that keeps fstr_Newton's loop on the host (the Fortran binding of INTEGRATION.md section 5:
// fistr1's own fstr_Newton drives them).  unode / dunode are the host's (fstrSOLID%unode, %dunode: 3*NP doubles each travel per
// call, the 6.5 GB matrix does not); no boundary conditions, no right-hand side: fstr_AddBC and fstr_Update_NDForce stay the
// reference's, their hecmw_mat_ass_bc calls reach the resident matrix through fx_mat_ass_bc.
extern "C" int fx_nl_stiffness_at(fx_context *c, const double *unode, const double *dunode, float *ms_assemble) {
  NL_READY("fx_nl_stiffness_at");
  NlDev &n = c->nl;
  const size_t np3 = (size_t)3 * c->A.NP * 8;
  if (unode) HIP_TRY(hipMemcpyAsync(n.unode, unode, np3, hipMemcpyHostToDevice, c->stream));
  if (dunode) HIP_TRY(hipMemcpyAsync(n.dunode, dunode, np3, hipMemcpyHostToDevice, c->stream));
  return fx_nl_stiffness(c, 0, nullptr, nullptr, nullptr, ms_assemble);
}

// fstr_UpdateNewton (fstr_Update.f90:25-293) for the host's dunode (the host has already added the solver's X, fstr_solve_NonLinear.f90:95-97):
// stresses / strains / plastic state of every quadrature point on the device, internal force QFORCE back to the host (before the
// caller's hecmw_update_3_R, :284).
extern "C" int fx_nl_update_at(fx_context *c, const double *dunode, double *qforce, float *ms_update) {
  NL_READY("fx_nl_update_at");
  NlDev &n = c->nl;
  const size_t np3 = (size_t)3 * c->A.NP * 8;
  if (dunode) HIP_TRY(hipMemcpyAsync(n.dunode, dunode, np3, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  HIP_TRY(hipMemsetAsync(n.qforce, 0, np3, c->stream));
  if (int rc = nl_run_update(c, nullptr, c->ev1)) return rc;
  if (n.dl.on && n.dl.follow)  // the follower load of the new configuration: fx_nl_get_load hands it to the host's loop
    if (int rc = nl_dload_rebuild(c, false)) return rc;
  if (qforce) HIP_TRY(hipMemcpyAsync(qforce, n.qforce, np3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (ms_update) HIP_TRY(hipEventElapsedTime(ms_update, c->ev0, c->ev1));
  return 0;
}

// hecmw_mat_ass_bc (hecmw_mat_ass.f90:292-429) for a list of prescribed dofs on the RESIDENT matrix and right-hand side: column
// times value moved to B, row and column zeroed, unit diagonal, B = value.  The list is what fstr_AddBC would have passed call by call.
extern "C" int fx_mat_ass_bc(fx_context *c, int32_t n_bc, const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->have_values) { g_fx_error = "fx_mat_ass_bc: no matrix values resident"; return FX_ERROR_RUNTIME; }
  if (n_bc <= 0) return 0;
  DevCSR &A = c->A;
  for (int32_t k = 0; k < n_bc; k++)
    if (bc_node[k] < 1 || bc_node[k] > A.NP || bc_dof[k] < 1 || bc_dof[k] > 3) { g_fx_error = "fx_mat_ass_bc: node id / dof out of range"; return FX_ERROR_RUNTIME; }
  DevScratch tmp;
  uint8_t *d_flag = nullptr;
  double *d_bcv = nullptr, *d_val = nullptr;
  int32_t *d_node = nullptr, *d_dof = nullptr;
  if (tmp.alloc(&d_flag, (size_t)3 * A.NP) || tmp.alloc(&d_bcv, (size_t)3 * A.NP) || tmp.alloc(&d_node, (size_t)n_bc) ||
      tmp.alloc(&d_dof, (size_t)n_bc) || tmp.alloc(&d_val, (size_t)n_bc))
    return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(d_node, bc_node, (size_t)n_bc * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_dof, bc_dof, (size_t)n_bc * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_val, bc_val, (size_t)n_bc * 8, hipMemcpyHostToDevice, c->stream));
  if (bc_eliminate(c, n_bc, d_node, d_dof, d_val, d_flag, d_bcv)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->bell_valid = false;  // the streaming layouts re-gather the values on next use
  return 0;
}

// End of a converged substep (fstr_Newton :156-162): unode += dunode, fstr_UpdateState.
extern "C" int fx_nl_commit(fx_context *c) {
  NL_READY("fx_nl_commit");
  NlDev &n = c->nl;
  const int64_t np3 = (int64_t)3 * c->A.NP;
  hipLaunchKernelGGL(k_axpy_plain, dim3(grid_for(np3)), dim3(256), 0, c->stream, np3, 1.0, n.dunode, n.unode);
  for (const NlPart &p : n.parts) {  // the kernels find a point's material through its element: part by part
    const NlPartState s = nl_part_state(n, p);
    const int64_t npt = (int64_t)p.nq * p.n_elem;
    hipLaunchKernelGGL(k_nl_commit, dim3(grid_for(6 * npt)), dim3(256), 0, c->stream, npt, p.nq, n.mat.plastic, s.fstat, s.plstrain,
                       s.stress, s.strain, s.stress_bak, s.strain_bak, (const NlMat *)n.mats, (const int32_t *)p.emat);
    if (n.hist && n.tincr > 0.0)  // updateViscoElasticState under `tincr > 0.d0` (fstr_Update.f90:333-337)
      hipLaunchKernelGGL(k_nl_commit_visco, dim3(grid_for(npt)), dim3(256), 0, c->stream, npt, p.nq, n.mat, (const NlMat *)n.mats,
                         (const int32_t *)p.emat, (const double *)s.strain, nl_part_hist(n, p));
  }
  if (n.th.on)  // last_temp = temperature (fstr_Update.f90:308-312)
    HIP_TRY(hipMemcpyAsync(n.th.last_temp, n.th.temp, (size_t)c->A.NP * 8, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// fstr_cutback_save (load = 0) / fstr_cutback_load (load = 1), fstr_Cutback.f90:108-198, for the state that lives on the device:
// the quadrature-point history (fstr_copy_gauss of every point: strain, stress, their _bak copies, plstrain, istatus, fstatus).
// unode and QFORCE are the host's (the *_at entry points take them from fstrSOLID at every call) and are restored there by the
// reference's own routine; MatlMatrix's saved flag (`latch`) is process state the reference does not roll back either.
extern "C" int fx_nl_snapshot(fx_context *c, int load) {
  NL_READY("fx_nl_snapshot");
  NlDev &n = c->nl;
  const size_t npt = (size_t)n.n_pt;
  if (load && !n.bk_valid) { g_fx_error = "fx_nl_snapshot: nothing was saved"; return FX_ERROR_RUNTIME; }
  // a save from before fx_nl_set_thermal (or before a repeated one) holds no last_temp of this set-up: nothing is restored then
  if (load && n.th.on && !n.th.bk_valid)
    return fx_fail("fx_nl_snapshot", FX_ERROR_RUNTIME, "the saved state holds no last_temp: fx_nl_set_thermal was called after the save");
  if (!n.bk.stress && nl_alloc_point_arrays(n.bk, npt)) return FX_ERROR_RUNTIME;
  if (for_each_point_array([&](size_t b, void *live, void *bk) {
        HIP_TRY(hipMemcpyAsync(load ? live : bk, load ? bk : live, npt * b, hipMemcpyDeviceToDevice, c->stream));
        return 0;
      }, n.st, n.bk))
    return FX_ERROR_RUNTIME;
  if (n.hist) {  // fstatus(:) of the viscoelastic points (fstr_copy_gauss)
    const size_t nh = (size_t)n.hist_w * npt;
    if (!n.hist_bk && dev_alloc(&n.hist_bk, nh)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpyAsync(load ? n.hist : n.hist_bk, load ? n.hist_bk : n.hist, nh * 8, hipMemcpyDeviceToDevice, c->stream));
  }
  if (n.th.on) {  // last_temp travels with the history (fstr_Cutback.f90:127, :173)
    if (!n.th.last_temp_bk && dev_alloc(&n.th.last_temp_bk, (size_t)c->A.NP)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpyAsync(load ? n.th.last_temp : n.th.last_temp_bk, load ? n.th.last_temp_bk : n.th.last_temp, (size_t)c->A.NP * 8,
                           hipMemcpyDeviceToDevice, c->stream));
    if (!load) n.th.bk_valid = true;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  n.bk_valid = true;
  return 0;
}

static int nl_creep_fstat(fx_context *c, int to_fstat);
static int nl_copy_state(fx_context *c, const fx_nl_state_view *s, bool to_device) {
  NlDev &n = c->nl;
  const size_t np3 = (size_t)3 * c->A.NP * 8, npt = (size_t)n.n_pt;
  auto copy = [&](size_t bytes, void *h, void *d) {  // a null host array is skipped
    if (h) HIP_TRY(hipMemcpyAsync(to_device ? d : h, to_device ? h : d, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  if (for_each_point_array([&](size_t b, void *h, void *d) { return copy(npt * b, h, d); }, *s, n.st) || copy(np3, s->unode, n.unode) ||
      copy(np3, s->dunode, n.dunode) || copy(np3, s->qforce, n.qforce))
    return FX_ERROR_RUNTIME;
  if (to_device && s->fstat)
    if (int rc = nl_creep_fstat(c, 0)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int fx_nl_get_state(fx_context *c, fx_nl_state_view *s) {
  NL_READY("fx_nl_get_state");
  s->latch = c->nl.latch;
  return nl_copy_state(c, s, false);
}
extern "C" int fx_nl_set_state(fx_context *c, const fx_nl_state_view *s) {
  NL_READY("fx_nl_set_state");
  if (s->latch >= 0) c->nl.latch = s->latch ? 1 : 0;
  return nl_copy_state(c, s, true);
}

// ---- thermal strain (see the header): the context's temperatures, expansion coefficients and tables
extern "C" int fx_nl_set_thermal(fx_context *c, const fx_nl_thermal_view *v) {
  const char *who = "fx_nl_set_thermal";
  NL_READY("fx_nl_set_thermal");
  NlDev &n = c->nl;
  if (!v) { nl_thermal_free(n.th); return 0; }
  if (!v->alpha) return fx_fail(who, FX_ERROR_RUNTIME, "expansion coefficients missing");
  if (n.hist_w > 0)
    return fx_fail(who, FX_ERROR_UNSUPPORTED,
                   "the context holds a viscoelastic or NORTON material: their thermal branches (the WLF / Arrhenius shift of !TRS, "
                   "the temperature tables inside UpdateViscoelastic, iso_creep and update_iso_creep) are not on the device");
  // everything is checked, and the new data is on the device, before the context changes
  std::vector<double> tabs;
  std::vector<int32_t> idx((size_t)4 * n.n_mat, 0);
  NlDev::Thermal t;
  for (int32_t k = 0; k < n.n_mat; k++) {
    const double *tab[2] = {v->alpha_tab ? v->alpha_tab[k] : nullptr, v->elastic_tab ? v->elastic_tab[k] : nullptr};
    for (int w = 0; w < 2; w++) {
      if (!tab[w]) continue;
      const int32_t *nrows = w == 0 ? v->alpha_rows : v->elastic_rows;
      const int nc = w == 0 ? 2 : 3, rows = nrows ? nrows[k] : 0;
      if (rows < 1) return fx_fail(who, FX_ERROR_RUNTIME, "material %d: a table with %d rows", (int)k + 1, rows);
      if (w == 1 && n.h_mats[k].group == 3)
        return fx_fail(who, FX_ERROR_UNSUPPORTED, "material %d: an elastic table on a hyperelastic material, which reads no E, nu", (int)k + 1);
      for (int r = 1; r < rows; r++)
        if (!(tab[w][nc * r + nc - 1] > tab[w][nc * (r - 1) + nc - 1]))
          return fx_fail(who, FX_ERROR_UNSUPPORTED, "material %d: the temperatures of the %s table are not strictly ascending (row %d)",
                         (int)k + 1, w == 0 ? "expansion" : "elastic", r + 1);
      idx[4 * k + 2 * w] = (int32_t)tabs.size();
      idx[4 * k + 2 * w + 1] = rows;
      tabs.insert(tabs.end(), tab[w], tab[w] + (size_t)nc * rows);
      t.any_tab = true;
      t.elastic_tab |= w == 1;
    }
  }
  // the elastic matrices of the constants, for the thermal-load kernels (nl_thermal_load); a hyperelastic material has none
  std::vector<double> mtab((size_t)3 * n.n_mat);
  for (int32_t k = 0; k < n.n_mat; k++) {
    const bool hyper = n.h_mats[k].group == 3;
    elastic_constants(hyper ? 0.0 : n.h_mats[k].E, hyper ? 0.0 : n.h_mats[k].nu, mtab[3 * k], mtab[3 * k + 1], mtab[3 * k + 2]);
  }
  for (int i = 0; i < 3; i++) t.D0[i] = mtab[i];
  const size_t np = (size_t)c->A.NP;
  if (dev_alloc(&t.mtab, mtab.size()) || dev_alloc(&t.xc, 3 * np) || dev_alloc(&t.temp, np) || dev_alloc(&t.last_temp, np) || dev_alloc(&t.temp_init, np) || dev_alloc(&t.alpha, (size_t)n.n_mat) ||
      dev_alloc(&t.tabs, std::max<size_t>(tabs.size(), 1)) || dev_alloc(&t.tab_idx, idx.size())) {
    nl_thermal_free(t);
    return FX_ERROR_RUNTIME;
  }
  const std::vector<double> ref(v->temp_init ? 0 : np, v->ref_temp);
  auto up = [&]() {
    if (v->temp_init) HIP_TRY(hipMemcpyAsync(t.temp_init, v->temp_init, np * 8, hipMemcpyHostToDevice, c->stream));
    else HIP_TRY(hipMemsetAsync(t.temp_init, 0, np * 8, c->stream));
    // last_temp = the initial condition (fstr_solve_NLGEOM.f90:53-57), or 0 (fstr_setup.f90:788)
    HIP_TRY(hipMemcpyAsync(t.last_temp, t.temp_init, np * 8, hipMemcpyDeviceToDevice, c->stream));
    // the temperature until fx_nl_set_temperature gives one: the initial condition, or without one REF_TEMP (fstr_setup.f90:780)
    if (v->temp_init) HIP_TRY(hipMemcpyAsync(t.temp, t.temp_init, np * 8, hipMemcpyDeviceToDevice, c->stream));
    else HIP_TRY(hipMemcpyAsync(t.temp, ref.data(), np * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(t.alpha, v->alpha, (size_t)n.n_mat * 8, hipMemcpyHostToDevice, c->stream));
    if (!tabs.empty()) HIP_TRY(hipMemcpyAsync(t.tabs, tabs.data(), tabs.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(t.tab_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(t.mtab, mtab.data(), mtab.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // tabs and idx are host temporaries
    return 0;
  };
  if (int rc = up()) { nl_thermal_free(t); return rc; }
  t.on = true;
  t.ref_temp = v->ref_temp;
  nl_thermal_free(n.th);
  n.th = t;
  return 0;
}
#define NL_THERMAL_ON(name)                                                                                  \
  NL_READY(name);                                                                                            \
  if (!c->nl.th.on) return fx_fail(name, FX_ERROR_RUNTIME, "thermal strain is off: call fx_nl_set_thermal first"); \
  if (!temp) return fx_fail(name, FX_ERROR_RUNTIME, "temperature array missing")
static int nl_copy_temp(fx_context *c, void *dst, const void *src, hipMemcpyKind kind) {
  HIP_TRY(hipMemcpyAsync(dst, src, (size_t)c->A.NP * 8, kind, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int fx_nl_set_temperature(fx_context *c, const double *temp) {
  NL_THERMAL_ON("fx_nl_set_temperature");
  return nl_copy_temp(c, c->nl.th.temp, temp, hipMemcpyHostToDevice);
}
extern "C" int fx_nl_get_last_temp(fx_context *c, double *temp) {
  NL_THERMAL_ON("fx_nl_get_last_temp");
  return nl_copy_temp(c, temp, c->nl.th.last_temp, hipMemcpyDeviceToHost);
}
extern "C" int fx_nl_set_last_temp(fx_context *c, const double *temp) {
  NL_THERMAL_ON("fx_nl_set_last_temp");
  return nl_copy_temp(c, c->nl.th.last_temp, temp, hipMemcpyHostToDevice);
}

// ---- time-dependent materials (see the header)
extern "C" int fx_nl_set_time(fx_context *c, double time, double tincr) {
  NL_READY("fx_nl_set_time");
  return nl_apply_time(c, "fx_nl_set_time", time, tincr);
}
// fstatus(1) of the NORTON points is in the context's fstat array and in component 0 of the history: after a transfer into one, the other
static int nl_creep_fstat(fx_context *c, int to_fstat) {
  NlDev &n = c->nl;
  if (!n.has_creep) return 0;
  for (const NlPart &p : n.parts) {
    const int64_t npt = (int64_t)p.nq * p.n_elem;
    hipLaunchKernelGGL(k_nl_creep_fstat, dim3(grid_for(npt)), dim3(256), 0, c->stream, npt, p.nq, n.mat, (const NlMat *)n.mats,
                       (const int32_t *)p.emat, n.st.fstat + p.pt_off, nl_part_hist(n, p), to_fstat);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
// fstatus(1..W) of every point, [point][W] on the host side; the device keeps it component-major (fx_visco.h)
static int nl_copy_history(fx_context *c, const char *who, double *hist, int32_t *width, bool to_device) {
  NlDev &n = c->nl;
  if (width) *width = n.hist_w;
  if (!hist || n.hist_w == 0) return 0;
  const size_t npt = (size_t)n.n_pt, W = (size_t)n.hist_w;
  std::vector<double> t(W * npt);
  if (to_device) {
    for (size_t p = 0; p < npt; p++)
      for (size_t k = 0; k < W; k++) t[k * npt + p] = hist[p * W + k];
    HIP_TRY(hipMemcpyAsync(n.hist, t.data(), t.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (int rc = nl_creep_fstat(c, 1)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  }
  HIP_TRY(hipMemcpyAsync(t.data(), n.hist, t.size() * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t p = 0; p < npt; p++)
    for (size_t k = 0; k < W; k++) hist[p * W + k] = t[k * npt + p];
  return 0;
}
extern "C" int fx_nl_get_history(fx_context *c, double *hist, int32_t *width) {
  NL_READY("fx_nl_get_history");
  return nl_copy_history(c, "fx_nl_get_history", hist, width, false);
}
extern "C" int fx_nl_set_history(fx_context *c, const double *hist, int32_t width) {
  NL_READY("fx_nl_set_history");
  if (width != c->nl.hist_w)
    return fx_fail("fx_nl_set_history", FX_ERROR_RUNTIME, "width %d, the context's history has %d components per point", (int)width,
                   (int)c->nl.hist_w);
  return nl_copy_history(c, "fx_nl_set_history", const_cast<double *>(hist), nullptr, true);
}

// Element-level outputs of the two kernels (tests): tangents ke (per element 3 nn x 3 nn row-major) of the current state
// with u = unode + dunode, or the stress update with per-element internal forces qf (3 nn per element), no scatter; the parts
// one after the other.
extern "C" int fx_nl_element_tangents(fx_context *c, double *ke) {
  NL_READY("fx_nl_element_tangents");
  NlDev &n = c->nl;
  DevScratch tmp;
  double *d = nullptr;
  const size_t nk = n.n_k;
  if (tmp.alloc(&d, nk)) return FX_ERROR_RUNTIME;
  if (nl_update_err_clear(c)) return FX_ERROR_RUNTIME;
  if (nl_launch_stiffness(c, d)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ke, d, nk * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return nl_update_err_check(c);
}
extern "C" int fx_nl_element_update(fx_context *c, double *qf) {
  NL_READY("fx_nl_element_update");
  NlDev &n = c->nl;
  DevScratch tmp;
  double *d = nullptr;
  const size_t nqf = n.n_qf;
  if (tmp.alloc(&d, nqf)) return FX_ERROR_RUNTIME;
  if (int rc = nl_run_update(c, d)) return rc;
  HIP_TRY(hipMemcpyAsync(qf, d, nqf * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// One substep of fstr_Newton (fstr_solve_NonLinear.f90:29-167) around fx_solve_resident.
//   factor0/factor1: load factors at the start / end of the increment (fstr_solve_NLGEOM.f90:112-115);
//   bc_val, cload: values at load factor 1.  log: 7 doubles per Newton iteration
//   (iter, linear-solver iterations, solver return code, |B|, |X|, |QFORCE|, |dunode|).
// Returns 0 when the substep converged, FX_ERROR_NOCONV_MAXIT when max_iter ran out (the reference cuts back;
// the state is committed as fstr_Newton's caller would after its last iteration only on convergence).
extern "C" int fx_newton_substep(fx_context *c, double factor0, double factor1, int32_t n_bc, const int32_t *bc_node,
                                 const int32_t *bc_dof, const double *bc_val, const double *cload, int32_t max_iter, double converg,
                                 int32_t *Iarray, double *Rarray, double *log, int32_t *n_iter, int commit_unconverged) {
  NL_READY("fx_newton_substep");
  if (max_iter < 1) { g_fx_error = "fx_newton_substep: max_iter must be >= 1"; return FX_ERROR_RUNTIME; }
  const size_t np3 = (size_t)3 * c->A.NP;
  std::vector<double> gl, inc((size_t)std::max(n_bc, 1)), zero((size_t)std::max(n_bc, 1), 0.0);
  if (cload) {
    gl.resize(np3);
    for (size_t i = 0; i < np3; i++) gl[i] = cload[i] * factor1;
  }
  for (int32_t k = 0; k < n_bc; k++) inc[k] = bc_val[k] * (factor1 - factor0);
  if (c->nl.dl.on) c->nl.dl.factor = factor1;  // fstrSOLID%factor(2)
  int e = fx_nl_begin_substep(c, cload ? gl.data() : nullptr);
  if (e) return e;
  bool done = false, blown = false;
  int32_t it = 0;
  for (it = 1; it <= max_iter; it++) {
    e = fx_nl_stiffness(c, n_bc, bc_node, bc_dof, it == 1 ? inc.data() : zero.data(), nullptr);
    if (e) return e;
    Iarray[96] = (it == 1) ? 2 : 1;  // Iarray(97): force / need numerical factorisation (:82-86)
    HIP_TRY(hipMemsetAsync(c->A.X, 0, np3 * 8, c->stream));
    fx_solve_info info;
    memset(&info, 0, sizeof info);
    const int code = fx_solve_resident(c, Iarray, Rarray, &info, nullptr, 0);
    if (code < 0 || code == FX_ERROR_ZERO_DIAG || code == FX_ERROR_INCONS_PC) return code;
    double nrm[4];
    e = fx_nl_update(c, nrm, nullptr);
    if (e) return e;
    const double res = sqrt(nrm[0]), xnrm = sqrt(nrm[1]);
    double qnrm = sqrt(nrm[2]);
    if (qnrm < 1.0e-8) qnrm = 1.0;
    const double dunrm = (it == 1) ? xnrm : sqrt(nrm[3]);
    if (log) {
      double *l = log + (size_t)7 * (it - 1);
      l[0] = it; l[1] = info.iterations; l[2] = code; l[3] = res; l[4] = xnrm; l[5] = qnrm; l[6] = dunrm;
    }
    if (c->nl.is_linear) { done = true; break; }  // `if( isLinear ) exit` (:107): a linear analysis takes one pass, no convergence test
    if (Iarray[80] == 1) {  // hecmw_mat_get_flag_converged (:132-135)
      if (res / qnrm < converg) done = true;
      if (xnrm / dunrm < converg) done = true;
    }
    if (done) break;
    if (res / qnrm > c->nl.maxres) { blown = true; break; }  // `rres > maxres` (:140): give up at once, the caller cuts back (knstDRESN = 2)
  }
  if (n_iter) *n_iter = std::min(it, max_iter);
  if (blown) return FX_NEWTON_MAXRES;  // like the reference's `return`: nothing is committed
  if (done || commit_unconverged) {
    e = fx_nl_commit(c);
    if (e) return e;
  }
  return done ? 0 : FX_ERROR_NOCONV_MAXIT;
}

// step_ctrl(cstep)%maxres (m_step.f90:31, default 1.d+10 :78) and fstr_Newton's isLinear (.not. fstrPR%nlgeom, :50-51).
extern "C" int fx_nl_set_step_control(fx_context *c, double maxres, int is_linear) {
  c->nl.maxres = maxres > 0.0 ? maxres : 1.0e10;
  c->nl.is_linear = is_linear != 0;
  return 0;
}
