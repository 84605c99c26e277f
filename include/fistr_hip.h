/* fistr_hip.h -- C ABI of the MI355X-native HEC-MW linear-solve hot path.
 *
 * Drop-in boundary.  The reference exposes Fortran module
 * procedures only; the entry points below are what a thin Fortran shim
 * (frontistr_amd/shim/hecmw_solver_hip.f90) binds with
 * bind(C) after taking c_loc() of the members of hecmwST_matrix /
 * hecmwST_local_mesh.  Plain pointers and sizes only.
 *
 * Conventions are the reference's (hecmw1/src/common/hecmw_util_f.F90:15-16,
 * :433-468): int32 indices, 1-based `item` arrays, `index` arrays with NP+1
 * entries starting at 0, fp64 values, 3x3 blocks row-major (A(9j-8..9j) = row 1,
 * row 2, row 3 of block j).
 *
 * All functions return 0 on success, a HEC-MW solver code (fx_status) for the
 * conditions the reference reports through hecmw_solve_error
 * (hecmw1/src/solver/init/hecmw_solve_error.f90:9-15), or a negative value for
 * a HIP/RCCL runtime failure (fx_last_error() then holds the message).
 */
#ifndef FISTR_HIP_H
#define FISTR_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* hecmw_solve_error.f90:9-15 */
enum fx_status {
  FX_OK = 0,
  FX_ERROR_INCONS_PC = 1001,    /* E: inconsistent solver/preconditioner        */
  FX_ERROR_ZERO_DIAG = 2001,    /* E: zero component in diagonal block          */
  FX_ERROR_ZERO_RHS = 2002,     /* W: zero RHS norm (X = 0 is returned)         */
  FX_ERROR_NOCONV_MAXIT = 3001, /* W: not converged within ceratin iterations   */
  FX_ERROR_DIVERGE_MAT = 3002,  /* W: diverged due to indefinite/neg-def matrix */
  FX_ERROR_DIVERGE_PC = 3003,   /* W: diverged due to indefinite preconditioner */
  FX_NEWTON_MAXRES = 4002,      /* fx_newton_substep: NR residual above step_ctrl%maxres (knstDRESN = 2): cut back */
  FX_ERROR_RUNTIME = -1,        /* HIP / RCCL failure, see fx_last_error()      */
  FX_ERROR_UNSUPPORTED = -2     /* NDOF outside 1..6, or an option outside the hot path */
};

/* Borrowed view of hecmwST_matrix (hecmw_util_f.F90:433-468).  The caller owns
 * every array (m_fstr.f90:807-857 allocates them once); the library writes X
 * (all 3*NP entries, halo included: hecmw_solver_CG.f90:280) and never frees or
 * reallocates anything. */
typedef struct fx_matrix_view {
  int32_t N, NP, NPL, NPU, NDOF;
  const int32_t *indexL, *itemL; /* (0:NP), (NPL) */
  const int32_t *indexU, *itemU; /* (0:NP), (NPU) */
  const double *D, *AL, *AU;     /* NDOF^2 * NP, NPL, NPU (row-major NDOF x NDOF blocks) */
  const double *B;               /* NDOF*NP */
  double *X;                     /* NDOF*NP, in: initial guess, out: solution */
} fx_matrix_view;

/* Borrowed view of the communication part of hecmwST_local_mesh
 * (hecmw_util_f.F90:298-310).  Serial runs pass n_neighbor_pe = 0 and PETOT = 1
 * (or a NULL pointer). */
typedef struct fx_comm_view {
  int32_t my_rank, PETOT, nn_internal, n_node;
  int32_t n_neighbor_pe;
  const int32_t *neighbor_pe;  /* ranks, 0-based as in HEC-MW */
  const int32_t *import_index; /* (0:n_neighbor_pe) */
  const int32_t *import_item;  /* 1-based local node ids (> nn_internal) */
  const int32_t *export_index; /* (0:n_neighbor_pe) */
  const int32_t *export_item;  /* 1-based local node ids (<= nn_internal) */
} fx_comm_view;

/* What the reference prints / keeps per solve (hecmw_solver_Iterative.f90:192-208). */
typedef struct fx_solve_info {
  int32_t iterations;     /* ITER as in the '### summary of linear solver' line        */
  int32_t method, precond;
  int32_t ncolor;         /* SSOR: number of colours actually used                     */
  int32_t n_hist;         /* residual-history entries written                          */
  double resid;           /* RESID of the last iteration (sqrt(DNRM2/BNRM2))           */
  double rel_resid;       /* final ||b-Ax||/||b|| (hecmw_rel_resid_L2)                 */
  double time_setup, time_sol, time_comm, time_matvec, time_precond; /* seconds       */
} fx_solve_info;

typedef struct fx_context fx_context; /* device state the reference keeps in module `save` data */

/* ---- life cycle ------------------------------------------------------- */
/* device < 0: use LOCAL_RANK (or 0).  One context per MPI rank / subdomain. */
int fx_create(int device, fx_context **out);
void fx_destroy(fx_context *ctx);
const char *fx_last_error(void);
const char *fx_version(void);
int fx_device_synchronize(fx_context *ctx);

/* ---- the drop-in pair --------------------------------------------------- */
/* hecmw_solve(hecMESH, hecMAT), hecmw1/src/solver/hecmw_solver.f90:9 ->
 * hecmw_solve_iterative, iterative/hecmw_solver_Iterative.f90:13.
 * Iarray/Rarray are hecMAT%Iarray/Rarray (slot map hecmw_matrix_misc.f90:89-121);
 * on return Iarray(81) converged, (82) diverged, (96) nrecycle, (97),(98) are
 * updated exactly as the reference does.  hist (may be NULL) receives RESID per
 * iteration = the ITERLOG channel (hecmw_solver_CG.f90:245), at most hist_len.
 * METHOD Iarray(2): 1 CG (hecmw_solver_CG.f90:19), 2 BiCGSTAB (hecmw_solver_BiCGSTAB.f90:16),
 * 3 GMRES(NREST=Iarray(6)) (hecmw_solver_GMRES.f90:17), 4 GPBiCG (hecmw_solver_GPBiCG.f90:17);
 * PRECOND Iarray(3): 1,2 SSOR, 3 DIAG (block Jacobi), 10 ILU(0); anything else E-1001.
 * SCALING Iarray(7) /= 0: symmetric diagonal scaling around every attempt (las/hecmw_solver_scaling_33.f90);
 * SIGMA_DIAG Rarray(2) < 0: the reference's automatic retry for the ILU family; METHOD2 Iarray(8) take-over.
 * NDOF = 3 is the tuned path.  NDOF = 1, 2, 4, 5, 6 (hecmw_matvec_nn las_nn.f90:135, precond/nn + 11/22/44/66) take the
 * generic-block path: METHOD 1-4; PRECOND 1, 2, 3, and 10 (block ILU(0), with the SIGMA_DIAG retry) for NDOF 4, 5, 6;
 * SCALING; anything else (PRECOND 11 / 12 at any size, 10 with NDOF 1 or 2) E-1001 / FX_ERROR_UNSUPPORTED. */
int fx_solve(fx_context *ctx, const fx_matrix_view *mat, const fx_comm_view *comm, int32_t *Iarray,
             double *Rarray, fx_solve_info *info, double *hist, int32_t hist_len);

/* hecmw_matvec(hecMESH, hecMAT, X, Y, COMMtime), las/hecmw_solver_las.f90:57:
 * halo update of X (X's halo part is written, as hecmw_update_3_R does), then
 * Y(1:NDOF*N) = (D + AL + AU) X.  x, y are host arrays of NDOF*NP doubles.  The reference's hecmw_matvec has no
 * "matrix changed" flag and its external callers modify hecMAT between calls, so the values in `mat` are uploaded on every
 * call; mat->D == NULL means "the resident values" (repeated products with one matrix: no PCIe traffic but x and y). */
int fx_matvec(fx_context *ctx, const fx_matrix_view *mat, const fx_comm_view *comm, double *x,
              double *y, double *commtime);

/* ---- staged, device-resident form (what fx_solve is made of) ------------ */
/* Upload / refresh the system.  what: bit 0 profile (Iarray(98) semantics),
 * bit 1 values (Iarray(97)), bit 2 B, bit 3 X. */
enum { FX_UP_PROFILE = 1, FX_UP_VALUES = 2, FX_UP_RHS = 4, FX_UP_X = 8, FX_UP_ALL = 15 };
int fx_upload(fx_context *ctx, const fx_matrix_view *mat, const fx_comm_view *comm, int what);
/* hecmw_precond_setup, precond/hecmw_precond.f90:28-50 (DIAG_33 / SSOR_33 / BILU_33). */
int fx_precond_setup(fx_context *ctx, const int32_t *Iarray, const double *Rarray);
/* hecmw_solve_CG / hecmw_solve_BiCGSTAB on the resident system; no host<->device
 * traffic except the status word.  This is the region bench.py times. */
int fx_solve_resident(fx_context *ctx, int32_t *Iarray, double *Rarray, fx_solve_info *info,
                      double *hist, int32_t hist_len);
/* The same loop in pieces, for callers that time an exact number of iterations:
 * begin = r0 = b - A x0 and ||b|| (hecmw_solver_CG.f90:120-129); steps = enqueue up to
 * nsteps iterations (never past Iarray(1)) and return the device state after them
 * (iter = Fortran ITER, status 0 = still running, 1 = converged, else an fx_status). */
int fx_krylov_begin(fx_context *ctx, const int32_t *Iarray, const double *Rarray);
int fx_krylov_steps(fx_context *ctx, int32_t nsteps, int32_t *iter, int32_t *status, double *resid);
/* The ITERLOG lines of the staged loop (hecmw_solver_CG.f90:245: RESID per iteration, line i = iteration i) executed since
 * fx_krylov_begin: *n_lines = lines written so far, at most cap of them copied to hist. */
int fx_krylov_history(fx_context *ctx, double *hist, int32_t cap, int32_t *n_lines);
int fx_download_x(fx_context *ctx, double *X, int32_t n);          /* 3*NP doubles */
int fx_download_matrix(fx_context *ctx, double *D, double *AL, double *AU, double *B);
/* Resident single operations (tests, roofline timing). */
int fx_matvec_resident(fx_context *ctx, int nrepeat, float *ms_per_call); /* y = A x on work vectors */
/* The same with the launch variant chosen: 0 plain (hecmw_solver_BiCGSTAB.f90:184, :210), 1 fused partial of x.y (the
 * product of every CG iteration, hecmw_solver_CG.f90:204-211), 2 r = b - A x with the partial of r.r (hecmw_matresid,
 * las/hecmw_solver_las.f90:105-122).  HIP events on the solver stream; one untimed call first.  The product reads and
 * writes the work vectors the CG loop multiplies (p and q) and overwrites them: not to be called while a Krylov loop is
 * between fx_krylov_begin and its last step. */
int fx_spmv_resident(fx_context *ctx, int variant, int nrepeat, float *ms_per_call);
/* The same for the resident NDOF != 3 system of the last fx_solve / fx_matvec (hecmw_matvec_nn, las_nn.f90:135-310).
 * stats: NDOF, N, padded blocks of the layout, blocks of the matrix (N + NPL + NPU). */
int fx_nn_matvec_resident(fx_context *ctx, int nrepeat, float *ms_per_call, int64_t stats[4]);
/* hecmw_precond_setup + hecmw_precond_apply (hecmw_precond.f90:28, :75-123) for an NDOF != 3 system: uploads `mat`, sets up
 * the preconditioner Iarray / Rarray select (or reuses the resident one, with the flags and SIGMA_DIAG fx_solve reads), then
 * z = M^-1 r with iterPREmax = Iarray(5).  r, z: host arrays of NDOF*NP doubles; r's halo part is ignored (ZP(halo) = 0),
 * z's is 0. */
int fx_nn_precond_apply(fx_context *ctx, const fx_matrix_view *mat, const fx_comm_view *comm, int32_t *Iarray,
                        double *Rarray, const double *r, double *z);
/* Timed applies of the resident NDOF != 3 preconditioner on resident work vectors (HIP events, one untimed call first). */
int fx_nn_precond_apply_resident(fx_context *ctx, int nrepeat, float *ms_per_call);
/* out[0..9]: kind (1 SSOR, 3 DIAG, 10 block ILU(0), 0 none) | levels or colours | sweep slices | longest L + U row (ILU) |
 * factor kernel lanes per row, 32 or 1 (ILU) | padded L blocks | padded U blocks | last ILU set-up, microseconds |
 * ILU sweep form: 1 one persistent dataflow launch per apply (FX_DATAFLOW >= 1), 0 one launch per level (FX_DATAFLOW=0, or
 * after a dataflow sweep timed out) | workgroups of the last dataflow launch (bits 0-31), timed-out sweeps (bits 32-63).
 * The dataflow sweep honours FX_DATAFLOW, FX_DF_GRID and FX_DEBUG_DF_FAIL, none of the other FX_DF_* settings. */
int fx_nn_precond_stats(fx_context *ctx, int64_t out[10]);
int fx_precond_apply_resident(fx_context *ctx, int nrepeat, float *ms_per_call); /* z = M^-1 b, timed */
int fx_precond_apply_host(fx_context *ctx, const double *r, double *z);   /* z = M^-1 r, 3*NP doubles */
/* out[0..14]: N NP NPL NPU | M pairs, blocks, slices | ncolor | L pairs, blocks | U pairs, blocks | slices |
 * SpMV workgroups overlapped with the halo exchange (interior), ordered after it (boundary) | [15] bit 0: the last Krylov
 * loop ran in Eisenstat's form (the default for CG + multicolour SSOR, FX_EISENSTAT=0 opts out); bit 1: the ILU(0) sweeps are chain sweeps (FX_DATAFLOW=3) */
int fx_get_stats(fx_context *ctx, int64_t out[16]);
/* The dataflow tail of the Eisenstat sweeps (FX_DATAFLOW >= 1, one rank, CG + multicolour SSOR in Eisenstat's form): the colours at
 * the end of the colour order with at most 4 x G slices each, G the co-resident grid of the tail kernels, run as ONE launch per half
 * sweep instead of one per colour; bit-identical to FX_DATAFLOW=0.  out[0] first tail colour of the last iteration (== ncolor: no
 * tail), [1] its slices, [2] workgroups of the backward tail launch, [3] tail launches enqueued or captured by this context,
 * [4] colours, [5] G.  A tail launch that times out raises the same fallback as the other dataflow sweeps (df_fallbacks). */
int fx_eis_tail_stats(fx_context *ctx, int64_t out[6]);
/* Where the value arrays of the sliced layouts live: out[0] bytes of the context's value arena (one large allocation taken when the
 * size of a large system first becomes known, before anything else of it: 0 = none), [1] bytes in use, [2] arrays placed in it,
 * [3..5] 1 if the value array of the SpMV layout / the lower / the upper sweep layout lies in it, [6] bytes of the SpMV layout's
 * value array, [7] arenas the one-off verification timed (the loop's SpMV on the arena, 5 ms; a slow one is replaced by another arena,
 * at most FX_ARENA_TRIES = 4, the fastest kept), [8] the SpMV's ms on the arena kept.  FX_ARENA_GB (0 = off, default 32 = at least 32 GiB). */
int fx_placement_report(fx_context *ctx, double out[9]);
/* The plane march of the level-scheduled sweeps (ILU(0) hecmw_precond_BILU_33.f90:90-157, natural-order SSOR
 * hecmw_precond_SSOR_33.f90:300-410; csrc/fx_march.h): out[0] 1 if this context's preconditioner has the march programs, [1] rows per
 * chunk, [2] chunks, [3] pair waves per workgroup, [4] / [5] rounds of the forward / backward program, [6] blocks gathered from the LDS
 * ring, [7] from memory, [8] of those in the row's own chunk, [9] / [10] the cost model's microseconds per half sweep as a march / as
 * dependency levels, [11] seconds the build took, [12] applies that took the march, [13] workgroups of the last launch, [14] rows of the
 * largest round, [15] dependency levels.  FX_MARCH = 0 off, 1 (default) when the cost model prefers it, 2 whenever the structure admits it. */
int fx_march_report(fx_context *ctx, double out[16]);
/* Host-only (no device): plan the two march programs for a block profile (indexL / itemL / indexU / itemU as hecMAT's, 1-based items, N
 * internal rows) with `chunk` rows per chunk and `waves` pair waves (1, 2, 3), replay them on the host and report: out[0] 1 = both programs
 * pass their replay (every in-chunk dependency found in its ring slot, every other one produced by an earlier chunk or round), 0 = the
 * structure is not admitted (a row with more than 14 lower or upper blocks), [1] chunks, [2] / [3] rounds forward / backward, [4] / [5]
 * blocks gathered from the ring / from memory (forward), [6] rows of the largest round, [7] dependency levels of the matrix. */
int fx_march_plan(int32_t N, const int32_t *indexL, const int32_t *itemL, const int32_t *indexU, const int32_t *itemU, int32_t chunk,
                  int32_t waves, double out[8]);
/* The passes of the auto-SIGMA_DIAG / METHOD2 loop of the last solve on this context (hecmw_solver_Iterative.f90:117-157: banner
 * :125 before every pass, 'Increasing SIGMA_DIAG to' :149 before a retry): METHOD, the SIGMA_DIAG in effect and the number of
 * residual-history lines of every pass, and the lines themselves.  fx_solve's own `hist` holds the LAST pass. */
int fx_solve_attempts(fx_context *ctx, int32_t cap, int32_t *n_attempts, int32_t *method, double *sigma_diag, int32_t *n_hist);
int fx_solve_attempt_history(fx_context *ctx, int32_t attempt, double *hist, int32_t cap);
/* Tuning knob of a live context (kernel variants, workgroup sizes, sweep modes: the FX_* names documented in
 * frontistr_amd/csrc/fx_internal.h; the same names are read from the environment at fx_create).  No counterpart in the
 * reference (its equivalents are build-time choices such as the OpenMP thread count).  Unknown name: FX_ERROR_UNSUPPORTED.
 * A knob changed on a live context gives the answer a fresh context created with it gives: kernel choices take effect at the next
 * apply / product / solve (a solve captures its graph again at its begin), layout choices (FX_SPMV_BS, FX_SPMV_SPATIAL,
 * FX_LAYOUT_DEVICE) leave every row's sum unchanged, and the one numbering choice, FX_SSOR_MODE, takes effect at the next
 * fx_precond_setup: changing it invalidates a resident multicolour SSOR, which the next solve or fx_precond_setup rebuilds in the
 * new numbering (fx_precond_apply_* report it as not set up until then).  FX_DATAFLOW allocates the private backward vector the
 * dataflow sweeps need when the resident preconditioner was set up without it. */
int fx_set_option(fx_context *ctx, const char *name, double value);
/* measured read-streaming rate (GB/s) of this device over the resident matrix values: the on-box
 * ceiling reported beside the 8 TB/s vendor peak */
int fx_stream_ceiling(fx_context *ctx, int nrepeat, double *gbs);
/* diagnostics: rho rho1 beta c1 alpha omega c2 cg0 cg1 dnrm2 bnrm2 resid tol iter status need_verify */
int fx_debug_state(fx_context *ctx, double out[16]);
int fx_dot_host(fx_context *ctx, const double *x, const double *y, double *result);

/* ---- assembly side ------------------------------------------------------ */
/* hecmw_mat_con, matrix/hecmw_mat_con.f90:23: CRS block profile from element
 * connectivity (conn 1-based, nn nodes per element).  Two-call protocol: with
 * itemL == NULL only indexL/indexU (NP+1 each) are filled. */
int fx_mat_con(int32_t NP, int32_t n_elem, int32_t nn, const int32_t *conn, int32_t *indexL,
               int32_t *indexU, int32_t *itemL, int32_t *itemU);

/* Host only: the ordering of the multicolour SSOR as the library computes it (reference: hecmw_precond_SSOR_33.f90:102-111 ->
 * hecmw_matrix_ordering_CM.f90:16-178 "RCM" + hecmw_matrix_ordering_MC.f90:15-72 greedy capped multicolouring; the path the
 * reference takes with more than one OpenMP thread).  perm: N entries, new -> old, 1-based; colorindex: COLORindex(0:ncolor). */
int fx_ssor_ordering(int32_t N, const int32_t *indexL, const int32_t *itemL, const int32_t *indexU, const int32_t *itemU,
                     int32_t ncolor_in, int32_t *perm, int32_t *colorindex, int32_t colorindex_cap, int32_t *ncolor);

/* The same two arrays as the resident preconditioner was built with (large systems run the level ordering on the device). */
int fx_get_ssor_ordering(fx_context *ctx, int32_t *perm, int32_t *colorindex, int32_t colorindex_cap, int32_t *ncolor);

/* Host only: the element colouring behind the atomic-free stiffness scatter (no two elements of a colour share a node;
 * the reference serialises the same conflicts with `!$omp atomic`, hecmw_mat_ass.f90:72-134).  order: n_elem element ids
 * (0-based) grouped by colour; offsets: 65 entries, offsets[k]..offsets[k+1] = colour k; *ncolor = 0 when a node belongs
 * to more than 64 elements (the device then falls back to atomics). */
int fx_color_elements(int32_t NP, int32_t n_elem, int32_t nn, const int32_t *conn, int32_t *order, int32_t *offsets,
                      int32_t *ncolor);

/* fstr_StiffMatrix (fistr1/src/analysis/static/fstr_StiffMatrix.f90:18-212) for one
 * TYPE=361 element group with one isotropic linear-elastic material, then
 * hecmw_mat_ass_bc (matrix/hecmw_mat_ass.f90:292) for the listed dofs:
 * element stiffness (elemopt 1 = C3D8 incompatible modes STF_C3D8IC, 2 = B-bar
 * STF_C3D8Bbar, 3 = full integration STF_C3) and scatter-add run on the device
 * into the resident D/AL/AU; `load` (3*NP, may be NULL) becomes B.
 * Requires a profile uploaded with fx_upload(..., FX_UP_PROFILE). */
typedef struct fx_mesh_view {
  int32_t n_node, n_elem;
  const double *coord;  /* 3*n_node, hecMESH%node */
  const int32_t *conn;  /* nn*n_elem (8 at 361, 4 at 341, 10 at 342, 6 at 351, 15 at 352, 20 at 362), 1-based, hecMESH%elem_node_item */
} fx_mesh_view;
int fx_assemble_c3d8(fx_context *ctx, const fx_mesh_view *mesh, double E, double nu, int elemopt,
                     const double *load, int32_t n_bc, const int32_t *bc_node,
                     const int32_t *bc_dof, const double *bc_val, float *ms_assemble);
/* The same for a group whose elements belong to several sections / materials (hecMESH%section_ID ->
 * fstrSOLID%materials, fstr_setup.f90:325-400): elem_mat[e] in 1..n_mat selects (E[m-1], nu[m-1]). */
int fx_assemble_c3d8_sections(fx_context *ctx, const fx_mesh_view *mesh, int32_t n_mat, const double *E,
                              const double *nu, const int32_t *elem_mat, int elemopt, const double *load,
                              int32_t n_bc, const int32_t *bc_node, const int32_t *bc_dof,
                              const double *bc_val, float *ms_assemble);
/* fstr_UpdateNewton of a LINEAR static analysis (`!SOLUTION, TYPE=STATIC`; fistr1/src/analysis/static/fstr_Update.f90:25-293) for
 * one TYPE=361 group of isotropic ELASTIC materials: UpdateST_C3D8IC (static_LIB_3dIC.f90:220-455, elemopt 1), Update_C3D8Bbar
 * (static_LIB_C3D8.f90:203-547, elemopt 2) or UPDATE_C3 (static_LIB_3d.f90:516-837, elemopt 3) per element, small strain.
 * disp = total displacement unode + dunode (3*n_node).  *strain, *stress: pinned host arrays OWNED BY THE CONTEXT, valid until the
 * next update or prepare ON THE SAME CONTEXT or fx_destroy (other contexts have their own staging), [n_elem][8][6] = gausses(1:8)%strain(1:6) / %stress(1:6) of every element; qforce (3*n_node, caller's, may be NULL) =
 * fstrSOLID%QFORCE before its halo update.  n_mat materials, elem_mat 1-based per element (NULL with one material). */
int fx_update_c3d8_linear(fx_context *ctx, const fx_mesh_view *mesh, int32_t n_mat, const double *E, const double *nu,
                          const int32_t *elem_mat, int elemopt, const double *disp, const double **strain,
                          const double **stress, double *qforce, float *ms_kernel);
/* Optional: start pinning the context's host staging of fx_update_c3d8_linear for n_elem elements on a helper thread and return
 * at once.  Pointers that an earlier update on this context returned are no longer valid after it. */
int fx_update_c3d8_linear_prepare(fx_context *ctx, int32_t n_elem);
/* One element stiffness through the device kernel (tests): ecoord 8x3, stiff 24x24 row-major. */
int fx_element_stiffness_c3d8(fx_context *ctx, int elemopt, const double *ecoord, double E, double nu,
                              double *stiff);

/* Tetrahedra, wedges and 20-node hexahedra: fstr_StiffMatrix + hecmw_mat_ass_bc for one group of elements of one of the
 * types that fstr_StiffMatrix.f90:134-144 sends through STF_C3 (static_LIB_3d.f90:47-205), FrontISTR's node order:
 *   TYPE=341  4 nodes,  1 quadrature point      TYPE=351  6 nodes,  2 points      TYPE=362  20 nodes, 27 points
 *   TYPE=342 10 nodes,  4 points                TYPE=352 15 nodes,  9 points
 * small strain, isotropic ELASTIC; element stiffness and the coloured scatter run on the device into the resident D/AL/AU
 * as for fx_assemble_c3d8.  mesh->conn holds that many node ids per element.  n_mat materials (E[m-1], nu[m-1]); elem_mat
 * (1-based per element) may be NULL with one material.  An element that names a node twice (degenerate) is refused
 * (FX_ERROR_RUNTIME, nothing assembled); any other etype: FX_ERROR_UNSUPPORTED. */
int fx_assemble_c3(fx_context *ctx, const fx_mesh_view *mesh, int32_t etype, int32_t n_mat, const double *E,
                   const double *nu, const int32_t *elem_mat, const double *load, int32_t n_bc,
                   const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val, float *ms_assemble);
/* fstr_UpdateNewton of a linear static analysis for one group of the same types: UPDATE_C3 (static_LIB_3d.f90:516-837), small
 * strain.  As fx_update_c3d8_linear, with *strain, *stress [n_elem][nq][6] (nq = the type's quadrature points: 1, 4, 2, 9,
 * 27) in the context's pinned staging, valid until the next update or prepare on the same context or fx_destroy. */
int fx_update_c3_linear(fx_context *ctx, const fx_mesh_view *mesh, int32_t etype, int32_t n_mat, const double *E,
                        const double *nu, const int32_t *elem_mat, const double *disp, const double **strain,
                        const double **stress, double *qforce, float *ms_kernel);
/* One element's stiffness through the device kernel (tests), etype as above: ecoord nn x 3, stiff (3 nn) x (3 nn) row-major. */
int fx_element_stiffness_c3(fx_context *ctx, int32_t etype, const double *ecoord, double E, double nu, double *stiff);

/* A mesh of several solid element types: fstr_StiffMatrix's loop over itype (fstr_StiffMatrix.f90:43-212) restated.
 * hecMESH%elem_node_item holds the elements type by type (elem_type_index / elem_type_item), so a group is a pointer into it
 * and its element count; nothing is copied or re-sorted by the caller.  A type may appear in several groups, and 361 groups
 * may differ in elemopt. */
typedef struct fx_elem_group {
  int32_t etype;           /* 361, 341, 342, 351, 352, 362 */
  int32_t elemopt;         /* 361 only: 1 IC, 2 B-bar, 3 FI, and for fx_nl_init_groups alone 4 F-bar; ignored otherwise */
  int32_t n_elem;
  const int32_t *conn;     /* nn(etype) * n_elem, 1-based */
  const int32_t *elem_mat; /* 1-based per element, may be NULL with one material */
} fx_elem_group;
/* All groups into the one resident matrix: cleared (or first-written) once, group after group in the order given, each group
 * colour by colour (no atomics, bitwise reproducible); `load` and the boundary conditions once after the last group
 * (hecmw_mat_ass_bc, matrix/hecmw_mat_ass.f90:292).  The colouring and the position map are kept per group and re-used by the
 * next call with the same groups.  fx_assemble_c3d8, fx_assemble_c3d8_sections and fx_assemble_c3 are this call with ONE group:
 * the same driver, the same argument checks (messages name the entry point called) and the same one cache per context, so
 * alternating different group sets on one context colours and maps again each time.
 * An unknown etype in any group: FX_ERROR_UNSUPPORTED; n_group < 1, missing materials, a material or node id out of range, a
 * degenerate element of a type other than 361 (named with its group and element): FX_ERROR_RUNTIME.  Nothing is assembled then. */
int fx_assemble_groups(fx_context *ctx, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                       int32_t n_mat, const double *E, const double *nu, const double *load, int32_t n_bc,
                       const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val, float *ms_assemble);
/* fstr_UpdateNewton's element loop (fstr_Update.f90:73-264) over the same groups.  strain[g], stress[g] (n_group pointers each,
 * the caller's arrays of pointers): group g's [n_elem][nq(etype)][6] in the context's pinned staging, valid until the next
 * update or prepare on the same context or fx_destroy; qforce (3*n_node, may be NULL) summed over all groups. */
int fx_update_groups_linear(fx_context *ctx, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                            int32_t n_mat, const double *E, const double *nu, const double *disp, const double **strain,
                            const double **stress, double *qforce, float *ms_kernel);
/* As fx_update_c3d8_linear_prepare, for the staging that fx_update_groups_linear needs for these groups (conn is not read). */
int fx_update_groups_linear_prepare(fx_context *ctx, int32_t n_group, const fx_elem_group *groups);

/* ---- thermal strain in the linear static paths (!TEMPERATURE, !REFTEMP, !INITIAL CONDITION TYPE=TEMPERATURE) ----
 * Every material carries ONE constant isotropic expansion coefficient (fstrSOLID%materials(m)%variables(M_EXAPNSION)); tables
 * of E, nu or the coefficient over temperature, MC_ORTHOEXP and section orientation are not restated: keep such decks on the host.
 * The stiffness matrix does not depend on the temperature then -- fstr_StiffMatrix.f90:72-73 passes it to the element routines
 * for table lookups only -- so fx_assemble_groups serves thermal decks unchanged and there is no thermal variant of it. */
typedef struct fx_thermal_view {
  const double *temp;   /* n_node: fstrSOLID%temperature */
  const double *temp0;  /* n_node: the reference state's, tt0 of fstr_Update.f90:92-102 (initial condition, or 0) */
  double ref_temp;      /* !REFTEMP */
  const double *alpha;  /* n_mat */
} fx_thermal_view;
/* The thermal load of fstr_ass_load.f90:287-428 for the solid types: TLOAD_C3D8IC / TLOAD_C3D8Bbar / TLOAD_C3 of every element,
 * ADDED to load_inout (3*n_node, host), so it composes with the `load` of fx_assemble_groups.  Elements that share a node add
 * with fp64 atomics (as QFORCE): equal to rounding from call to call, not bit for bit.  Errors as fx_assemble_groups, and a NULL
 * temperature array or NULL alpha: FX_ERROR_RUNTIME; load_inout is untouched on any error.  Needs no profile. */
int fx_thermal_load_groups(fx_context *ctx, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                           int32_t n_mat, const double *E, const double *nu, const fx_thermal_view *thermal,
                           double *load_inout, float *ms_kernel);
/* fx_update_groups_linear with the routines' thermal branches: stored strain = the total strain, stress = D (strain - EPSTH),
 * qforce from that stress; the IC element also subtracts its TLOAD_C3D8IC vector (static_LIB_3dIC.f90:337-342).  Same pinned
 * staging (valid until the next update or prepare on the same context or fx_destroy) and results layout.  With temp == temp0 == ref_temp everywhere the strain and
 * stress are those of fx_update_groups_linear. */
int fx_update_groups_linear_thermal(fx_context *ctx, int32_t n_node, const double *coord, int32_t n_group,
                                    const fx_elem_group *groups, int32_t n_mat, const double *E, const double *nu,
                                    const fx_thermal_view *thermal, const double *disp, const double **strain,
                                    const double **stress, double *qforce, float *ms_kernel);

/* ---- nonlinear static loop: the steps of fstr_Newton either side of the solve -------------
 * (fistr1/src/analysis/static/fstr_solve_NonLinear.f90:29-167).  One TYPE=361 group with the
 * B-bar formulation (the reference's default for NLSTATIC, fstr_setup.f90:366-368) and one
 * isotropic material: ELASTIC or Mises elastoplastic (!PLASTIC, YIELD=MISES) with BILINEAR /
 * MULTILINEAR / SWIFT / RAMBERG-OSGOOD isotropic hardening, INFINITE / TOTALLAG (KIRCHHOFF) /
 * UPDATELAG kinematics.  Everything stays resident: gauss-point history, unode/dunode, QFORCE.
 *
 * Hyperelastic materials (!HYPERELASTIC, fstr_ctrl_material.f90:166-255; Hyperelastic.f90): `plastic` is the material kind, 2 for
 * NEOHOOKE / MOONEYRIVLIN with plconst = C10, C01, D1 (Neo-Hooke: C01 = 0) and 3 for ARRUDABOYCE with plconst = mu, lambda_m, D.
 * E, nu, harden and tab are not read for them.  They need nlgeom = 1 (TOTALLAG, the card's default): the tangent comes from the
 * point's stored Green-Lagrange strain, the 2nd Piola-Kirchhoff stress from the total strain; no history, no latch.  Every
 * fx_nl_init* refuses with FX_ERROR_UNSUPPORTED: kind 2 / 3 with another nlgeom (CAUCHY -> UPDATELAG is a different algorithm in the
 * reference), plconst[2] == 0 ("cannot deal with incompressible"), Arruda-Boyce with plconst[1] == 0, and a Mises and a hyperelastic
 * material in one context.  A hyperelastic section beside ELASTIC sections of any NLGEOM flag is served.  A kind outside 0..3 is
 * refused too (before the kinds 2 and 3 existed, every non-zero value was read as Mises).
 *
 * Mohr-Coulomb and Drucker-Prager (!PLASTIC, YIELD=MOHR-COULOMB | DRUCKER-PRAGER; Elastoplastic.f90 yield types 1 and 2, restated as
 * written in csrc/fx_yield.h): kind 4 with plconst = c, H, phi in radians, and kind 5 with plconst = c, H, eta and plconst4 = xi --
 * M_PLCONST1..4 as fstr_ctrl_get_PLASTICITY leaves them (fstr_ctrl_material.f90:451-469).  Hardening is the linear law c + H p; harden
 * must be 0 (the card forces the digit), any of the three nlgeom flags is served.  Both are "plastic" for every piece of history
 * (plstrain, fstat, istat, commit, snapshot) and for the latch: after the first stress update every tangent is the elastic one.
 * Refused with FX_ERROR_UNSUPPORTED: cos(phi) == 0, xi == 0, harden != 0, kind 6 and any kind above 8, and kind 4 / 5 beside a hyperelastic
 * material (as Mises is); beside Mises or ELASTIC sections they are served.  The reference's `stop` statements of these branches --
 * `Math Error in Mohr-Coulomb calculation`, `Math error in return mapping`, `Jacobi iteration unable to converge` -- set the
 * context's device error word: fx_nl_stiffness, fx_nl_update, their _at forms and the element-level entry points then return
 * FX_ERROR_RUNTIME with that text.
 * plconst4 was appended at the end of the struct: every older member keeps its offset, the struct grew from 56 to 64 bytes.
 *
 * Viscoelastic materials (!VISCOELASTIC; Viscoelastic.f90, restated as written in csrc/fx_visco.h): kind 7 reads E, nu, nlgeom and
 * tab / ntab as the Prony rows (g_n, tau_n), any number >= 1.  nlgeom is 0 (INFINITE) or 1 (TOTALLAG, the card's default), the two
 * flags the card reaches (fstr_ctrl_material.f90:277-279); all six solid types and 361 F-bar; beside ELASTIC, Mises, Mohr-Coulomb /
 * Drucker-Prager and hyperelastic sections.  The material is time-dependent: see fx_nl_set_time below.  MatlMatrix tests
 * isViscoelastic before its saved flag (calMatMatrix.f90:51), so the latch neither changes this tangent nor is set by this material.
 * Refused with FX_ERROR_UNSUPPORTED: nlgeom 2, a Prony row with tau == 0, and fx_nl_set_thermal on a context that holds the kind
 * (the WLF / Arrhenius shift of !TRS and the temperature tables of the card stay out).
 *
 * NORTON creep (!CREEP, TYPE=NORTON; creep.f90, restated in csrc/fx_visco.h): kind 8 reads E, nu, nlgeom and plconst = A, n, m.
 * nlgeom must be 2 (UPDATELAG, the card's default); the five STF_C3 types and 361 B-bar; beside ELASTIC, Mises, Mohr-Coulomb /
 * Drucker-Prager and viscoelastic sections.  The update routines set isEp for a NORTON element (static_LIB_3d.f90:595): its first
 * stress update sets the latch whatever tincr is, and iso_creep's tangent is taken only while the latch is clear.  The update writes
 * gauss%plstrain = dg (the creep strain increment) and fstatus(1) = eqvs; fx_nl_commit adds plstrain to fstatus(2) under tincr > 0.
 * Refused with FX_ERROR_UNSUPPORTED: nlgeom 0 or 1 (under TOTALLAG the reference relaxes the point's stored stress instead of the
 * trial one, which defines no usable result), an F-bar group (UPDATELAG is refused there), kind 8 beside a hyperelastic material (the
 * latch, as for Mises), a time exponent m <= -1 (the law divides by m + 1), fx_nl_set_thermal.  The iteration of update_iso_creep on dg has no bound in the reference (a purely
 * hydrostatic non-zero stress never leaves it); here it ends after 100 passes or at a dg that is not finite, the point keeps its trial
 * stress, and fx_nl_update* / fx_nl_element_update return FX_ERROR_RUNTIME with a text that names creep. */
typedef struct fx_material_view { /* tMaterial after fstr_ctrl_get_ELASTICITY/_PLASTICITY (fstr_ctrl_material.f90:60-106, :341-480) */
  double E, nu;         /* M_YOUNGS, M_POISSON */
  int32_t plastic;      /* material kind.  0: mtype ELASTIC; 1: elastoplastic, Mises; 2: Neo-Hooke / Mooney-Rivlin; 3: Arruda-Boyce;
                         * 4: elastoplastic, Mohr-Coulomb; 5: elastoplastic, Drucker-Prager; 7: viscoelastic; 8: NORTON creep */
  int32_t harden;       /* fifth digit of mtype: 0 BILINEAR 1 MULTILINEAR 2 SWIFT 3 RAMBERG-OSGOOD */
  int32_t nlgeom;       /* nlgeom_flag: 0 INFINITE 1 TOTALLAG 2 UPDATELAG */
  int32_t ntab;         /* MULTILINEAR: rows of the MC_YIELD table */
  double plconst[3];    /* M_PLCONST1..3 */
  const double *tab;    /* ntab rows (yield stress, plastic strain); kind 7: ntab Prony rows (g, tau) */
  double plconst4;      /* M_PLCONST4: xi of Drucker-Prager; not read for another kind */
} fx_material_view;
typedef struct fx_nl_state_view { /* host arrays, any may be NULL (skipped).  tGaussStatus members (mechgauss.f90:13-22) */
  double *stress, *strain, *stress_bak, *strain_bak; /* n_elem*nq*6 (nq = 8 at 361); several groups: see fx_nl_init_groups */
  double *plstrain, *fstat;                           /* n_elem*nq: plstrain, fstatus(1) */
  int32_t *istat;                                     /* n_elem*nq: istatus(1) */
  double *unode, *dunode, *qforce;                    /* 3*NP: fstrSOLID%unode, %dunode, %QFORCE */
  int32_t latch; /* MatlMatrix's saved flag (calMatMatrix.f90:39); set_state: <0 leaves it */
} fx_nl_state_view;
/* fstr_solid / gauss-point set-up (zero state).  Needs a profile (fx_upload FX_UP_PROFILE).
 * fx_nl_init, _sections, _c3 and _type check what is their own (the types they take, nn_elem, null arguments) and hand the mesh as
 * ONE group (361: B-bar) to the set-up that fx_nl_init_groups runs: the same checks in the same order, every message under the
 * name of the entry point called, group and element named ("group 1, element N: ..."), and nothing of the context that was there
 * is touched by a call that is refused.  With n_mat == 1 elem_mat is not read. */
int fx_nl_init(fx_context *ctx, const fx_mesh_view *mesh, const fx_material_view *mat);
/* The same for a group whose elements belong to several sections / materials: elem_mat[e] in 1..n_mat selects mats[m-1]
 * (hecMESH%section_ID -> fstrSOLID%materials, fstr_setup.f90:325-400; every tGaussStatus%pMaterial points at its section's
 * tMaterial).  The materials may carry different NLGEOM flags (an ELASTIC TOTALLAG part next to a PLASTIC UPDATELAG part). */
int fx_nl_init_sections(fx_context *ctx, const fx_mesh_view *mesh, int32_t n_mat, const fx_material_view *mats,
                        const int32_t *elem_mat);
/* The same context for a mesh of tetrahedra: etype 341 (4 nodes, 1 quadrature point) or 342 (10 nodes, 4 points), STF_C3 /
 * UPDATE_C3 (static_LIB_3d.f90:47-205, :516-837) in their INFINITE / TOTALLAG / UPDATELAG branches.  elem_mat may be NULL with
 * n_mat == 1.  Another etype: FX_ERROR_UNSUPPORTED; a tetrahedron that names a node twice: FX_ERROR_RUNTIME.  Every fx_nl_* entry
 * point below works on either context; the per-point arrays hold nq(etype) points per element ([elem][point][.]), the element
 * outputs (3 nn)^2 and 3 nn doubles per element. */
int fx_nl_init_c3(fx_context *ctx, const fx_mesh_view *mesh, int32_t etype, int32_t n_mat, const fx_material_view *mats,
                  const int32_t *elem_mat);
/* The same context for a mesh of any one of the five types STF_C3 / UPDATE_C3 serve: etype 341, 342, 351 (6 nodes, 2 quadrature
 * points), 352 (15 nodes, 9 points) or 362 (20 nodes, 27 points).  fx_mesh_view carries no nodes-per-element, so the caller states
 * the row length of mesh->conn in nn_elem: another etype, or an nn_elem that is not the type's node count, is refused with
 * FX_ERROR_UNSUPPORTED before the connectivity is read; an element that names a node twice: FX_ERROR_RUNTIME.  Otherwise as
 * fx_nl_init_c3 (which keeps its two types). */
int fx_nl_init_type(fx_context *ctx, const fx_mesh_view *mesh, int32_t etype, int32_t nn_elem, int32_t n_mat,
                    const fx_material_view *mats, const int32_t *elem_mat);
/* The same context for a mesh of SEVERAL solid element types (hex-dominant meshes with wedge or tetrahedron transitions): the
 * groups of fx_assemble_groups, one material table for all of them, elem_mat of every group 1-based into it (may be NULL with
 * n_mat == 1).  etype of a group: 361 with elemopt 2 (B-bar, what the 361 nonlinear kernels are), 341, 342, 351, 352 or 362; a
 * type may appear in several groups; a group with n_elem == 0 is skipped.  Needs a profile.
 *   Layout of the per-point arrays (fx_nl_state_view, snapshot, commit): flat, the groups one after the other in the order given;
 *     group g starts at point P_g = sum over h < g of n_elem_h * nq(etype_h) and is [elem][point][.] inside.  With one group per
 *     hecMESH%elem_type_item entry that is hecMESH's element order.
 *   Layout of the element outputs (fx_nl_element_tangents, fx_nl_element_update): the groups one after the other in the same
 *     order, (3 nn_g)^2 doubles (row-major) and 3 nn_g doubles per element of group g.
 * Every other fx_nl_* entry point, fx_mat_ass_bc, fx_newton_substep and fx_solve_device_matrix work on such a context unchanged.
 * The latch (MatlMatrix's saved flag is the process's), the Mohr-Coulomb / Drucker-Prager error word and the refusal of an
 * elastoplastic beside a hyperelastic material are the context's: the first elastoplastic stress update in ANY group latches the
 * tangents of EVERY group.  The scatter runs group after group, NLGEOM flag after flag, colour after colour on one stream, each
 * group with its own colouring: no atomics, two fx_nl_stiffness calls on the same state give bitwise equal D / AL / AU.  Collapsed
 * hexahedra of a 361 group are served as in fx_nl_init.  The single-type entry points are this call with one group, so with ONE
 * non-empty group the context and all it computes are bit for bit those of fx_nl_init_sections / fx_nl_init_c3 / fx_nl_init_type.
 * A 361 group is B-bar (elemopt 2) or F-bar (elemopt 4: !SECTION, FORM361=FBAR; STF_C3D8Fbar / Update_C3D8Fbar,
 * static_LIB_Fbar.f90:26-769, in their INFINITE and TOTALLAG branches, with every material kind the loop has under those flags);
 * groups of either formulation and of the other five types may share one context.  Layouts, colouring, latch, snapshot, commit
 * and the state views are the same for both.  The two `stop` statements of the F-bar routines (`too small element volume`,
 * |V0| <= 1e-12, and `too small average jacob`) come back from fx_nl_stiffness* / fx_nl_update* / fx_nl_element_* as
 * FX_ERROR_RUNTIME with that text.  F-bar with an UPDATELAG material is refused: Update_C3D8Fbar's UPDATELAG branch builds `rot`
 * from the local array Fbar (:600-602), which only the TOTALLAG branch assigns (:556), so the reference defines no result there.
 * Refused, the previous context untouched: an unknown etype, an elemopt other than 2 and 4 on a 361 group (1 IC and 3 FI among
 * them; named), an F-bar group with an element whose material has nlgeom 2 (group and element named): FX_ERROR_UNSUPPORTED, as
 * are the materials fx_nl_init* refuse; n_group < 1, no element at all, missing materials, a material or node id out of range, a
 * degenerate element of a type other than 361 (named with group and element): FX_ERROR_RUNTIME.
 * fx_nl_init and fx_nl_init_sections stay B-bar; the linear entry points (fx_assemble_groups, ...) keep refusing elemopt 4. */
int fx_nl_init_groups(fx_context *ctx, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                      int32_t n_mat, const fx_material_view *mats);
/* fstr_Newton :63-68 + fstr_ass_load: dunode = 0, GL (3*NP, may be NULL), B = GL - QFORCE. */
int fx_nl_begin_substep(fx_context *ctx, const double *GL);
/* fstr_StiffMatrix (fstr_StiffMatrix.f90:18-212) + fstr_AddBC (fstr_AddBC.f90:17-190) with the
 * given increments of the prescribed dofs; result in the resident D/AL/AU/B. */
int fx_nl_stiffness(fx_context *ctx, int32_t n_bc, const int32_t *bc_node, const int32_t *bc_dof,
                    const double *bc_val, float *ms_assemble);
/* dunode += X, fstr_UpdateNewton (fstr_Update.f90:25-293), fstr_Update_NDForce
 * (fstr_Residual.f90:23-71); out = {|B|^2,|X|^2,|QFORCE|^2,|dunode|^2} (may be NULL). */
int fx_nl_update(fx_context *ctx, double out[4], float *ms_update);
/* hecmw_solve (hecmw_solver.f90:9) for a matrix that was assembled ON the device: B and X of `mat` go up, the prescribed dofs
 * fstr_AddBC passed to hecmw_mat_ass_bc (hecmw_mat_ass.f90:292-429) are applied to the resident matrix and B, the resident system
 * is solved as fx_solve does, X comes back.  mat->D / AL / AU are ignored. */
int fx_solve_device_matrix(fx_context *ctx, const fx_matrix_view *mat, const fx_comm_view *comm, int32_t n_bc, const int32_t *bc_node,
                           const int32_t *bc_dof, const double *bc_val, int32_t *Iarray, double *Rarray, fx_solve_info *info,
                           double *hist, int32_t hist_len);
/* The two element loops for a caller that keeps fstr_Newton's own loop on the host (the Fortran binding of INTEGRATION.md section 5).
 * fx_nl_stiffness_at: fstr_StiffMatrix (fstr_StiffMatrix.f90:18-212) for the host's unode / dunode (3*NP each, may be NULL = keep the
 *   resident ones), tangent into the resident D / AL / AU, no boundary conditions (fstr_AddBC follows on the host side).
 * fx_nl_update_at: fstr_UpdateNewton (fstr_Update.f90:25-293) for the host's dunode; QFORCE (3*NP) is written back.
 * fx_mat_ass_bc: hecmw_mat_ass_bc (hecmw_mat_ass.f90:292-429) for a list of prescribed dofs on the resident matrix and B. */
int fx_nl_stiffness_at(fx_context *ctx, const double *unode, const double *dunode, float *ms_assemble);
int fx_nl_update_at(fx_context *ctx, const double *dunode, double *qforce, float *ms_update);
int fx_mat_ass_bc(fx_context *ctx, int32_t n_bc, const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val);
/* unode += dunode, fstr_UpdateState (fstr_Update.f90:296-345). */
int fx_nl_commit(fx_context *ctx);
/* fstr_cutback_save (load = 0) / fstr_cutback_load (load = 1) for the device-resident quadrature-point history
 * (fistr1/src/analysis/static/fstr_Cutback.f90:108-198: fstr_copy_gauss of every point): an automatic incrementation rolls the
 * state back to the last converged sub-step when Newton fails (fstr_solve_NLGEOM.f90:156-197).  unode / QFORCE stay with the host. */
int fx_nl_snapshot(fx_context *ctx, int load);
int fx_nl_get_state(fx_context *ctx, fx_nl_state_view *s);
int fx_nl_set_state(fx_context *ctx, const fx_nl_state_view *s);
/* element-level outputs of the two kernels, no scatter (tests): ke n_elem*(3 nn)^2, qf n_elem*3 nn (nn = 8 at 361); a context of
 * several groups: group after group, see fx_nl_init_groups */
int fx_nl_element_tangents(fx_context *ctx, double *ke);
int fx_nl_element_update(fx_context *ctx, double *qf);
/* One substep of fstr_Newton around fx_solve_resident.  log: 7 doubles per Newton iteration
 * (iter, solver iterations, solver code, |B|, |X|, |QFORCE|, |dunode|).  Returns 0 (converged),
 * FX_ERROR_NOCONV_MAXIT (max_iter ran out; committed only if commit_unconverged), FX_NEWTON_MAXRES (residual above maxres,
 * fx_nl_set_step_control; never committed) or an error. */
int fx_newton_substep(fx_context *ctx, double factor0, double factor1, int32_t n_bc,
                      const int32_t *bc_node, const int32_t *bc_dof, const double *bc_val,
                      const double *cload, int32_t max_iter, double converg, int32_t *Iarray,
                      double *Rarray, double *log, int32_t *n_iter, int commit_unconverged);

/* step_ctrl(cstep)%maxres (fistr1/src/lib/m_step.f90:31, default 1.d+10): fx_newton_substep returns FX_NEWTON_MAXRES as soon as
 * |B|/|QFORCE| exceeds it (fstr_solve_NonLinear.f90:140-152, nothing committed); is_linear = fstr_Newton's isLinear
 * (.not. fstrPR%nlgeom, :50-51, :107): one pass without a convergence test. */
int fx_nl_set_step_control(fx_context *ctx, double maxres, int is_linear);

/* ---- time in the nonlinear static loop (time-dependent materials) ----
 * fx_nl_set_time: ctime and tincr of the coming sub-step or call, as fstr_Newton hands them to fstr_StiffMatrix, fstr_UpdateNewton
 *   and fstr_UpdateState (fstr_solve_NonLinear.f90:74, :100, :162; a `!STEP, TYPE=STATIC` step forces tincr = 0, :60-61).  The
 *   default after any fx_nl_init* is (0, 0).  fx_nl_stiffness*, fx_nl_update*, fx_nl_element_*, fx_nl_commit and fx_newton_substep
 *   read it.  With tincr == 0 a viscoelastic material computes what an ELASTIC one of the same flag computes
 *   (calViscoelasticMatrix :108-115; the update routines call StressUpdate only under tincr /= 0, static_LIB_3d.f90:659, :685).
 *   With tincr > 0 fx_nl_commit also runs updateViscoElasticState and updateViscoState (fstr_Update.f90:327-337).  NORTON reads
 *   both numbers: aa = A ((time + tincr)**(m+1) - time**(m+1)) / (m+1) with time at the START of the increment (creep.f90:66, :165);
 *   on a context with a NORTON material a negative or non-finite time or tincr is refused with FX_ERROR_RUNTIME, nothing changed.
 * fx_nl_get_history / fx_nl_set_history: fstatus(1..W) of every point, hist[point][W] on the host side (points in the order of the
 *   per-point arrays), W = the largest 12 nrow + 6 of the context's viscoelastic materials (Viscoelastic.f90:247-258: per Prony
 *   term 6 old and 6 new components of q_n, then the deviatoric strain of the last committed state; a NORTON point has 2: eqvs,
 *   which is also fstat of the state view, and the accumulated creep strain), zero padding for points
 *   whose material needs fewer, W = 0 in a context without such a material.  get: *width = W (hist may be NULL to ask for it);
 *   set: width must be W.  fx_nl_snapshot saves and restores this history with the rest.  (The device keeps it component-major
 *   over all points, hist[k * n_point + p]: consecutive lanes are consecutive points and read consecutive doubles.) */
int fx_nl_set_time(fx_context *ctx, double time, double tincr);
int fx_nl_get_history(fx_context *ctx, double *hist, int32_t *width);
int fx_nl_set_history(fx_context *ctx, const double *hist, int32_t width);

/* ---- thermal strain in the nonlinear static loop (!TEMPERATURE in an NLSTATIC deck) ----
 * The thermal branches of Update_C3D8Bbar (static_LIB_C3D8.f90:309-455), UPDATE_C3 (static_LIB_3d.f90:602-757) and Update_C3D8Fbar
 * (static_LIB_Fbar.f90:487-651): EPSTH(1:3) = alp (ttc - ref_temp) - alp0 (tt0 - ref_temp) with ttc = H . temperature and
 * tt0 = H . last_temp for an element of an elastoplastic material, H . temp_init for every other (fstr_Update.f90:92-102).
 * Isotropic expansion: one constant per material (M_EXAPNSION) or a table over temperature (MC_THEMOEXP); E and nu constant or a
 * table over temperature (MC_ISOELASTIC).  A table has one dependency, rows in ascending temperature, and is looked up as
 * fetch_TableData does (ttable.f90:282-354).  Not served: MC_ORTHOEXP, section orientation, a temperature column in the yield
 * table, NORTON and viscoelastic materials.
 *
 * fx_nl_set_thermal: after any fx_nl_init*.  Sets last_temp = temp_init (fstr_solve_NLGEOM.f90:53-57) and the temperature to temp_init
 *   or, without one, to ref_temp (fstr_setup.f90:780) until fx_nl_set_temperature gives another, and switches the thermal
 *   variants of the element kernels on; thermal = NULL switches them off again.  FX_ERROR_UNSUPPORTED, context untouched: a table
 *   whose temperatures are not strictly ascending, an elastic_tab on a hyperelastic material.
 * fx_nl_set_temperature: fstrSOLID%temperature (n_node) of the coming sub-step or call; NULL while thermal is on: FX_ERROR_RUNTIME.
 * With thermal on, fx_nl_stiffness* / fx_nl_update* / fx_nl_element_* read that temperature; fx_nl_commit copies it to last_temp
 * (fstr_UpdateState, fstr_Update.f90:308-312); fx_nl_snapshot saves and restores last_temp with the point history
 * (fstr_Cutback.f90:127, :173); fx_nl_begin_substep and fx_newton_substep add the thermal load of fstr_ass_load.f90:287-428 to
 * the first right-hand side: TLOAD_C3D8Bbar for every 361 element whatever its formulation, TLOAD_C3 for the other types, on
 * coord + unode with TEMP0 = last_temp for every element.  (Elements of a hyperelastic material add no thermal load: the vector only
 * steers the first correction of a sub-step.)  fx_nl_stiffness_at / fx_nl_update_at add no load. */
typedef struct fx_nl_thermal_view {
  double ref_temp;            /* !REFTEMP */
  const double *temp_init;    /* n_node: !INITIAL CONDITION, TYPE=TEMPERATURE; NULL = 0 */
  const double *alpha;        /* n_mat: M_EXAPNSION */
  const double *const *alpha_tab;   /* NULL, or n_mat pointers (each may be NULL): rows (alpha, T) */
  const int32_t *alpha_rows;        /* rows of each alpha_tab (read where alpha_tab[m] is not NULL) */
  const double *const *elastic_tab; /* NULL, or n_mat pointers (each may be NULL): rows (E, nu, T) */
  const int32_t *elastic_rows;
} fx_nl_thermal_view;
int fx_nl_set_thermal(fx_context *ctx, const fx_nl_thermal_view *thermal);
int fx_nl_set_temperature(fx_context *ctx, const double *temp);
/* last_temp (n_node), for tests and restart; FX_ERROR_RUNTIME while thermal is off */
int fx_nl_get_last_temp(fx_context *ctx, double *last_temp);
int fx_nl_set_last_temp(fx_context *ctx, const double *last_temp);

/* ---- nodal and element stress output (fstr_NodalStress3D, fstr_NodalStress.f90:13-272) ----
 * What `!WRITE,RESULT` writes and the `Global Summary` block is taken from, for TYPE=341, 342, 351, 352, 361 (every formulation:
 * the rule depends on the type only) and 362 in any mix of groups (csrc/fx_nodal_stress.h has the rules):
 *   estrain, estress [n_elem][6]  mean over all quadrature points of the element (ElementStress_C3)
 *   strain, stress   [n_node][6]  mean over the elements that name the node of the element's nodal values (341, 351: the element
 *                                 mean; 361, 342, 352, 362: extrapolation with inverse_func's inverse, mid-edge nodes the half-sum of
 *                                 their two vertices); a node named twice by a collapsed element is added and counted twice; a node
 *                                 that no element names keeps zeros
 *   mises [n_node], emises [n_elem]   get_mises of stress / estress
 * Elements are numbered through the groups in the order given (hecMESH's order with one group per elem_type_item entry); the sum
 * at a node runs in ascending element number, as the reference's loop does, without atomics: the result is bitwise the same from
 * run to run.  tnstrain, shells, beams, trusses, 301 and decomposed meshes are not served.
 * flags: make_principal's bit mask (:889-980).  bit 0 / 1: principal values / vectors of the nodal stress, 2 / 3 of the nodal strain
 * (shear components as stored, as the reference passes them), 4 / 5 of the element stress, 6 / 7 of the element strain; get_principal
 * (utilities.f90:362-406): values in descending order, vector j scaled by value j.  Index order of a vector array:
 * vect[(i * 3 + j) * 3 + r] = component r of vector j of node or element i = PSTRESS_VECT(3 * i + r + 1, j + 1) of the reference
 * (0-based i, j, r).  An array whose flag is off is NULL.  eigen3's `stop` (`Jacobi iteration unable to converge`): FX_ERROR_RUNTIME.
 * All pointers lie in pinned staging of the context that belongs to this pass alone (not the staging of the update results), so an
 * update or prepare call leaves them alone: they are valid until the next nodal-stress call on the same context or fx_destroy. */
typedef struct fx_nodal_result {
  int32_t n_node, n_elem;
  const double *strain, *stress, *mises;       /* STRAIN, STRESS, MISES */
  const double *estrain, *estress, *emises;    /* ESTRAIN, ESTRESS, EMISES */
  const double *pstress, *pstress_vect;        /* flags bit 0, 1: [n_node][3], [n_node][3][3] */
  const double *pstrain, *pstrain_vect;        /* bit 2, 3 */
  const double *epstress, *epstress_vect;      /* bit 4, 5: [n_elem][3], [n_elem][3][3] */
  const double *epstrain, *epstrain_vect;      /* bit 6, 7 */
} fx_nodal_result;
enum { FX_PRINC_NSTRESS = 1, FX_PRINCV_NSTRESS = 2, FX_PRINC_NSTRAIN = 4, FX_PRINCV_NSTRAIN = 8,
       FX_PRINC_ESTRESS = 16, FX_PRINCV_ESTRESS = 32, FX_PRINC_ESTRAIN = 64, FX_PRINCV_ESTRAIN = 128 };
/* The linear path: strain, stress are host arrays in the layout fx_update_groups_linear returns, the groups one after the other,
 * [elem][point][6] inside a group (nq(etype) points per element); groups / n_group as fx_update_groups_linear takes them (elemopt
 * and elem_mat are not read).  The node -> element list is built once per (n_node, groups, connectivity) and kept in the context.
 * fx_elem_group carries no row length, so a connectivity with the wrong number of nodes per element cannot be seen here: conn is
 * read as nn(etype) ids per element.  The Python layer, which has the array's shape, refuses such a group with the code
 * FX_ERROR_UNSUPPORTED before the call.
 * Errors, *out untouched: an etype outside the six: FX_ERROR_UNSUPPORTED; a node id outside 1..n_node (group and element named),
 * missing arrays, flags outside 0..255: FX_ERROR_RUNTIME. */
int fx_nodal_stress_groups(fx_context *ctx, int32_t n_node, int32_t n_group, const fx_elem_group *groups, const double *strain,
                           const double *stress, int32_t flags, fx_nodal_result *out, float *ms_kernel);
/* The same over the resident stress and strain of a nonlinear context (any fx_nl_init*), whatever groups, F-bar parts and
 * materials it holds: nothing but the results crosses the bus.  The list is built at the first call after an fx_nl_init*. */
int fx_nl_nodal_stress(fx_context *ctx, int32_t flags, fx_nodal_result *out, float *ms_kernel);
/* The inverse the kernels of `etype` take (tests): inv n x n row-major, *n = 8, 4, 6, 8 at 361, 342, 352, 362 and 0 at 341, 351. */
int fx_nodal_inverse(int32_t etype, double *inv, int32_t *n);
/* out[0] lists built for fx_nodal_stress_groups on this context, [1] for fx_nl_nodal_stress, [2] entries and [3] vertex records
 * of the list fx_nodal_stress_groups last used, [4] workgroup size of the node kernel, [5..10] elements per workgroup of the element
 * kernel of 341, 342, 351, 352, 361, 362. */
int fx_nodal_get_stats(fx_context *ctx, int64_t out[12]);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) -------------------- */
/* 128-byte ncclUniqueId made by rank 0 and broadcast by the host side
 * (torch.distributed / MPI); then every rank calls fx_comm_init. */
int fx_comm_unique_id(unsigned char id[128]);
int fx_comm_init(fx_context *ctx, const unsigned char id[128], int rank, int nranks);
/* Alternative transport (tests on one GPU, MPI builds of fistr1 without RCCL): the library
 * stages through pinned host buffers and calls back.  halo: send holds 3*n_export doubles in
 * export_item order, recv must be filled with 3*n_import doubles in import_item order
 * (hecmw_solve_send_recv_33, hecmw_solver_SR_33.F90:42-124).  allreduce: in-place SUM over
 * ranks of n doubles (hecmw_allreduce_R, hecmw_comm_f.F90:346-379). */
/* Ranks the transport itself reports (ncclCommCount of the RCCL communicator, or the count given with the host
 * callbacks; 1 without either) and the device the communicator / context is bound to. */
int fx_comm_size(fx_context *ctx, int32_t *nranks, int32_t *device);
/* What this rank asked of the transport since it was set up, for a cross-rank consistency check (bench.py --gpus N compares the
 * ledgers of all ranks over its control plane; hecmw_solver_SR_33.F90:42-124 and hecmw_comm_f.F90:346-379 are the calls counted):
 * out[0] operations, [1] hash of their sequence (kind and size of every all-reduce, position of every halo exchange: equal on all
 * ranks), [2] all-reduces, [3] their bytes, [4] halo exchanges, [5] neighbours, [6] 1 = the halo exchange has a communicator of its
 * own, then 5 per neighbour: rank, messages sent, bytes sent, messages received, bytes received.  *n_out = entries available. */
int fx_comm_ledger(fx_context *ctx, int64_t *out, int32_t cap, int32_t *n_out);
typedef void (*fx_halo_fn)(const double *send, double *recv, void *user);
typedef void (*fx_allreduce_fn)(double *v, int n, void *user);
int fx_comm_set_host_callbacks(fx_context *ctx, int rank, int nranks, fx_halo_fn halo, fx_allreduce_fn allreduce,
                               void *user);

/* ---- heat conduction (!SOLUTION, TYPE=HEAT) ----------------------------- */
/* heat_mat_ass_conductivity.f90 + heat_mat_ass_capacity.f90 on the device for TYPE=341, 342, 351, 352, 361, 362 in any mix of
 * groups: heat_THERMAL_3xx / heat_CAPACITY_3xx / heat_GET_CONDUCTIVITY / _CP / _DENSITY (heat_LIB_THERMAL.f90, heat_LIB_CAPACITY.f90)
 * restated with their own point sets and, where they have them, their default-real constants.  One table is what heat_init_material (heat_init.f90:197-231) leaves in fstrHEAT: ntab rows,
 * temp[ntab], funcA[ntab + 1], funcB[ntab + 1]. */
typedef struct fx_heat_table {
  int32_t ntab;
  const double *temp, *funcA, *funcB;
} fx_heat_table;
typedef struct fx_heat_material_view {
  fx_heat_table cond, cp, rho; /* cp and rho are read only with dtime > 0 */
} fx_heat_material_view;
typedef struct fx_heat_view {
  const double *temp, *temp0; /* fstrHEAT%TEMP, %TEMP0 (n_node each; temp0 may be NULL when beta == 1 and dtime == 0) */
  double beta;                /* 1 steady, 0.5 transient; ALFA = 1 - beta */
  double dtime;               /* 0: no capacity term */
} fx_heat_view;
/* Clears the matrix and B, adds every element's SS(TEMP) * beta, B -= SS * TEMP0 * (1 - beta) and, with dtime > 0, the lumped
 * S0(TEMP0): D += S0 / dtime, B += S0 * TEMP0 / dtime; then B += flux (!CFLUX; n_node, may be NULL) and hecmw_mat_ass_bc(node, 1,
 * val) for the n_fix nodes in the order given (!FIXTEMP).  Surface terms (!FILM, !RADIATE, !DFLUX): fx_heat_assemble_groups_bc.
 *   groups: fx_elem_group as above, elemopt ignored; elem_mat 1-based into mats when n_mat > 1.
 *   mat: NDOF = 1; the caller's profile, and the caller's D, AL, AU, B as the place the result is WRITTEN (X is not touched).
 * The scatter is coloured and atomic-free through a position map cached in the context (one cache per context, by group
 * position, as fx_assemble_groups): a call with the same groups and profile and new temperatures colours and maps nothing, and
 * results are bitwise reproducible from call to call.
 * Errors, all before anything is written: unknown etype or mat->NDOF != 1: FX_ERROR_UNSUPPORTED; missing arrays, ids out of
 * range, ntab < 1, a connectivity entry absent from the profile, an element (of any type) that names a node twice (group and
 * element named): FX_ERROR_RUNTIME.  A group that cannot be coloured -- a node in more than 64 of its elements, or FX_ASM_ATOMIC
 * set -- is refused with FX_ERROR_RUNTIME as well: this assembly has no atomic scatter to fall back to (fx_assemble_groups has). */
int fx_heat_assemble_groups(fx_context *ctx, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                            int32_t n_mat, const fx_heat_material_view *mats, const fx_heat_view *heat, const fx_matrix_view *mat,
                            const double *flux, int32_t n_fix, const int32_t *fix_node, const double *fix_val, float *ms_kernel);
/* One element through the device kernels (tests): ss (nn x nn) at the node temperatures tt and, with dtime > 0, s0 (nn) at tt0. */
int fx_heat_element(fx_context *ctx, int32_t etype, const double *ecoord, const double *tt, const double *tt0,
                    const fx_heat_material_view *mat, double dtime, double *ss, double *s0);
/* out[0] colourings made, [1] position maps made, [2] profiles uploaded, [3] calls of fx_heat_assemble_groups, [4] microseconds
 * of the last copy of D, AL, AU, B to the caller, [5] lanes per element, [6] elements per workgroup of the element kernel. */
int fx_heat_get_stats(fx_context *ctx, int64_t out[8]);

/* The surface terms of heat_mat_ass_boundary for the six solid types: heat_mat_ass_bc_DFLUX (faces S1.. and, as face 0, the body
 * flux BF; without the weld line), heat_mat_ass_bc_FILM and heat_mat_ass_bc_RADIATE, that is heat_DFLUX_3xx, heat_FILM_3xx and
 * heat_RADIATE_3xx (heat_LIB_DFLUX.f90, heat_LIB_FILM.f90, heat_LIB_RADIATE.f90) with their own face node tables, point sets, loop
 * order and default-real Gauss constants.  One list entry is one (element, face) of the reference's Q_SUF / H_SUF / R_SUF lists;
 * its values arrive already multiplied by their amplitudes (heat_get_amplitude at the call's time, resolved by the caller). */
typedef struct fx_heat_surface {
  int32_t n;
  const int32_t *group, *elem, *face; /* position in groups[] (0-based), element within the group (0-based), LTYPE of the routine */
  const double *val, *sink;           /* Q | HH | RR, and SINK (NULL for dflux) -- amplitude already applied */
} fx_heat_surface;
typedef struct fx_heat_bc {
  fx_heat_surface dflux, film, radiate; /* face 0 is allowed in dflux only (BF) */
  double tzero;                         /* hecMESH%zero_temp (!ZERO) */
} fx_heat_bc;
/* fx_heat_assemble_groups with the surface terms.  Order: clear, the elements, then DFLUX, FILM and RADIATE on the device copy
 * of the matrix (D, AL, AU -= TERM1; B -= TERM2 on the diagonal pass; B -= VECT), then the copy-back, then B += flux and the
 * !FIXTEMP elimination on the host as in fx_heat_assemble_groups.  The reference adds !CFLUX before the surface terms; adding it
 * after them reorders only a sum into B.
 * Each list's faces are coloured as elements of mm nodes (3, 4, 6 or 8; per group and face shape) and scattered colour by colour
 * without atomics through a position map of their own; colouring and map are cached in the context by a checksum of the list and
 * of its group, beside the groups' (calling fx_heat_assemble_groups in between invalidates neither).  Results are bitwise
 * reproducible from call to call.  The same (element, face) may appear more than once in a list and is added as often.
 * Errors, all before anything is written, FX_ERROR_RUNTIME: bc NULL, a group or element index out of range, a face outside
 * 1..nface (0..nface for dflux), a null array with n > 0, a list that cannot be coloured (a node in more than 64 of its faces, or
 * FX_ASM_ATOMIC set), a face node pair absent from the profile.  Everything else as fx_heat_assemble_groups. */
int fx_heat_assemble_groups_bc(fx_context *ctx, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                               int32_t n_mat, const fx_heat_material_view *mats, const fx_heat_view *heat, const fx_matrix_view *mat,
                               const double *flux, int32_t n_fix, const int32_t *fix_node, const double *fix_val,
                               const fx_heat_bc *bc, float *ms_kernel);
/* One face (or, face 0 of kind 0, the body flux) through the device kernels (tests).  kind: 0 dflux, 1 film, 2 radiate; ecoord
 * (nn x 3) and tt (nn, read by radiate only) of the whole element.  film, radiate: term1 (mm x mm), term2 (mm); dflux: VECT (nn)
 * in term2, term1 untouched.  nsuf: NOD of the routine (mm, 1-based; 1..nn for the body flux), *mm its length. */
int fx_heat_face(fx_context *ctx, int32_t etype, int32_t kind, int32_t face, const double *ecoord, const double *tt, double val,
                 double sink, double tzero, double *term1, double *term2, int32_t *nsuf, int32_t *mm);
/* out[0] face colourings made, [1] face position maps made, [2] microseconds of the element kernels and [3] of the surface
 * kernels of the last fx_heat_assemble_groups_bc, [4] lanes per face, [5] faces per workgroup of the face kernel. */
int fx_heat_get_bc_stats(fx_context *ctx, int64_t out[8]);

/* ---- distributed loads (!DLOAD) of the six solid types ----
 * The DLOAD block of fstr_ass_load (fstr_ass_load.f90:138-257) with DL_C3 (static_LIB_3d.f90:210-377): volume loads BX, BY, BZ
 * (not multiplied by RHO), GRAV (RHO val times the normalised PARAMS(1:3)) and CENT (RHO val^2 times the distance vector from the
 * axis through PARAMS(1:3) along PARAMS(4:6)) over the element's own quadrature rule (361: the 8 points of gauss3d2 whatever its
 * elemopt), and pressure on face f (LTYPE 10 f) with getSubFace's node tables, the face type's rule and SurfaceNormal's
 * un-normalised normal.  A surface group (LTYPE 100) is resolved by the caller into (element, 10 face) entries; an amplitude is
 * applied by the caller.  Loads on shells, beams, trusses and 2-D types, uloading and torque CLOADs are not served. */
typedef struct fx_dload {        /* one entry = one (element, LTYPE) of fstr_ass_load's loop :157-256 */
  int32_t n;
  const int32_t *group, *elem;   /* position in groups[] and element within it, 0-based (as fx_heat_surface) */
  const int32_t *ltype;          /* DL_C3's LTYPE: 1..5, or 10*face */
  const double *params;          /* n x 7: PARAMS(0:6), amplitude already applied */
  const uint8_t *held;           /* may be NULL; 1: the entry takes factor 1 (fstr_ass_load.f90:141-142) */
} fx_dload;
/* factor * VECT of every entry (1 * VECT where held) ADDED to load_inout (3*n_node, host), on coord (+ disp, 3*n_node, when not
 * NULL): it composes with the `load` of fx_assemble_groups and with fx_thermal_load_groups.  rho: n_mat densities (M_DENSITY),
 * picked by the group's elem_mat (material 1 without); may be NULL when the list has neither GRAV nor CENT.  Entries that share a
 * node add with fp64 atomics (as QFORCE): equal to rounding from call to call, not bit for bit; an entry given twice is added
 * twice.  Needs no profile.  ms_kernel (may be NULL): the face and volume kernels together.
 * Refused before anything is written, load_inout untouched: an etype outside the six, or a context of more than one rank (the
 * reference exchanges GL with hecmw_update_3_R): FX_ERROR_UNSUPPORTED.  An ltype that is none of 1..5 and no face of the
 * element's type, a group or element index out of range, a null array with n > 0, GRAV or CENT without rho, and -- where the
 * reference divides by zero and carries NaN on -- a zero GRAV direction or CENT axis direction, each named with its entry and
 * group (1-based), and what fx_assemble_groups refuses of the groups: FX_ERROR_RUNTIME. */
int fx_dload_groups(fx_context *ctx, int32_t n_node, const double *coord, int32_t n_group, const fx_elem_group *groups,
                    int32_t n_mat, const double *rho, const fx_dload *dl, double factor, const double *disp,
                    double *load_inout, float *ms_kernel);
/* One element through the device kernels (tests): DL_C3's VECT (3 nn, zero off the face), no factor, no atomics.  ecoord nn x 3,
 * params PARAMS(0:6).  Refusals as above. */
int fx_dload_element(fx_context *ctx, int32_t etype, int32_t ltype, const double *ecoord, double rho, const double *params,
                     double *vect);
/* The nonlinear loop (after any fx_nl_init*).  The list -- group = position of the element group given to fx_nl_init_groups, 0 for
 * the single-type set-ups -- is checked as above, resolved to node ids and uploaded once; dl == NULL clears it.  The positions are
 * the caller's: a group with n_elem == 0, which fx_nl_init_groups skips, keeps its number, so the groups behind it are named as
 * the caller numbers them, an entry on the empty group itself is refused ("element E is not in group G"), and every message
 * carries the caller's 1-based group number.  A refused list leaves the list that was in force untouched.  From then on
 *   fx_nl_begin_substep builds GL = the nodal load it is handed + factor * DLOAD before B = GL - QFORCE, on coord + unode when
 *     `follow` is set (DLOAD_follow, the reference's default; !DLOAD, FOLLOW=NO clears it) and on coord otherwise;
 *   with `follow` set, fx_nl_update and fx_nl_update_at rebuild GL on coord + unode + dunode after the stress update and before
 *     the residual: fstr_Newton's second fstr_ass_load (fstr_solve_NonLinear.f90:103).  The nodal part is kept in a vector of its
 *     own, allocated only while a list is set.
 * The list is launched in colours of entries that share no node (one launch per colour and batch), so a rebuilt GL depends on
 * its inputs alone: the same nodal load, list, factor and displacements give the same GL bit for bit (fx_dload_groups makes no
 * such promise).  An entry that names a node twice, a collapsed hexahedron, is outside this.
 * Without a list every fx_nl_* call runs what it ran before these entry points existed.  factor: fstrSOLID%factor(2), default 1;
 * fx_newton_substep sets it to its factor1.  fx_nl_get_load: the resident GL (3*NP) back to the host. */
int fx_nl_set_dload(fx_context *ctx, int32_t n_mat, const double *rho, const fx_dload *dl, int follow);
int fx_nl_set_dload_factor(fx_context *ctx, double factor);
int fx_nl_get_load(fx_context *ctx, double *GL);
/* out[0] entries on triangles and [1] on quadrilaterals, [2] BX / BY / BZ, [3] GRAV and [4] CENT entries of the last list given to
 * fx_dload_groups or fx_nl_set_dload, [5] microseconds of the face kernels and [6] of the volume kernels of the last
 * fx_dload_groups, [7] lanes per face (the volume kernels take 4, 16, 8, 16, 8, 32 lanes per element of 341 .. 362). */
int fx_dload_get_stats(fx_context *ctx, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* FISTR_HIP_H */
