// Internal declarations of libfistr_hip (gfx950 only).  See include/fistr_hip.h for the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/fistr_hip.h"

extern thread_local std::string g_fx_error;
int fx_fail(const char *what, const char *file, int line);

#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      g_fx_error = std::string(#expr) + ": " + hipGetErrorString(_e);        \
      return fx_fail(g_fx_error.c_str(), __FILE__, __LINE__);                \
    }                                                                        \
  } while (0)

// ---------------------------------------------------------------------------
// Device copy of the reference layout (D / AL / AU with 1-based items), kept so
// that assembly and BC elimination work on the arrays fistr1 owns and so the
// matrix can be handed back bit-for-bit.
// ---------------------------------------------------------------------------
struct DevCSR {
  int32_t N = 0, NP = 0, NPL = 0, NPU = 0;
  int32_t *indexL = nullptr, *itemL = nullptr, *indexU = nullptr, *itemU = nullptr;
  double *D = nullptr, *AL = nullptr, *AU = nullptr, *B = nullptr, *X = nullptr;
};

// ---------------------------------------------------------------------------
// BELL-64: sliced block-ELL, the layout every sweep kernel streams.
//   slot  = 64*slice + lane; one thread owns one block row.
//   slice s holds block positions [pair_ptr[s], pair_ptr[s+1]) ("halves": one 3x3 block per lane
//   each), consumed two at a time: for the pair starting at position h and block element e
//   (row-major, 0..8) the two values of lane l sit in one 16-byte word
//       ((double2*)(val + h*576))[e*64 + l] = (block h, block h+1)[e]
//   and the two column ids (0-based vector slots) in one 8-byte word ((int2*)(col + h*64))[l].
//   An odd last position of a slice is stored alone (val[h*576 + e*64 + l], col[h*64 + l]):
//   hex-mesh rows have 27 blocks, pair padding would waste 1/27 of the stream.
//   => every wave-level load is 1 KiB (values) / 512 B (columns), fully coalesced,
//   and a lane never needs a cross-lane reduction.
//   Padding blocks carry value 0 and the row's own column (always a valid address).
// ---------------------------------------------------------------------------
struct Bell {
  int32_t nslots = 0, nslices = 0;
  int64_t npairs = 0;           // total block positions (halves) over all slices
  int32_t *pair_ptr = nullptr;  // nslices+1, in halves
  double *val2 = nullptr;       // npairs*9*64 doubles
  void *val2_base = nullptr;    // allocation holding val2 (placement experiments: FX_VAL2_PAD)
  int *col2 = nullptr;          // npairs*64
  int *src2 = nullptr;          // npairs*64: source block codes 3*idx+{0 D,1 AL,2 AU}, -1 padding (kept for numeric refresh)
  int32_t *slot_row = nullptr;  // nslots: 0-based node id of the slot, -1 = padding slot (may be null = identity)
  int32_t *slice_order = nullptr;  // nslices: order in which the SpMV walks the slices (null = ascending)
  // Domain-decomposed systems: the SpMV's virtual workgroups (4 consecutive entries of the slice walk each) split into those
  // none of whose rows has a halo column (interior: run while the halo exchange is in flight) and the rest (boundary).
  int32_t *wg_interior = nullptr, *wg_boundary = nullptr;
  int32_t n_wg_interior = 0, n_wg_boundary = 0;
  int64_t nblocks = 0;          // real (non padding) blocks
  size_t val2_bytes = 0;        // bytes val2_base was allocated with (its share of the arena, the power-of-two request, or the exact size)
  struct fx_context *arena_owner = nullptr;  // val2_base lies in this context's value arena (DevArena): released there, not with hipFree
  bool values_filled = false;   // bell_fill_values has written val2 (arena_switch may only re-point arrays that hold no values yet)
  size_t bytes() const { return (size_t)npairs * 64 * (9 * 8 + 4) + (size_t)(nslices + 1) * 4; }
};

// Solver numbering.  All Krylov vectors and the BELL structures live in "slot" space:
//   kind 0 (natural):      slot = node, padded to a multiple of 64;
//   kind 1 (colour-major): the multicolour SSOR ordering of the reference (same colours), each
//                          colour starting a new 64-slot slice, natural node order inside a
//                          colour.  Neighbouring lanes then gather neighbouring vector entries
//                          both in the colour sweeps and in the SpMV (full cache lines), which
//                          the reference's old-numbering ZP indexing does not give a GPU.
// Halo nodes N+h keep slot nslots+h.  Padding slots carry no blocks, an identity diagonal
// factor and zeros in every vector, so kernels treat every slot as a row.
struct Ordering {
  int kind = -1;
  int32_t nslots = 0, nhalo = 0;
  std::vector<int32_t> slot_node;  // nslots+nhalo: 0-based node of a slot, -1 = padding
  std::vector<int32_t> slot_of;    // NP: node -> slot
  int32_t *d_slot_node = nullptr, *d_slot_of = nullptr;
  int32_t vslots() const { return nslots + nhalo; }
};

// Multicolour SSOR state (hecmw_precond_SSOR_33.f90 module variables).
// Plane march of the level-scheduled sweeps (fx_march.h): one direction's program.  The rows of a chunk (a contiguous range of the
// natural numbering, one workgroup) are executed in ROUNDS -- the chunk's own dependency levels, split to at most R rows -- and the
// matrix is stored in exactly that order: 8 lanes per row, lanes 0..6 one block pair each, lane 7 the LU of the diagonal block.
struct MarchProg {
  int64_t nrounds = 0;
  int32_t *round_ptr = nullptr;  // device [nchunks + 1]: rounds of chunk c = [round_ptr[c], round_ptr[c + 1])
  int32_t *rstart = nullptr;     // device [nrounds + 1]: march position of each round's first row
  double *val = nullptr;         // device: per round [9][8 n] double2 (n = rows of the round)
  int32_t *col = nullptr;        // device: int2 per lane (>= 0 far: row whose entry is gathered from memory; -1 padding;
                                 //   <= -2 near: -(ring slot) - 2; lane 7: (row, 0))
  int32_t *src = nullptr;        // device: int2 per lane, source codes of the two blocks (k_bell_fill's; lane 7: 3 * row)
  std::vector<int32_t> h_round_ptr, h_rstart;
};
struct MarchDev {
  bool ok = false;
  int32_t S = 0, NW = 0, nchunks = 0;  // rows per chunk, pair waves per workgroup (8 rows each), chunks
  MarchProg F, B;                      // forward (L) and backward (U) programs
  double *zf = nullptr;                // forward sweep's vector, 3 N, natural numbering
  double est_us = 0.0, est_level_us = 0.0;  // cost model: one half sweep as a march / as dependency levels
  double build_s = 0.0;
  int32_t max_round_rows = 0, far_same_chunk = 0;
  int64_t near_blocks = 0, far_blocks = 0;
};

struct SsorDev {
  int32_t ncolor = 0;
  std::vector<int32_t> color_slice;  // slice range per colour: [color_slice[c], color_slice[c+1])
  Bell L, U;                         // strictly-lower / strictly-upper parts in colour-slot order
  Bell H;                            // Eisenstat form on a subdomain: the halo-column blocks (what the localized L / U drop)
  double *alu = nullptr;             // LU of the diagonal blocks, [slice][e][lane] layout
  double sigma_diag = 1.0;           // SIGMA_DIAG the factors in alu were built with
  int64_t values_epoch = -1;         // fx_context::values_epoch the sweep layouts were filled at
  int32_t nslots = 0;                // colour-major slots (each colour padded to a 64 multiple)
  int32_t *slot_node = nullptr;      // device: slot -> 0-based node, -1 = padding
  double *zs = nullptr;              // private sweep vector, 3*nslots, colour-major
  double *zb = nullptr;              // dataflow sweeps: the backward sweep's vector (zs holds the forward one), 3*nslots
  double *lu_D = nullptr, *lu_AL = nullptr, *lu_AU = nullptr;  // ILU(0): factor values in the reference CSR layout
  std::vector<int32_t> slot_start;   // ILU(0): first slot of each level (ncolor+1)
  int32_t max_row_blocks = 0;        // ILU(0): largest number of off-diagonal blocks in a row (<= 32: lane-per-block factorisation)
  std::vector<int32_t> perm;         // new -> old (1-based), as the reference's perm(:)
  std::vector<int32_t> colorindex;   // COLORindex(0:ncolor)
  MarchDev march;                    // level-scheduled sweeps as a plane march (fx_march.h)
  int32_t *slice_level = nullptr;    // device: dependency level of every slice of the level-major layouts (ILU(0), natural SSOR)
};

struct DiagDev {
  double *alu = nullptr;  // [slice][e][lane]
  int32_t nslices = 0;
};

// Scalars of the Krylov loops, resident on the device; the host only polls `status`.
#define FX_DF_RETRY (-77)  // internal: a dataflow sweep timed out, the context switched to df_mode 0, redo the work
// The dataflow tail of the Eisenstat sweeps (eis_tail, fistr_hip.hip): a colour of at most EIS_TAIL_GRIDS x G slices is latency-bound,
// G = the smaller co-resident grid of k_eis_*_df (at most EIS_DF_MAX_PER_CU workgroups per CU).  At 10.1 M DOF on 256 CUs the big
// colours have 5,274 slices and the others at most 1,456 (profiles/r05_eis_colour_times_before.txt): any G from 364 to 1,318 separates
// them, and G is 768 there (3 forward workgroups per CU); EIS_DF_MAX_PER_CU keeps G at or below 1,024 on such a device.
#define EIS_TAIL_GRIDS 4
#define EIS_DF_MAX_PER_CU 4
#define FX_ST_PAUSED 2  // KrylovState::status: waiting for the host to enqueue the true-residual check (hecmw_solver_CG.f90:259-266)
struct KrylovState {
  double rho, rho1, beta, c1, alpha, omega, c2, cg0, cg1, dnrm2, bnrm2, resid, tol;
  int32_t iter;         // Fortran ITER of the iteration being executed
  int32_t status;       // 0 running, 1 converged/exit, else fx_status code
  int32_t need_verify;  // RESID<=TOL seen, true residual check pending
  int32_t n_indef;
  int32_t maxit;
  int32_t error;        // 3001 set while running (reference sets error and falls out of the DO)
  int32_t n_hist;       // residual-history lines written (the ITERLOG lines the reference would have printed)
  int32_t pause_verify; // 1: RESID <= TOL by the recurrence parks the loop (status = FX_ST_PAUSED) and the HOST enqueues the true-residual
                        // check at its next poll -- the rare path costs no launches per iteration; 0: the check rides in every iteration, gated
  int32_t t_current;    // Eisenstat form: 1 = t = (D~+L)^-1 r is current; 0 = r was replaced by the true residual, refresh t (set by OP_VERIFY, cleared by OP_CG_RHO)
};

struct HaloDev {
  int32_t n_neighbor = 0;
  std::vector<int32_t> neighbor, import_index, export_index;
  std::vector<int32_t> h_export, h_import;                 // host, 0-based node ids
  int32_t *export_item = nullptr, *import_item = nullptr;  // device, slot ids
  double *sendbuf = nullptr, *recvbuf = nullptr;
  int32_t n_export = 0, n_import = 0;
};

// Material of one section as the nonlinear kernels take it: isotropic ELASTIC, elastoplastic (Mises, Mohr-Coulomb, Drucker-Prager), or
// hyperelastic.  The layout is part of every element kernel's argument list, so a hyperelastic material reuses the slot of the
// hardening law for its kind (a hyperelastic material has no hardening law): read it through nl_hyper_kind().
struct NlMat {
  double E, nu, pl[3];      // pl: M_PLCONST1..3 (hardening constants; c / H / phi or eta; C10 / C01 / D1; mu / lambda_m / D)
  int32_t plastic;          // non-zero: elastoplastic (state history, the latch) -- 1 Mises, FX_MAT_MOHR, FX_MAT_DRUCKER; 0: ELASTIC and hyperelastic
  int32_t harden;           // Mises: hardening law 0..3 (0 for the other two yield functions); group 3: the kind, FX_MAT_MOONEY or FX_MAT_ARRUDA
  int32_t group;            // compile-time group of the element kernels: 0 INFINITE, 1 TOTALLAG, 2 UPDATELAG, 3 hyperelastic (total Lagrange),
                            // 4..6: the three flags again for Mohr-Coulomb / Drucker-Prager (nl_group_flag, nl_group_yield),
                            // 7, 8: INFINITE / TOTALLAG of a viscoelastic material (fx_visco.h: there pl = mu_0, gfac, tincr and
                            // tab = ntab rows (exp_n, dq_n), rewritten by fx_nl_set_time), 9: UPDATELAG of a NORTON material
                            // (pl = aa, n, tincr, rewritten by fx_nl_set_time)
  int32_t ntab;
  const double *tab;  // device, ntab rows (yield stress, plastic strain)
  double pl4;         // M_PLCONST4: xi of Drucker-Prager
};
static_assert(sizeof(NlMat) == 72 && offsetof(NlMat, plastic) == 40 && offsetof(NlMat, harden) == 44 && offsetof(NlMat, group) == 48 &&
                  offsetof(NlMat, tab) == 56 && offsetof(NlMat, pl4) == 64,
              "NlMat is an argument of every element kernel: every member keeps the offset it had before the hyperelastic kinds; the "
              "struct grew from 64 to 72 bytes by M_PLCONST4 at its end, which only Drucker-Prager reads");

// fstr_solid members of the nonlinear static loop (m_fstr.f90:560-700), resident.
// Elements grouped by colour (fxo::color_elements): the atomic-free scatter of the stiffness kernels.
struct ElemColors {
  int32_t n_elem = 0;
  uint64_t key = 0;                 // checksum of the connectivity the colouring belongs to
  int32_t etype = 361;              // element type of that connectivity (361, 341, 342, 351, 352, 362): a map of one type is never used for another
  int32_t *order = nullptr;         // device: element ids, colour by colour
  std::vector<int32_t> offsets;     // host: first position of each colour (+ end); empty = not coloured (atomics)
  int32_t *pos = nullptr;           // device: nn^2 per element, position of block (a, b) in AL / AU (k_scatter_map), or null
  bool dup_nodes = false;           // an element names a node twice: two of its blocks coincide, no first-write flags
  int32_t *dup = nullptr;           // device: those elements (collapsed hexahedra), colour by colour; they are not in `order`
  std::vector<int32_t> dup_off;     // host: first position of each colour in `dup` (+ end); empty = none
  bool first_write = false;         // pos carries the first-write flags (k_scatter_first_flag) and every block of the profile is covered:
                                    // the coloured scatter stores the first contribution to a block and the matrix is not cleared first
};

// The one cache of the linear assembly (fx_assemble_c3d8, _sections, fx_assemble_c3 and fx_assemble_groups all run the group
// driver; a single-type call is one group): one ElemColors per group (by position in the call), and the first-write flags of
// their maps in the launch order of ALL groups (group after group, colour after colour).
struct AsmGroups {
  std::vector<ElemColors> ec;
  uint64_t flag_sig = 0;     // checksum of the (key, etype, n_elem) sequence the maps' first-write flags were made for; 0 = none
  bool first_write = false;  // the maps carry those flags and every block of the profile is covered: no clearing
};

// One list of faces (or, shape 2, of whole elements under a body flux) of the surface terms of a heat analysis: the faces as
// elements of nn nodes with a colouring and, for !FILM and !RADIATE, a position map of their own.
struct HeatFaceList {
  uint64_t key = 0;            // checksum of the (group, element, face) entries and of the group's connectivity; 0 = none
  int32_t n = 0, nn = 0;       // faces, nodes per face
  int32_t *conn = nullptr;     // device: n x nn node ids, in the routine's NOD order
  int32_t *src = nullptr;      // device: position of each face in the caller's list (its val and sink)
  ElemColors ec;
};

// The one cache of the heat assembly (fx_heat.h): the caller's scalar profile with room for its values, one ElemColors per
// group (by position in the call; `pos` is the position map into that profile, without first-write flags: the matrix is cleared),
// the quadrature tables of the element types used so far, and what the tests read through fx_heat_get_stats.
struct HeatAsm {
  uint64_t prof_key = 0;  // checksum of the profile the device copy (and every map) belongs to; 0 = none
  int32_t NP = 0, NPL = 0, NPU = 0;
  int32_t *indexL = nullptr, *itemL = nullptr, *indexU = nullptr, *itemU = nullptr;
  double *D = nullptr, *AL = nullptr, *AU = nullptr, *B = nullptr;
  std::vector<ElemColors> ec;
  double *rule[6][2] = {};  // per type (341, 342, 351, 352, 361, 362): conductivity and capacity tables (H, dR, dS, dT, W)
  int64_t n_colourings = 0, n_maps = 0, n_profile = 0, n_calls = 0, copy_us = 0;
  // the surface terms (fx_heat_bc.h): one list per (kind, group, face shape), kept while the caller's list stays the same
  std::vector<HeatFaceList> fl;
  double *frule[4] = {};   // face point tables (H, d1, d2, W) of the 4-node and 8-node quadrilateral, the 6-node triangle and
                           // heat_DFLUX_352's collapsed triangle
  double *bfrule[6] = {};  // per type: the volume points of heat_DFLUX_3xx (H, dR, dS, dT, W)
  hipEvent_t ev_surf = nullptr;  // between the element kernels and the surface kernels
  int64_t n_face_colourings = 0, n_face_maps = 0, elem_us = 0, surf_us = 0;
};

// Pinned host staging of the results of the linear stress update (grown on demand, owned by the context): 2 x 6 nq doubles per
// element would otherwise cross PCIe through pageable memory at a fraction of the link rate.  The pointers an update returns
// are valid until the next update or prepare on the same context, or fx_destroy.
struct UpdStage {
  double *strain = nullptr, *stress = nullptr;
  size_t cap = 0;     // doubles per array
  std::thread maker;  // pinning 2.5 GB of host memory takes 0.3 s at 3.3M elements: the *_prepare entry points do it beside the solve
  int make_err = 0;   // the maker's result: read only after the join (upd_stage_wait)
};

// fstr_NodalStress3D on the device (fx_nodal_stress.h).  NodalList: per node, in the reference's order of addition, the pairs of
// vertex records its value is made of; built on the host once per (n_node, groups, connectivity) and kept like the colourings.
struct NodalList {
  uint64_t key = 0;          // checksum of what it was built for (fx_nodal_stress_groups); 0 with fx_nl_nodal_stress, whose list lives as long as the nonlinear context
  int32_t n_node = 0;
  int64_t n_elem = 0, n_rec = 0, n_ent = 0;  // elements, vertex records and list entries of all groups
  int32_t *row = nullptr;    // device: n_node + 1
  int2 *ent = nullptr;       // device: n_ent pairs (record a, record b); a == b: that record, else the half-sum of the two
  int64_t builds = 0;        // lists made on this context (fx_nodal_get_stats)
};
// Results of the pass: one device block and its pinned host copy (the pointers of fx_nodal_result), the vertex records, the error word.
struct NodalStage {
  double *dev = nullptr, *host = nullptr;
  size_t cap = 0;            // doubles of each
  double *rec = nullptr;     // device: 12 doubles per record
  size_t rec_cap = 0;
  int32_t *err = nullptr;
};

// Distributed loads (fx_dload.h).  A checked fx_dload list on the device: one batch per face shape (3, 4, 6, 8 nodes; kind 0..3,
// the faces of all groups together) and one per element type with volume entries (kind 4..9: 341, 342, 351, 352, 361, 362).
struct DloadBatch {
  int kind = 0;
  int32_t n = 0;
  int32_t *nodes = nullptr;  // device: n x (nodes of the face | of the element), 1-based node ids in getSubFace's / the element's order
  double *par = nullptr;     // device: n x 8, PARAMS(0:6) and RHO of the entry's element
  uint8_t *held = nullptr;   // device: n, 1: the entry takes factor 1
  int32_t *ltype = nullptr;  // device: n, DL_C3's LTYPE
  // Empty: one launch over the n entries.  Otherwise the entries are sorted by colour, colour k is color_off[k]..color_off[k+1] and
  // gets a launch of its own: no two entries of a colour share a node, so every address is added to in the order of the launches
  std::vector<int32_t> color_off;
};
struct DloadList {
  std::vector<DloadBatch> b;
  int64_t count[5] = {0, 0, 0, 0, 0};  // entries on triangles, on quadrilaterals, BX / BY / BZ, GRAV, CENT
};
struct DloadCtx {  // what fx_dload_get_stats reads (the list of an fx_dload_groups call is freed when the call ends)
  hipEvent_t ev_mid = nullptr;  // between the face kernels and the volume kernels
  int64_t count[5] = {0, 0, 0, 0, 0}, face_us = 0, vol_us = 0;
};

// One element group of the nonlinear context: its type, connectivity and colouring.  The element kernels index the history,
// conn and emat by the element id inside their group, so a part hands them pointers offset to its block of the shared arrays.
constexpr int NL_GROUPS = 10;  // compile-time groups of the nonlinear element kernels (nl_group_flag, fx_nl_point.h)
struct NlPart {
  int32_t etype = 361;                // 361 (B-bar, or F-bar: fbar), 341, 342, 351, 352 or 362
  bool fbar = false;                  // a 361 part of F-bar elements (elemopt 4): k_nl_stiffness_fbar / k_nl_update_fbar
  int nn = 8, nq = 8;                 // its nodes and quadrature points per element
  int32_t n_elem = 0;
  int64_t elem_off = 0, pt_off = 0;   // elements / quadrature points of the parts before this one
  size_t k_off = 0, qf_off = 0;       // doubles of the parts before this one in the element outputs ((3 nn)^2 and 3 nn per element)
  int32_t *conn = nullptr;            // device, nn * n_elem
  int32_t *emat = nullptr;            // device, 1-based material id per element; null with one material
  ElemColors colors;                  // order: elements grouped by NLGEOM flag, then by colour; pos: scatter position map
  std::vector<int32_t> grp_off[NL_GROUPS];  // per group (0 INFINITE, 1 TOTALLAG, 2 UPDATELAG, 3 hyperelastic, 4..6 Mohr-Coulomb / Drucker-Prager, 7, 8 viscoelastic, 9 NORTON): positions of its colours in order (+ end)
  std::vector<int32_t> dup_off[NL_GROUPS];  // per group: its collapsed elements' colours in colors.dup (+ end); empty = none
  bool scatter_atomic = false;        // colouring failed (a node in more than 64 elements) or FX_ASM_ATOMIC=1: one range per group, fp64 atomics
  int32_t n_dup = 0;                  // collapsed elements taken out of the colours (colors.dup)
};

// tGaussStatus (mechgauss.f90:13-22), flat over (element, quadrature point): the seven per-point arrays of the context, or one
// part's block of them (nl_part_state)
struct NlPartState {
  double *stress = nullptr, *strain = nullptr, *stress_bak = nullptr, *strain_bak = nullptr;  // 6 per point
  double *plstrain = nullptr, *fstat = nullptr;                                               // 1 per point
  int32_t *istat = nullptr;
};
// f(bytes per point, that array of every struct given) for the seven, in this order; true: an f returned non-zero and the rest
// was not visited.  A new piece of history is one member above and one term here.
template <class F, class... S>
static bool for_each_point_array(F &&f, S &...s) {
  return f((size_t)48, s.stress...) || f((size_t)48, s.strain...) || f((size_t)48, s.stress_bak...) || f((size_t)48, s.strain_bak...) ||
         f((size_t)8, s.plstrain...) || f((size_t)8, s.fstat...) || f((size_t)4, s.istat...);
}

// The context of the nonlinear static loop: element groups (parts) of the six solid types over one set of nodes, materials and
// per-point arrays.  fx_nl_init / _sections / _c3 / _type make the one-part case, fx_nl_init_groups any number of parts.
struct NlDev {
  bool ready = false;
  std::vector<NlPart> parts;          // in the order given; the per-point arrays and the element outputs hold them one after the other
  std::vector<int32_t> group_part;    // the caller's group position -> index into parts, -1: an empty group (no part is made for it)
  std::vector<int32_t> group_etype;   // the caller's group position -> its etype (the empty groups' too)
  bool first_write = false;           // every part's map carries first-write flags in the launch order of ALL parts and every block is covered: no clearing
  bool has_yield = false;             // a Mohr-Coulomb or Drucker-Prager section: the stress update reports through the error word too
  bool has_creep = false;             // a NORTON section: so does its creep iteration (FX_CERR_CREEP)
  bool has_fbar = false;              // an F-bar part: so does its stress update (`too small element volume`, `too small average jacob`)
  int32_t n_mat = 1;
  NlMat *mats = nullptr;              // device, n_mat entries (several sections); null with one material
  std::vector<NlMat> h_mats;
  std::vector<double *> tabs;         // device tables of the materials
  int32_t n_elem = 0, n_bc = 0;       // n_elem: all parts'
  int64_t n_pt = 0;                   // quadrature points of all parts
  size_t n_k = 0, n_qf = 0;           // doubles of the element outputs of all parts
  NlMat mat = {};
  double *tab = nullptr;
  double *coord = nullptr;
  NlPartState st;                     // the per-point arrays of all parts
  double *unode = nullptr, *dunode = nullptr, *qforce = nullptr, *GL = nullptr;  // 3*NP
  uint8_t *bc_flag = nullptr;   // prescribed dofs of the current step (3*NP)
  double *bc_val = nullptr;     // their values (3*NP)
  int32_t *bc_node = nullptr, *bc_dof = nullptr;
  double *bc_v = nullptr;
  int32_t bc_cap = 0;
  int32_t *err = nullptr;
  double maxres = 1.0e10;  // step_ctrl%maxres (m_step.f90:78): Newton gives up when rres exceeds it
  bool is_linear = false;   // fstr_Newton's isLinear: one pass, no convergence test
  int latch = 0;  // MatlMatrix's saved `flag` (calMatMatrix.f90:39): set by the first elastoplastic stress update
  // Time of the coming sub-step or call (fx_nl_set_time): ctime and tincr as fstr_Newton hands them to fstr_StiffMatrix,
  // fstr_UpdateNewton and fstr_UpdateState (fstr_solve_NonLinear.f90:74, :100, :162); (0, 0) after every fx_nl_init*
  double time = 0.0, tincr = 0.0;
  // History of the viscoelastic and NORTON points (fx_visco.h), allocated only where such a material is present: hist_w components per point,
  // component-major over all points of the context (hist[k * n_pt + p]); hist_bk: fx_nl_snapshot's copy
  int32_t hist_w = 0;
  double *hist = nullptr, *hist_bk = nullptr;
  std::vector<std::vector<double>> prony;  // per material: its rows (g, tau) as given, or (A, n, m) of a NORTON material; empty for another kind
  // fstr_cutback_save / _load (fstr_Cutback.f90:108-198): a device-side copy of the quadrature-point history to roll back to when a
  // sub-step of an automatic incrementation does not converge (fx_nl_snapshot); allocated at the first save
  NlPartState bk;
  bool bk_valid = false;
  // Thermal strain (fx_nl_set_thermal; NlThermalDev of fx_nl_point.h is made from these).  Off: every pointer null, and the
  // launchers take the instantiations without the switch.
  struct Thermal {
    bool on = false;
    bool elastic_tab = false;         // some material has an E(T), nu(T) table: the tangent kernels' thermal variant is launched
    bool any_tab = false;             // some material has a table of either kind: the thermal load looks them up at the point
    double ref_temp = 0.0;
    double *temp = nullptr, *last_temp = nullptr, *temp_init = nullptr, *last_temp_bk = nullptr;  // NP each
    double *alpha = nullptr;          // n_mat
    double *tabs = nullptr;           // the tables of all materials, one after the other
    double *xc = nullptr;             // 3 NP: coord + unode, the configuration the thermal load is taken on (nl_thermal_load)
    double *mtab = nullptr;           // n_mat x (D11, D12, D44) of the constants E, nu: what the thermal-load kernels take per material
    double D0[3] = {0.0, 0.0, 0.0};   // material 1's, the kernels' by-value arguments
    bool bk_valid = false;            // last_temp_bk holds a saved last_temp of THIS thermal set-up
    int32_t *tab_idx = nullptr;       // per material: offset and rows of its alpha table (alpha, T), offset and rows of its elastic table (E, nu, T)
  } th;
  // Distributed loads (fx_nl_set_dload).  Off: nothing allocated, and every fx_nl_* call runs what it ran without them.
  struct Dload {
    bool on = false, follow = false;  // follow: DLOAD_follow, the load is taken on the current configuration and rebuilt in every iteration
    double factor = 1.0;              // fstrSOLID%factor(2) of the sub-step (fx_nl_set_dload_factor; fx_newton_substep sets factor1)
    DloadList list;
    double *nodal = nullptr;          // 3 NP: the nodal part of GL, kept aside so that GL can be rebuilt
  } dl;
};

// TIMELOG (hecmw_solver_Iterative.f90:192-208): device time of the three phases the reference reports -- solver/matvec
// (hecmw_matvec_get_timer, comm excluded as las_33.f90:345-349 does), solver/precond (hecmw_precond_get_timer), solver/comm --
// from HIP event pairs on the solver stream, collected whenever the host polls the Krylov state.  Off unless Iarray(22) >= 1.
struct PhaseClock {
  bool on = false;
  std::vector<hipEvent_t> ev;   // pairs: start, stop
  std::vector<int> kind;        // per pair: 0 matvec, 1 precond, 2 comm
  int used = 0;                 // pairs recorded since the last collect
  int open_kind[4] = {-1, -1, -1, -1};
  int depth = 0;
  double acc[3] = {0.0, 0.0, 0.0};  // seconds
};

// The value arena (round 4).  Where hipMalloc puts a BELL value array PHYSICALLY decides the speed class of the sweep that streams it:
// the identical SpMV on identical data runs at 1.03-1.05 ms or at 1.18 ms (10.1M DOF), and a fresh power-of-two request is a
// lottery between the two (scripts/r4/region_probe.py: 5 of 14 consecutive 8 GiB blocks slow on one box, the first allocation of
// the process among them).  What was ruled out with measurements of ONE context whose arrays were moved between allocations
// (scripts/r4/*.py, profiles/r04_placement_evidence.txt): the vectors x / y (twelve choices within 0.3 %), the column ids, the
// row pointers, the workgroup -> XCD map (eight maps within 1 %), the slice order, address translation (TCP_UTCL1 misses equal
// in both classes: 47.6k of 171M requests).  What holds on every box measured: inside ONE large allocation taken before anything
// else every offset runs in the same fast class (1.044-1.048 ms at sixteen offsets of a 64 GiB block on a box whose first
// power-of-two block ran at 1.180).  So the context takes one arena when it first learns the size of a large system -- before the
// CSR arrays, the layouts and the vectors -- and the value arrays of M, L and U live in it at 2 MiB-aligned offsets (first fit; the holes a rebuilt layout leaves are re-used).
// FX_ARENA_GB: 0 = off (every array its own hipMalloc), n = arena of at least n GiB (default 32), always a power of two.
struct DevArena {
  char *base = nullptr;
  size_t bytes = 0;
  std::vector<std::pair<size_t, size_t>> blocks;  // (offset, bytes) of the arrays placed in it, by offset: first fit at 2 MiB-aligned offsets
  size_t used() const { size_t u = 0; for (auto &b : blocks) u += b.second; return u; }
  int live() const { return (int)blocks.size(); }
};

// One pass of the auto-SIGMA_DIAG / METHOD2 loop of hecmw_solve_iterative (hecmw_solver_Iterative.f90:117-157): what the reference
// prints per pass (banner, ITERLOG lines, 'Increasing SIGMA_DIAG to') is replayed by the binding from this log.
struct AttemptLog {
  int method = 0;
  double sigma_diag = 1.0;       // SIGMA_DIAG in effect during the pass
  std::vector<double> hist;      // its residual-history lines
};

// What this rank asked of the transport, in program order: every all-reduce and every halo exchange (per neighbour: messages and
// bytes each way) since the communicator was set up.  All ranks of a correct run hold the same op count and the same sequence hash
// (the kinds and sizes of the collectives and the positions of the halo exchanges between them), and rank r's sends to p equal p's
// receives from r: bench.py --gpus N compares the ledgers over its gloo control plane (fx_comm_ledger), and its watchdog prints the
// local one when a step does not come back -- a mismatch shows as a message with the op index, not only as a hang.
struct CommLedger {
  int64_t n_ops = 0, n_allreduce = 0, allreduce_bytes = 0, n_halo = 0;
  uint64_t seq_hash = 1469598103934665603ull;  // FNV-1a over (kind, size) of the ops in order
  std::vector<int64_t> peer;                   // 5 per neighbour: rank, sends, send bytes, receives, receive bytes
  void mix(uint64_t v) { for (int k = 0; k < 8; k++) { seq_hash ^= (v >> (8 * k)) & 0xff; seq_hash *= 1099511628211ull; } }
};

struct fx_context {
  CommLedger ledger;
  void *nccl_halo = nullptr;  // the halo exchange's own communicator (ncclCommSplit of nccl; null: the exchanges share nccl)
  std::vector<AttemptLog> attempts;  // of the last fx_solve / fx_solve_resident (fx_solve_attempts)
  int device = 0;
  int n_cu = 256;  // compute units of the device
  hipStream_t stream = nullptr;
  DevCSR A;
  Ordering ord;
  Bell M;  // full matrix (D + AL + AU) in slot order, for SpMV
  bool have_profile = false, have_values = false, bell_valid = false;
  bool m_symbolic = false;   // M's source map matches the current ordering
  double *Bs = nullptr, *Xs = nullptr;  // B, X in slot space
  // host copies of the profile (ordering, conversion maps)
  std::vector<int32_t> h_indexL, h_itemL, h_indexU, h_itemU;
  // preconditioner
  int precond_kind = 0;  // 0 none, 1 SSOR (multicolour), 3 DIAG, 10 ILU0, 11 SSOR in the natural order (level-scheduled like ILU0)
  // PRECOND = 1 / 2 in the reference is TWO preconditioners: with one OpenMP thread the natural-order block Gauss-Seidel, with more
  // the RCM + multicolour ordering (hecmw_precond_SSOR_33.f90:93-114; 143 vs 204 iterations on SURVEY section 0's cube).  The GPU
  // default is the multicolour one (bandwidth-bound colour sweeps); FX_SSOR_NATURAL=1 / fx_set_option selects the other, whose
  // sweeps run level by level through the dataflow launch of ILU(0) (latency-bound: 1,044 levels at 150^3 nodes).
  bool ssor_natural = false;
  DiagDev diag;
  SsorDev ssor;
  bool precond_valid = false;
  int ssor_ncolor_in = 0;
  // SSOR numbering mode: 0 = Krylov vectors natural, sweep vector colour-major (hybrid);
  //                      1 = the whole Krylov loop in colour-major numbering (default).  FX_SSOR_MODE overrides.
  // Same-process A/B at 10.1M DOF with the tuned kernels: mode 0 336 it/s (SpMV 1.11 ms, SSOR 1.61 ms),
  // mode 1 351 it/s (SpMV 1.15 ms, SSOR 1.46 ms).
  int ssor_mode = 1;
  int ssor_mode_built = -1;   // ssor_mode the resident multicolour SSOR was set up in (a live FX_SSOR_MODE change re-runs its symbolic set-up)
  int ssor_spw = 1;            // consecutive slices per wave in the big-colour sweeps (FX_SSOR_SPW)
  int ssor_bs = 64;            // workgroup size of the colour sweeps: 64 (default) or 256. Measured 10M DOF: 1.78 -> 1.61 ms per apply
  int pipe_max_slices = 1 << 30;  // colours with more slices use the plain row loop (with 64-thread groups: pipelined everywhere wins, 1.61 vs 1.64/1.69 ms)
  int spmv_bs = 256;              // workgroup size of the SpMV (FX_SPMV_BS)
  // Colour-/level-major vectors: the SpMV walks the slices in SPATIAL order (slices of all colours that cover the same
  // part of the mesh next to each other), so the x entries a region gathers stay in L2 across its colours.  The data
  // layout is untouched; only the block -> slice map changes.  FX_SPMV_SPATIAL=0: ascending slices.
  bool spmv_spatial = true;
  // The wave-split sweep (k_ssor_color_split, split_wps waves per slice: each wave issues all the loads of its block pairs at
  // once, partial sums meet in LDS in a fixed order) hides latency by occupancy (64 VGPRs, 8 waves per SIMD) instead of the
  // software pipeline of k_ssor_color (174 VGPRs, 2 waves per SIMD).  Round 1-2: used for latency-bound launches only (colours /
  // ILU levels of <= 2048 slices): SSOR apply 1.46-1.49 -> 1.415 ms, ILU(0) level sweeps 19.9 -> 10.7 ms.  Round 3, same context
  // (scripts/r3/ab_opts.py): EVERY colour wave-split 1.502 -> 1.478 ms per apply, Eisenstat iteration 1.918 -> 1.871 ms; forcing the
  // pipelined kernel to 3 waves per SIMD (__launch_bounds__(BS, 3): 168 VGPRs + 6-8 spills) 1.47 -> 1.58 ms.  So the default is
  // "all colours"; FX_SPLIT_MAX_SLICES brings the pipelined kernel back for larger colours, FX_SPLIT_WPS (2, 4, 8; 0 = auto:
  // 8 for ILU(0) levels, 4 for SSOR colours) sets the waves per slice.
  int split_max_slices = 1 << 30;
  int split_wps = 0;
  // Dataflow triangular sweeps (k_tri_dataflow): one persistent launch per apply, rows synchronised through
  // sentinel-tagged data instead of one launch per colour / level.  FX_DATAFLOW=0 off, 1 (default) ILU(0) levels and the
  // latency-bound tail colours of the fused Eisenstat sweeps (k_eis_*_df, eis_tail),
  // 2 also the multicolour SSOR (measured slower than the colour launches: 1.59-1.71 against 1.50 ms per apply -- the big
  // colours are bandwidth-bound and a few hundred workgroups with one slice each in flight do not saturate HBM).
  // FX_DF_GRID workgroups (default: one per two CUs), FX_DF_WPS waves per slice (2, 4, 8), FX_DF_POLL 0 = every poll
  // re-reads all entries, 1 = only the unpublished ones, FX_DF_SLEEP s_sleep(1)s between polls.
  // Measured at 10.1M DOF, ILU(0), 1,044 levels (same process, scripts/experiments/ab_dataflow3.py): launch per level
  // 10.7 ms per apply; dataflow 4.80-4.87 ms with 128 workgroups x 8 waves (96: 5.3, 160: 4.89, 192: 4.92, 256: 5.0-5.1,
  // 512: 8.0; 4 waves per slice 5.2; re-reading all entries per poll 5.6; two polls in flight 5.9; 0.4-1.5 us of sleep
  // between polls 4.9-5.3): 2,088 dependent hand-offs of ~2.3 us each -- the polls of the waiting workgroups compete
  // with the frontier's hand-offs, so fewer pollers and fewer re-read entries are faster.
  // Round 3, same context (scripts/r3/ab_opts.py, ILU(0) at 10.1M DOF): sweep vectors in the [slice][k][lane] layout (df_soa) 4.73 -> 4.44 ms
  // per apply; with that layout one workgroup per CU instead of one per two 4.44 -> 4.27; no sleep between polls 4.27 -> 4.20; the
  // hand-off vectors in uncached device memory 4.20 -> 4.15 (not kept); re-reading all entries per poll 5.11; 4 waves per slice 5.04.
  // Round 4: the re-reads of a polling pass are issued together (no branch, hence no wait, between them: df_gather) -- one round trip per
  // pass instead of one per missing entry: 4.19 -> 3.43 ms per apply; with that, re-reading every entry per pass (FX_DF_POLL=0) is the
  // faster form, 3.33 ms (scripts/r3/ab_opts.py, same context), and the default.
  int df_mode = 1, df_grid = 0, df_wps = 8, df_poll = 0, df_sleep = 0;
  int df_presleep = 2;        // FX_DF_PRESLEEP: x 0.1 us of sleep per level of lead before a workgroup starts to poll for its next slice (round 4, same context: 0 -> 3.27, 1 -> 3.14, 2 -> 3.13, 3 -> 3.13, 5 -> 3.16, 8 -> 3.24, 12 -> 3.57 ms per apply)
  bool df_soa = true;         // private sweep vectors of the dataflow sweeps in the [slice][k][lane] layout (FX_DF_SOA=0: 3 s + k)
  int df_grid_max[3] = {128, 128, 128};  // co-resident workgroups of k_tri_dataflow<2 / 4 / 8 waves> (occupancy query at fx_create)
  int df_grid_last = 0;       // workgroups of the last dataflow launch (after the co-residency clamp)
  bool dbg_df_fail = false;   // test hook (FX_DEBUG_DF_FAIL): the dataflow launches report a timeout at once
  int df_fallbacks = 0;       // times a timed-out dataflow sweep made this context fall back to the launch-per-level sweeps (fx_get_stats)
  int32_t *df_err = nullptr;  // device: raised by a sweep whose bounded spin ran out
  // Plane march (fx_march.h, k_tri_march): the level-scheduled sweeps (ILU(0), natural-order SSOR) with whole chunks of rows per
  // workgroup, dependencies inside a chunk through an LDS ring, between chunks through the sentinel-tagged vectors.  FX_MARCH=0 (default)
  // off: bit-identical to k_tri_dataflow but, as measured at 10.1 M DOF, slower (6.3 against 3.3 ms per apply; DESIGN.md section 4 has the
  // per-round timeline); 1 when the cost model prefers it, 2 whenever the structure admits it.  FX_MARCH_CHUNK rows per chunk (0 = from
  // the matrix profile), FX_MARCH_WAVES pair waves per workgroup (1, 2, 3; 0 = from the level sizes).
  int march_mode = 0, march_chunk = 0, march_waves = 0, march_grid = 0, march_xcd = 1;
  int march_grid_max[4] = {0, 0, 0, 0};  // co-resident workgroups of k_tri_march<1 / 2 / 3 pair waves>
  int march_launches = 0;                // applies that took the march (fx_march_report)
  // software-pipelined row loop (2-deep: values + gathers of pair i+1 and ids of pair i+2 in flight while pair i
  // is multiplied; 116 VGPRs, 4 waves/SIMD).  Measured on MI355X at 10.1M DOF with the final layout (odd-tail BELL,
  // non-temporal stream loads): SpMV 1.14-1.17 -> 1.105-1.11 ms; colour sweeps 1.685 -> 1.61 ms per apply.
  // (With the earlier padded layout it cost the SpMV 1.19 -> 1.30 ms: re-measure when the layout changes.)
  bool pipe_spmv = true, pipe_ssor = true;  // FX_PIPE_SPMV / FX_PIPE_SSOR override
  // Eisenstat's form of CG + SSOR (the default since round 4; FX_EISENSTAT=0 runs hecmw_solve_CG's loop as written): with
  // M = (D~+L) D~^-1 (D~+U) and A = (D~+L) + (D~+U) + (D - 2D~), one backward and one forward triangular sweep per iteration deliver
  // p, q = A p and w = (D~+L)^-1 q -- the matrix is streamed ONCE instead of twice (SpMV + the two half sweeps).  Same x_k, r_k,
  // rho_k, alpha_k in exact arithmetic; the summation order of q and of the dot products differs, so histories agree to rounding
  // (the parity bounds of tests/test_gpu_parity.py hold in both modes), not bit for bit.  It is taken only where it is exact:
  // multicolour SSOR with iterPREmax = 1, colour-major numbering, preconditioner built from the resident values (subdomains: plus
  // the halo term H p); anything else -- a recycled preconditioner, iterPREmax != 1, BiCGSTAB -- runs the standard loop on its own.
  bool eisenstat = true, eis_active = false;
  // Eisenstat's form: rho of the NEXT iteration was already reduced together with ||r||^2 of the last one (OP_RESID_RHO: one scalar
  // stage -- on a decomposed system one 2-double all-reduce -- instead of two).  False after a begin, after an iteration that
  // recomputed the true residual and after a true-residual check: those refresh t and leave new rho partials (FX_EIS_MERGE=0: never).
  bool eis_rho_done = false, eis_merge = true;
  int eis_grid = 0;  // FX_EIS_GRID: most workgroups of one colour launch of the wave-split Eisenstat sweeps (a workgroup then walks slices b, b + grid, ...); 0 = one workgroup per slice
  bool dbg_onecolor = false; // measurement only (FX_DEBUG_ONECOLOR): the half sweeps as one launch each, dependencies ignored
  bool eis_fuse = true;      // direction update fused into the backward sweep (FX_EIS_FUSE=0: k_cg_update_p + the plain sweep)
  // The latency-bound tail of the fused Eisenstat sweeps as one dataflow launch per half sweep (k_eis_backward_df / k_eis_forward_df,
  // FX_DATAFLOW >= 1, one rank): the run of colours at the end of the colour order with at most EIS_TAIL_GRIDS x grid slices each.
  int eis_df_grid_max[2] = {128, 128};  // co-resident workgroups of k_eis_backward_df<4> / k_eis_forward_df<4> (occupancy query at fx_create)
  int eis_tail_color0 = 0, eis_tail_slices = 0, eis_tail_grid = 0;  // the tail of the last iteration: first colour, slices, workgroups
  int64_t eis_tail_launches = 0;        // dataflow tail launches enqueued (or captured) by this context
  int64_t values_epoch = 0;  // counts the refreshes of the SpMV layout's values
  bool layout_device = true;        // BELL source maps built by k_bell_count / k_bell_map (FX_LAYOUT_DEVICE=0: host threads)
  int32_t mc_batch = 32;            // rounds of the device multicolouring between two looks at the queue length by the host (FX_MC_BATCH)
  int32_t mc_device_min = 100000;   // block rows from which the multicolouring of the SSOR set-up runs on the device (FX_MC_DEVICE_MIN)
  bool val2_pow2 = true;            // BELL value arrays of a gigabyte or more that do not fit the arena: ask hipMalloc for the next power of two (FX_VAL2_POW2=0: the exact size)
  DevArena arena;                   // the value arena of this context (see DevArena)
  // The arena makes the class the same for every array and every offset, it does not make it the fast one: a box was met whose
  // first 32 GiB were a slow region (SpMV 1.17 ms in 8 of 8 processes).  So the arena is VERIFIED once, when M's values are first
  // filled: the loop's own SpMV (p = W[2] -> q = W[1], fused p.q partial) is timed on it (1 untimed + 3 launches, 5 ms); below
  // arena_good_gbs the context takes ANOTHER arena (the earlier ones held meanwhile, so that it is different memory), moves the
  // value arrays and times again, at most arena_tries arenas; the fastest is kept, the others are freed before the set-up returns.
  // Measured consistency of this timing with the loop's: within 0.3 % (profiles/r04_placement_evidence.txt, "loop" vs "probe").
  int arena_tries = 4;              // FX_ARENA_TRIES (1 = no verification)
  double arena_good_gbs = 6450.0;   // the fast classes stream 6.57-6.8 TB/s algorithmic, the slow ones 5.9-6.4
  std::vector<DevArena> arena_tried; // earlier arenas of a verification in progress (held so that the next request is different memory)
  std::vector<float> arena_ms;      // what the verification measured, in order (fx_placement_report)
  bool arena_verified = false;
  size_t arena_min_bytes = (size_t)32 << 30;  // FX_ARENA_GB (GiB, fractions allowed; 0 = no arena)
  size_t arena_threshold = (size_t)1 << 30;   // estimated value-array bytes from which a system gets an arena (FX_ARENA_THRESHOLD_MB)
  size_t arena_max_bytes = 0;                 // FX_ARENA_MAX_MB: never take more than this (0 = no cap); arrays that do not fit get their own allocations
  int32_t bfs_batch = 16;           // levels of the device level ordering between two looks at the level state by the host (FX_BFS_BATCH)
  int32_t bfs_device_min = 100000;  // block rows from which the level ordering of the SSOR set-up runs on the device (FX_BFS_DEVICE_MIN)
  // work vectors (3*NP each)
  double *W[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool precond_valid_sweeps = false;  // multicolour SSOR layouts filled
  int iterpremax = 1;  // additive-Schwarz sweeps of hecmw_precond_33_apply
  int32_t wlen = 0;
  double *scale_vec = nullptr;  // SCALING=YES: 1/sqrt|diag|, reference numbering, 3*NP (+ slack)
  double *extra = nullptr;  // further work vectors (GMRES basis, GPBiCG), extra_n x extra_len
  int extra_n = 0;
  int32_t extra_len = 0;
  // reductions
  double *partials = nullptr;  // 3 * max_partials
  int32_t max_partials = 0;
  double *red_out = nullptr;  // small device scratch for reduced sums (8 doubles)
  KrylovState *st = nullptr;   // device
  KrylovState *st_host = nullptr;  // pinned
  double *hist = nullptr;      // device residual history
  int32_t hist_cap = 0;
  int k_method = 1, k_maxit = 0, k_it = 1;  // host mirror of the running Krylov loop
  int k_method_last = 1;       // METHOD of the last fx_solve_resident attempt
  double host_dbg[16] = {0};   // scalars of the host-driven recurrences (fx_debug_state)
  // Launch-bound sizes (<= graph_max_rows block rows, single rank): one CG / BiCGSTAB iteration is captured once per
  // solve into hipGraphs (ordinary iteration; the one that recomputes r = b - A x; in Eisenstat's form each with / without its own rho stage) and replayed -- every kernel
  // argument is constant over a solve, what changes lives in the device-resident KrylovState.
  // FX_GRAPH=0 off, 1 auto (default: SSOR / ILU(0) only, where an iteration is 40+ launches), 2 always.
  int graph_mode = 1;
  int32_t graph_max_rows = 1 << 19;
  bool k_graph = false;
  hipGraphExec_t g_iter[4] = {nullptr, nullptr, nullptr, nullptr};  // by kind of iteration: bit 0 = recomputes the true residual, bit 1 = starts with its own rho stage
  // communication
  int rank = 0, nranks = 1;
  int view_petot = 1;        // PETOT of the comm view the profile came with (require_transport)
  int32_t nn_internal = 0;
  void *nccl = nullptr;
  // host-staged communication hooks (testing / non-RCCL transports): see fx_comm_set_host_callbacks
  void (*cb_halo)(const double *, double *, void *) = nullptr;
  void (*cb_allreduce)(double *, int, void *) = nullptr;
  void *cb_user = nullptr;
  double *h_send = nullptr, *h_recv = nullptr;  // pinned staging
  HaloDev halo;
  // Interior / boundary overlap of the SpMV (the design the reference sketched and left commented out,
  // hecmw_solver_las_33.f90:242-246, :312-343 with hecmw_solver_SR_33.F90:129-273): pack on the solver stream, the
  // exchange + unpack on comm_stream while the interior rows are multiplied, the boundary rows after it.  FX_OVERLAP=0: serial.
  bool overlap = true;
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_packed = nullptr, ev_halo = nullptr;
  NlDev nl;
  AsmGroups asm_groups;   // the linear assembly entry points
  UpdStage upd_stage;     // the linear stress update entry points
  HeatAsm heat;           // fx_heat_assemble_groups
  DloadCtx dload;         // fx_dload_groups
  NodalList nodal_list, nodal_list_nl;  // fx_nodal_stress_groups; fx_nl_nodal_stress (freed with the nonlinear context)
  NodalStage nodal_stage; // both
  void *nn = nullptr;  // NnDev (fx_nn_host.h): systems with NDOF != 3
  const void *host_D = nullptr, *host_AL = nullptr, *host_AU = nullptr;  // the caller's arrays of the last value upload (fx_solve)
  // timing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  PhaseClock clock;
};

