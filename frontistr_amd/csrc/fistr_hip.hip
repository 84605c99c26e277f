// libfistr_hip: MI355X-native HEC-MW linear-solve hot path behind the C ABI of
// include/fistr_hip.h.  Host orchestration; the kernels live in fx_kernels.h /
// fx_assemble.h.  gfx950 only -- there is no CPU fallback anywhere in this library.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <thread>

#include "fx_assemble.h"
#include "fx_assemble_tet.h"
#include "fx_assemble_c3.h"
#include "fx_kernels.h"
#include "fx_nonlinear.h"
#include "fx_nonlinear_fbar.h"
#include "fx_nonlinear_tet.h"
#include "fx_nonlinear_c3.h"

namespace fxo {
struct Graph {
  int32_t n = 0;
  std::vector<int64_t> ptr;
  std::vector<int32_t> adj;
};
Graph build_graph(int32_t N, const int32_t *indexL, const int32_t *itemL, const int32_t *indexU,
                  const int32_t *itemU);
std::vector<int32_t> rcm_sequence(const Graph &g);
std::vector<int32_t> rcm_starts(const Graph &g);
std::vector<int32_t> rcm_starts_deg(int32_t n, const int32_t *deg);
int32_t level_order_host(const Graph &g, int32_t start, std::vector<int32_t> &seq);
void multicolor(const Graph &g, const std::vector<int32_t> &seq, int ncolor_in, std::vector<int32_t> &perm,
                std::vector<int32_t> &colorindex);
bool color_elements(int32_t n_elem, int nn, const int32_t *conn, int32_t NP, std::vector<int32_t> &order,
                    std::vector<int32_t> &offsets);
}  // namespace fxo

thread_local std::string g_fx_error;

int fx_fail(const char *what, const char *file, int line) {
  char buf[64];
  snprintf(buf, sizeof buf, " (%s:%d)", strrchr(file, '/') ? strrchr(file, '/') + 1 : file, line);
  if (g_fx_error.empty()) g_fx_error = what;
  g_fx_error += buf;
  return FX_ERROR_RUNTIME;
}

// RCCL is bound lazily (dlopen) the first time a communicator is requested: single-GPU runs never
// load the 0.5 GB library, and a process that already holds an RCCL (e.g. through torch.distributed)
// shares that copy instead of mixing two.
struct RcclApi {
  void *h = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*CommCuDevice)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*CommSplit)(ncclComm_t, int, int, ncclComm_t *, void *) = nullptr;  // optional (RCCL >= 2.18)
};
static RcclApi g_rccl;

static int rccl_load() {
  if (g_rccl.h) return 0;
  const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char *n : names) {
    g_rccl.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (g_rccl.h) break;
  }
  if (!g_rccl.h) { g_fx_error = std::string("cannot load RCCL: ") + dlerror(); return FX_ERROR_RUNTIME; }
#define RCCL_SYM(field, name)                                                                  \
  g_rccl.field = (decltype(g_rccl.field))dlsym(g_rccl.h, name);                                  \
  if (!g_rccl.field) { g_fx_error = std::string("RCCL symbol missing: ") + name; return FX_ERROR_RUNTIME; }
  RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
  RCCL_SYM(CommInitRank, "ncclCommInitRank")
  RCCL_SYM(CommDestroy, "ncclCommDestroy")
  RCCL_SYM(GroupStart, "ncclGroupStart")
  RCCL_SYM(GroupEnd, "ncclGroupEnd")
  RCCL_SYM(Send, "ncclSend")
  RCCL_SYM(Recv, "ncclRecv")
  RCCL_SYM(AllReduce, "ncclAllReduce")
  RCCL_SYM(GetErrorString, "ncclGetErrorString")
  RCCL_SYM(CommCount, "ncclCommCount")
  RCCL_SYM(CommCuDevice, "ncclCommCuDevice")
#undef RCCL_SYM
  g_rccl.CommSplit = (decltype(g_rccl.CommSplit))dlsym(g_rccl.h, "ncclCommSplit");
  return 0;
}

#define NCCL_TRY(expr)                                                       \
  do {                                                                       \
    ncclResult_t _e = (expr);                                                \
    if (_e != ncclSuccess) {                                                 \
      g_fx_error = std::string(#expr) + ": " + g_rccl.GetErrorString(_e);    \
      return fx_fail(g_fx_error.c_str(), __FILE__, __LINE__);                \
    }                                                                        \
  } while (0)

struct PhaseTimer {  // FX_TIMING=1: wall time of the host-side set-up phases on stderr
  double t0;
  bool on;
  const char *what;
  explicit PhaseTimer(const char *w);
  void lap(const char *phase);
};
static double now_s();
PhaseTimer::PhaseTimer(const char *w) : t0(now_s()), on(getenv("FX_TIMING") && atoi(getenv("FX_TIMING")) != 0), what(w) {}
void PhaseTimer::lap(const char *phase) {
  if (!on) return;
  const double t = now_s();
  fprintf(stderr, "[fx timing] %s / %s: %.6f s\n", what, phase, t - t0);
  t0 = t;
}

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int nthreads_host() {
  const char *e = getenv("FX_HOST_THREADS");
  int n = e ? atoi(e) : (int)std::thread::hardware_concurrency();
  return std::max(1, std::min(n, 32));
}

template <class F>
static void parallel_for(int64_t n, F f) {
  const int nt = (int)std::min<int64_t>(nthreads_host(), std::max<int64_t>(1, n / 4096));
  if (nt <= 1) { f(0, n); return; }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++) {
    const int64_t a = n * t / nt, b = n * (t + 1) / nt;
    th.emplace_back([=] { f(a, b); });
  }
  for (auto &t : th) t.join();
}

template <class T>
static int dev_alloc(T **p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  HIP_TRY(hipMalloc((void **)p, count * sizeof(T)));
  return 0;
}
template <class T>
static void dev_free(T *&p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

// ---- PhaseClock (TIMELOG) ----
static int clock_collect(fx_context *c) {  // the stream must be idle (called right after a synchronize)
  PhaseClock &k = c->clock;
  for (int i = 0; i < k.used; i++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, k.ev[2 * i], k.ev[2 * i + 1]) == hipSuccess) k.acc[k.kind[i]] += 1e-3 * ms;
  }
  k.used = 0;
  return 0;
}
static int clock_begin(fx_context *c, int kind) {
  PhaseClock &k = c->clock;
  if (!k.on) return -1;
  if (k.used >= 512) {  // pool exhausted between two polls: drain it
    HIP_TRY(hipStreamSynchronize(c->stream));
    clock_collect(c);
  }
  if ((int)k.ev.size() < 2 * (k.used + 1)) {
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    k.ev.push_back(a); k.ev.push_back(b);
    k.kind.push_back(kind);
  }
  const int id = k.used++;
  k.kind[id] = kind;
  HIP_TRY(hipEventRecord(k.ev[2 * id], c->stream));
  return id;
}
static void clock_end(fx_context *c, int id) {
  if (id >= 0) (void)hipEventRecord(c->clock.ev[2 * id + 1], c->stream);
}
struct ClockScope {  // records the pair around a scope
  fx_context *c;
  int id;
  ClockScope(fx_context *ctx, int kind) : c(ctx), id(clock_begin(ctx, kind)) {}
  ~ClockScope() { clock_end(c, id); }
};

// Temporary device buffers of one entry point: released on every return path.
struct DevScratch {
  std::vector<void *> ptrs;
  template <class T>
  int alloc(T **p, size_t count) {
    if (dev_alloc(p, count)) return FX_ERROR_RUNTIME;
    ptrs.push_back((void *)*p);
    return 0;
  }
  ~DevScratch() {
    for (void *q : ptrs) (void)hipFree(q);
  }
};

static inline int grid_for(int64_t n, int per_block = FX_BLOCK, int cap = 256 * 16) {
  int64_t g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (int)std::min<int64_t>(g, cap);
}

// ---------------------------------------------------------------------------
// life cycle
// ---------------------------------------------------------------------------
extern "C" const char *fx_last_error(void) { return g_fx_error.c_str(); }
extern "C" const char *fx_version(void) { return "fistr_hip 0.1 (gfx950)"; }

#include "fx_march.h"  // the plane march of the level-scheduled sweeps: kernels, program builder, launch

static int context_init(fx_context *c) {
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  {  // the exchange must not queue behind the interior rows it overlaps with: highest priority the device offers
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, hi));
  }
  HIP_TRY(hipEventCreateWithFlags(&c->ev_packed, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_halo, hipEventDisableTiming));
  if (dev_alloc(&c->st, 1) || dev_alloc(&c->red_out, 16) || dev_alloc(&c->df_err, 4)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemset(c->df_err, 0, 16));
  HIP_TRY(hipHostMalloc((void **)&c->st_host, sizeof(KrylovState) * 4, hipHostMallocDefault));
  return 0;
}

// ---------------------------------------------------------------------------
// Tuning knobs of a context: ONE table, settable on a live context through fx_set_option (same data, same placement: what an
// A/B measurement needs) and, under the same names, from the environment at fx_create.  Defaults and what was measured with
// each knob: fx_internal.h.
// ---------------------------------------------------------------------------
static int spmv_walk(fx_context *c);
struct FxOption { const char *name; void (*set)(fx_context *, double); };
static const FxOption g_fx_options[] = {
    {"FX_ARENA_GB", [](fx_context *c, double v) { c->arena_min_bytes = v > 0.0 ? (size_t)(v * 1073741824.0) : 0; }},
    {"FX_ARENA_GOOD_GBS", [](fx_context *c, double v) { c->arena_good_gbs = v; }},
    {"FX_ARENA_TRIES", [](fx_context *c, double v) { c->arena_tries = std::max(1, std::min(8, (int)v)); }},
    {"FX_ARENA_MAX_MB", [](fx_context *c, double v) { c->arena_max_bytes = (size_t)(std::max(0.0, v) * 1048576.0); }},
    {"FX_ARENA_THRESHOLD_MB", [](fx_context *c, double v) { c->arena_threshold = (size_t)(std::max(0.0, v) * 1048576.0); }},
    {"FX_BFS_DEVICE_MIN", [](fx_context *c, double v) { c->bfs_device_min = (int)v; }},
    {"FX_MC_DEVICE_MIN", [](fx_context *c, double v) { c->mc_device_min = (int)v; }},
    {"FX_BFS_BATCH", [](fx_context *c, double v) { c->bfs_batch = std::max(1, (int)v); }},
    {"FX_VAL2_POW2", [](fx_context *c, double v) { c->val2_pow2 = (int)v != 0; }},
    {"FX_MC_BATCH", [](fx_context *c, double v) { c->mc_batch = std::max(1, (int)v); }},
    {"FX_LAYOUT_DEVICE", [](fx_context *c, double v) { c->layout_device = (int)v != 0; }},
    {"FX_PIPE_SPMV", [](fx_context *c, double v) { c->pipe_spmv = (int)v != 0; }},
    {"FX_PIPE_SSOR", [](fx_context *c, double v) { c->pipe_ssor = (int)v != 0; }},
    {"FX_SSOR_MODE", [](fx_context *c, double v) {
       // the numbering is chosen by the symbolic set-up of the multicolour SSOR: a resident one built in the other numbering is
       // invalidated (the next solve or fx_precond_setup rebuilds it; until then fx_precond_apply_* report it as not set up)
       if ((int)v != c->ssor_mode && c->precond_kind == 1) c->precond_valid = false;
       c->ssor_mode = (int)v;
     }},
    {"FX_PIPE_MAX_SLICES", [](fx_context *c, double v) { c->pipe_max_slices = (int)v; }},
    {"FX_SSOR_BS", [](fx_context *c, double v) { c->ssor_bs = ((int)v == 64) ? 64 : 256; }},
    {"FX_SSOR_SPW", [](fx_context *c, double v) { c->ssor_spw = std::max(1, std::min(8, (int)v)); }},
    {"FX_SPMV_BS", [](fx_context *c, double v) { c->spmv_bs = ((int)v == 64) ? 64 : 256; }},
    {"FX_SPMV_SPATIAL", [](fx_context *c, double v) { c->spmv_spatial = (int)v != 0; }},
    {"FX_GRAPH", [](fx_context *c, double v) { c->graph_mode = (int)v; }},
    {"FX_OVERLAP", [](fx_context *c, double v) { c->overlap = (int)v != 0; }},
    {"FX_EISENSTAT", [](fx_context *c, double v) { c->eisenstat = (int)v != 0; }},
    {"FX_EIS_FUSE", [](fx_context *c, double v) { c->eis_fuse = (int)v != 0; }},
    {"FX_EIS_MERGE", [](fx_context *c, double v) { c->eis_merge = (int)v != 0; }},
    {"FX_EIS_GRID", [](fx_context *c, double v) { c->eis_grid = std::max(0, (int)v); }},
    {"FX_SPLIT_MAX_SLICES", [](fx_context *c, double v) { c->split_max_slices = (int)v; }},
    {"FX_DATAFLOW", [](fx_context *c, double v) {
       c->df_mode = (int)v;
       // leaving the dataflow sweeps on a live context: their sweep vector is full of tags, and the level sweeps multiply a padding
       // block (value 0) with the row's own stale entry
       if (c->ssor.zs && hipSetDevice(c->device) == hipSuccess) (void)hipMemset(c->ssor.zs, 0, (size_t)3 * c->ssor.nslots * 8);
       // entering them: the backward vector of a private-numbering sweep is allocated by the set-up only when it is asked for then
       // (never inside an apply: that may be inside a graph capture)
       const bool lvl = c->precond_kind == 10 || c->precond_kind == 11;
       if (c->ssor.zs && !c->ssor.zb && ((lvl && c->df_mode >= 1) || (c->precond_kind == 1 && c->df_mode >= 2 && c->ord.kind != 1)))
         (void)dev_alloc(&c->ssor.zb, (size_t)3 * c->ssor.nslots);
     }},
    {"FX_DF_SOA", [](fx_context *c, double v) { c->df_soa = (int)v != 0; }},
    {"FX_DF_GRID", [](fx_context *c, double v) { c->df_grid = (int)v; }},
    {"FX_DF_POLL", [](fx_context *c, double v) { c->df_poll = (int)v; }},
    {"FX_DF_SLEEP", [](fx_context *c, double v) { c->df_sleep = std::max(0, (int)v); }},
    {"FX_DF_PRESLEEP", [](fx_context *c, double v) { c->df_presleep = std::max(0, (int)v); }},
    {"FX_DF_WPS", [](fx_context *c, double v) { c->df_wps = ((int)v == 2 || (int)v == 4) ? (int)v : 8; }},
    {"FX_MARCH", [](fx_context *c, double v) { c->march_mode = std::max(0, std::min(2, (int)v)); }},
    {"FX_MARCH_CHUNK", [](fx_context *c, double v) { c->march_chunk = std::max(0, (int)v); }},
    {"FX_MARCH_WAVES", [](fx_context *c, double v) { c->march_waves = (int)v; }},
    {"FX_MARCH_GRID", [](fx_context *c, double v) { c->march_grid = std::max(0, (int)v); }},
    {"FX_MARCH_XCD", [](fx_context *c, double v) { c->march_xcd = (int)v != 0; }},
    {"FX_DEBUG_DF_FAIL", [](fx_context *c, double v) { c->dbg_df_fail = (int)v != 0; }},
    {"FX_DEBUG_ONECOLOR", [](fx_context *c, double v) { c->dbg_onecolor = (int)v != 0; }},
    {"FX_SSOR_NATURAL", [](fx_context *c, double v) { c->ssor_natural = (int)v != 0; }},
    {"FX_SPLIT_WPS", [](fx_context *c, double v) { c->split_wps = ((int)v == 2 || (int)v == 4 || (int)v == 8) ? (int)v : 0; }},
};

extern "C" int fx_set_option(fx_context *c, const char *name, double value) {
  if (!c || !name) { g_fx_error = "fx_set_option: null argument"; return FX_ERROR_RUNTIME; }
  for (const FxOption &o : g_fx_options)
    if (strcmp(o.name, name) == 0) {
      const bool spatial = c->spmv_spatial;
      const int bs = c->spmv_bs;
      o.set(c, value);
      // the SpMV's slice walk and workgroup lists of a resident layout follow these two at once (values untouched)
      if (c->m_symbolic && (spatial != c->spmv_spatial || bs != c->spmv_bs)) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return spmv_walk(c);
      }
      return 0;
    }
  g_fx_error = std::string("fx_set_option: unknown option ") + name;
  return FX_ERROR_UNSUPPORTED;
}

extern "C" int fx_create(int device, fx_context **out) {
  *out = nullptr;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0) { g_fx_error = "no HIP device: libfistr_hip has no CPU path"; return FX_ERROR_RUNTIME; }
  if (device < 0) {
    const char *lr = getenv("LOCAL_RANK");                          // torchrun
    if (!lr) lr = getenv("OMPI_COMM_WORLD_LOCAL_RANK");             // Open MPI
    if (!lr) lr = getenv("MPI_LOCALRANKID");                        // MPICH / Intel MPI
    if (!lr) lr = getenv("SLURM_LOCALID");
    device = lr ? atoi(lr) % ndev : 0;
  }
  HIP_TRY(hipSetDevice(device));
  fx_context *c = new fx_context();
  c->device = device;
  HIP_TRY(hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device));
  if (context_init(c)) {  // release whatever was created before the failing call
    fx_destroy(c);
    return FX_ERROR_RUNTIME;
  }
  for (const FxOption &o : g_fx_options)
    if (const char *e = getenv(o.name)) o.set(c, atof(e));
  {  // dataflow sweeps: the co-residency bound of each instantiation (workgroups per CU x CUs), the clamp of FX_DF_GRID
    int pc[3] = {64, 64, 64};
    auto occ = [&](int k, auto kernel, int threads) {  // the minimum over the instantiations of one wave count (POLL 0 / 1, SOA on / off): whichever is launched fits
      int n = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, 0) != hipSuccess) n = 1;
      pc[k] = std::min(pc[k], n);
    };
    occ(0, k_tri_dataflow<2, 1, true>, 128); occ(0, k_tri_dataflow<2, 0, true>, 128); occ(0, k_tri_dataflow<2, 1, false>, 128); occ(0, k_tri_dataflow<2, 0, false>, 128);
    occ(1, k_tri_dataflow<4, 1, true>, 256); occ(1, k_tri_dataflow<4, 0, true>, 256); occ(1, k_tri_dataflow<4, 1, false>, 256); occ(1, k_tri_dataflow<4, 0, false>, 256);
    occ(2, k_tri_dataflow<8, 1, true>, 512); occ(2, k_tri_dataflow<8, 0, true>, 512); occ(2, k_tri_dataflow<8, 1, false>, 512); occ(2, k_tri_dataflow<8, 0, false>, 512);
    (void)hipGetLastError();
    for (int k = 0; k < 3; k++) c->df_grid_max[k] = std::max(1, c->n_cu * std::max(1, std::min(pc[k], 8)));
    int pe[2] = {1, 1};
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pe[0], k_eis_backward_df<4>, 256, 0) != hipSuccess) pe[0] = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pe[1], k_eis_forward_df<4>, 256, 0) != hipSuccess) pe[1] = 1;
    (void)hipGetLastError();
    for (int k = 0; k < 2; k++) c->eis_df_grid_max[k] = std::max(1, c->n_cu * std::max(1, std::min(pe[k], EIS_DF_MAX_PER_CU)));
    int pm[4] = {1, 1, 1, 1};
    auto occm = [&](int k, auto kernel, int threads) {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pm[k], kernel, threads, 0) != hipSuccess) pm[k] = 1;
    };
    occm(0, k_tri_march<1>, 64 * 2); occm(1, k_tri_march<2>, 64 * 3); occm(2, k_tri_march<3>, 64 * 4); pm[3] = pm[2];
    (void)hipGetLastError();
    for (int k = 0; k < 4; k++) c->march_grid_max[k] = std::max(8, c->n_cu * std::max(1, std::min(pm[k], 4)));
  }
  *out = c;
  return 0;
}

// ---------------------------------------------------------------------------
// The value arena (DevArena, fx_internal.h): one large allocation taken before anything else of a large system, the BELL value
// arrays placed in it first-fit at 2 MiB-aligned offsets.
// ---------------------------------------------------------------------------
static void arena_destroy(fx_context *c) {
  if (c->arena.base) (void)hipFree(c->arena.base);
  c->arena = DevArena();
  for (DevArena &a : c->arena_tried)
    if (a.base) (void)hipFree(a.base);
  c->arena_tried.clear();
  c->arena_verified = false;
}
// Called when the size of a system becomes known (fx_upload of a profile, before the CSR arrays are allocated): `need` = estimated
// bytes of the value arrays of M, L and U.  Keeps a large enough arena, replaces an empty smaller one, does nothing for small
// systems, with FX_ARENA_GB=0 or when the device cannot spare the memory (the arrays then get their own allocations as before).
static void arena_reserve(fx_context *c, size_t need) {
  DevArena &a = c->arena;
  if (c->arena_min_bytes == 0 || need < c->arena_threshold) return;
  need += (size_t)4 << 21;  // alignment slack of four arrays
  if (a.base && a.bytes >= need) return;
  if (a.base && a.live() > 0) return;  // in use and too small: the new arrays fall back to their own allocations
  arena_destroy(c);
  size_t want = (size_t)1 << 20;
  while (want < need || want < c->arena_min_bytes) want <<= 1;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
  // what else this system will allocate is about 2.5x the value arrays (CSR arrays, column ids, source maps, vectors): leave it room
  while (want > need && want + 3 * need > free_b) want >>= 1;
  if (want < need || want + 2 * need > free_b) return;
  if (c->arena_max_bytes) {  // a cap set by the user: what does not fit gets its own allocation (val2_alloc)
    while (want > c->arena_max_bytes && want > ((size_t)1 << 20)) want >>= 1;
  }
  char *p = nullptr;
  if (hipMalloc((void **)&p, want) != hipSuccess) { (void)hipGetLastError(); return; }
  a.base = p; a.bytes = want; a.blocks.clear();
}
static char *arena_alloc(fx_context *c, size_t bytes) {
  DevArena &a = c->arena;
  if (!a.base || bytes == 0) return nullptr;
  const size_t al = ((size_t)2 << 20) - 1;
  size_t off = 0;
  size_t at = 0;  // index in blocks before which the new one goes
  for (; at < a.blocks.size(); at++) {
    if (off + bytes <= a.blocks[at].first) break;  // the gap before block `at` holds it
    off = (a.blocks[at].first + a.blocks[at].second + al) & ~al;
  }
  if (off + bytes > a.bytes) return nullptr;
  a.blocks.insert(a.blocks.begin() + at, {off, bytes});
  return a.base + off;
}
static void arena_release(fx_context *c, const void *p) {
  DevArena &a = c->arena;
  if (!a.base) return;
  const size_t off = (size_t)((const char *)p - a.base);
  for (size_t k = 0; k < a.blocks.size(); k++)
    if (a.blocks[k].first == off) { a.blocks.erase(a.blocks.begin() + k); return; }
}

static void bell_free(Bell &b) {
  if (b.arena_owner) { arena_release(b.arena_owner, b.val2_base); b.val2_base = nullptr; }
  dev_free(b.pair_ptr); dev_free(b.val2_base); dev_free(b.col2); dev_free(b.slot_row); dev_free(b.src2); dev_free(b.slice_order);
  dev_free(b.wg_interior); dev_free(b.wg_boundary);
  b.val2 = nullptr;
  b = Bell();
}

static void nl_free(fx_context *c);  // fx_nonlinear_host.h
static void nn_free(fx_context *c);  // fx_nn_host.h
static void graphs_destroy(fx_context *c);
static void upd_stage_free(fx_context *c);  // fx_assemble_groups.h
static void heat_free(fx_context *c);       // fx_heat.h
static void nodal_free(fx_context *c);      // fx_nodal_stress.h
static void dload_free(fx_context *c);      // fx_dload.h
static void nodal_list_free(NodalList &L);
static void asm_groups_free(fx_context *c) {  // the cache of the linear assembly: colourings and maps of the last call's groups
  for (ElemColors &ec : c->asm_groups.ec) { dev_free(ec.order); dev_free(ec.pos); dev_free(ec.dup); }
  c->asm_groups = AsmGroups();
}
static void free_matrix(fx_context *c) {
  DevCSR &A = c->A;
  dev_free(A.indexL); dev_free(A.itemL); dev_free(A.indexU); dev_free(A.itemU);
  dev_free(A.D); dev_free(A.AL); dev_free(A.AU); dev_free(A.B); dev_free(A.X);
  A = DevCSR();
  bell_free(c->M);
  dev_free(c->ord.d_slot_node); dev_free(c->ord.d_slot_of);
  c->ord = Ordering();
  c->m_symbolic = false;
  dev_free(c->Bs); dev_free(c->Xs);
  for (auto &w : c->W) dev_free(w);
  dev_free(c->partials); dev_free(c->scale_vec);
  c->wlen = 0;
  c->max_partials = 0;
  c->have_profile = c->have_values = c->bell_valid = false;
  asm_groups_free(c);  // the colourings' scatter maps belong to the profile
}

static void free_precond(fx_context *c) {
  dev_free(c->diag.alu);
  bell_free(c->ssor.L); bell_free(c->ssor.U); bell_free(c->ssor.H);
  dev_free(c->ssor.alu); dev_free(c->ssor.slot_node); dev_free(c->ssor.zs); dev_free(c->ssor.zb);
  dev_free(c->ssor.lu_D); dev_free(c->ssor.lu_AL); dev_free(c->ssor.lu_AU); dev_free(c->ssor.slice_level);
  march_free(c->ssor.march);
  c->ssor = SsorDev();
  c->precond_valid = false;
  c->precond_valid_sweeps = false;
  c->precond_kind = 0;
}

extern "C" void fx_destroy(fx_context *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  graphs_destroy(c);
  nl_free(c);
  nn_free(c);
  upd_stage_free(c);
  heat_free(c);
  dload_free(c);
  nodal_free(c);
  free_precond(c);
  free_matrix(c);
  arena_destroy(c);
  dev_free(c->halo.export_item); dev_free(c->halo.import_item);
  dev_free(c->halo.sendbuf); dev_free(c->halo.recvbuf);
  dev_free(c->st); dev_free(c->red_out); dev_free(c->hist); dev_free(c->extra); dev_free(c->df_err);
  if (c->st_host) (void)hipHostFree(c->st_host);
  if (c->h_send) (void)hipHostFree(c->h_send);
  if (c->h_recv) (void)hipHostFree(c->h_recv);
  if (c->nccl_halo && g_rccl.CommDestroy) g_rccl.CommDestroy((ncclComm_t)c->nccl_halo);
  if (c->nccl && g_rccl.CommDestroy) g_rccl.CommDestroy((ncclComm_t)c->nccl);
  for (hipEvent_t e : c->clock.ev) (void)hipEventDestroy(e);
  if (c->comm_stream) { (void)hipStreamSynchronize(c->comm_stream); (void)hipStreamDestroy(c->comm_stream); }
  if (c->ev_packed) (void)hipEventDestroy(c->ev_packed);
  if (c->ev_halo) (void)hipEventDestroy(c->ev_halo);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

extern "C" int fx_device_synchronize(fx_context *c) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// BELL construction on the host (profile only; values are gathered on the device)
// entries(slot, out): ordered list of (src code, 0-based column) of that slot's row.
// ---------------------------------------------------------------------------
struct BellEntry { int32_t src, col; };

// Memory of a BELL value array: its place in the context's arena when there is one with room; otherwise an allocation of its own --
// for arrays of a gigabyte or more the next power of two (ONE block of the driver's VRAM allocator instead of 4 + 2 + 0.5 GB pieces:
// more often the fast class than the exact request, scripts/r4/placement_probe.py), the exact size when memory does not allow it.
static int val2_alloc(fx_context *c, Bell &b, size_t bytes) {
  b.val2_base = nullptr; b.val2 = nullptr; b.arena_owner = nullptr; b.val2_bytes = bytes;
  if (char *p = arena_alloc(c, bytes)) {
    b.val2_base = p; b.val2 = (double *)p; b.arena_owner = c;
    return 0;
  }
  char *base = nullptr;
  if (c->val2_pow2 && bytes >= ((size_t)1 << 30)) {
    size_t want = (size_t)1 << 30;
    while (want < bytes) want <<= 1;
    size_t free_b = 0, total_b = 0;
    if (want > bytes && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > want + ((size_t)8 << 30) &&
        hipMalloc((void **)&base, want) == hipSuccess) {
      b.val2_base = base; b.val2 = (double *)base; b.val2_bytes = want;
      return 0;
    }
    (void)hipGetLastError();
    base = nullptr;
  }
  if (dev_alloc(&base, bytes)) return FX_ERROR_RUNTIME;
  b.val2_base = base; b.val2 = (double *)base;
  return 0;
}

template <class CountFn, class FillFn>
static int bell_build2(fx_context *c, Bell &b, int32_t nslots, const std::vector<int32_t> *slot_row,
                       CountFn count, FillFn fill) {
  bell_free(b);
  b.nslots = nslots;
  b.nslices = (nslots + 63) / 64;
  std::vector<int32_t> pair_ptr((size_t)b.nslices + 1, 0);
  std::vector<int64_t> blocks_per_slice((size_t)b.nslices, 0);
  parallel_for(b.nslices, [&](int64_t s0, int64_t s1) {
    for (int64_t s = s0; s < s1; s++) {
      int32_t w = 0;
      int64_t nb = 0;
      for (int l = 0; l < 64; l++) {
        const int64_t slot = s * 64 + l;
        if (slot >= nslots) break;
        const int32_t k = count((int32_t)slot);
        w = std::max(w, k);
        nb += k;
      }
      pair_ptr[s + 1] = w;  // block positions of the slice (pairs + an optional single last block)
      blocks_per_slice[s] = nb;
    }
  });
  int64_t tot = 0;
  b.nblocks = 0;
  for (int32_t s = 0; s < b.nslices; s++) {
    tot += pair_ptr[s + 1];
    if (tot > INT32_MAX) { g_fx_error = "BELL: block-position count overflows int32"; return FX_ERROR_RUNTIME; }
    pair_ptr[s + 1] = (int32_t)tot;
    b.nblocks += blocks_per_slice[s];
  }
  b.npairs = tot;
  std::vector<int32_t> col2((size_t)tot * 64), src2((size_t)tot * 64);
  parallel_for(b.nslices, [&](int64_t s0, int64_t s1) {
    std::vector<BellEntry> ent;
    for (int64_t s = s0; s < s1; s++) {
      const int32_t h0 = pair_ptr[s], h1 = pair_ptr[s + 1];
      const int32_t npair2 = ((h1 - h0) >> 1) << 1;
      for (int l = 0; l < 64; l++) {
        const int64_t slot = s * 64 + l;
        ent.clear();
        const int32_t self = (int32_t)std::min<int64_t>(slot, (int64_t)b.nslices * 64 - 1);  // always a valid vector slot
        if (slot < nslots && (!slot_row || (*slot_row)[slot] >= 0)) fill((int32_t)slot, ent);
        for (int32_t k = 0; k < h1 - h0; k++) {
          const int32_t cc = (size_t)k < ent.size() ? ent[k].col : self;
          const int32_t ss = (size_t)k < ent.size() ? ent[k].src : -1;
          const size_t idx = k < npair2 ? (size_t)(h0 + (k & ~1)) * 64 + (size_t)l * 2 + (k & 1) : (size_t)(h0 + k) * 64 + l;
          col2[idx] = cc;
          src2[idx] = ss;
        }
      }
    }
  });
  if (dev_alloc(&b.pair_ptr, (size_t)b.nslices + 1)) return FX_ERROR_RUNTIME;
  if (dev_alloc(&b.col2, (size_t)tot * 64)) return FX_ERROR_RUNTIME;
  if (dev_alloc(&b.src2, (size_t)tot * 64)) return FX_ERROR_RUNTIME;
  if (val2_alloc(c, b, (size_t)tot * 576 * 8)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(b.pair_ptr, pair_ptr.data(), pair_ptr.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(b.col2, col2.data(), col2.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(b.src2, src2.data(), src2.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // host staging vectors die here
  return 0;
}

// The same layout built on the device (kernels k_bell_count / k_bell_map, fx_kernels.h): d_slot_row, d_slot_of (node -> vector
// slot, NP entries) and d_newpos (node -> new index, SSOR variants only) are device arrays.  Returns 1 when a row is longer than
// the kernels' per-thread buffer (the caller then uses the host builder), 0 on success, < 0 on a runtime failure.
static int bell_build_device(fx_context *c, Bell &b, int variant, int32_t nslots, const int32_t *d_slot_row,
                             const int32_t *d_slot_of, const int32_t *d_newpos) {
  if (!c->layout_device) return 1;
  bell_free(b);
  b.nslots = nslots;
  b.nslices = (nslots + 63) / 64;
  const DevCSR &A = c->A;
  DevScratch tmp;
  int32_t *width = nullptr;
  unsigned long long *totals = nullptr;
  if (tmp.alloc(&width, (size_t)b.nslices + 1) || tmp.alloc(&totals, 4)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemsetAsync(totals, 0, 32, c->stream));
  if (dev_alloc(&b.pair_ptr, (size_t)b.nslices + 1)) return FX_ERROR_RUNTIME;
  const dim3 g1((nslots + 255) / 256), b1(256);
#define BELL_VAR(K, ...)                                                        \
  switch (variant) {                                                            \
    case BV_FULL: hipLaunchKernelGGL((K<BV_FULL>), __VA_ARGS__); break;         \
    case BV_SSOR_L: hipLaunchKernelGGL((K<BV_SSOR_L>), __VA_ARGS__); break;     \
    case BV_SSOR_U: hipLaunchKernelGGL((K<BV_SSOR_U>), __VA_ARGS__); break;     \
    case BV_ILU_L: hipLaunchKernelGGL((K<BV_ILU_L>), __VA_ARGS__); break;       \
    case BV_HALO: hipLaunchKernelGGL((K<BV_HALO>), __VA_ARGS__); break;         \
    default: hipLaunchKernelGGL((K<BV_ILU_U>), __VA_ARGS__); break;             \
  }
  BELL_VAR(k_bell_count, g1, b1, 0, c->stream, nslots, d_slot_row, A.N, A.indexL, A.itemL, A.indexU, A.itemU, d_newpos, width, totals)
  hipLaunchKernelGGL(k_scan_excl, dim3(1), dim3(1024), 0, c->stream, b.nslices, width, b.pair_ptr, b.pair_ptr + b.nslices);
  unsigned long long h_tot[4];
  HIP_TRY(hipMemcpyAsync(h_tot, totals, 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipGetLastError());
  if (h_tot[2] > FX_BELL_MAXROW) { bell_free(b); return 1; }
  if (h_tot[1] > (unsigned long long)INT32_MAX) { g_fx_error = "BELL: block-position count overflows int32"; return FX_ERROR_RUNTIME; }
  b.nblocks = (int64_t)h_tot[0];
  b.npairs = (int64_t)h_tot[1];
  const size_t tot = (size_t)b.npairs;
  if (dev_alloc(&b.col2, tot * 64) || dev_alloc(&b.src2, tot * 64)) return FX_ERROR_RUNTIME;
  if (val2_alloc(c, b, tot * 576 * 8)) return FX_ERROR_RUNTIME;
  BELL_VAR(k_bell_map, dim3(b.nslices), dim3(64), 0, c->stream, nslots, b.nslices, d_slot_row, A.N, A.indexL, A.itemL, A.indexU,
           A.itemU, d_slot_of, d_newpos, b.pair_ptr, b.col2, b.src2)
#undef BELL_VAR
  HIP_TRY(hipGetLastError());
  return 0;
}

static int bell_fill_values(fx_context *c, Bell &b, const double *D = nullptr, const double *AL = nullptr,
                            const double *AU = nullptr) {
  if (b.nslices == 0) return 0;
  b.values_filled = true;
  hipLaunchKernelGGL(k_bell_fill, dim3((b.nslices + 3) / 4), dim3(FX_BLOCK), 0, c->stream, b.nslices, b.pair_ptr,
                     b.src2, D ? D : c->A.D, AL ? AL : c->A.AL, AU ? AU : c->A.AU, b.val2);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// solver numbering (Ordering) and the structures that depend on it
// ---------------------------------------------------------------------------
static int set_ordering(fx_context *c, int kind, const std::vector<int32_t> *color_slots /* slot -> node, -1 pad */) {
  Ordering &o = c->ord;
  const int32_t N = c->A.N, NP = c->A.NP;
  dev_free(o.d_slot_node); dev_free(o.d_slot_of);
  o = Ordering();
  o.kind = kind;
  o.nhalo = NP - N;
  if (kind == 0) {
    o.nslots = (N + 63) / 64 * 64;
    o.slot_node.assign((size_t)o.nslots + o.nhalo, -1);
    for (int32_t i = 0; i < N; i++) o.slot_node[i] = i;
  } else {
    o.nslots = (int32_t)color_slots->size();
    o.slot_node.assign((size_t)o.nslots + o.nhalo, -1);
    std::copy(color_slots->begin(), color_slots->end(), o.slot_node.begin());
  }
  for (int32_t h = 0; h < o.nhalo; h++) o.slot_node[(size_t)o.nslots + h] = N + h;
  o.slot_of.assign((size_t)NP, 0);
  for (int32_t s = 0; s < o.vslots(); s++)
    if (o.slot_node[s] >= 0) o.slot_of[o.slot_node[s]] = s;
  if (dev_alloc(&o.d_slot_node, o.slot_node.size()) || dev_alloc(&o.d_slot_of, o.slot_of.size())) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpy(o.d_slot_node, o.slot_node.data(), o.slot_node.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(o.d_slot_of, o.slot_of.data(), o.slot_of.size() * 4, hipMemcpyHostToDevice));
  c->m_symbolic = false;
  c->bell_valid = false;
  // halo tables in slot numbering
  HaloDev &h = c->halo;
  if (h.n_neighbor > 0) {
    std::vector<int32_t> ei(h.h_export), ii(h.h_import);
    for (auto &v : ei) v = o.slot_of[v];
    for (auto &v : ii) v = o.slot_of[v];
    HIP_TRY(hipMemcpy(h.export_item, ei.data(), ei.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h.import_item, ii.data(), ii.size() * 4, hipMemcpyHostToDevice));
  }
  return 0;
}

// full matrix M = [D | AL | AU] per row in the reference's summation order, rows and columns
// in slot numbering
static int build_full_bell(fx_context *c) {
  const Ordering &o = c->ord;
  const int32_t *iL = c->h_indexL.data(), *jL = c->h_itemL.data(), *iU = c->h_indexU.data(), *jU = c->h_itemU.data();
  const int32_t *sn = o.slot_node.data(), *so = o.slot_of.data();
  auto count = [=](int32_t slot) {
    const int32_t r = sn[slot];
    return r < 0 ? 0 : 1 + (iL[r + 1] - iL[r]) + (iU[r + 1] - iU[r]);
  };
  auto fill = [=](int32_t slot, std::vector<BellEntry> &e) {
    const int32_t r = sn[slot];
    e.push_back({3 * r + 0, slot});
    for (int32_t j = iL[r]; j < iL[r + 1]; j++) e.push_back({3 * j + 1, so[jL[j] - 1]});
    for (int32_t j = iU[r]; j < iU[r + 1]; j++) e.push_back({3 * j + 2, so[jU[j] - 1]});
  };
  if ((int64_t)3 * std::max(c->A.NPL, c->A.NPU) + 2 > INT32_MAX) {
    g_fx_error = "matrix too large for int32 block codes";
    return FX_ERROR_UNSUPPORTED;
  }
  std::vector<int32_t> sr(o.slot_node.begin(), o.slot_node.begin() + o.nslots);
  {
    const int e = bell_build_device(c, c->M, BV_FULL, o.nslots, o.d_slot_node, o.d_slot_of, nullptr);
    if (e < 0) return FX_ERROR_RUNTIME;
    if (e > 0 && bell_build2(c, c->M, o.nslots, &sr, count, fill)) return FX_ERROR_RUNTIME;  // a row longer than the device buffer
  }
  if (spmv_walk(c)) return FX_ERROR_RUNTIME;
  c->m_symbolic = true;
  c->bell_valid = false;
  return 0;
}

// The SpMV's walk over M's slices (FX_SPMV_SPATIAL) and, on a decomposed system, its interior / boundary workgroup lists (FX_SPMV_BS
// slices each).  Neither touches M's values: fx_set_option re-runs it when one of the two knobs changes on a resident layout, so
// the partial sums of the SpMV's dot products are grouped as a fresh context would group them.
static int spmv_walk(fx_context *c) {
  const Ordering &o = c->ord;
  const int32_t *iU = c->h_indexU.data(), *jU = c->h_itemU.data();
  const int32_t *sr = o.slot_node.data();
  dev_free(c->M.slice_order); dev_free(c->M.wg_interior); dev_free(c->M.wg_boundary);
  c->M.n_wg_interior = c->M.n_wg_boundary = 0;
  if (o.kind == 1 && c->spmv_spatial) {  // walk the slices by the mesh position of their rows, all colours of a region together
    const int32_t nsl = c->M.nslices;
    std::vector<int32_t> key((size_t)nsl, INT32_MAX), ordv((size_t)nsl);
    for (int32_t sl = 0; sl < nsl; sl++) {
      ordv[sl] = sl;
      for (int l = 0; l < 64; l++) {
        const int32_t r = sr[(size_t)sl * 64 + l];
        if (r >= 0) { key[sl] = r; break; }  // rows of a slice are in natural order inside their colour: the first is the smallest
      }
    }
    std::stable_sort(ordv.begin(), ordv.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    if (dev_alloc(&c->M.slice_order, (size_t)nsl)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpy(c->M.slice_order, ordv.data(), (size_t)nsl * 4, hipMemcpyHostToDevice));
  }
  if (c->halo.n_neighbor > 0) {  // interior / boundary split of the SpMV's virtual workgroups (4 slices of the walk each)
    const int32_t nsl = c->M.nslices, N = c->A.N;
    std::vector<int32_t> walk((size_t)nsl);
    if (c->M.slice_order) HIP_TRY(hipMemcpy(walk.data(), c->M.slice_order, (size_t)nsl * 4, hipMemcpyDeviceToHost));
    else for (int32_t i = 0; i < nsl; i++) walk[i] = i;
    std::vector<uint8_t> bnd((size_t)nsl, 0);
    parallel_for(nsl, [&](int64_t a, int64_t b) {
      for (int64_t sl = a; sl < b; sl++)
        for (int l = 0; l < 64; l++) {
          const int32_t r = sr[(size_t)sl * 64 + l];
          if (r >= 0 && iU[r + 1] > iU[r] && jU[iU[r + 1] - 1] > N) { bnd[sl] = 1; break; }  // itemU ascending: halo ids (> N) come last
        }
    });
    const int spb = c->spmv_bs / 64;
    const int32_t nwg = (nsl + spb - 1) / spb;
    std::vector<int32_t> wi, wb;
    for (int32_t w = 0; w < nwg; w++) {
      bool b = false;
      for (int k = 0; k < spb && (int64_t)w * spb + k < nsl; k++) b |= bnd[walk[(size_t)w * spb + k]] != 0;
      (b ? wb : wi).push_back(w);
    }
    c->M.n_wg_interior = (int32_t)wi.size(); c->M.n_wg_boundary = (int32_t)wb.size();
    if (dev_alloc(&c->M.wg_interior, wi.size()) || dev_alloc(&c->M.wg_boundary, wb.size())) return FX_ERROR_RUNTIME;
    if (!wi.empty()) HIP_TRY(hipMemcpy(c->M.wg_interior, wi.data(), wi.size() * 4, hipMemcpyHostToDevice));
    if (!wb.empty()) HIP_TRY(hipMemcpy(c->M.wg_boundary, wb.data(), wb.size() * 4, hipMemcpyHostToDevice));
  }
  return 0;
}

static int ensure_work(fx_context *c);

static int spmv_launch(fx_context *c, int mode, int dot, double *x, const double *b, double *y, const int32_t *gate,
                       int32_t gate_val, const int32_t *wg_list, int nwg);
static inline int spmv_nparts(fx_context *c);

// Move every value array that lives in the context's arena to the same offsets of `to` (which becomes the context's arena; the
// old one is returned in *from).  Nothing is copied: only M may hold values at the time this is used (the sweep layouts are filled
// after it, and the caller refills M); a sweep layout that already holds values is an error, not a silent loss of its values.
static int arena_switch(fx_context *c, DevArena &to, DevArena *from) {
  for (Bell *b : {&c->ssor.L, &c->ssor.U, &c->ssor.H})
    if (b->arena_owner == c && b->val2_base && b->values_filled) {
      g_fx_error = "arena_switch: a sweep layout already holds values (only M may, when the arena is switched)";
      return FX_ERROR_RUNTIME;
    }
  to.blocks = c->arena.blocks;
  for (Bell *b : {&c->M, &c->ssor.L, &c->ssor.U, &c->ssor.H})
    if (b->arena_owner == c && b->val2_base) {
      const size_t off = (size_t)((char *)b->val2_base - c->arena.base);
      b->val2_base = to.base + off;
      b->val2 = (double *)(to.base + off);
    }
  *from = c->arena;
  from->blocks.clear();
  c->arena = to;
  return 0;
}

// Verification of the arena (fx_context::arena_tries): see fx_internal.h.  M's values have just been filled.
static int arena_verify(fx_context *c) {
  c->arena_verified = true;
  Bell &M = c->M;
  if (c->arena_tries <= 1 || !c->arena.base || M.arena_owner != c || M.nslices < 8192) return 0;
  const double bytes = (double)M.npairs * 64 * 76 + 48.0 * c->ord.nslots;
  auto time_ms = [&](float *ms) -> int {
    const int nwg = spmv_nparts(c);
    if (spmv_launch(c, 0, 1, c->W[2], nullptr, c->W[1], nullptr, 0, nullptr, nwg)) return FX_ERROR_RUNTIME;  // untimed
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < 3; i++)
      if (spmv_launch(c, 0, 1, c->W[2], nullptr, c->W[1], nullptr, 0, nullptr, nwg)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    *ms /= 3.f;
    return 0;
  };
  c->arena_ms.clear();
  float best = 1e30f;
  int best_k = -1;  // index in arena_tried of the best arena so far; -1 = the current one
  for (int attempt = 0; attempt < c->arena_tries; attempt++) {
    float ms = 0.f;
    if (time_ms(&ms)) return FX_ERROR_RUNTIME;
    c->arena_ms.push_back(ms);
    if (ms < best) { best = ms; best_k = -1; }
    if (bytes / (1e-3 * ms) / 1e9 >= c->arena_good_gbs || attempt + 1 == c->arena_tries) break;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < c->arena.bytes + 3 * c->arena.used() + ((size_t)8 << 30)) break;
    DevArena next;
    if (hipMalloc((void **)&next.base, c->arena.bytes) != hipSuccess) { (void)hipGetLastError(); break; }
    next.bytes = c->arena.bytes;
    DevArena old;
    if (arena_switch(c, next, &old)) { (void)hipFree(next.base); return FX_ERROR_RUNTIME; }
    c->arena_tried.push_back(old);
    if (best_k == -1) best_k = (int)c->arena_tried.size() - 1;  // the best so far is the one just left
    if (bell_fill_values(c, M)) return FX_ERROR_RUNTIME;
  }
  if (best_k >= 0) {  // an earlier arena was the fastest: back to it
    DevArena back = c->arena_tried[best_k], old;
    if (arena_switch(c, back, &old)) return FX_ERROR_RUNTIME;
    c->arena_tried[best_k] = old;
    if (bell_fill_values(c, M)) return FX_ERROR_RUNTIME;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (DevArena &a : c->arena_tried)
    if (a.base) (void)hipFree(a.base);
  c->arena_tried.clear();
  if (getenv("FX_TIMING") && atoi(getenv("FX_TIMING"))) {
    fprintf(stderr, "[fx timing] arena verification (SpMV ms per arena tried):");
    for (float v : c->arena_ms) fprintf(stderr, " %.4f", v);
    fprintf(stderr, "  kept %.4f\n", best);
  }
  return 0;
}

// Make the ordering, M (symbolic + values) and the work vectors current.
static int ensure_solver(fx_context *c) {
  if (c->ord.kind < 0 && set_ordering(c, 0, nullptr)) return FX_ERROR_RUNTIME;
  if (!c->m_symbolic && build_full_bell(c)) return FX_ERROR_RUNTIME;
  if (ensure_work(c)) return FX_ERROR_RUNTIME;
  if (!c->bell_valid && c->have_values) {
    if (bell_fill_values(c, c->M)) return FX_ERROR_RUNTIME;
    c->bell_valid = true;
    c->values_epoch++;  // the SpMV layout holds new values from here on
    if (!c->arena_verified && arena_verify(c)) return FX_ERROR_RUNTIME;
  }
  return 0;
}

static int to_slots(fx_context *c, const double *nat, double *out) {
  const int vs = c->ord.vslots();
  hipLaunchKernelGGL(k_to_slots, dim3((vs + 255) / 256), dim3(256), 0, c->stream, vs, c->ord.d_slot_node, nat, out);
  HIP_TRY(hipGetLastError());
  return 0;
}
static int from_slots(fx_context *c, const double *in, double *nat) {
  const int np = c->A.NP;
  hipLaunchKernelGGL(k_from_slots, dim3((np + 255) / 256), dim3(256), 0, c->stream, np, c->ord.d_slot_of, in, nat);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// upload
// ---------------------------------------------------------------------------
static int ensure_work(fx_context *c) {
  const int32_t len = 3 * c->ord.vslots();
  if (c->wlen != len) {
    for (auto &w : c->W) dev_free(w);
    dev_free(c->Bs); dev_free(c->Xs);
    for (auto &w : c->W) {
      if (dev_alloc(&w, (size_t)len)) return FX_ERROR_RUNTIME;
      HIP_TRY(hipMemsetAsync(w, 0, (size_t)len * 8, c->stream));
    }
    if (dev_alloc(&c->Bs, (size_t)len) || dev_alloc(&c->Xs, (size_t)len)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemsetAsync(c->Bs, 0, (size_t)len * 8, c->stream));
    HIP_TRY(hipMemsetAsync(c->Xs, 0, (size_t)len * 8, c->stream));
    c->wlen = len;
  }
  const int32_t need = c->ord.nslots / 64 + 4096 + 8;  // per-block partials of the largest grid + one slot per colour
  if (c->max_partials < need) {
    dev_free(c->partials);
    if (dev_alloc(&c->partials, (size_t)need * 3)) return FX_ERROR_RUNTIME;
    c->max_partials = need;
  }
  return 0;
}

static int setup_halo(fx_context *c, const fx_comm_view *cm) {
  HaloDev &h = c->halo;
  dev_free(h.export_item); dev_free(h.import_item); dev_free(h.sendbuf); dev_free(h.recvbuf);
  // the pinned staging pair of the host-callback transport is sized by n_export / n_import: it goes with the tables
  if (c->h_send) { (void)hipHostFree(c->h_send); c->h_send = nullptr; }
  if (c->h_recv) { (void)hipHostFree(c->h_recv); c->h_recv = nullptr; }
  h = HaloDev();
  c->nn_internal = c->A.N;
  c->view_petot = 1;
  if (!cm) return 0;
  c->view_petot = std::max(1, (int)cm->PETOT);
  c->nn_internal = cm->nn_internal > 0 ? cm->nn_internal : c->A.N;
  h.n_neighbor = cm->n_neighbor_pe;
  if (h.n_neighbor <= 0) return 0;
  h.neighbor.assign(cm->neighbor_pe, cm->neighbor_pe + h.n_neighbor);
  h.import_index.assign(cm->import_index, cm->import_index + h.n_neighbor + 1);
  h.export_index.assign(cm->export_index, cm->export_index + h.n_neighbor + 1);
  h.n_import = h.import_index.back();
  h.n_export = h.export_index.back();
  h.h_export.assign(cm->export_item, cm->export_item + h.n_export);
  h.h_import.assign(cm->import_item, cm->import_item + h.n_import);
  for (auto &v : h.h_export) v -= 1;
  for (auto &v : h.h_import) v -= 1;
  if (dev_alloc(&h.export_item, h.h_export.size()) || dev_alloc(&h.import_item, h.h_import.size())) return FX_ERROR_RUNTIME;
  if (dev_alloc(&h.sendbuf, (size_t)3 * h.n_export) || dev_alloc(&h.recvbuf, (size_t)3 * h.n_import)) return FX_ERROR_RUNTIME;
  return 0;  // device item lists are written (in slot numbering) by set_ordering
}

extern "C" int fx_upload(fx_context *c, const fx_matrix_view *m, const fx_comm_view *cm, int what) {
  HIP_TRY(hipSetDevice(c->device));
  if (m->NDOF != 3) { g_fx_error = "only NDOF=3 (3x3 blocks) is on the hot path"; return FX_ERROR_UNSUPPORTED; }
  DevCSR &A = c->A;
  const bool shape_changed = (A.N != m->N || A.NP != m->NP || A.NPL != m->NPL || A.NPU != m->NPU);
  if (shape_changed || !c->have_profile) what |= FX_UP_PROFILE;
  if (what & FX_UP_PROFILE) {
    free_precond(c);
    free_matrix(c);
    nl_free(c);  // the nonlinear state (and its scatter map) belongs to the old profile: fx_nl_init again
    A.N = m->N; A.NP = m->NP; A.NPL = m->NPL; A.NPU = m->NPU;
    // the value arena first, while nothing of this system has been allocated: the value arrays of M (every block) and of the
    // sweep layouts L + U (the off-diagonal blocks once more), 72 bytes per block, 3 % of slice padding
    arena_reserve(c, (size_t)(74.2 * ((double)A.NP + 2.0 * ((double)A.NPL + (double)A.NPU))));
    if (dev_alloc(&A.indexL, (size_t)A.NP + 1) || dev_alloc(&A.indexU, (size_t)A.NP + 1) ||
        dev_alloc(&A.itemL, (size_t)A.NPL) || dev_alloc(&A.itemU, (size_t)A.NPU) ||
        dev_alloc(&A.D, (size_t)9 * A.NP) || dev_alloc(&A.AL, (size_t)9 * A.NPL) ||
        dev_alloc(&A.AU, (size_t)9 * A.NPU) || dev_alloc(&A.B, (size_t)3 * A.NP) || dev_alloc(&A.X, (size_t)3 * A.NP))
      return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpyAsync(A.indexL, m->indexL, ((size_t)A.NP + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(A.indexU, m->indexU, ((size_t)A.NP + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(A.itemL, m->itemL, (size_t)A.NPL * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(A.itemU, m->itemU, (size_t)A.NPU * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(A.B, 0, (size_t)3 * A.NP * 8, c->stream));
    HIP_TRY(hipMemsetAsync(A.X, 0, (size_t)3 * A.NP * 8, c->stream));
    c->h_indexL.assign(m->indexL, m->indexL + A.NP + 1);
    c->h_indexU.assign(m->indexU, m->indexU + A.NP + 1);
    c->h_itemL.assign(m->itemL, m->itemL + A.NPL);
    c->h_itemU.assign(m->itemU, m->itemU + A.NPU);
    if (setup_halo(c, cm)) return FX_ERROR_RUNTIME;
    c->have_profile = true;  // ordering, BELL layout and work vectors are built on first use (ensure_solver)
    what |= FX_UP_VALUES;
    if (!m->D) what &= ~FX_UP_VALUES;  // profile-only upload (device assembly follows)
  }
  if ((what & FX_UP_VALUES) && m->D) {
    HIP_TRY(hipMemcpyAsync(A.D, m->D, (size_t)9 * A.NP * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(A.AL, m->AL, (size_t)9 * A.NPL * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(A.AU, m->AU, (size_t)9 * A.NPU * 8, hipMemcpyHostToDevice, c->stream));
    c->have_values = true;
    c->bell_valid = false;
    // the preconditioner keeps its own copy of what it was built from: new values alone do not invalidate it -- it is
    // refreshed when Iarray(97) / (98) ask, after the recycle policy (hecmw_matrix_misc.f90:678-697), as in the reference
  }
  if ((what & FX_UP_RHS) && m->B)
    HIP_TRY(hipMemcpyAsync(A.B, m->B, (size_t)3 * A.NP * 8, hipMemcpyHostToDevice, c->stream));
  if ((what & FX_UP_X) && m->X)
    HIP_TRY(hipMemcpyAsync(A.X, m->X, (size_t)3 * A.NP * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int fx_download_x(fx_context *c, double *X, int32_t n) {
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(X, c->A.X, (size_t)std::min(n, 3 * c->A.NP) * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int fx_download_matrix(fx_context *c, double *D, double *AL, double *AU, double *B) {
  HIP_TRY(hipSetDevice(c->device));
  if (D) HIP_TRY(hipMemcpyAsync(D, c->A.D, (size_t)9 * c->A.NP * 8, hipMemcpyDeviceToHost, c->stream));
  if (AL) HIP_TRY(hipMemcpyAsync(AL, c->A.AL, (size_t)9 * c->A.NPL * 8, hipMemcpyDeviceToHost, c->stream));
  if (AU) HIP_TRY(hipMemcpyAsync(AU, c->A.AU, (size_t)9 * c->A.NPU * 8, hipMemcpyDeviceToHost, c->stream));
  if (B) HIP_TRY(hipMemcpyAsync(B, c->A.B, (size_t)3 * c->A.NP * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// communication: halo exchange (C1) and scalar all-reduce (C2) over RCCL
// ---------------------------------------------------------------------------
extern "C" int fx_comm_unique_id(unsigned char id[128]) {
  if (rccl_load()) return FX_ERROR_RUNTIME;
  ncclUniqueId u;
  NCCL_TRY(g_rccl.GetUniqueId(&u));
  static_assert(sizeof(ncclUniqueId) <= 128, "ncclUniqueId larger than the ABI slot");
  memset(id, 0, 128);
  memcpy(id, &u, sizeof u);
  return 0;
}

extern "C" int fx_comm_init(fx_context *c, const unsigned char id[128], int rank, int nranks) {
  HIP_TRY(hipSetDevice(c->device));
  if (rccl_load()) return FX_ERROR_RUNTIME;
  ncclUniqueId u;
  memcpy(&u, id, sizeof u);
  ncclComm_t comm;
  NCCL_TRY(g_rccl.CommInitRank(&comm, nranks, u, rank));
  c->nccl = comm;
  c->rank = rank;
  c->nranks = nranks;
  c->ledger = CommLedger();
  // The halo exchange (grouped ncclSend / ncclRecv on comm_stream) gets a communicator of its own, the scalar all-reduces (solver
  // stream) keep `comm`: two streams never share a communicator.  Order across ranks does not depend on that split: on every rank
  // halo k is enqueued, the solver stream waits for its event (halo_end) before the boundary rows, and the next all-reduce is
  // enqueued behind those -- at most one RCCL operation of a rank is in flight at any time, in the same program order on all ranks.
  // FX_HALO_COMM=0 (or an RCCL without ncclCommSplit): both use `comm`, which RCCL permits for operations that are ordered like this.
  const char *hc = getenv("FX_HALO_COMM");
  if (g_rccl.CommSplit && nranks > 1 && !(hc && atoi(hc) == 0)) {
    ncclComm_t halo = nullptr;
    if (g_rccl.CommSplit(comm, 0, rank, &halo, nullptr) == ncclSuccess && halo) c->nccl_halo = halo;
  }
  return 0;
}

// The communication ledger of this context (CommLedger, fx_internal.h): out[0] ops, [1] sequence hash, [2] all-reduces, [3] their
// bytes, [4] halo exchanges, [5] neighbours, [6] 1 = the halo exchange has its own communicator; then 5 per neighbour: rank, sends,
// send bytes, receives, receive bytes.  *n_out = entries the ledger holds, at most cap are written.
extern "C" int fx_comm_ledger(fx_context *c, int64_t *out, int32_t cap, int32_t *n_out) {
  if (!c) { g_fx_error = "fx_comm_ledger: null context"; return FX_ERROR_RUNTIME; }
  const CommLedger &g = c->ledger;
  std::vector<int64_t> v = {g.n_ops, (int64_t)g.seq_hash, g.n_allreduce, g.allreduce_bytes, g.n_halo, (int64_t)(g.peer.size() / 5),
                            c->nccl_halo ? 1 : 0};
  v.insert(v.end(), g.peer.begin(), g.peer.end());
  if (n_out) *n_out = (int32_t)v.size();
  for (int32_t k = 0; k < cap && k < (int32_t)v.size(); k++) out[k] = v[k];
  return 0;
}

extern "C" int fx_comm_set_host_callbacks(fx_context *c, int rank, int nranks, fx_halo_fn halo, fx_allreduce_fn allreduce,
                                          void *user) {
  c->cb_halo = halo; c->cb_allreduce = allreduce; c->cb_user = user;
  c->rank = rank; c->nranks = nranks;
  c->ledger = CommLedger();
  return 0;
}

// What the transport itself reports: ranks in the RCCL communicator (ncclCommCount) and the device it is bound to; with
// the host-callback transport the rank count given to fx_comm_set_host_callbacks; 1 / the context's device otherwise.
extern "C" int fx_comm_size(fx_context *c, int32_t *nranks, int32_t *device) {
  int n = c->nranks, d = c->device;
  if (c->nccl) {
    NCCL_TRY(g_rccl.CommCount((ncclComm_t)c->nccl, &n));
    NCCL_TRY(g_rccl.CommCuDevice((ncclComm_t)c->nccl, &d));
  }
  if (nranks) *nranks = n;
  if (device) *device = d;
  return 0;
}

// FX_FORCE_COMM=1 routes the scalar reductions through the communicator even with one rank
// (lets a single-GPU box exercise the RCCL all-reduce path).
// A comm view that says PETOT > 1 describes ONE SUBDOMAIN of a decomposed system: its dot products are partial sums and its halo
// columns need their owners' values.  Without a transport (fx_comm_init / fx_comm_set_host_callbacks) a solve would silently
// use rank-local reductions -- the reference would be inside MPI_Allreduce here (hecmw_comm_f.F90:346-379) -- so it is refused.
static int require_transport(const fx_context *c, const char *who) {
  if (c->view_petot > 1 && !c->nccl && !c->cb_allreduce) {
    g_fx_error = std::string(who) + ": the comm view describes a decomposed run (PETOT = " + std::to_string(c->view_petot) +
                 ") but this context has no transport: call fx_comm_init (RCCL) or fx_comm_set_host_callbacks first";
    return FX_ERROR_RUNTIME;
  }
  if (c->view_petot > 1 && c->nranks != c->view_petot) {
    g_fx_error = std::string(who) + ": the comm view says PETOT = " + std::to_string(c->view_petot) + " but the transport was set up for " +
                 std::to_string(c->nranks) + " ranks";
    return FX_ERROR_RUNTIME;
  }
  return 0;
}

static inline bool multi_rank(const fx_context *c) {
  static const bool force = getenv("FX_FORCE_COMM") && atoi(getenv("FX_FORCE_COMM")) != 0;
  return (c->nranks > 1 || force) && (c->nccl || c->cb_allreduce);
}

// SUM over ranks of n (<= 8) doubles living at device address v, on the solver stream.
static int allreduce_dev(fx_context *c, double *v, int n) {
  ClockScope cs(c, 2);
  { CommLedger &g = c->ledger; g.n_ops++; g.n_allreduce++; g.allreduce_bytes += 8 * n; g.mix(0xA11ull << 32 | (uint64_t)n); }
  if (c->nccl) {
    NCCL_TRY(g_rccl.AllReduce(v, v, n, ncclDouble, ncclSum, (ncclComm_t)c->nccl, c->stream));
    return 0;
  }
  double h[8];
  HIP_TRY(hipMemcpyAsync(h, v, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->cb_allreduce(h, n, c->cb_user);
  HIP_TRY(hipMemcpyAsync(v, h, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// hecmw_update_3_R (hecmw_comm_f.F90:669-694): persistent device buffers, one grouped send/recv per neighbour, no host
// synchronisation with RCCL.  Two halves so that the SpMV can multiply its interior rows in between:
//   halo_pack:     pack on the solver stream, comm_stream ordered after it by an event;
//   halo_exchange: the transfer + unpack on comm_stream (RCCL: enqueued; host callbacks: the host blocks on comm_stream only,
//                  so whatever was queued on the solver stream before -- the interior rows -- runs meanwhile);
//   halo_end:      the solver stream waits for the unpack.
// halo_update = the three back to back.
static inline bool halo_active(const fx_context *c) {
  // one rank WITH a communicator and a neighbour table exchanges with itself (periodic tables; tests use it to drive the
  // grouped ncclSend/ncclRecv on a single GPU)
  return c->halo.n_neighbor > 0 && !(c->nranks <= 1 && !c->nccl && !c->cb_halo);
}

static int halo_pack(fx_context *c, double *x) {
  HaloDev &h = c->halo;
  if (!halo_active(c)) return 0;
  if (!c->nccl && !c->cb_halo) { g_fx_error = "halo exchange requested but no communicator (fx_comm_init) was set"; return FX_ERROR_RUNTIME; }
  if (h.n_export > 0)
    hipLaunchKernelGGL(k_halo_pack, dim3((h.n_export + 255) / 256), dim3(256), 0, c->stream, h.n_export, h.export_item, x,
                       h.sendbuf);
  HIP_TRY(hipEventRecord(c->ev_packed, c->stream));
  HIP_TRY(hipStreamWaitEvent(c->comm_stream, c->ev_packed, 0));
  return 0;
}

static int halo_exchange(fx_context *c, double *x) {  // after halo_pack; everything on comm_stream
  HaloDev &h = c->halo;
  if (!halo_active(c)) return 0;
  hipStream_t cs = c->comm_stream;
  {
    CommLedger &g = c->ledger;
    g.n_ops++; g.n_halo++; g.mix(0x4A10ull << 32);
    if (g.peer.size() != (size_t)5 * h.n_neighbor) {
      g.peer.assign((size_t)5 * h.n_neighbor, 0);
      for (int k = 0; k < h.n_neighbor; k++) g.peer[5 * k] = h.neighbor[k];
    }
    for (int k = 0; k < h.n_neighbor; k++) {
      const int64_t ns = h.export_index[k + 1] - h.export_index[k], nr = h.import_index[k + 1] - h.import_index[k];
      if (ns > 0) { g.peer[5 * k + 1]++; g.peer[5 * k + 2] += 24 * ns; }
      if (nr > 0) { g.peer[5 * k + 3]++; g.peer[5 * k + 4] += 24 * nr; }
    }
  }
  if (!c->nccl) {  // host-staged transport: the host blocks on comm_stream only; what is queued on the solver stream keeps running
    if (!c->h_send) {
      HIP_TRY(hipHostMalloc((void **)&c->h_send, (size_t)3 * std::max(h.n_export, 1) * 8, hipHostMallocDefault));
      HIP_TRY(hipHostMalloc((void **)&c->h_recv, (size_t)3 * std::max(h.n_import, 1) * 8, hipHostMallocDefault));
    }
    HIP_TRY(hipMemcpyAsync(c->h_send, h.sendbuf, (size_t)3 * h.n_export * 8, hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipStreamSynchronize(cs));
    c->cb_halo(c->h_send, c->h_recv, c->cb_user);
    HIP_TRY(hipMemcpyAsync(h.recvbuf, c->h_recv, (size_t)3 * h.n_import * 8, hipMemcpyHostToDevice, cs));
  } else {
    const ncclComm_t hcomm = (ncclComm_t)(c->nccl_halo ? c->nccl_halo : c->nccl);
    NCCL_TRY(g_rccl.GroupStart());
    for (int k = 0; k < h.n_neighbor; k++) {
      const int32_t ns = h.export_index[k + 1] - h.export_index[k], nr = h.import_index[k + 1] - h.import_index[k];
      if (ns > 0)
        NCCL_TRY(g_rccl.Send(h.sendbuf + (size_t)3 * h.export_index[k], (size_t)3 * ns, ncclDouble, h.neighbor[k], hcomm, cs));
      if (nr > 0)
        NCCL_TRY(g_rccl.Recv(h.recvbuf + (size_t)3 * h.import_index[k], (size_t)3 * nr, ncclDouble, h.neighbor[k], hcomm, cs));
    }
    NCCL_TRY(g_rccl.GroupEnd());
  }
  if (h.n_import > 0)
    hipLaunchKernelGGL(k_halo_unpack, dim3((h.n_import + 255) / 256), dim3(256), 0, cs, h.n_import, h.import_item, h.recvbuf, x);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev_halo, cs));
  return 0;
}

static int halo_end(fx_context *c) {
  if (!halo_active(c)) return 0;
  HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_halo, 0));
  return 0;
}

static int halo_update(fx_context *c, double *x) {
  if (!halo_active(c)) return 0;
  ClockScope cs(c, 2);
  if (halo_pack(c, x) || halo_exchange(c, x)) return FX_ERROR_RUNTIME;
  return halo_end(c);
}

// ---------------------------------------------------------------------------
// building blocks on the solver stream
// ---------------------------------------------------------------------------
// level-scheduled sweeps in the natural numbering: ILU(0) (kind 10) and the natural-order SSOR (kind 11)
static inline bool level_sched(const fx_context *c) { return c->precond_kind == 10 || c->precond_kind == 11; }
static inline const int32_t *gate_status(fx_context *c) { return &c->st->status; }
static inline const int32_t *gate_verify(fx_context *c) { return &c->st->need_verify; }

// y = A x (mode 0) or y = b - A x (mode 1), optional fused dot partial (dot 1: x.y, 2: y.y).
// Domain-decomposed systems (FX_OVERLAP, default on): the interior virtual workgroups are launched while the halo exchange
// is in flight on comm_stream, the boundary ones after it -- same workgroup -> slices -> partial-slot mapping as the single
// launch, so y and the dot partials are bit-identical to it.
static int spmv_launch(fx_context *c, int mode, int dot, double *x, const double *b, double *y, const int32_t *gate,
                       int32_t gate_val, const int32_t *wg_list, int nwg) {
  const Bell &M = c->M;
  const int bs = c->spmv_bs;
  const dim3 g(nwg), blk(bs);
  double *part = c->partials;
  if (nwg <= 0) return 0;
#define SPMV_LAUNCH3(MODE, DOT, PIPE, B)                                                                              \
  hipLaunchKernelGGL((k_spmv<MODE, DOT, PIPE, B>), g, blk, 0, c->stream, M.nslices, c->ord.nslots, M.pair_ptr, M.val2, \
                     M.col2, x, b, y, part, gate, gate_val, M.slice_order, wg_list)
#define SPMV_LAUNCH(MODE, DOT)                                     \
  do {                                                             \
    if (c->pipe_spmv) {                                            \
      if (bs == 64) SPMV_LAUNCH3(MODE, DOT, true, 64);             \
      else SPMV_LAUNCH3(MODE, DOT, true, 256);                     \
    } else {                                                       \
      if (bs == 64) SPMV_LAUNCH3(MODE, DOT, false, 64);            \
      else SPMV_LAUNCH3(MODE, DOT, false, 256);                    \
    }                                                              \
  } while (0)
  if (mode == 0 && dot == 0) SPMV_LAUNCH(0, 0);
  else if (mode == 0 && dot == 1) SPMV_LAUNCH(0, 1);
  else if (mode == 1 && dot == 0) SPMV_LAUNCH(1, 0);
  else if (mode == 1 && dot == 2) SPMV_LAUNCH(1, 2);
  else { g_fx_error = "spmv: bad mode"; return FX_ERROR_RUNTIME; }
#undef SPMV_LAUNCH
#undef SPMV_LAUNCH3
  HIP_TRY(hipGetLastError());
  return 0;
}

static inline int spmv_nparts(fx_context *c);
static int spmv(fx_context *c, int mode, int dot, double *x, const double *b, double *y, const int32_t *gate,
                int32_t gate_val) {
  const Bell &M = c->M;
  const int nwg = spmv_nparts(c);
  if (c->overlap && halo_active(c) && M.wg_interior && M.n_wg_interior > 0) {
    if (halo_pack(c, x)) return FX_ERROR_RUNTIME;
    {
      ClockScope cs(c, 0);
      if (spmv_launch(c, mode, dot, x, b, y, gate, gate_val, M.wg_interior, M.n_wg_interior)) return FX_ERROR_RUNTIME;
    }
    if (halo_exchange(c, x)) return FX_ERROR_RUNTIME;  // in flight beside the interior rows
    { ClockScope cs(c, 2); if (halo_end(c)) return FX_ERROR_RUNTIME; }  // what the solver stream still waits for = exposed comm time
    ClockScope cs(c, 0);
    return spmv_launch(c, mode, dot, x, b, y, gate, gate_val, M.wg_boundary, M.n_wg_boundary);
  }
  if (halo_update(c, x)) return FX_ERROR_RUNTIME;
  ClockScope cs(c, 0);
  return spmv_launch(c, mode, dot, x, b, y, gate, gate_val, nullptr, nwg);
}
static inline int spmv_nparts(fx_context *c) { return (c->M.nslices + c->spmv_bs / 64 - 1) / (c->spmv_bs / 64); }

template <int OP>
static int scalar_stage(fx_context *c, int nparts, int stride, int recompute_every, const double *parts = nullptr) {
  if (!parts) parts = c->partials;
  if (multi_rank(c)) {
    hipLaunchKernelGGL((k_scalar<OP>), dim3(1), dim3(1024), 0, c->stream, parts, nparts, stride, c->st, c->hist,
                       c->red_out, 1, recompute_every);
    if (allreduce_dev(c, c->red_out, 2)) return FX_ERROR_RUNTIME;
    hipLaunchKernelGGL((k_scalar<OP>), dim3(1), dim3(64), 0, c->stream, parts, nparts, stride, c->st, c->hist,
                       c->red_out, 2, recompute_every);
  } else {
    hipLaunchKernelGGL((k_scalar<OP>), dim3(1), dim3(1024), 0, c->stream, parts, nparts, stride, c->st, c->hist,
                       c->red_out, 0, recompute_every);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// preconditioner setup (hecmw_precond_33_setup, 33/hecmw_precond_33.f90:27-50)
// ---------------------------------------------------------------------------
static int diag_setup(fx_context *c, double sigma_diag) {
  const int32_t nslots = c->ord.nslots;
  c->diag.nslices = nslots / 64;
  dev_free(c->diag.alu);
  if (dev_alloc(&c->diag.alu, (size_t)c->diag.nslices * 576)) return FX_ERROR_RUNTIME;
  hipLaunchKernelGGL(k_alu_setup, dim3((nslots + 255) / 256), dim3(256), 0, c->stream, nslots, c->A.N, c->ord.d_slot_node,
                     c->A.D, sigma_diag, c->diag.alu);
  HIP_TRY(hipGetLastError());
  return 0;
}

// hecmw_matrix_ordering_CM's "RCM" (level ordering from the best of <= 5 minimum-degree starts + the id mirror of
// reverse_ordering, hecmw_matrix_ordering_CM.f90:16-55, :169-178) with the breadth-first levels on the DEVICE: kernels
// k_bfsb_* walk all candidate starts at once with the level state resident (five launches per level for all starts, the
// host looks at the state every `bfs_batch` levels; 150 levels at 150^3 nodes).  A start whose graph is disconnected (the
// reference then jumps to the lowest unvisited node) falls back to the host walk for that start.
template <class GetGraph>
static int rcm_sequence_device(fx_context *c, const DevCSR &A, const std::vector<int32_t> &starts, GetGraph graph,
                               std::vector<int32_t> &seq_out) {
  const int32_t N = A.N;
  const int S = (int)starts.size();
  const int32_t nvb_max = (N + 255) / 256 + 1;
  DevScratch tmp;
  uint8_t *seen = nullptr;
  uint32_t *claim = nullptr;
  int32_t *seq = nullptr, *cnt = nullptr, *bsum = nullptr, *boff = nullptr;
  BfsState *st = nullptr;  // [2][S]
  if (tmp.alloc(&seen, (size_t)N * S) || tmp.alloc(&claim, (size_t)N * S) || tmp.alloc(&seq, (size_t)N * S) ||
      tmp.alloc(&cnt, (size_t)N * S) || tmp.alloc(&bsum, (size_t)nvb_max * S) || tmp.alloc(&boff, (size_t)nvb_max * S) ||
      tmp.alloc(&st, (size_t)2 * S))
    return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemsetAsync(seen, 0, (size_t)N * S, c->stream));
  HIP_TRY(hipMemsetAsync(claim, 0xFF, (size_t)N * S * 4, c->stream));
  std::vector<BfsState> h_st((size_t)2 * S);
  const uint8_t one = 1;
  for (int s = 0; s < S; s++) {
    h_st[s] = h_st[S + s] = BfsState{0, 1, 1, 0};
    HIP_TRY(hipMemcpyAsync(seq + (size_t)s * N, &starts[s], 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(seen + (size_t)s * N + starts[s], &one, 1, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(st, h_st.data(), h_st.size() * sizeof(BfsState), hipMemcpyHostToDevice, c->stream));
  const dim3 grid(std::max(1, std::min(2 * c->n_cu, (N + 255) / 256)), S), blk(256);
  int par = 0;
  for (int64_t level = 0;; ) {
    for (int i = 0; i < c->bfs_batch; i++, level++, par ^= 1) {
      const BfsState *cur = st + (size_t)par * S;
      BfsState *nxt = st + (size_t)(par ^ 1) * S;
      hipLaunchKernelGGL(k_bfsb_claim, grid, blk, 0, c->stream, N, cur, A.indexL, A.itemL, A.indexU, A.itemU, seq, seen, claim);
      hipLaunchKernelGGL(k_bfsb_count, grid, blk, 0, c->stream, N, nvb_max, cur, A.indexL, A.itemL, A.indexU, A.itemU, seq, seen, claim, cnt, bsum);
      hipLaunchKernelGGL(k_bfsb_scan, dim3(S), dim3(1024), 0, c->stream, N, nvb_max, cur, nxt, bsum, boff);
      hipLaunchKernelGGL(k_bfsb_write, grid, blk, 0, c->stream, N, nvb_max, cur, A.indexL, A.itemL, A.indexU, A.itemU, seq, seen, claim, cnt, boff);
      hipLaunchKernelGGL(k_bfsb_mark, grid, blk, 0, c->stream, N, cur, nxt, seq, seen);
    }
    HIP_TRY(hipMemcpyAsync(h_st.data(), st + (size_t)par * S, (size_t)S * sizeof(BfsState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    bool all = true;
    for (int s = 0; s < S; s++) all = all && (h_st[s].hi >= N || h_st[s].stuck);
    if (all) break;
    if (level > (int64_t)N + c->bfs_batch) { g_fx_error = "level ordering on the device made no progress"; return FX_ERROR_RUNTIME; }
  }
  HIP_TRY(hipGetLastError());
  int32_t best_levels = -1;
  int best = -1;  // >= 0: a device sequence; -2: seq_out already holds a host walk
  std::vector<int32_t> cur;
  for (int s = 0; s < S; s++) {  // strictly more levels wins: the first of equals stays (hecmw_matrix_ordering_CM.f90:41-47)
    int32_t nlevel = h_st[s].nlevel;
    const bool on_device = h_st[s].hi == N && !h_st[s].stuck;
    if (!on_device) nlevel = fxo::level_order_host(graph(), starts[s], cur);
    if (nlevel > best_levels) {
      best_levels = nlevel;
      if (on_device) best = s;
      else { best = -2; seq_out = cur; }
    }
  }
  if (best >= 0) {
    seq_out.resize((size_t)N);
    HIP_TRY(hipMemcpy(seq_out.data(), seq + (size_t)best * N, (size_t)N * 4, hipMemcpyDeviceToHost));
  }
  for (auto &v : seq_out) v = N - 1 - v;  // reverse_ordering: id mirror
  return 0;
}

// hecmw_matrix_ordering_MC (hecmw_matrix_ordering_MC.f90:15-72) on the device: kernels k_mc_* (fx_kernels.h).  Every
// `mc_batch` rounds the host looks at the length of the next IN queue; an empty one ends the colour.  perm: new -> old
// (0-based), colour by colour.  Returns 1 (nothing changed, the caller takes the host walk) when a colour needs more
// rounds than the queue-length table holds: a graph whose decisions form one long chain.
static int multicolor_device(fx_context *c, const DevCSR &A, const std::vector<int32_t> &seq_h, int ncolor_in,
                             std::vector<int32_t> &perm, std::vector<int32_t> &colorindex) {
  const int32_t N = A.N, cap = N / ncolor_in;
  DevScratch tmp;
  const int32_t nb16 = (int32_t)(((int64_t)N + 4095) / 4096);
  const int max_rounds = 1 << 16;
  int32_t *seq = nullptr, *info = nullptr, *cnt = nullptr, *inq = nullptr, *outq = nullptr, *n_in = nullptr, *n_out = nullptr,
          *tot = nullptr, *bsum = nullptr, *boff = nullptr, *d_perm = nullptr;
  if (tmp.alloc(&seq, (size_t)N) || tmp.alloc(&info, (size_t)N) || tmp.alloc(&cnt, (size_t)N) || tmp.alloc(&inq, (size_t)N) ||
      tmp.alloc(&outq, (size_t)N) || tmp.alloc(&n_in, (size_t)max_rounds + 1) || tmp.alloc(&n_out, (size_t)max_rounds) ||
      tmp.alloc(&tot, 4) || tmp.alloc(&bsum, (size_t)nb16) || tmp.alloc(&boff, (size_t)nb16 + 1) || tmp.alloc(&d_perm, (size_t)N))
    return FX_ERROR_RUNTIME;
  int32_t *h = (int32_t *)(c->st_host + 3) + 4;  // pinned
  HIP_TRY(hipMemcpyAsync(seq, seq_h.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_mc_pos, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, seq, info);
  const int batch = std::max(1, c->mc_batch);
  const dim3 qgrid(std::max(1, std::min(16 * c->n_cu, (N + 7) / 8))), blk(256);
  colorindex.assign(1, 0);
  int32_t done = 0;
  int64_t rounds_total = 0;
  const double t_begin = now_s();
  while (done < N) {
    HIP_TRY(hipMemsetAsync(n_in, 0, ((size_t)max_rounds + 1) * 4, c->stream));
    HIP_TRY(hipMemsetAsync(n_out, 0, (size_t)max_rounds * 4, c->stream));
    hipLaunchKernelGGL(k_mc_init, dim3((N + 7) / 8), blk, 0, c->stream, N, A.indexL, A.itemL, A.indexU, A.itemU, info, cnt, inq, n_in);
    int r = 0;
    for (;;) {
      if (r + batch > max_rounds) return 1;
      for (int i = 0; i < batch; i++, r++) {
        hipLaunchKernelGGL(k_mc_in, qgrid, blk, 0, c->stream, N, A.indexL, A.itemL, A.indexU, A.itemU, info, inq, n_in + r, outq, n_out + r);
        hipLaunchKernelGGL(k_mc_out, qgrid, blk, 0, c->stream, N, A.indexL, A.itemL, A.indexU, A.itemU, info, cnt, outq, n_out + r, inq,
                           n_in + r + 1);
      }
      HIP_TRY(hipMemcpyAsync(h, n_in + r, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (h[0] == 0) break;  // no new pick: no new block either, every node of the pool is decided
    }
    hipLaunchKernelGGL(k_mc_blockcount, dim3(nb16), blk, 0, c->stream, N, seq, info, bsum);
    hipLaunchKernelGGL(k_scan_excl, dim3(1), dim3(1024), 0, c->stream, nb16, bsum, boff, tot);
    hipLaunchKernelGGL(k_mc_assign, dim3(nb16), blk, 0, c->stream, N, cap > 0 ? cap : N, done, seq, boff, info, d_perm);
    HIP_TRY(hipMemcpyAsync(h, tot, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int32_t picked = cap > 0 ? std::min(h[0], cap) : h[0];
    if (picked <= 0) { g_fx_error = "multicolouring on the device picked nothing"; return FX_ERROR_RUNTIME; }
    done += picked;
    colorindex.push_back(done);
    rounds_total += r;
  }
  HIP_TRY(hipGetLastError());
  if (getenv("FX_TIMING") && atoi(getenv("FX_TIMING")))
    fprintf(stderr, "[fx timing] multicolour on the device: %zu colours, %lld rounds, %.3f s\n", colorindex.size() - 1,
            (long long)rounds_total, now_s() - t_begin);
  perm.resize((size_t)N);
  HIP_TRY(hipMemcpy(perm.data(), d_perm, (size_t)N * 4, hipMemcpyDeviceToHost));
  return 0;
}

// The reference's ordering of the multicolour SSOR (hecmw_matrix_ordering_CM + _MC): level sequence from the best of the
// minimum-degree starts, capped greedy colouring -- on the device from bfs_device_min / mc_device_min block rows on (A: the
// profile resident on the device; iL .. jU: the same arrays on the host), with the host walks of fx_order.cpp for small
// systems and as the fallback.  deg: node degrees inside the subdomain; perm0: new -> old (0-based), colour by colour.
static int ssor_ordering(fx_context *c, const DevCSR &A, const int32_t *iL, const int32_t *jL, const int32_t *iU, const int32_t *jU,
                         int ncolor_in, std::vector<int32_t> &deg, std::vector<int32_t> &perm0, std::vector<int32_t> &cidx,
                         PhaseTimer &pt) {
  const int32_t N = A.N;
  // halo columns -- ids > N, last in the ascending itemU -- are not part of the graph
  deg.resize((size_t)N);
  parallel_for(N, [&](int64_t a, int64_t b) {
    for (int64_t r = a; r < b; r++) {
      int32_t e = iU[r + 1];
      while (e > iU[r] && jU[e - 1] > N) e--;
      deg[r] = (iL[r + 1] - iL[r]) + (e - iU[r]);
    }
  });
  fxo::Graph g_store;  // the host adjacency is only built when a host walk needs it (small systems, disconnected graphs)
  bool g_built = false;
  auto graph = [&]() -> const fxo::Graph & {
    if (!g_built) { g_store = fxo::build_graph(N, iL, jL, iU, jU); g_built = true; }
    return g_store;
  };
  pt.lap("degrees");
  std::vector<int32_t> seq;
  if (N >= c->bfs_device_min) {
    if (rcm_sequence_device(c, A, fxo::rcm_starts_deg(N, deg.data()), graph, seq)) return FX_ERROR_RUNTIME;
  } else seq = fxo::rcm_sequence(graph());
  pt.lap("level ordering");
  int mc = 1;
  if (N >= c->mc_device_min && ncolor_in > 0 && N / ncolor_in > 0) {
    mc = multicolor_device(c, A, seq, ncolor_in, perm0, cidx);
    if (mc < 0) return FX_ERROR_RUNTIME;
  }
  if (mc > 0) fxo::multicolor(graph(), seq, ncolor_in, perm0, cidx);
  pt.lap("multicolour");
  return 0;
}

// hecmw_precond_SSOR_33_setup (hecmw_precond_SSOR_33.f90:55-223), always on the
// multicolour path (the reference's nthreads > 1 branch :102-111): ordering on the
// host, values gathered on the device.  Within a colour the slots are sorted by the
// number of lower blocks (rows of one colour are independent, so the order inside a
// colour does not change the result) which keeps the BELL padding of L and U small.
static int ssor_setup_symbolic(fx_context *c, int ncolor_in) {
  const int32_t N = c->A.N;
  SsorDev &S = c->ssor;
  const int32_t *iL = c->h_indexL.data(), *jL = c->h_itemL.data(), *iU = c->h_indexU.data(), *jU = c->h_itemU.data();
  PhaseTimer pt("ssor symbolic");
  std::vector<int32_t> deg, perm0, cidx;
  if (ssor_ordering(c, c->A, iL, jL, iU, jU, ncolor_in, deg, perm0, cidx, pt)) return FX_ERROR_RUNTIME;
  S.ncolor = (int32_t)cidx.size() - 1;
  S.colorindex = cidx;
  S.perm.resize(N);
  std::vector<int32_t> newpos((size_t)N);  // old -> new (0-based), the reference's iperm
  for (int32_t i = 0; i < N; i++) { S.perm[i] = perm0[i] + 1; newpos[perm0[i]] = i; }
  // number of lower blocks per old row under the new numbering
  std::vector<int32_t> nlow((size_t)N);
  parallel_for(N, [&](int64_t a, int64_t b) {
    for (int64_t r = a; r < b; r++) {
      int32_t k = 0;
      for (int32_t e = iL[r]; e < iL[r + 1]; e++) k += (newpos[jL[e] - 1] < newpos[r]);
      for (int32_t e = iU[r]; e < iU[r + 1] && jU[e] <= N; e++) k += (newpos[jU[e] - 1] < newpos[r]);
      nlow[r] = k;
    }
  });
  // slot order: colour by colour (each colour starts a new slice); inside a colour natural node
  // order (rows of one colour are independent), split only by the lower-block count so that
  // boundary rows do not pad the interior slices
  std::vector<int32_t> slot_row;
  slot_row.reserve((size_t)N + 64 * S.ncolor);
  S.color_slice.assign(1, 0);
  std::vector<std::vector<int32_t>> color_rows((size_t)S.ncolor);
  {  // the colours are sorted independently: one host thread each
    std::vector<std::thread> th;
    const int nt = std::max(1, std::min(nthreads_host(), (int)S.ncolor));
    for (int t = 0; t < nt; t++)
      th.emplace_back([&, t] {
        for (int32_t col = t; col < S.ncolor; col += nt) {
          std::vector<int32_t> &rows = color_rows[col];
          rows.assign(perm0.begin() + cidx[col], perm0.begin() + cidx[col + 1]);
          std::sort(rows.begin(), rows.end());
          std::stable_sort(rows.begin(), rows.end(), [&](int32_t a, int32_t b) { return nlow[a] < nlow[b]; });
          if (c->halo.n_neighbor > 0)  // subdomain: rows with a halo column last, so that they share few slices (interior / boundary split of the SpMV)
            std::stable_sort(rows.begin(), rows.end(), [&](int32_t a, int32_t b) {
              const bool ha = iU[a + 1] > iU[a] && jU[iU[a + 1] - 1] > N, hb = iU[b + 1] > iU[b] && jU[iU[b + 1] - 1] > N;
              return ha < hb;
            });
        }
      });
    for (auto &t : th) t.join();
  }
  for (int32_t col = 0; col < S.ncolor; col++) {
    const std::vector<int32_t> &rows = color_rows[col];
    slot_row.insert(slot_row.end(), rows.begin(), rows.end());
    while (slot_row.size() % 64) slot_row.push_back(-1);
    S.color_slice.push_back((int32_t)(slot_row.size() / 64));
  }
  const int32_t nslots = (int32_t)slot_row.size();
  pt.lap("slot order");
  // node -> slot of the sweep's private colour-major vector
  std::vector<int32_t> slot_of((size_t)N, 0);
  for (int32_t sl = 0; sl < nslots; sl++)
    if (slot_row[sl] >= 0) slot_of[slot_row[sl]] = sl;
  const int32_t *so = slot_of.data();
  S.nslots = nslots;
  dev_free(S.slot_node); dev_free(S.zs); dev_free(S.zb);
  if (dev_alloc(&S.slot_node, (size_t)nslots) || dev_alloc(&S.zs, (size_t)3 * nslots)) return FX_ERROR_RUNTIME;
  if (c->df_mode >= 2 && dev_alloc(&S.zb, (size_t)3 * nslots)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpy(S.slot_node, slot_row.data(), (size_t)nslots * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(S.zs, 0, (size_t)3 * nslots * 8));
  c->ssor_mode_built = c->ssor_mode;
  if (c->ssor_mode == 1) {  // the whole solver runs in this numbering (vectors, SpMV layout, halo lists)
    if (set_ordering(c, 1, &slot_row)) return FX_ERROR_RUNTIME;
  } else if (c->ord.kind != 0) {
    if (set_ordering(c, 0, nullptr)) return FX_ERROR_RUNTIME;
  }
  pt.lap("solver ordering + full-matrix layout");
  // lower / upper parts per slot, entries ordered by the reference's new index (ascending for the
  // forward sweep, descending for the backward sweep, as SSOR_33.f90:312 / :369 walk them)
  auto collect = [&](int32_t slot, std::vector<BellEntry> &e, bool lower) {
    const int32_t r = slot_row[slot];
    const int32_t me = newpos[r];
    thread_local std::vector<std::pair<int32_t, BellEntry>> tmp;  // one scratch per host thread, not one malloc per row
    tmp.clear();
    for (int32_t j = iL[r]; j < iL[r + 1]; j++) {
      const int32_t co = jL[j] - 1;
      if ((newpos[co] < me) == lower) tmp.push_back({newpos[co], {3 * j + 1, so[co]}});
    }
    for (int32_t j = iU[r]; j < iU[r + 1]; j++) {
      const int32_t co = jU[j] - 1;
      if (co >= N) continue;  // halo columns are dropped (hecmw_matrix_reorder.f90:50)
      if ((newpos[co] < me) == lower) tmp.push_back({newpos[co], {3 * j + 2, so[co]}});
    }
    if (lower) std::sort(tmp.begin(), tmp.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    else std::sort(tmp.begin(), tmp.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    for (auto &t : tmp) e.push_back(t.second);
  };
  auto countL = [&](int32_t slot) { const int32_t r = slot_row[slot]; return r < 0 ? 0 : nlow[r]; };
  auto countU = [&](int32_t slot) {
    const int32_t r = slot_row[slot];
    return r < 0 ? 0 : deg[r] - nlow[r];
  };
  auto fillL = [&](int32_t slot, std::vector<BellEntry> &e) { collect(slot, e, true); };
  auto fillU = [&](int32_t slot, std::vector<BellEntry> &e) { collect(slot, e, false); };
  {  // the two sweep layouts on the device (host builder only for rows longer than the kernels' buffer)
    DevScratch tmp;
    int32_t *d_so = nullptr, *d_np = nullptr;
    if (tmp.alloc(&d_so, (size_t)N) || tmp.alloc(&d_np, (size_t)N)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpy(d_so, slot_of.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_np, newpos.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    int e = bell_build_device(c, S.L, BV_SSOR_L, nslots, S.slot_node, d_so, d_np);
    if (e < 0 || (e > 0 && bell_build2(c, S.L, nslots, &slot_row, countL, fillL))) return FX_ERROR_RUNTIME;
    pt.lap("lower layout");
    e = bell_build_device(c, S.U, BV_SSOR_U, nslots, S.slot_node, d_so, d_np);
    if (e < 0 || (e > 0 && bell_build2(c, S.U, nslots, &slot_row, countU, fillU))) return FX_ERROR_RUNTIME;
    pt.lap("upper layout");
  }
  dev_free(S.alu);
  if (dev_alloc(&S.alu, (size_t)(nslots / 64) * 576)) return FX_ERROR_RUNTIME;
  return 0;
}

static int precond_apply_once(fx_context *c, const double *r, double *z, bool want_dot, int *nparts);

static int ssor_setup_numeric(fx_context *c, double sigma_diag) {
  SsorDev &S = c->ssor;
  if (bell_fill_values(c, S.L) || bell_fill_values(c, S.U)) return FX_ERROR_RUNTIME;
  const int nslots = S.L.nslices * 64;
  hipLaunchKernelGGL(k_alu_setup, dim3((nslots + 255) / 256), dim3(256), 0, c->stream, nslots, c->A.N, S.slot_node, c->A.D,
                     sigma_diag, S.alu);
  S.sigma_diag = sigma_diag;
  S.values_epoch = c->values_epoch;  // the sweep layouts hold the values the SpMV layout holds (fx_precond_setup ran ensure_solver first)
  if (c->eisenstat) {  // Eisenstat form: the diagonal blocks themselves, next to their factors
    if (c->halo.n_neighbor > 0 && c->ord.kind == 1) {  // subdomain: the halo-column blocks, in the same slot order, columns = Krylov vector slots
      if (S.H.nslices == 0) {
        const int e = bell_build_device(c, S.H, BV_HALO, nslots, S.slot_node, c->ord.d_slot_of, nullptr);
        if (e < 0) return FX_ERROR_RUNTIME;
        if (e > 0) bell_free(S.H);  // rows longer than the device buffer: no halo layout, the standard loop serves this system
      }
      if (S.H.nslices > 0 && bell_fill_values(c, S.H)) return FX_ERROR_RUNTIME;
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// hecmw_precond_BILU_33_setup / FORM_ILU0_33 (hecmw_precond_BILU_33.f90:34-88, :185-362) by dependency
// levels.  The level structure reuses the SSOR machinery: "colours" = levels, a private level-major
// sweep vector, BELL copies of the strictly lower / upper FACTOR blocks; the apply (:90-157) is then the
// same pair of sweeps as SSOR's, forward over ascending levels, backward over descending ones.
static int ilu_setup_symbolic(fx_context *c) {
  const int32_t N = c->A.N;
  SsorDev &S = c->ssor;
  const int32_t *iL = c->h_indexL.data(), *jL = c->h_itemL.data(), *iU = c->h_indexU.data(), *jU = c->h_itemU.data();
  PhaseTimer pt("ilu symbolic");
  std::vector<int32_t> level((size_t)N, 0);
  int32_t nlev = 0;
  for (int32_t i = 0; i < N; i++) {  // rows in natural order: every k in L(i) is < i
    int32_t l = 0;
    for (int32_t j = iL[i]; j < iL[i + 1]; j++) l = std::max(l, level[jL[j] - 1]);
    level[i] = l + 1;
    nlev = std::max(nlev, l + 1);
  }
  std::vector<int32_t> cnt((size_t)nlev + 1, 0);
  for (int32_t i = 0; i < N; i++) cnt[level[i]]++;
  // slot order: level by level, natural order inside a level, each level padded to a 64 multiple
  std::vector<int32_t> start((size_t)nlev + 2, 0);
  for (int32_t l = 1; l <= nlev; l++) start[l + 1] = start[l] + (cnt[l] + 63) / 64 * 64;
  const int32_t nslots = start[nlev + 1];
  std::vector<int32_t> slot_row((size_t)nslots, -1), fillpos(start.begin(), start.end());
  for (int32_t i = 0; i < N; i++) slot_row[fillpos[level[i]]++] = i;
  std::vector<int32_t> slot_of((size_t)N);
  for (int32_t sl = 0; sl < nslots; sl++)
    if (slot_row[sl] >= 0) slot_of[slot_row[sl]] = sl;
  S.ncolor = nlev;
  S.color_slice.assign((size_t)nlev + 1, 0);
  S.max_row_blocks = 0;
  for (int32_t i = 0; i < N; i++) S.max_row_blocks = std::max(S.max_row_blocks, (iL[i + 1] - iL[i]) + (c->h_indexU[i + 1] - c->h_indexU[i]));
  S.slot_start.assign((size_t)nlev + 1, 0);
  for (int32_t l = 1; l <= nlev; l++) { S.color_slice[l] = start[l + 1] / 64; S.slot_start[l] = start[l + 1]; }
  S.nslots = nslots;
  dev_free(S.slot_node); dev_free(S.zs); dev_free(S.zb);
  if (dev_alloc(&S.slot_node, (size_t)nslots) || dev_alloc(&S.zs, (size_t)3 * nslots)) return FX_ERROR_RUNTIME;
  if (c->df_mode >= 1 && dev_alloc(&S.zb, (size_t)3 * nslots)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpy(S.slot_node, slot_row.data(), (size_t)nslots * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(S.zs, 0, (size_t)3 * nslots * 8));
  if (c->ord.kind > 0 && set_ordering(c, 0, nullptr)) return FX_ERROR_RUNTIME;
  const int32_t *so = slot_of.data(), *sr = slot_row.data();
  auto countL = [=](int32_t slot) { const int32_t r = sr[slot]; return r < 0 ? 0 : iL[r + 1] - iL[r]; };
  auto countU = [=](int32_t slot) {
    const int32_t r = sr[slot];
    if (r < 0) return 0;
    int32_t k = 0;
    for (int32_t j = iU[r]; j < iU[r + 1]; j++) k += (jU[j] <= N);
    return k;
  };
  auto fillL = [=](int32_t slot, std::vector<BellEntry> &e) {  // ascending columns (:104-111)
    const int32_t r = sr[slot];
    for (int32_t j = iL[r]; j < iL[r + 1]; j++) e.push_back({3 * j + 1, so[jL[j] - 1]});
  };
  auto fillU = [=](int32_t slot, std::vector<BellEntry> &e) {  // descending columns (:133 `do j= ieU, isU, -1`)
    const int32_t r = sr[slot];
    for (int32_t j = iU[r + 1] - 1; j >= iU[r]; j--)
      if (jU[j] <= N) e.push_back({3 * j + 2, so[jU[j] - 1]});
  };
  {
    DevScratch tmp;
    int32_t *d_so = nullptr;
    if (tmp.alloc(&d_so, (size_t)N)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpy(d_so, slot_of.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    int e = bell_build_device(c, S.L, BV_ILU_L, nslots, S.slot_node, d_so, nullptr);
    if (e < 0 || (e > 0 && bell_build2(c, S.L, nslots, &slot_row, countL, fillL))) return FX_ERROR_RUNTIME;
    pt.lap("lower layout");
    e = bell_build_device(c, S.U, BV_ILU_U, nslots, S.slot_node, d_so, nullptr);
    if (e < 0 || (e > 0 && bell_build2(c, S.U, nslots, &slot_row, countU, fillU))) return FX_ERROR_RUNTIME;
    pt.lap("upper layout");
  }
  dev_free(S.alu);
  if (dev_alloc(&S.alu, (size_t)(nslots / 64) * 576)) return FX_ERROR_RUNTIME;
  {  // level of every slice (FX_DF_PRESLEEP)
    std::vector<int32_t> sl((size_t)nslots / 64, 0);
    for (int32_t l = 1; l <= nlev; l++)
      for (int32_t k = S.color_slice[l - 1]; k < S.color_slice[l]; k++) sl[k] = l;
    dev_free(S.slice_level);
    if (dev_alloc(&S.slice_level, sl.size())) return FX_ERROR_RUNTIME;
    HIP_TRY(hipMemcpy(S.slice_level, sl.data(), sl.size() * 4, hipMemcpyHostToDevice));
  }
  pt.lap("level layouts");
  if (march_build(c)) return FX_ERROR_RUNTIME;  // the same sweeps as a plane march (fx_march.h), when the structure and the cost model admit it
  pt.lap("march programs");
  return 0;
}

// factor = false: the natural-order block SSOR (hecmw_precond_SSOR_33.f90:93-101 with the sweeps :300-410, the reference's
// behaviour in a serial or flat-MPI build): the same dependency levels -- row i waits for its lower neighbours -- with the ORIGINAL
// off-diagonal blocks and the LU of the sigma-scaled diagonal blocks, which is what Dlu0 is too (k_dlu_natural).
static int ilu_setup_numeric(fx_context *c, double sigma_diag, bool factor) {
  SsorDev &S = c->ssor;
  const DevCSR &A = c->A;
  dev_free(S.lu_D); dev_free(S.lu_AL); dev_free(S.lu_AU);
  if (!factor) {
    if (bell_fill_values(c, S.L) || bell_fill_values(c, S.U)) return FX_ERROR_RUNTIME;
    hipLaunchKernelGGL(k_alu_setup, dim3((S.nslots + 255) / 256), dim3(256), 0, c->stream, S.nslots, A.N, S.slot_node, A.D, sigma_diag, S.alu);
    HIP_TRY(hipGetLastError());
    if (march_fill_values(c, A.AL, A.AU, sigma_diag)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  }
  if (dev_alloc(&S.lu_D, (size_t)9 * A.N) || dev_alloc(&S.lu_AL, (size_t)9 * A.NPL) || dev_alloc(&S.lu_AU, (size_t)9 * A.NPU))
    return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(S.lu_AL, A.AL, (size_t)9 * A.NPL * 8, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(S.lu_AU, A.AU, (size_t)9 * A.NPU * 8, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_dlu_natural, dim3((A.N + 255) / 256), dim3(256), 0, c->stream, A.N, A.D, sigma_diag, S.lu_D);
  for (int32_t l = 1; l <= S.ncolor; l++) {
    const int32_t s0 = S.slot_start[l - 1], s1 = S.slot_start[l];
    if (l == 1 || s1 <= s0) continue;  // level 1 rows have no lower blocks
    if (S.max_row_blocks <= 32)        // 32 lanes per row, one destination block each
      hipLaunchKernelGGL(k_ilu0_factor_level32, dim3((s1 - s0 + 7) / 8), dim3(256), 0, c->stream, s0, s1, S.slot_node, A.N,
                         A.indexL, A.itemL, A.indexU, A.itemU, S.lu_D, S.lu_AL, S.lu_AU);
    else
      hipLaunchKernelGGL(k_ilu0_factor_level, dim3((s1 - s0 + 127) / 128), dim3(128), 0, c->stream, s0, s1, S.slot_node, A.N,
                         A.indexL, A.itemL, A.indexU, A.itemU, S.lu_D, S.lu_AL, S.lu_AU);
  }
  HIP_TRY(hipGetLastError());
  if (bell_fill_values(c, S.L, S.lu_D, S.lu_AL, S.lu_AU) || bell_fill_values(c, S.U, S.lu_D, S.lu_AL, S.lu_AU)) return FX_ERROR_RUNTIME;
  const int nslots = S.nslots;
  hipLaunchKernelGGL(k_alu_setup, dim3((nslots + 255) / 256), dim3(256), 0, c->stream, nslots, A.N, S.slot_node, A.D, sigma_diag,
                     S.alu);
  HIP_TRY(hipGetLastError());
  if (march_fill_values(c, S.lu_AL, S.lu_AU, sigma_diag)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipStreamSynchronize(c->stream));
  dev_free(S.lu_D); dev_free(S.lu_AL); dev_free(S.lu_AU);  // the sweeps only stream the BELL copies
  return 0;
}

// Which physical buffer plays which work vector.  In the first context of a process the first two or three work vectors
// can sit in a slow spot: the same CG + SSOR iteration ran at 2.92 ms with r, z/q, p on buffers 0, 1, 2 and at 2.66 ms on
// 3, 4, 5 (or 5, 6, 7, or 7, 8, 9), while later contexts of that process showed no spread at all
// (scripts/experiments/ab_wperm.py) -- the run-to-run spread of the bench line.  The ten buffers are interchangeable, so
// each is timed as the sweep vector of the preconditioner, as the output and as the gathered input of the SpMV, and the
// fastest take the roles the loops hammer: z/q, p, r of CG; p~, s~, v, t of BiCGSTAB.  Large systems, once per allocation.
extern "C" int fx_precond_setup(fx_context *c, const int32_t *Iarray, const double *Rarray) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->have_values) { g_fx_error = "fx_precond_setup: no matrix values resident"; return FX_ERROR_RUNTIME; }
  const int precond = Iarray[2], iterpremax = Iarray[4], ncolor_in = Iarray[33] > 0 ? Iarray[33] : 10;
  double sigma_diag = Rarray[1];
  if (sigma_diag < 0.0) sigma_diag = 1.0;  // auto mode starts from 1 (hecmw_solver_Iterative.f90:68-73)
  c->iterpremax = iterpremax;
  if (iterpremax <= 0) {
    free_precond(c);
    if (ensure_solver(c)) return FX_ERROR_RUNTIME;
    c->precond_valid = true;
    return 0;
  }
  int kind;
  switch (precond) {
    case 1: case 2: kind = c->ssor_natural ? 11 : 1; break;  // 11: the reference's nthreads == 1 branch (hecmw_precond_SSOR_33.f90:93-101)
    case 3: kind = 3; break;
    case 10: kind = 10; break;
    default:
      g_fx_error = "PRECOND=" + std::to_string(precond) + " is not on the GPU hot path (1,2 SSOR, 3 DIAG, 10 ILU(0) are)";
      return FX_ERROR_INCONS_PC;
  }
  const bool symbolic = (kind != c->precond_kind) ||
                        (kind == 1 && (c->ssor.ncolor == 0 || c->ssor_ncolor_in != ncolor_in || c->ssor_mode_built != c->ssor_mode)) ||
                        ((kind == 10 || kind == 11) && c->ssor.ncolor == 0);
  if (symbolic) { free_precond(c); c->precond_kind = kind; }
  if (kind == 3) {
    if (c->ord.kind > 0 && set_ordering(c, 0, nullptr)) return FX_ERROR_RUNTIME;  // block-Jacobi: natural numbering
    if (ensure_solver(c)) return FX_ERROR_RUNTIME;
    if (diag_setup(c, sigma_diag)) return FX_ERROR_RUNTIME;
  } else if (kind == 10 || kind == 11) {
    if (symbolic && ilu_setup_symbolic(c)) return FX_ERROR_RUNTIME;
    if (ensure_solver(c)) return FX_ERROR_RUNTIME;
    if (ilu_setup_numeric(c, sigma_diag, kind == 10)) return FX_ERROR_RUNTIME;
  } else {
    PhaseTimer pt("precond setup");
    if (symbolic) {
      c->ssor_ncolor_in = ncolor_in;
      if (ssor_setup_symbolic(c, ncolor_in)) return FX_ERROR_RUNTIME;
    }
    pt.lap("symbolic");
    if (ensure_solver(c)) return FX_ERROR_RUNTIME;
    pt.lap("solver layout values");
    if (ssor_setup_numeric(c, sigma_diag)) return FX_ERROR_RUNTIME;
    if (pt.on) HIP_TRY(hipStreamSynchronize(c->stream));
    pt.lap("numeric");
    c->precond_valid_sweeps = true;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->precond_valid = true;
  return 0;
}

// Where the BELL value arrays of this context live (DevArena, fx_internal.h): out[0] bytes of the arena (0: none -- small system,
// FX_ARENA_GB=0, or no memory to spare), [1] bytes in use, [2] arrays placed in it, [3..5] 1 if the value array of M / L / U lies in
// it, [6] bytes of M's value array, [7] arenas the one-off verification timed, [8] the loop's SpMV ms on the arena kept (arena_verify).
extern "C" int fx_placement_report(fx_context *c, double out[9]) {
  if (!c || !out) { g_fx_error = "fx_placement_report: null argument"; return FX_ERROR_RUNTIME; }
  for (int k = 0; k < 9; k++) out[k] = 0.0;
  out[0] = (double)c->arena.bytes; out[1] = (double)c->arena.used(); out[2] = c->arena.live();
  out[3] = c->M.arena_owner ? 1 : 0; out[4] = c->ssor.L.arena_owner ? 1 : 0; out[5] = c->ssor.U.arena_owner ? 1 : 0;
  out[6] = (double)c->M.npairs * 576 * 8;
  out[7] = (double)c->arena_ms.size();                                  // arenas the verification timed (0: not verified -- small system, no arena, FX_ARENA_TRIES=1)
  out[8] = c->arena_ms.empty() ? 0.0 : *std::min_element(c->arena_ms.begin(), c->arena_ms.end());  // SpMV ms on the arena kept
  return 0;
}

// The plane march of this context's level-scheduled preconditioner (fx_march.h): out[0] 1 if the programs are built, [1] rows per
// chunk, [2] chunks, [3] pair waves per workgroup, [4] / [5] rounds of the forward / backward program, [6] blocks gathered from
// the LDS ring, [7] from memory, [8] of those from the row's own chunk, [9] / [10] the cost model's microseconds per half sweep as a
// march / as dependency levels, [11] seconds the build took, [12] applies that took the march, [13] workgroups of the last launch,
// [14] largest round (rows), [15] dependency levels.
extern "C" int fx_march_report(fx_context *c, double out[16]) {
  if (!c || !out) { g_fx_error = "fx_march_report: null argument"; return FX_ERROR_RUNTIME; }
  const MarchDev &M = c->ssor.march;
  for (int k = 0; k < 16; k++) out[k] = 0.0;
  out[0] = M.ok ? 1 : 0; out[1] = M.S; out[2] = M.nchunks; out[3] = M.NW;
  out[4] = (double)M.F.nrounds; out[5] = (double)M.B.nrounds;
  out[6] = (double)M.near_blocks; out[7] = (double)M.far_blocks; out[8] = M.far_same_chunk;
  out[9] = M.est_us; out[10] = M.est_level_us; out[11] = M.build_s;
  out[12] = c->march_launches; out[13] = c->df_grid_last; out[14] = M.max_round_rows; out[15] = c->ssor.ncolor;
  return 0;
}

// z = M^-1 r  (hecmw_precond_apply hecmw_precond.f90:75-123 with iterPREmax = 1; the
// ZP/Z prologue is folded into the kernels).  want_dot: leave partials of r.z.
// Returns the number of partials written (0 if none).
static int precond_apply_once(fx_context *c, const double *r, double *z, bool want_dot, int *nparts) {
  const int32_t N = c->ord.nslots;
  *nparts = 0;
  if (c->precond_kind == 3) {
    const int g = (N + FX_BLOCK - 1) / FX_BLOCK;
    hipLaunchKernelGGL(k_diag_apply, dim3(g), dim3(FX_BLOCK), 0, c->stream, N, c->diag.alu, r, z,
                       want_dot ? c->partials : (double *)nullptr, gate_status(c));
    if (want_dot) *nparts = g;
  } else if (c->precond_kind == 1 || level_sched(c)) {
    SsorDev &S = c->ssor;
    if (want_dot) {  // fused r.z partials need one slot per backward block; fall back to a separate dot otherwise
      int64_t tot = 0;
      for (int col = 0; col < S.ncolor; col++) {
        const int nsl = S.color_slice[col + 1] - S.color_slice[col];
        tot += (nsl <= c->split_max_slices) ? nsl : nsl / ((c->ssor_bs / 64) * c->ssor_spw) + 1;
      }
      if (tot > c->max_partials) want_dot = false;
    }
    const bool full = (c->ord.kind == 1);  // Krylov vectors already colour-major: sweep in place on z
    const int32_t *sn = full ? (const int32_t *)nullptr : S.slot_node;
    double *zsweep = full ? z : S.zs, *znat = full ? (double *)nullptr : z;
    if (level_sched(c) && c->df_mode >= 1 && S.march.ok && !full && (c->march_mode == 2 || (c->march_mode == 1 && c->df_wps == 8))) {  // its sums are those of 8 waves per slice
      // plane march: chunks of rows per workgroup, in-chunk dependencies through LDS (fx_march.h); r.z by a separate dot
      if (march_apply(c, r, z, gate_status(c))) return FX_ERROR_RUNTIME;
      *nparts = 0;
      return 0;
    }
    if ((level_sched(c) && c->df_mode >= 1) || (c->precond_kind == 1 && c->df_mode >= 2)) {
      // one persistent launch: forward values in S.zs, backward values in z itself (colour-major Krylov vectors) or in
      // S.zb (+ z in the caller's numbering); both start as the sentinel pattern (0xFF bytes)
      const int32_t nsl = S.L.nslices;
      const size_t vbytes = (size_t)3 * S.nslots * 8;
      if (!full && !S.zb) { g_fx_error = "dataflow sweep: backward vector not allocated"; return FX_ERROR_RUNTIME; }  // set-up allocates it (no hipMalloc here: the iteration may be inside a graph capture)
      double *zbk = full ? z : S.zb;
      if (want_dot && nsl > c->max_partials) want_dot = false;
      hipLaunchKernelGGL(k_df_fill, dim3(grid_for((int64_t)(vbytes / 16), 256, 2048)), dim3(256), 0, c->stream, (int64_t)(vbytes / 16),
                         (fx_u4 *)S.zs, (fx_u4 *)zbk);  // 3 * 64 * 8 bytes per slice: a multiple of 16
      // every workgroup of the launch must be resident at once (the progress argument of k_tri_dataflow): the default is one per
      // CU; FX_DF_GRID is clamped to what the occupancy query admits per CU (df_grid_max, fx_create)
      int grid = c->df_grid > 0 ? std::min(c->df_grid, c->df_grid_max[c->df_wps == 2 ? 0 : (c->df_wps == 8 ? 2 : 1)]) : std::min(c->n_cu, c->df_grid_max[c->df_wps == 2 ? 0 : (c->df_wps == 8 ? 2 : 1)]);
      grid = std::max(1, std::min(grid, (int)nsl));
      c->df_grid_last = grid;
      double *part = want_dot ? c->partials : (double *)nullptr;
#define DF_LAUNCH3(W, P, SOA)                                                                                                       \
  hipLaunchKernelGGL((k_tri_dataflow<W, P, SOA>), dim3(grid), dim3(64 * W), 0, c->stream, nsl, S.L.pair_ptr, S.L.val2, S.L.col2, \
                     S.U.pair_ptr, S.U.val2, S.U.col2, sn, S.alu, r, S.zs, zbk, znat, part, gate_status(c), c->df_err, c->dbg_df_fail ? -1 : c->df_sleep, \
                     level_sched(c) ? S.slice_level : (const int32_t *)nullptr, c->df_presleep)
#define DF_LAUNCH2(W, P)                                    \
  do {                                                      \
    if (!full && c->df_soa) DF_LAUNCH3(W, P, true);         \
    else DF_LAUNCH3(W, P, false);                           \
  } while (0)
#define DF_LAUNCH(W)                    \
  do {                                  \
    if (c->df_poll == 0) DF_LAUNCH2(W, 0); \
    else DF_LAUNCH2(W, 1);              \
  } while (0)
      if (c->df_wps == 2) DF_LAUNCH(2);
      else if (c->df_wps == 8) DF_LAUNCH(8);
      else DF_LAUNCH(4);
#undef DF_LAUNCH3
#undef DF_LAUNCH
#undef DF_LAUNCH2
      HIP_TRY(hipGetLastError());
      *nparts = want_dot ? nsl : 0;
      return 0;
    }
    // Workgroup size per colour: 64-thread groups (one slice each) spread a colour evenly over the 256 CUs
    // (a 150^3 colour has 5276 slices = 5.2 four-slice groups per CU: a 6-vs-5 imbalance); FX_SSOR_BS overrides.
    const int bs = c->ssor_bs;
    const int spb = (bs / 64) * c->ssor_spw;  // slices per workgroup
#define SSOR_LAUNCH(FWD, B, g, s0, s1, part)                                                                          \
  do {                                                                                                                \
    if (c->pipe_ssor && (s1 - s0) <= c->pipe_max_slices)                                                              \
      hipLaunchKernelGGL((k_ssor_color<FWD, true, B>), dim3(g), dim3(B), 0, c->stream, s0, s1, BL.pair_ptr, BL.val2,  \
                         BL.col2, sn, S.alu, r, zsweep, znat, part, gate_status(c), c->ssor_spw);                     \
    else                                                                                                              \
      hipLaunchKernelGGL((k_ssor_color<FWD, false, B>), dim3(g), dim3(B), 0, c->stream, s0, s1, BL.pair_ptr, BL.val2, \
                         BL.col2, sn, S.alu, r, zsweep, znat, part, gate_status(c), c->ssor_spw);                     \
  } while (0)
#define SPLIT_LAUNCH(FWD, s0, s1, part)                                                                                  \
  do {                                                                                                                  \
    const int wps = c->split_wps ? c->split_wps : (level_sched(c) ? 8 : 4);                                              \
    if (wps == 2)                                                                                                       \
      hipLaunchKernelGGL((k_ssor_color_split<FWD, 2>), dim3(s1 - s0), dim3(128), 0, c->stream, s0, s1, BL.pair_ptr, BL.val2, \
                         BL.col2, sn, S.alu, r, zsweep, znat, part, gate_status(c));                                    \
    else if (wps == 8)                                                                                                  \
      hipLaunchKernelGGL((k_ssor_color_split<FWD, 8>), dim3(s1 - s0), dim3(512), 0, c->stream, s0, s1, BL.pair_ptr, BL.val2, \
                         BL.col2, sn, S.alu, r, zsweep, znat, part, gate_status(c));                                    \
    else                                                                                                                \
      hipLaunchKernelGGL((k_ssor_color_split<FWD, 4>), dim3(s1 - s0), dim3(256), 0, c->stream, s0, s1, BL.pair_ptr, BL.val2, \
                         BL.col2, sn, S.alu, r, zsweep, znat, part, gate_status(c));                                    \
  } while (0)
    if (c->dbg_onecolor) {  // MEASUREMENT ONLY (wrong numbers): both half sweeps as ONE launch each, dependencies ignored -- what the sweeps would cost without 2 x ncolor dependent launches
      const int s0 = 0, s1 = S.L.nslices, g = (s1 - s0 + spb - 1) / spb;
      { const Bell &BL = S.L; if (bs == 64) SSOR_LAUNCH(true, 64, g, s0, s1, (double *)nullptr); else SSOR_LAUNCH(true, 256, g, s0, s1, (double *)nullptr); }
      { const Bell &BL = S.U; if (bs == 64) SSOR_LAUNCH(false, 64, g, s0, s1, (double *)nullptr); else SSOR_LAUNCH(false, 256, g, s0, s1, (double *)nullptr); }
      *nparts = 0;
      HIP_TRY(hipGetLastError());
      return 0;
    }
    for (int col = 0; col < S.ncolor; col++) {
      const int s0 = S.color_slice[col], s1 = S.color_slice[col + 1];
      if (s1 <= s0) continue;
      const Bell &BL = S.L;
      if (s1 - s0 <= c->split_max_slices) { SPLIT_LAUNCH(true, s0, s1, (double *)nullptr); continue; }
      const int g = (s1 - s0 + spb - 1) / spb;
      if (bs == 64) SSOR_LAUNCH(true, 64, g, s0, s1, (double *)nullptr);
      else SSOR_LAUNCH(true, 256, g, s0, s1, (double *)nullptr);
    }
    int off = 0;
    for (int col = S.ncolor - 1; col >= 0; col--) {
      const int s0 = S.color_slice[col], s1 = S.color_slice[col + 1];
      if (s1 <= s0) continue;
      const Bell &BL = S.U;
      double *part = want_dot ? c->partials + off : (double *)nullptr;
      if (s1 - s0 <= c->split_max_slices) {
        SPLIT_LAUNCH(false, s0, s1, part);
        if (want_dot) off += s1 - s0;
        continue;
      }
      const int g = (s1 - s0 + spb - 1) / spb;
      if (bs == 64) SSOR_LAUNCH(false, 64, g, s0, s1, part);
      else SSOR_LAUNCH(false, 256, g, s0, s1, part);
      if (want_dot) off += g;
    }
#undef SSOR_LAUNCH
#undef SPLIT_LAUNCH
    *nparts = off;
  } else {  // iterPREmax <= 0: Z = R (hecmw_precond.f90:89-94)
    hipLaunchKernelGGL(k_copy, dim3(grid_for(3 * (int64_t)N)), dim3(256), 0, c->stream, (int64_t)3 * N, r, z);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

static int spmv(fx_context *c, int mode, int dot, double *x, const double *b, double *y, const int32_t *gate, int32_t gate_val);

// hecmw_precond_33_apply (33/hecmw_precond_33.f90:74-115): iterPREmax additive-Schwarz sweeps,
//   Z = 0; ZP = R; repeat { ZP <- M^-1 ZP; Z += ZP; ZP = R - A Z }.
// The common iterPREmax = 1 case is the single fused sweep.
static int precond_apply(fx_context *c, const double *r, double *z, bool want_dot, int *nparts) {
  ClockScope cs(c, 1);
  if (c->iterpremax <= 1 || c->precond_kind == 0) return precond_apply_once(c, r, z, want_dot, nparts);
  *nparts = 0;  // r.z is taken by a separate dot afterwards
  int np;
  double *zp = c->W[8], *dz = c->W[9];
  const int64_t n3 = (int64_t)3 * c->ord.nslots;
  if (precond_apply_once(c, r, z, false, &np)) return FX_ERROR_RUNTIME;
  for (int it = 2; it <= c->iterpremax; it++) {
    if (spmv(c, 1, 0, z, r, zp, gate_status(c), 0)) return FX_ERROR_RUNTIME;  // ZP = R - A Z (halo update of Z inside)
    if (precond_apply_once(c, zp, dz, false, &np)) return FX_ERROR_RUNTIME;
    hipLaunchKernelGGL(k_axpy_plain, dim3(grid_for(n3)), dim3(256), 0, c->stream, n3, 1.0, dz, z);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

static int dot_into_partials(fx_context *c, const double *x, const double *y, const int32_t *gate, int32_t gate_val,
                             int *nparts) {
  const int64_t n = (int64_t)3 * c->ord.nslots;  // internal slots (padding entries are zero); the halo tail is excluded
  const int g = grid_for(n, FX_BLOCK, 2048);
  hipLaunchKernelGGL(k_dot, dim3(g), dim3(FX_BLOCK), 0, c->stream, n, x, y, c->partials, gate, gate_val);
  HIP_TRY(hipGetLastError());
  *nparts = g;
  return 0;
}

// ---------------------------------------------------------------------------
// Krylov drivers.  Device-resident state machine; the host enqueues whole
// iterations and only polls the status word every `chunk` iterations.
// ---------------------------------------------------------------------------
static int krylov_init_state(fx_context *c, int maxit, double tol, bool pause_verify = false) {
  KrylovState s;
  memset(&s, 0, sizeof s);
  s.iter = 1;
  s.pause_verify = pause_verify ? 1 : 0;
  s.maxit = maxit;
  s.tol = tol;
  HIP_TRY(hipMemcpyAsync(c->st, &s, sizeof s, hipMemcpyHostToDevice, c->stream));
  if (c->hist_cap < maxit + 1) {
    dev_free(c->hist);
    if (dev_alloc(&c->hist, (size_t)maxit + 1)) return FX_ERROR_RUNTIME;
    c->hist_cap = maxit + 1;
  }
  return 0;
}

// A dataflow sweep whose bounded wait ran out (its workgroups were not all resident -- a device shared with other contexts or
// processes -- or a producer failed) raises the device word df_err and drains without waiting: what it wrote is unusable.  The
// context then leaves the dataflow sweeps for good (df_mode = 0: one launch per colour / level, no residency assumption) and the
// caller redoes its work.  Called after every host-visible synchronisation of a path that ran precond_apply.
static bool df_take_error(fx_context *c) {
  if (!level_sched(c) && c->precond_kind != 1) return false;
  int32_t e = 0;
  if (hipMemcpy(&e, c->df_err, 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
  if (e == 0) return false;
  (void)hipMemset(c->df_err, 0, 4);
  c->df_mode = 0;
  c->df_fallbacks++;
  // the sweep vector is full of tags: the level sweeps multiply a padding block (value 0) with the row's own stale entry
  if (c->ssor.zs) (void)hipMemset(c->ssor.zs, 0, (size_t)3 * c->ssor.nslots * 8);
  return true;
}

static int poll_state(fx_context *c, KrylovState *out) {
  int32_t *herr = (int32_t *)(c->st_host + 3);  // pinned
  HIP_TRY(hipMemcpyAsync(c->st_host, c->st, sizeof(KrylovState), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(herr, c->df_err, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *out = *c->st_host;
  if (c->clock.on) clock_collect(c);
  if (*herr != 0) {
    (void)hipMemset(c->df_err, 0, 4);
    c->df_mode = 0;  // from now on: one launch per colour / level
    c->df_fallbacks++;
    g_fx_error = "dataflow sweep: a bounded wait ran out (workgroups not co-resident, or a producer failed); the context now uses the launch-per-level sweeps";
    return FX_DF_RETRY;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Eisenstat's form of CG + multicolour SSOR (the default where it is exact, fx_context::eisenstat; kernels and recurrences: fx_kernels.h).
// Vectors: R W[0], P W[1], PH W[2] (= (D~+U) p), T W[3] (= (D~+L)^-1 r), DT W[4] (= D~ t), V W[5], WH W[6] (= (D~+L)^-1 A p), Q W[7].
// Partial sums: ||r||^2 and ph.w in region 0 of c->partials, rho = t.dt in region 1 (it is consumed one scalar stage later).
// ---------------------------------------------------------------------------
static int eis_sweep_backward(fx_context *c, const double *rhs, double *out, const int32_t *gate) {  // out = (D~+U)^-1 rhs
  ClockScope cs(c, 1);  // TIMELOG: the triangular solves count as solver/precond, the pass that delivers q = A p as solver/matvec
  SsorDev &S = c->ssor;
  const int spb = c->ssor_bs / 64;
  for (int col = S.ncolor - 1; col >= 0; col--) {
    const int s0 = S.color_slice[col], s1 = S.color_slice[col + 1];
    if (s1 <= s0) continue;
    if (s1 - s0 <= c->split_max_slices)
      hipLaunchKernelGGL((k_ssor_color_split<true, 4>), dim3(s1 - s0), dim3(256), 0, c->stream, s0, s1, S.U.pair_ptr, S.U.val2, S.U.col2,
                         (const int32_t *)nullptr, S.alu, rhs, out, (double *)nullptr, (double *)nullptr, gate);
    else if (c->ssor_bs == 64)
      hipLaunchKernelGGL((k_ssor_color<true, true, 64>), dim3((s1 - s0 + spb - 1) / spb), dim3(64), 0, c->stream, s0, s1, S.U.pair_ptr,
                         S.U.val2, S.U.col2, (const int32_t *)nullptr, S.alu, rhs, out, (double *)nullptr, (double *)nullptr, gate, 1);
    else
      hipLaunchKernelGGL((k_ssor_color<true, true, 256>), dim3((s1 - s0 + spb - 1) / spb), dim3(256), 0, c->stream, s0, s1, S.U.pair_ptr,
                         S.U.val2, S.U.col2, (const int32_t *)nullptr, S.alu, rhs, out, (double *)nullptr, (double *)nullptr, gate, 1);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
static int eis_sweep_forward_solve(fx_context *c, const double *rhs, double *out, const int32_t *gate) {  // out = (D~+L)^-1 rhs
  ClockScope cs(c, 1);
  SsorDev &S = c->ssor;
  const int spb = c->ssor_bs / 64;
  for (int col = 0; col < S.ncolor; col++) {
    const int s0 = S.color_slice[col], s1 = S.color_slice[col + 1];
    if (s1 <= s0) continue;
    if (s1 - s0 <= c->split_max_slices)
      hipLaunchKernelGGL((k_ssor_color_split<true, 4>), dim3(s1 - s0), dim3(256), 0, c->stream, s0, s1, S.L.pair_ptr, S.L.val2, S.L.col2,
                         (const int32_t *)nullptr, S.alu, rhs, out, (double *)nullptr, (double *)nullptr, gate);
    else if (c->ssor_bs == 64)
      hipLaunchKernelGGL((k_ssor_color<true, true, 64>), dim3((s1 - s0 + spb - 1) / spb), dim3(64), 0, c->stream, s0, s1, S.L.pair_ptr,
                         S.L.val2, S.L.col2, (const int32_t *)nullptr, S.alu, rhs, out, (double *)nullptr, (double *)nullptr, gate, 1);
    else
      hipLaunchKernelGGL((k_ssor_color<true, true, 256>), dim3((s1 - s0 + spb - 1) / spb), dim3(256), 0, c->stream, s0, s1, S.L.pair_ptr,
                         S.L.val2, S.L.col2, (const int32_t *)nullptr, S.alu, rhs, out, (double *)nullptr, (double *)nullptr, gate, 1);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
// t = (D~+L)^-1 r, dt = D~ t, partials of rho = t.dt -> region 1
static int eis_refresh_t(fx_context *c, const int32_t *gate) {
  SsorDev &S = c->ssor;
  const int32_t ns = c->ord.nslots;
  if (eis_sweep_forward_solve(c, c->W[0], c->W[3], gate)) return FX_ERROR_RUNTIME;
  hipLaunchKernelGGL((k_eis_update<0>), dim3((ns + FX_BLOCK - 1) / FX_BLOCK), dim3(FX_BLOCK), 0, c->stream, ns, c->st, S.alu,
                     (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (double *)nullptr,
                     (double *)nullptr, c->W[3], c->W[4], c->partials, c->partials + c->max_partials, gate);
  HIP_TRY(hipGetLastError());
  return 0;
}
static int eis_begin(fx_context *c) {  // after the standard begin (r0 = b - A x0 in W[0], ||b||^2)
  c->eis_rho_done = false;
  for (int k : {1, 2, 5, 6, 7}) HIP_TRY(hipMemsetAsync(c->W[k], 0, (size_t)c->wlen * 8, c->stream));
  HIP_TRY(hipMemsetAsync(c->W[3], 0, (size_t)c->wlen * 8, c->stream));
  return eis_refresh_t(c, nullptr);
}
// The latency-bound tail of the fused Eisenstat sweeps (k_eis_*_df): the longest run of colours at the
// end of the colour order with at most EIS_TAIL_GRIDS x G slices each, G the co-resident grid of the dataflow kernels.  Only where it
// is exact and safe: FX_DATAFLOW >= 1, one rank (a one-rank retry inside a collective solve is not safe), the fused backward sweep,
// one workgroup per slice (eis_grid 0: the partial of every slice sits where OP_CG_C1 expects it), every tail colour a split launch.
// Returns the first tail colour (ncolor: no tail) and the grids of the backward and forward tail launches.
static int eis_tail(fx_context *c, int *grid) {
  const SsorDev &S = c->ssor;
  grid[0] = grid[1] = 0;
  if (c->df_mode < 1 || multi_rank(c) || c->nranks > 1 || halo_active(c) || !c->eis_fuse || c->eis_grid > 0 || S.ncolor <= 0)
    return S.ncolor;
  int gk[2];
  for (int k = 0; k < 2; k++) gk[k] = c->df_grid > 0 ? std::min(c->df_grid, c->eis_df_grid_max[k]) : c->eis_df_grid_max[k];
  const int g = std::min(gk[0], gk[1]);
  int c0 = S.ncolor;
  while (c0 > 0) {
    const int nsl = S.color_slice[c0] - S.color_slice[c0 - 1];
    if (nsl > EIS_TAIL_GRIDS * g || nsl > c->split_max_slices) break;
    c0--;
  }
  const int nt = S.color_slice[S.ncolor] - S.color_slice[c0];
  if (nt <= 0) return S.ncolor;
  for (int k = 0; k < 2; k++) grid[k] = std::min(gk[k], nt);
  return c0;
}

static int eis_cg_iteration(fx_context *c, int it) {
  SsorDev &S = c->ssor;
  const int32_t ns = c->ord.nslots;
  const int64_t n3 = (int64_t)3 * ns;
  double *R = c->W[0], *P = c->W[1], *PH = c->W[2], *T = c->W[3], *DT = c->W[4], *V = c->W[5], *WH = c->W[6], *Q = c->W[7];
  double *X = c->Xs, *B = c->Bs;
  const int RECOMPUTE = 50, vgrid = grid_for(n3, FX_BLOCK, 2048), ugrid = (ns + FX_BLOCK - 1) / FX_BLOCK;
  const double esc = (S.sigma_diag - 1.0) / S.sigma_diag;  // (D~ - D) = esc * diag(D~)
  double *part_rho = c->partials + c->max_partials;
  // rho = r.M^-1 r = t.D~t (:168), beta (:193); ph = D~ t + beta ph  [= (D~+U)(z + beta p)]
  // (already done by the previous iteration's OP_RESID_RHO stage unless t was refreshed since)
  if (!c->eis_rho_done && scalar_stage<OP_CG_RHO>(c, ugrid, 0, RECOMPUTE, part_rho)) return FX_ERROR_RUNTIME;
  c->eis_rho_done = false;
  int tgrid[2];
  const int tc0 = eis_tail(c, tgrid);  // colours [tc0, ncolor): one dataflow launch per half sweep
  const int ts0 = S.color_slice[tc0], ts1 = S.color_slice[S.ncolor];
  c->eis_tail_color0 = tc0; c->eis_tail_slices = ts1 - ts0; c->eis_tail_grid = tgrid[0];
  if (tc0 < S.ncolor) {  // tags into the tail ranges of p and v (nothing reads them before the sweeps that produce them)
    const int64_t n16 = (int64_t)(ts1 - ts0) * 64 * 3 * 8 / 16;
    hipLaunchKernelGGL(k_eis_tag, dim3(grid_for(n16, 256, 2048)), dim3(256), 0, c->stream, n16, (fx_u4 *)(P + (size_t)3 * 64 * ts0),
                       (fx_u4 *)(V + (size_t)3 * 64 * ts0), gate_status(c));
  }
  if (c->eis_fuse) {  // p = (D~+U)^-1 ph with ph = D~ t + beta ph formed by each row's own lane on the way (k_eis_backward)
    ClockScope cs(c, 1);
    const int spb = c->ssor_bs / 64;
    if (tc0 < S.ncolor) {
      hipLaunchKernelGGL((k_eis_backward_df<4>), dim3(tgrid[0]), dim3(256), 0, c->stream, ts0, ts1, S.U.pair_ptr, S.U.val2, S.U.col2, S.alu,
                         c->st, DT, PH, P, gate_status(c), c->df_err, c->dbg_df_fail ? 1 : 0);
      c->eis_tail_launches++;
    }
    for (int col = tc0 - 1; col >= 0; col--) {
      const int s0 = S.color_slice[col], s1 = S.color_slice[col + 1];
      if (s1 <= s0) continue;
      if (s1 - s0 <= c->split_max_slices)
        hipLaunchKernelGGL((k_eis_backward_split<4>), dim3(c->eis_grid > 0 ? std::min(s1 - s0, c->eis_grid) : s1 - s0), dim3(256), 0, c->stream, s0, s1, S.U.pair_ptr, S.U.val2, S.U.col2, S.alu,
                           c->st, DT, PH, P, gate_status(c));
      else if (c->ssor_bs == 64)
        hipLaunchKernelGGL((k_eis_backward<64>), dim3((s1 - s0 + spb - 1) / spb), dim3(64), 0, c->stream, s0, s1, S.U.pair_ptr, S.U.val2,
                           S.U.col2, S.alu, c->st, DT, PH, P, gate_status(c));
      else
        hipLaunchKernelGGL((k_eis_backward<256>), dim3((s1 - s0 + spb - 1) / spb), dim3(256), 0, c->stream, s0, s1, S.U.pair_ptr, S.U.val2,
                           S.U.col2, S.alu, c->st, DT, PH, P, gate_status(c));
    }
  } else {
    hipLaunchKernelGGL(k_cg_update_p, dim3(vgrid), dim3(FX_BLOCK), 0, c->stream, n3, c->st, DT, PH);
    // p = (D~+U)^-1 ph
    if (eis_sweep_backward(c, PH, P, gate_status(c))) return FX_ERROR_RUNTIME;
  }
  const double *HP = nullptr;
  if (halo_active(c)) {  // subdomain: halo part of p from its owners, then hp = H p (W[8])
    if (halo_update(c, P)) return FX_ERROR_RUNTIME;
    ClockScope cs(c, 0);
    hipLaunchKernelGGL(k_eis_halo, dim3((S.H.nslices + 3) / 4), dim3(256), 0, c->stream, S.H.nslices, S.H.pair_ptr, S.H.val2, S.H.col2, P,
                       c->W[8], gate_status(c));
    HP = c->W[8];
  }
  // one pass over L: v, w = (D~+L)^-1 A p, q = A p, partial of p.q = ph.w (:204-211)
  {
    ClockScope cs(c, 0);
    const int spb = c->ssor_bs / 64;
    int off = 0;
    for (int col = 0; col < tc0; col++) {
      const int s0 = S.color_slice[col], s1 = S.color_slice[col + 1];
      if (s1 <= s0) continue;
      int g = (s1 - s0 + spb - 1) / spb;
      if (s1 - s0 <= c->split_max_slices) {
        g = c->eis_grid > 0 ? std::min(s1 - s0, c->eis_grid) : s1 - s0;
        hipLaunchKernelGGL((k_eis_forward_split<4>), dim3(g), dim3(256), 0, c->stream, s0, s1, S.L.pair_ptr, S.L.val2, S.L.col2, S.alu,
                           esc, PH, P, V, WH, Q, c->partials, off, gate_status(c), HP);
      } else if (c->ssor_bs == 64)
        hipLaunchKernelGGL((k_eis_forward<64>), dim3(g), dim3(64), 0, c->stream, s0, s1, S.L.pair_ptr, S.L.val2, S.L.col2, S.alu,
                           esc, PH, P, V, WH, Q, c->partials, off, gate_status(c), HP);
      else
        hipLaunchKernelGGL((k_eis_forward<256>), dim3(g), dim3(256), 0, c->stream, s0, s1, S.L.pair_ptr, S.L.val2, S.L.col2, S.alu,
                           esc, PH, P, V, WH, Q, c->partials, off, gate_status(c), HP);
      off += g;
    }
    if (tc0 < S.ncolor) {  // the tail: one partial per slice, where the launch per colour puts it
      hipLaunchKernelGGL((k_eis_forward_df<4>), dim3(tgrid[1]), dim3(256), 0, c->stream, ts0, ts1, S.L.pair_ptr, S.L.val2, S.L.col2, S.alu,
                         esc, PH, P, V, WH, Q, c->partials, off, gate_status(c), c->df_err, c->dbg_df_fail ? 1 : 0);
      c->eis_tail_launches++;
      off += ts1 - ts0;
    }
    HIP_TRY(hipGetLastError());
    if (off > c->max_partials) { g_fx_error = "eisenstat: partial-sum buffer too small"; return FX_ERROR_RUNTIME; }
    if (scalar_stage<OP_CG_C1>(c, off, 0, RECOMPUTE)) return FX_ERROR_RUNTIME;
  }
  int np;
  if (it % RECOMPUTE == 0) {  // x += alpha p ; r = b - A x (:232-233) ; t, dt, rho from the new r
    hipLaunchKernelGGL((k_eis_update<2>), dim3(ugrid), dim3(FX_BLOCK), 0, c->stream, ns, c->st, S.alu, P, Q, WH, X, R, T, DT,
                       c->partials, part_rho, gate_status(c));
    if (spmv(c, 1, 2, X, B, R, gate_status(c), 0)) return FX_ERROR_RUNTIME;
    np = spmv_nparts(c);
    if (scalar_stage<OP_RESID>(c, np, 0, RECOMPUTE)) return FX_ERROR_RUNTIME;
    if (eis_refresh_t(c, gate_status(c))) return FX_ERROR_RUNTIME;  // overwrites region 0 after OP_RESID has consumed it
  } else {
    hipLaunchKernelGGL((k_eis_update<1>), dim3(ugrid), dim3(FX_BLOCK), 0, c->stream, ns, c->st, S.alu, P, Q, WH, X, R, T, DT,
                       c->partials, part_rho, gate_status(c));
    // converged by the recurrence: the loop parks, verify_stage() follows from the host.  ||r||^2 (region 0) and the next iteration's
    // rho = t.D~t (region 1, max_partials further) left k_eis_update together: one stage, one 2-double all-reduce
    if (c->eis_merge) {
      if (scalar_stage<OP_RESID_RHO>(c, ugrid, c->max_partials, RECOMPUTE)) return FX_ERROR_RUNTIME;
      c->eis_rho_done = true;
    } else if (scalar_stage<OP_RESID>(c, ugrid, 0, RECOMPUTE)) return FX_ERROR_RUNTIME;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// hecmw_solve_CG (hecmw_solver_CG.f90:19-312) / hecmw_solve_BiCGSTAB (hecmw_solver_BiCGSTAB.f90:16-297)
// split into begin (r0, ||b||) / steps (n iterations enqueued) / poll, so that callers can
// time an exact number of iterations with nothing else in the bracket.
static int krylov_begin(fx_context *c, int method, int maxit, double tol) {
  const int64_t n3 = (int64_t)3 * c->ord.nslots;
  double *X = c->Xs, *B = c->Bs, *R = c->W[0];
  int np;
  if (ensure_solver(c)) return FX_ERROR_RUNTIME;
  if (to_slots(c, c->A.B, c->Bs) || to_slots(c, c->A.X, c->Xs)) return FX_ERROR_RUNTIME;
  c->k_method = method; c->k_maxit = maxit; c->k_it = 1;
  graphs_destroy(c);  // buffers / grids may have changed since the last solve: re-capture
  // auto: only the sweep-heavy preconditioners (40+ launches per iteration); measured at 98k DOF: CG + SSOR 293 -> 270 us,
  // BiCGSTAB + SSOR 562 -> 517 us per iteration, but CG + block-Jacobi (8 launches) 42.8 -> 45.1 us
  const bool sweepy = (c->precond_kind == 1 || level_sched(c));
  c->k_graph = !c->clock.on && !multi_rank(c) && c->nranks <= 1 && c->halo.n_neighbor <= 0 &&
               (c->graph_mode == 2 || (c->graph_mode == 1 && sweepy && c->ord.nslots <= c->graph_max_rows));
  if (krylov_init_state(c, maxit, tol, true)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemsetAsync(c->W[2], 0, (size_t)c->wlen * 8, c->stream));  // P
  if (c->precond_kind == 1 || level_sched(c))  // padding blocks multiply (value 0) x (the row's own stale entry): keep that entry finite
    HIP_TRY(hipMemsetAsync(c->ssor.zs, 0, (size_t)3 * c->ssor.nslots * 8, c->stream));
  if (method == 2) HIP_TRY(hipMemsetAsync(c->W[6], 0, (size_t)c->wlen * 8, c->stream));  // V
  // r0 = b - A x0 (CG :120 / BiCGSTAB :107) ; ||b||^2 (:123-129 / :115-121)
  if (spmv(c, 1, 0, X, B, R, nullptr, 0)) return FX_ERROR_RUNTIME;
  if (method == 2) {
    hipLaunchKernelGGL(k_copy, dim3(grid_for(n3, FX_BLOCK, 2048)), dim3(256), 0, c->stream, n3, R, c->W[1]);  // r_tld = r0
  }
  if (dot_into_partials(c, B, B, nullptr, 0, &np)) return FX_ERROR_RUNTIME;
  if (scalar_stage<OP_BNRM2>(c, np, 0, 50)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipGetLastError());
  // Eisenstat's form: CG + multicolour SSOR(1) in the colour-major numbering, when asked for (subdomains: with the halo term H p)
  // ... and only while M was built from the very values A holds: a recycled preconditioner (hecmw_mat_recycle_precond_setting keeps
  // the old one for up to three changed matrices) is a different splitting, and the identity A = (D~+L) + (D~+U) + (D - 2D~) is gone
  c->eis_active = c->eisenstat && method == 1 && c->precond_kind == 1 && c->ord.kind == 1 && c->iterpremax == 1 &&
                  c->ssor.values_epoch == c->values_epoch && (!halo_active(c) || c->ssor.H.nslices > 0);
  if (c->eis_active && eis_begin(c)) return FX_ERROR_RUNTIME;  // (graph replay serves this form too: its arguments are as constant over a solve as the standard loop's)
  return 0;
}

static int cg_iteration(fx_context *c, int it) {
  if (c->eis_active) return eis_cg_iteration(c, it);
  const int64_t n3 = (int64_t)3 * c->ord.nslots;
  double *R = c->W[0], *Z = c->W[1], *Q = c->W[1], *P = c->W[2];
  double *X = c->Xs, *B = c->Bs;
  const int RECOMPUTE = 50;
  const int vgrid = grid_for(n3, FX_BLOCK, 2048);
  int np;
  // z = M^-1 r (:160) with the partial of rho = r.z (:168) fused in
  if (precond_apply(c, R, Z, true, &np)) return FX_ERROR_RUNTIME;
  if (np == 0 && dot_into_partials(c, R, Z, gate_status(c), 0, &np)) return FX_ERROR_RUNTIME;
  if (scalar_stage<OP_CG_RHO>(c, np, 0, RECOMPUTE)) return FX_ERROR_RUNTIME;
  // p = z + beta p (:188-197)
  hipLaunchKernelGGL(k_cg_update_p, dim3(vgrid), dim3(FX_BLOCK), 0, c->stream, n3, c->st, Z, P);
  // q = A p (:204) + partial of p.q (:211)
  if (spmv(c, 0, 1, P, nullptr, Q, gate_status(c), 0)) return FX_ERROR_RUNTIME;
  if (scalar_stage<OP_CG_C1>(c, spmv_nparts(c), 0, RECOMPUTE)) return FX_ERROR_RUNTIME;
  // x += alpha p ; r -= alpha q | r = b - A x every 50 iterations (:227-238) ; ||r||^2 (:240)
  if (it % RECOMPUTE == 0) {
    hipLaunchKernelGGL((k_cg_update_xr<false>), dim3(vgrid), dim3(FX_BLOCK), 0, c->stream, n3, c->st, P, Q, X, R, c->partials);
    if (spmv(c, 1, 2, X, B, R, gate_status(c), 0)) return FX_ERROR_RUNTIME;
    np = spmv_nparts(c);
  } else {
    hipLaunchKernelGGL((k_cg_update_xr<true>), dim3(vgrid), dim3(FX_BLOCK), 0, c->stream, n3, c->st, P, Q, X, R, c->partials);
    np = vgrid;
  }
  if (scalar_stage<OP_RESID>(c, np, 0, RECOMPUTE)) return FX_ERROR_RUNTIME;  // converged by the recurrence: the loop parks, verify_stage() follows from the host
  HIP_TRY(hipGetLastError());
  return 0;
}

// Converged by the recurrence (RESID <= TOL): recompute the true residual and re-test (hecmw_solver_CG.f90:259-266,
// hecmw_solver_BiCGSTAB.f90:256-262).  OP_RESID parked the device loop (FX_ST_PAUSED: whatever was enqueued behind it ran as
// no-ops); the host enqueues the check when its poll sees that -- once or twice per solve -- instead of carrying a gated SpMV, a
// gated scalar stage (and, in Eisenstat's form, 21 gated sweep launches) through every iteration.  OP_VERIFY either ends the
// loop or resumes it at the next iteration; in Eisenstat's form r then IS the true residual, so t is refreshed from it.
static int verify_stage(fx_context *c) {
  const int RECOMPUTE = (c->k_method == 1) ? 50 : 100;
  if (spmv(c, 1, 2, c->Xs, c->Bs, c->W[0], gate_verify(c), 1)) return FX_ERROR_RUNTIME;
  if (scalar_stage<OP_VERIFY>(c, spmv_nparts(c), 0, RECOMPUTE)) return FX_ERROR_RUNTIME;
  if (c->eis_active && eis_refresh_t(c, &c->st->t_current)) return FX_ERROR_RUNTIME;  // runs only if the loop goes on (t_current == 0)
  c->eis_rho_done = false;  // ... and then leaves new rho partials: the next iteration reduces them itself
  return 0;
}

static int bicgstab_iteration(fx_context *c, int it) {
  const int64_t n3 = (int64_t)3 * c->ord.nslots;
  // R=1 RT=2 P=3 PT=4 S=5 ST=1 T=6 V=7 (:45-53); ST aliases R as in the reference
  double *R = c->W[0], *RT = c->W[1], *P = c->W[2], *PT = c->W[3], *S = c->W[4], *ST = c->W[0], *T = c->W[5], *V = c->W[6];
  double *X = c->Xs, *B = c->Bs;
  const int RECOMPUTE = 100;
  const int vgrid = grid_for(n3, FX_BLOCK, 2048);
  int np;
  if (dot_into_partials(c, R, RT, gate_status(c), 0, &np)) return FX_ERROR_RUNTIME;           // :152
  if (scalar_stage<OP_BI_RHO>(c, np, 0, RECOMPUTE)) return FX_ERROR_RUNTIME;
  hipLaunchKernelGGL(k_bi_update_p, dim3(vgrid), dim3(FX_BLOCK), 0, c->stream, n3, c->st, R, V, P);  // :160-170
  if (precond_apply(c, P, PT, false, &np)) return FX_ERROR_RUNTIME;                            // :177
  if (spmv(c, 0, 0, PT, nullptr, V, gate_status(c), 0)) return FX_ERROR_RUNTIME;               // :184
  if (dot_into_partials(c, RT, V, gate_status(c), 0, &np)) return FX_ERROR_RUNTIME;            // :188
  if (scalar_stage<OP_BI_C2>(c, np, 0, RECOMPUTE)) return FX_ERROR_RUNTIME;
  hipLaunchKernelGGL(k_bi_update_s, dim3(vgrid), dim3(FX_BLOCK), 0, c->stream, n3, c->st, R, V, S);  // :194-196
  if (precond_apply(c, S, ST, false, &np)) return FX_ERROR_RUNTIME;                            // :203
  if (spmv(c, 0, 0, ST, nullptr, T, gate_status(c), 0)) return FX_ERROR_RUNTIME;               // :210
  hipLaunchKernelGGL(k_dot2, dim3(vgrid), dim3(FX_BLOCK), 0, c->stream, n3, T, S, c->partials, c->max_partials,
                     gate_status(c));                                                          // :217-218
  if (scalar_stage<OP_BI_OMEGA>(c, vgrid, c->max_partials, RECOMPUTE)) return FX_ERROR_RUNTIME;
  if (it % RECOMPUTE == 0) {                                                                   // :231-241
    hipLaunchKernelGGL((k_bi_update_xr<false>), dim3(vgrid), dim3(FX_BLOCK), 0, c->stream, n3, c->st, PT, ST, S, T, X, R,
                       c->partials);
    if (spmv(c, 1, 2, X, B, R, gate_status(c), 0)) return FX_ERROR_RUNTIME;
    np = spmv_nparts(c);
  } else {
    hipLaunchKernelGGL((k_bi_update_xr<true>), dim3(vgrid), dim3(FX_BLOCK), 0, c->stream, n3, c->st, PT, ST, S, T, X, R,
                       c->partials);
    np = vgrid;
  }
  if (scalar_stage<OP_RESID>(c, np, 0, RECOMPUTE)) return FX_ERROR_RUNTIME;  // converged by the recurrence: parks, see verify_stage()
  HIP_TRY(hipGetLastError());
  return 0;
}

// Enqueue up to n iterations (never past MAXIT).  The host polls the device status word
// every `chunk` iterations only; once the device has left the RUNNING state the already
// enqueued kernels are no-ops.  *st_out is the state after the last poll.
static void graphs_destroy(fx_context *c) {
  for (auto &g : c->g_iter) {
    if (g) (void)hipGraphExecDestroy(g);
    g = nullptr;
  }
}

// Capture one iteration (the kernels it enqueues on the solver stream) into an executable graph.
static int capture_iteration(fx_context *c, int it, hipGraphExec_t *out) {
  HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  const int e = (c->k_method == 1) ? cg_iteration(c, it) : bicgstab_iteration(c, it);
  hipGraph_t g = nullptr;
  const hipError_t ce = hipStreamEndCapture(c->stream, &g);
  if (e || ce != hipSuccess || !g) {
    if (g) (void)hipGraphDestroy(g);
    if (!e) g_fx_error = std::string("hipStreamEndCapture: ") + hipGetErrorString(ce);
    return FX_ERROR_RUNTIME;
  }
  const hipError_t ie = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ie != hipSuccess) { g_fx_error = std::string("hipGraphInstantiate: ") + hipGetErrorString(ie); return FX_ERROR_RUNTIME; }
  return 0;
}

static int krylov_steps(fx_context *c, int n, KrylovState *st_out) {
  const int chunk = (c->k_method == 1) ? 16 : 8;
  const int recompute = (c->k_method == 1) ? 50 : 100;
  KrylovState s;
  memset(&s, 0, sizeof s);
  const int last = (int)std::min<int64_t>((int64_t)c->k_it + n - 1, c->k_maxit);  // the last iteration this call may execute
  int enq = 0;
  while (c->k_it <= last) {
    const int it = c->k_it;
    int e = 0;
    if (c->k_graph) {
      // what an iteration enqueues depends on two things only: whether it recomputes the true residual, and (Eisenstat's form)
      // whether it starts with its own rho stage; eis_rho_done after it follows from the first alone
      const bool own_rho = c->eis_active && !c->eis_rho_done, recomp = (it % recompute == 0);
      hipGraphExec_t &g = c->g_iter[(recomp ? 1 : 0) | (own_rho ? 2 : 0)];
      if (!g) e = capture_iteration(c, it, &g);  // (the capture runs the host side of the iteration: eis_rho_done is updated by it)
      else if (c->eis_active) c->eis_rho_done = c->eis_merge && !recomp;
      if (!e) HIP_TRY(hipGraphLaunch(g, c->stream));
    } else {
      e = (c->k_method == 1) ? cg_iteration(c, it) : bicgstab_iteration(c, it);
    }
    if (e) return e;
    c->k_it++;
    enq++;
    if (enq % chunk == 0 || it == last) {
      if (int pe = poll_state(c, &s)) return pe;
      if (s.status == FX_ST_PAUSED) {  // RESID <= TOL by the recurrence at iteration s.iter: true-residual check, then go on from there
        if (verify_stage(c)) return FX_ERROR_RUNTIME;
        if (int pe = poll_state(c, &s)) return pe;
        if (s.status == 0) c->k_it = s.iter;  // the iterations enqueued behind the parked one were no-ops
      }
      if (s.status != 0) break;
    }
  }
  if (int pe = poll_state(c, &s)) return pe;
  *st_out = s;
  return 0;
}

extern "C" int fx_krylov_begin(fx_context *c, const int32_t *Iarray, const double *Rarray) {
  HIP_TRY(hipSetDevice(c->device));
  if (require_transport(c, "fx_krylov_begin")) return FX_ERROR_RUNTIME;
  if (!c->have_values || !c->precond_valid) { g_fx_error = "fx_krylov_begin: matrix / preconditioner not resident"; return FX_ERROR_RUNTIME; }
  if (Iarray[1] != 1 && Iarray[1] != 2) { g_fx_error = "METHOD must be 1 (CG) or 2 (BiCGSTAB)"; return FX_ERROR_INCONS_PC; }
  c->iterpremax = Iarray[4];
  c->clock.on = false;  // the staged API is what bench.py times: no event pairs inside
  const int e = krylov_begin(c, Iarray[1], Iarray[0], Rarray[0]);
  if (e) return e;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int fx_krylov_steps(fx_context *c, int32_t nsteps, int32_t *iter, int32_t *status, double *resid) {
  HIP_TRY(hipSetDevice(c->device));
  KrylovState s;
  const int e = krylov_steps(c, nsteps, &s);
  if (e) return FX_ERROR_RUNTIME;  // (a timed-out dataflow sweep included: the staged API has no restart; the context has left that mode)
  if (iter) *iter = s.iter;
  if (status) *status = s.status;
  if (resid) *resid = s.resid;
  return 0;
}

// The ITERLOG channel of the staged loop (hecmw_solver_CG.f90:245, '(i7,1pe16.6)'): RESID of the iterations executed since
// fx_krylov_begin, line i = iteration i.  *n_lines = lines the device has written, at most `cap` of them are copied.
extern "C" int fx_krylov_history(fx_context *c, double *hist, int32_t cap, int32_t *n_lines) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->st || !c->hist) { g_fx_error = "fx_krylov_history: no Krylov loop was started on this context"; return FX_ERROR_RUNTIME; }
  KrylovState s;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(&s, c->st, sizeof s, hipMemcpyDeviceToHost));
  const int32_t n = std::max(0, std::min(s.n_hist, c->hist_cap));
  if (n_lines) *n_lines = n;
  if (hist && cap > 0 && n > 0) HIP_TRY(hipMemcpy(hist, c->hist, (size_t)std::min(cap, n) * 8, hipMemcpyDeviceToHost));
  return 0;
}

// ---------------------------------------------------------------------------
// hecmw_solve_iterative on the resident system (hecmw_solver_Iterative.f90:13-210)
// ---------------------------------------------------------------------------
static int host_sum(fx_context *c, int nparts, int stride, double *v0, double *v1) {
  hipLaunchKernelGGL((k_scalar<OP_PLAIN>), dim3(1), dim3(1024), 0, c->stream, c->partials, nparts, stride, c->st,
                     (double *)nullptr, c->red_out, 1, 1);
  if (multi_rank(c) && allreduce_dev(c, c->red_out, 2)) return FX_ERROR_RUNTIME;
  double *h = (double *)(c->st_host + 2);  // pinned (st_host holds 4 KrylovState slots; polling uses the first)
  HIP_TRY(hipMemcpyAsync(h, c->red_out, 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *v0 = h[0];
  if (v1) *v1 = h[1];
  return 0;
}

#include "fx_krylov2_host.h"

// SCALING=YES: the resident D/AL/AU/B are scaled in place before the preconditioner set-up and the Krylov loop and
// divided back afterwards, as every solver of the reference does (hecmw_solver_CG.f90:104, :277).
static int scaling_apply(fx_context *c, bool back) {
  const DevCSR &A = c->A;
  if (ensure_solver(c)) return FX_ERROR_RUNTIME;
  if (!c->scale_vec && dev_alloc(&c->scale_vec, (size_t)3 * A.NP)) return FX_ERROR_RUNTIME;  // freed with the matrix
  double *scale = c->scale_vec;
  const int64_t n3 = (int64_t)3 * A.N;
  if (!back) {
    HIP_TRY(hipMemsetAsync(scale, 0, (size_t)3 * A.NP * 8, c->stream));
    hipLaunchKernelGGL(k_scaling_vector, dim3((A.N + 255) / 256), dim3(256), 0, c->stream, A.N, A.D, scale);
    if (multi_rank(c)) {  // hecmw_update_3_R(scale): natural numbering -> slots -> halo -> back
      if (to_slots(c, scale, c->W[6]) || halo_update(c, c->W[6]) || from_slots(c, c->W[6], scale)) return FX_ERROR_RUNTIME;
    }
    hipLaunchKernelGGL((k_scaling_matrix<false>), dim3((A.NP + 255) / 256), dim3(256), 0, c->stream, A.NP, A.indexL, A.itemL,
                       A.indexU, A.itemU, A.D, A.AL, A.AU, scale);
    hipLaunchKernelGGL((k_scaling_rhs<false>), dim3(grid_for(n3)), dim3(256), 0, c->stream, n3, scale, A.B, A.X);
  } else {
    hipLaunchKernelGGL((k_scaling_rhs<true>), dim3(grid_for(n3)), dim3(256), 0, c->stream, n3, scale, A.B, A.X);
    hipLaunchKernelGGL((k_scaling_matrix<true>), dim3((A.NP + 255) / 256), dim3(256), 0, c->stream, A.NP, A.indexL, A.itemL,
                       A.indexU, A.itemU, A.D, A.AL, A.AU, scale);
  }
  HIP_TRY(hipGetLastError());
  c->bell_valid = false;      // the streaming layouts are gathered again from the (un)scaled values
  c->precond_valid = false;
  return 0;
}

static int ensure_partials(fx_context *c) {  // the partial-sum buffer of the scalar stages and of the solve's checks
  if (c->max_partials < 4096 + 8) {
    dev_free(c->partials);
    if (dev_alloc(&c->partials, (size_t)(4096 + 8) * 3)) return FX_ERROR_RUNTIME;
    c->max_partials = 4096 + 8;
  }
  return 0;
}

// One driver for every block size.  The path (Ops33 below, OpsNN in fx_nn_host.h) supplies what differs: the norms and the
// zero-diagonal kernel, the preconditioner set-up before the loop / of the scaled matrix / on a retry, scaling, one attempt of
// METHOD 1-4 (a timed-out dataflow sweep is redone inside it), where X lives, the final ||b - Ax||^2, ncolor and the clocks.
// An attempt is recorded (fx_solve_attempts) once it has run; an error return leaves the records of the attempts before it.
template <class Path>
static int hecmw_solve_iterative(const Path &p, int32_t *Iarray, const double *Rarray, fx_solve_info *info, double *hist,
                                 int32_t hist_len) {
  fx_context *c = p.c;
  const int precond = Iarray[2], method2 = Iarray[7], iterpremax = Iarray[4];
  int method = Iarray[1];
  int ret = 0;
  const double t0 = now_s();
  c->attempts.clear();
  // hecmw_solve_check_zerorhs (:242-278): warning 2002, X = 0, the solve continues
  double rhs2 = 0.0;
  if (p.rhs_norm2(&rhs2)) return FX_ERROR_RUNTIME;
  if (rhs2 == 0.0) {
    ret = FX_ERROR_ZERO_RHS;
    if (p.zero_x()) return FX_ERROR_RUNTIME;
  }
  {  // hecmw_solve_check_zerodiag (:212-240)
    int32_t *flag = (int32_t *)(c->red_out + 8), hflag = 0;
    HIP_TRY(hipMemsetAsync(flag, 0, 4, c->stream));
    p.zero_diag(flag);
    HIP_TRY(hipMemcpyAsync(&hflag, flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (multi_rank(c)) {  // MAX of 0/1 flags == (SUM > 0)
      double f = hflag ? 1.0 : 0.0;
      HIP_TRY(hipMemcpyAsync(c->red_out + 4, &f, 8, hipMemcpyHostToDevice, c->stream));
      if (allreduce_dev(c, c->red_out + 4, 1)) return FX_ERROR_RUNTIME;
      HIP_TRY(hipMemcpyAsync(&f, c->red_out + 4, 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      hflag = f > 0.0;
    }
    if (hflag && precond < 10 && iterpremax > 0) return FX_ERROR_ZERO_DIAG;
  }
  // hecmw_mat_recycle_precond_setting (hecmw_matrix_misc.f90:678-697)
  if (Iarray[97] >= 1) { Iarray[96] = 1; Iarray[95] = 0; }
  else if (Iarray[96] > 1) { Iarray[95] = 0; Iarray[96] = 1; }
  else if (Iarray[96] == 1) {
    if (Iarray[95] < Iarray[34]) { Iarray[96] = 0; Iarray[95]++; }
    else Iarray[95] = 0;
  }
  if (int e = p.setup(Iarray, Rarray, Iarray[97] == 1 || Iarray[96] == 1)) return e;
  Iarray[97] = 0; Iarray[96] = 0;
  const double t_setup = now_s() - t0, t1 = now_s();
  const bool auto_sigma = Rarray[1] < 0.0;  // hecmw_solver_Iterative.f90:68-73
  const bool scaling = Iarray[6] != 0;      // SCALING=YES (IDX_I_SCALING = 7)
  double sigma = auto_sigma ? 1.0 : Rarray[1];
  HostKrylov res;
  for (;;) {
    Iarray[80] = 0; Iarray[81] = 0;
    if (method < 1 || method > 4) { g_fx_error = "METHOD must be 1 (CG), 2 (BiCGSTAB), 3 (GMRES) or 4 (GPBiCG)"; return FX_ERROR_INCONS_PC; }
    if (scaling) {  // scale, then build the preconditioner of the scaled matrix (hecmw_solver_CG.f90:104-112)
      if (int e = p.scale(Iarray, Rarray, sigma)) return e;
    }
    if (int e = p.attempt(Iarray, Rarray, method, &res)) return e;
    c->attempts.push_back({method, sigma, res.hist});  // the pass's ITERLOG lines (a retry starts its history again at line 1)
    if (scaling && p.unscale()) return FX_ERROR_RUNTIME;  // x <- D^-1/2 x, b and the matrix divided back (CG.f90:277)
    if (res.error == FX_ERROR_DIVERGE_PC || res.error == FX_ERROR_DIVERGE_MAT) {  // :145-156
      Iarray[81] = 1;
      // The retries call the Krylov routine again; its hecmw_precond_setup finds Iarray(97) = Iarray(98) = 0 and returns early
      // (hecmw_precond_BILU_33.f90:49-57, BILU_nn.f90:49-57; the hecmw_precond_clear at the end of every method is commented
      // out, hecmw_solver_CG.f90:285), so the reference's retry keeps the factors of the FIRST SIGMA_DIAG and only restarts from
      // the X the failed attempt left (hecMAT%X is not reset).  Reproduced literally (bit-exact oracle runs against the real
      // reference: tests/golden/retry.npz, nn_ilu.npz); `sigma` is tracked because it decides how many retries there are.
      if (precond >= 10 && precond < 20 && auto_sigma && sigma < 2.0) {  // 'Increasing SIGMA_DIAG' retry of the ILU family
        sigma += (double)0.1f;  // `SIGMA_DIAG = SIGMA_DIAG + 0.1` with a default-real literal (:147): what the reference adds, and prints
      } else if (method == 1 && method2 > 1) {
        if (auto_sigma) sigma = 1.0;  // :152 (no set-up follows in the reference either)
        method = method2;
      } else {
        break;
      }
      if (p.retry(Iarray, sigma)) return FX_ERROR_RUNTIME;
      continue;
    }
    break;
  }
  // X halo (hecmw_update_m_R, hecmw_solver_CG.f90:280), then back to the caller's numbering
  if (p.finish_x()) return FX_ERROR_RUNTIME;
  const double t_sol = now_s() - t1;
  if (res.error > 1) ret = res.error;
  // final true residual (hecmw_rel_resid_L2, hecmw_solver_las.f90:129-158) -> Iarray(81)
  double r2 = 0.0;
  if (p.resid2(&r2)) return FX_ERROR_RUNTIME;
  const double resid2 = sqrt(r2 / (rhs2 == 0.0 ? 1.0 : rhs2));
  if (resid2 < Rarray[0]) Iarray[80] = 1;
  const int nh = hist ? std::max(0, std::min((int)hist_len, (int)res.hist.size())) : 0;
  if (info) {
    memset(info, 0, sizeof *info);
    info->iterations = res.iter;
    info->method = method; info->precond = precond;
    info->resid = res.resid;
    info->rel_resid = resid2;
    info->time_setup = t_setup; info->time_sol = t_sol;
    info->n_hist = nh;
    if (p.fill_info(info)) return FX_ERROR_RUNTIME;
  }
  if (nh > 0) memcpy(hist, res.hist.data(), (size_t)nh * 8);
  return ret;
}

// --- the 3x3 path: vectors in slot order, the resident preconditioners ---------------------------------------------------
int Ops33::rhs_norm2(double *b2) const {  // sum over the internal rows of B (natural numbering: independent of the solver numbering)
  if (ensure_partials(c)) return FX_ERROR_RUNTIME;
  const int64_t n = (int64_t)3 * c->A.N;
  const int np = grid_for(n, FX_BLOCK, 2048);
  hipLaunchKernelGGL(k_dot, dim3(np), dim3(FX_BLOCK), 0, c->stream, n, c->A.B, c->A.B, c->partials, (const int32_t *)nullptr, 0);
  HIP_TRY(hipGetLastError());
  double tmp;
  return host_sum(c, np, 0, b2, &tmp);
}
int Ops33::zero_x() const {
  HIP_TRY(hipMemsetAsync(c->A.X, 0, (size_t)3 * c->A.NP * 8, c->stream));
  return 0;
}
void Ops33::zero_diag(int32_t *flag) const {
  hipLaunchKernelGGL(k_check_zero_diag, dim3(grid_for(c->A.N)), dim3(256), 0, c->stream, c->A.N, c->A.D, flag);
}
// rebuild when the flags ask for it, reuse otherwise (SSOR_33.f90:71-79); each preconditioner type has its own state
int Ops33::setup(const int32_t *I, const double *R, bool asked) const {
  const int precond = I[2];
  const int want_kind = (I[4] <= 0) ? 0 : ((precond == 1 || precond == 2) ? (c->ssor_natural ? 11 : 1) : precond);
  if (c->precond_valid && !asked && c->precond_kind == want_kind) return 0;
  return fx_precond_setup(c, I, R);
}
int Ops33::scale(const int32_t *I, const double *R, double) const {
  if (scaling_apply(c, false)) return FX_ERROR_RUNTIME;
  double R2[100];
  memcpy(R2, R, sizeof R2);
  R2[1] = R[1] < 0.0 ? 1.0 : R[1];  // every attempt scales the same matrix the same way: the first SIGMA_DIAG's factors
  return fx_precond_setup(c, I, R2);
}
int Ops33::unscale() const {  // then everything resident is refreshed
  if (from_slots(c, c->Xs, c->A.X) || scaling_apply(c, true) || ensure_solver(c)) return FX_ERROR_RUNTIME;
  return (to_slots(c, c->A.B, c->Bs) || to_slots(c, c->A.X, c->Xs)) ? FX_ERROR_RUNTIME : 0;
}
int Ops33::attempt(const int32_t *I, const double *R, int method, HostKrylov *res) const {
  const int maxit = I[0];
  const double tol = R[0];
  c->k_method_last = method;
  KrylovState s;
  int e;
  for (int redo = 0;; redo++) {
    *res = HostKrylov();
    if (method <= 2) {
      if (krylov_begin(c, method, maxit, tol)) return FX_ERROR_RUNTIME;
      e = krylov_steps(c, maxit, &s);
    } else {
      e = (method == 3) ? gmres_solve_t(*this, maxit, tol, I[5], res) : gpbicg_solve_t(*this, maxit, tol, res);
      // asked BEFORE looking at e: a timed-out sweep leaves tag values (NaN) in the vectors, which is what makes these methods
      // return a breakdown code in the first place
      if (df_take_error(c)) e = FX_DF_RETRY;
    }
    // a dataflow sweep gave up: the iterates are unusable, the context has switched to the launch-per-level sweeps -- the
    // attempt runs again from the X it started with (every method re-reads it from A.X; nothing was written back)
    if (e != FX_DF_RETRY || redo > 0) break;
  }
  if (e) return e == FX_DF_RETRY ? FX_ERROR_RUNTIME : e;
  if (method >= 3) {
    memcpy(c->host_dbg, res->dbg, sizeof res->dbg);
    c->host_dbg[14] = res->status;
    return 0;
  }
  res->iter = s.iter; res->resid = s.resid; res->status = s.status;
  res->error = s.status > 1 ? s.status : 0;
  res->hist.resize((size_t)std::max(0, s.n_hist));
  if (s.n_hist > 0) HIP_TRY(hipMemcpy(res->hist.data(), c->hist, (size_t)s.n_hist * 8, hipMemcpyDeviceToHost));
  return 0;
}
int Ops33::retry(const int32_t *, double) const {  // from the X the failed attempt left, halo included
  return (halo_update(c, c->Xs) || from_slots(c, c->Xs, c->A.X)) ? FX_ERROR_RUNTIME : 0;
}
int Ops33::finish_x() const {
  if (halo_update(c, c->Xs) || from_slots(c, c->Xs, c->A.X)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
int Ops33::resid2(double *r2) const {
  if (::spmv(c, 1, 2, c->Xs, c->Bs, c->W[7], nullptr, 0)) return FX_ERROR_RUNTIME;
  double tmp;
  return host_sum(c, spmv_nparts(c), 0, r2, &tmp);
}
int Ops33::fill_info(fx_solve_info *info) const {
  info->ncolor = (c->precond_kind == 1 || level_sched(c)) ? c->ssor.ncolor : 0;  // SSOR colours / ILU levels
  if (c->clock.on) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    clock_collect(c);
    info->time_matvec = c->clock.acc[0]; info->time_precond = c->clock.acc[1]; info->time_comm = c->clock.acc[2];
  }
  c->clock.on = false;
  return 0;
}

extern "C" int fx_solve_resident(fx_context *c, int32_t *Iarray, double *Rarray, fx_solve_info *info, double *hist,
                                 int32_t hist_len) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->have_values) { g_fx_error = "fx_solve_resident: no matrix resident"; return FX_ERROR_RUNTIME; }
  if (require_transport(c, "fx_solve_resident")) return FX_ERROR_RUNTIME;
  c->iterpremax = Iarray[4];
  c->clock.on = Iarray[21] >= 1;  // TIMELOG
  c->clock.used = 0;
  c->clock.acc[0] = c->clock.acc[1] = c->clock.acc[2] = 0.0;
  return hecmw_solve_iterative(Ops33{c}, Iarray, Rarray, info, hist, hist_len);
}

// hecmw_solve (hecmw_solver.f90:9): Iarray(99) = 1 selects the iterative solvers; the direct ones are outside the GPU hot path
static int refuse_direct(const int32_t *Iarray) {
  if (Iarray[98] == 1) return 0;
  g_fx_error = "Iarray(99) selects a direct solver: outside the GPU hot path";
  return FX_ERROR_UNSUPPORTED;
}

// The values of hecMAT changed: the flags say so, nothing is resident yet (`resident`), or another hecMAT of the same shape came
// without the flags raised (the reference would multiply with it, with the preconditioner it happens to have) -- recognised by
// the identity of the caller's arrays
static bool values_changed(const fx_context *c, const fx_matrix_view *m, const int32_t *Iarray, bool resident) {
  return Iarray[97] >= 1 || Iarray[96] >= 1 || !resident || m->D != c->host_D || m->AL != c->host_AL || m->AU != c->host_AU;
}

#include "fx_nn_host.h"

// X goes back to the caller unless the solve stopped before it had one: a run-time failure, E-2001 or E-1001
static int download_x_unless_failed(fx_context *c, const fx_matrix_view *m, int ret) {
  if (ret < 0 || ret == FX_ERROR_ZERO_DIAG || ret == FX_ERROR_INCONS_PC) return ret;
  if (m->NDOF == 3) {
    const int e = fx_download_x(c, m->X, 3 * m->NP);
    return e ? e : ret;
  }
  NnDev *n = nn_of(c);
  HIP_TRY(hipMemcpy(m->X, n->X, (size_t)n->ndof * n->NP * 8, hipMemcpyDeviceToHost));
  return ret;
}

// hecmw_solve (hecmw_solver.f90:9): host arrays in, host X out.
extern "C" int fx_solve(fx_context *c, const fx_matrix_view *m, const fx_comm_view *cm, int32_t *Iarray, double *Rarray,
                        fx_solve_info *info, double *hist, int32_t hist_len) {
  if (int e = refuse_direct(Iarray)) return e;
  int ret;
  if (m->NDOF != 3) {
    ret = nn_solve(c, m, cm, Iarray, Rarray, info, hist, hist_len);  // select case(NDOF): the nn path
  } else {
    int what = FX_UP_RHS | FX_UP_X;
    if (Iarray[97] >= 1 || !c->have_profile) what |= FX_UP_PROFILE;  // symbolic: profile changed
    if (values_changed(c, m, Iarray, c->have_values)) what |= FX_UP_VALUES;
    if (int e = fx_upload(c, m, cm, what)) return e;
    if (what & FX_UP_VALUES) { c->host_D = m->D; c->host_AL = m->AL; c->host_AU = m->AU; }
    ret = fx_solve_resident(c, Iarray, Rarray, info, hist, hist_len);
  }
  return download_x_unless_failed(c, m, ret);
}

// hecmw_solve for a system whose MATRIX was produced on the device (fx_nl_stiffness_at / fx_assemble_c3d8) and whose right-hand
// side and prescribed dofs come from the host -- what fistr1's fstr_Newton hands over when the binding of INTEGRATION.md section 5
// is in place: B and X go up (3*NP doubles each), the hecmw_mat_ass_bc calls fstr_AddBC made are applied to the resident matrix
// and B (fx_mat_ass_bc), the resident system is solved, X comes back.  D / AL / AU of `m` are ignored (may be NULL).
extern "C" int fx_solve_device_matrix(fx_context *c, const fx_matrix_view *m, const fx_comm_view *cm, int32_t n_bc, const int32_t *bc_node,
                                      const int32_t *bc_dof, const double *bc_val, int32_t *Iarray, double *Rarray, fx_solve_info *info,
                                      double *hist, int32_t hist_len) {
  if (int e = refuse_direct(Iarray)) return e;
  if (m->NDOF != 3) { g_fx_error = "fx_solve_device_matrix: NDOF = 3 only"; return FX_ERROR_UNSUPPORTED; }
  if (!c->have_profile || !c->have_values || c->A.N != m->N || c->A.NP != m->NP || c->A.NPL != m->NPL || c->A.NPU != m->NPU) {
    g_fx_error = "fx_solve_device_matrix: no device-assembled matrix of this shape is resident";
    return FX_ERROR_RUNTIME;
  }
  fx_matrix_view mv = *m;
  mv.D = nullptr; mv.AL = nullptr; mv.AU = nullptr;
  int e = fx_upload(c, &mv, cm, FX_UP_RHS | FX_UP_X);
  if (e) return e;
  if ((e = fx_mat_ass_bc(c, n_bc, bc_node, bc_dof, bc_val))) return e;
  c->host_D = nullptr; c->host_AL = nullptr; c->host_AU = nullptr;  // the resident values are nobody's host arrays: a later fx_solve uploads its own
  return download_x_unless_failed(c, m, fx_solve_resident(c, Iarray, Rarray, info, hist, hist_len));
}

extern "C" int fx_matvec(fx_context *c, const fx_matrix_view *m, const fx_comm_view *cm, double *x, double *y,
                         double *commtime) {
  if (m->NDOF != 3) return nn_matvec(c, m, cm, x, y, commtime);
  // hecmw_matvec carries no "matrix changed" flag (Iarray(97/98) belong to hecmw_solve), and its external callers (implicit
  // dynamics, eigen output) change hecMAT between calls: the values the caller passes are uploaded on every call.
  // mat->D == NULL says "use the resident values" (repeated products with one matrix).
  int what = m->D ? FX_UP_VALUES : 0;
  if (!c->have_profile || c->A.N != m->N || c->A.NP != m->NP || c->A.NPL != m->NPL || c->A.NPU != m->NPU) what |= FX_UP_PROFILE;
  if (!m->D && (!c->have_values || (what & FX_UP_PROFILE))) { g_fx_error = "fx_matvec: mat->D is NULL but no matrix values are resident"; return FX_ERROR_RUNTIME; }
  if (what) {
    fx_matrix_view mv = *m;
    mv.B = nullptr; mv.X = nullptr;
    int e = fx_upload(c, &mv, cm, what);
    if (e) return e;
    // the resident values are now this caller's: a later fx_solve of another hecMAT of the same shape (flags 0) must
    // see that the identity of the arrays changed and upload its own
    if (what & FX_UP_VALUES) { c->host_D = m->D; c->host_AL = m->AL; c->host_AU = m->AU; }
  }
  HIP_TRY(hipSetDevice(c->device));
  if (c->halo.n_neighbor > 0 && require_transport(c, "fx_matvec")) return FX_ERROR_RUNTIME;  // the halo part of X comes from the neighbours
  if (ensure_solver(c)) return FX_ERROR_RUNTIME;
  const size_t len = (size_t)3 * c->A.NP * 8;
  // natural-order staging in A.X's shadow: use W[5] (>= 3*NP doubles) for the host image
  HIP_TRY(hipMemcpyAsync(c->W[5], x, len, hipMemcpyHostToDevice, c->stream));
  if (to_slots(c, c->W[5], c->W[6])) return FX_ERROR_RUNTIME;
  const double t0 = now_s();
  if (halo_update(c, c->W[6])) return FX_ERROR_RUNTIME;
  if (commtime) { HIP_TRY(hipStreamSynchronize(c->stream)); *commtime += now_s() - t0; }
  HIP_TRY(hipMemsetAsync(c->W[7], 0, (size_t)c->wlen * 8, c->stream));
  if (spmv(c, 0, 0, c->W[6], nullptr, c->W[7], nullptr, 0)) return FX_ERROR_RUNTIME;  // (the halo update above made it current; a second one is idempotent)
  if (from_slots(c, c->W[7], c->W[5])) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(y, c->W[5], (size_t)3 * c->A.N * 8, hipMemcpyDeviceToHost, c->stream));
  if (from_slots(c, c->W[6], c->W[4])) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(x, c->W[4], len, hipMemcpyDeviceToHost, c->stream));  // halo part of X is updated
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int fx_nn_matvec_resident(fx_context *c, int nrepeat, float *ms_per_call, int64_t stats[4]) {
  HIP_TRY(hipSetDevice(c->device));
  if (int e = nn_matvec_resident(c, nrepeat, ms_per_call)) return e;
  NnDev *n = nn_of(c);
  if (stats) { stats[0] = n->ndof; stats[1] = n->N; stats[2] = n->M.nblocks_padded * 64; stats[3] = (int64_t)n->N + n->NPL + n->NPU; }
  return 0;
}

// z = M^-1 r once for a generic-block system (hecmw_precond_setup + hecmw_precond_apply, hecmw_precond.f90:28, :75-123 with
// the iterPREmax loop): upload, set up or reuse the preconditioner (PRECOND / SIGMA_DIAG / recycle flags as fx_solve reads
// them), ZP = r on the internal rows and 0 on the halo, then the apply.  r, z: host, NDOF * NP doubles (z's halo part is 0).
extern "C" int fx_nn_precond_apply(fx_context *c, const fx_matrix_view *m, const fx_comm_view *cm, int32_t *Iarray, double *Rarray,
                                   const double *r, double *z) {
  HIP_TRY(hipSetDevice(c->device));
  if (m->NDOF == 3 || m->NDOF < 1 || m->NDOF > 6) { g_fx_error = "fx_nn_precond_apply: NDOF must be 1, 2, 4, 5 or 6"; return FX_ERROR_UNSUPPORTED; }
  c->view_petot = cm ? std::max(1, (int)cm->PETOT) : 1;
  if (require_transport(c, "fx_nn_precond_apply")) return FX_ERROR_RUNTIME;
  fx_matrix_view mv = *m;
  mv.B = nullptr; mv.X = nullptr;
  const bool changed = values_changed(c, m, Iarray, nn_of(c)->have_matrix);
  if (nn_upload(c, &mv, cm, changed)) return FX_ERROR_RUNTIME;
  if (changed) { c->host_D = m->D; c->host_AL = m->AL; c->host_AU = m->AU; }
  NnDev *n = nn_of(c);
  n->cur_AL = m->AL; n->cur_AU = m->AU;
  const int precond = Iarray[2], iterpremax = Iarray[4];
  const double sigma = Rarray[1] < 0.0 ? 1.0 : Rarray[1];
  if (iterpremax > 0 && (!n->precond_valid || Iarray[97] >= 1 || Iarray[96] >= 1 || n->sigma != sigma ||
                         n->precond_kind != nn_precond_kind(precond))) {
    if (int e = nn_precond_setup(c, precond, sigma, Iarray[33])) return e;
  }
  Iarray[97] = 0; Iarray[96] = 0;
  n->iterpremax = iterpremax;
  const size_t len = (size_t)n->ndof * n->NP;
  HIP_TRY(hipMemcpyAsync(n->W[5], r, len * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(n->W[5] + (size_t)n->ndof * n->N, 0, (len - (size_t)n->ndof * n->N) * 8, c->stream));
  for (int attempt = 0; attempt < 2; attempt++) {
    if (nn_precond_apply(c, iterpremax, n->W[5], n->W[6])) return FX_ERROR_RUNTIME;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!nn_df_take_error(c)) break;  // a timed-out dataflow sweep: redone with per-level launches
  }
  HIP_TRY(hipMemsetAsync(n->W[6] + (size_t)n->ndof * n->N, 0, (len - (size_t)n->ndof * n->N) * 8, c->stream));
  HIP_TRY(hipMemcpyAsync(z, n->W[6], len * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// timed z = M^-1 r of the resident generic-block preconditioner (the one the last fx_solve / fx_nn_precond_apply set up) on
// resident work vectors, iterPREmax of that call
extern "C" int fx_nn_precond_apply_resident(fx_context *c, int nrepeat, float *ms_per_call) {
  HIP_TRY(hipSetDevice(c->device));
  NnDev *n = nn_of(c);
  if (!n->have_matrix || !n->precond_valid) { g_fx_error = "fx_nn_precond_apply_resident: no generic-block preconditioner set up"; return FX_ERROR_RUNTIME; }
  const int ipm = std::max(n->iterpremax, 1);
  float ms = 0.f;
  for (int attempt = 0; attempt < 2; attempt++) {
    if (nn_precond_apply(c, ipm, n->W[5], n->W[6])) return FX_ERROR_RUNTIME;  // untimed first touch
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < nrepeat; i++)
      if (nn_precond_apply(c, ipm, n->W[5], n->W[6])) return FX_ERROR_RUNTIME;
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (!nn_df_take_error(c)) break;  // a timed-out dataflow sweep: timed again with per-level launches
  }
  if (ms_per_call) *ms_per_call = ms / std::max(nrepeat, 1);
  return 0;
}

// out[0..9]: resident generic-block preconditioner kind (1 SSOR, 3 DIAG, 10 block ILU(0); 0 none) | levels (ILU) or colours
// (SSOR) | sweep slices | longest L + U row in blocks (ILU) | factor kernel lanes per row (32 or 1) | padded L blocks |
// padded U blocks | set-up wall time of the last ILU(0) set-up in microseconds | ILU sweep form now (1 dataflow, 0 per-level
// launches) | workgroups of the last dataflow launch (after the co-residency clamp) in bits 0-31, timed-out dataflow sweeps
// of this system in bits 32-63
extern "C" int fx_nn_precond_stats(fx_context *c, int64_t out[10]) {
  if (!c || !out) { g_fx_error = "fx_nn_precond_stats: null argument"; return FX_ERROR_RUNTIME; }
  memset(out, 0, 10 * sizeof(int64_t));
  if (!c->nn) return 0;
  NnDev *n = nn_of(c);
  if (!n->precond_valid) return 0;
  out[0] = n->precond_kind;
  out[1] = n->precond_kind == 3 ? 0 : n->ncolor;
  out[2] = n->precond_kind == 3 ? 0 : n->L.nslices;
  out[3] = n->precond_kind == 10 ? n->ilu_max_row_blocks : 0;
  out[4] = n->precond_kind == 10 ? n->ilu_factor_lanes : 0;
  out[5] = n->precond_kind == 3 ? 0 : n->L.nblocks_padded * 64;
  out[6] = n->precond_kind == 3 ? 0 : n->U.nblocks_padded * 64;
  out[7] = n->precond_kind == 10 ? (int64_t)(n->ilu_setup_ms * 1e3) : 0;
  out[8] = n->precond_kind == 10 && c->df_mode >= 1 ? 1 : 0;
  out[9] = n->precond_kind == 10 ? ((int64_t)n->ilu_df_grid_last | ((int64_t)n->ilu_df_fallbacks << 32)) : 0;
  return 0;
}

// y = A x on resident work vectors, timed with HIP events on the solver stream.  variant: 0 plain (BiCGSTAB's products),
// 1 with the fused partial of x.y (the launch of every CG iteration, hecmw_solver_CG.f90:204-211), 2 r = b - A x with the
// partial of r.r (the residual recomputation).  The halo exchange of a multi-rank system is part of every call.
extern "C" int fx_spmv_resident(fx_context *c, int variant, int nrepeat, float *ms_per_call) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->have_values) { g_fx_error = "fx_spmv_resident: no matrix resident"; return FX_ERROR_RUNTIME; }
  if (variant < 0 || variant > 2) { g_fx_error = "fx_spmv_resident: variant must be 0, 1 or 2"; return FX_ERROR_RUNTIME; }
  if (ensure_solver(c)) return FX_ERROR_RUNTIME;
  if (to_slots(c, c->A.B, c->Bs)) return FX_ERROR_RUNTIME;
  const int mode = variant == 2 ? 1 : 0, dot = variant;
  // x and y are the vectors the CG loop multiplies (p = W[2], q = W[1]: cg_iteration) -- which buffers the product reads and
  // writes moves its time by up to 4 % (scripts/experiments/ab_vectors.py), and the roofline figure is the loop's kernel.  The
  // call overwrites them: not between fx_krylov_begin and the end of the iterations.
  double *xin = c->W[2], *yout = c->W[1];
  HIP_TRY(hipMemcpyAsync(xin, c->Bs, (size_t)c->wlen * 8, hipMemcpyDeviceToDevice, c->stream));
  if (spmv(c, mode, dot, xin, c->Bs, yout, nullptr, 0)) return FX_ERROR_RUNTIME;  // untimed first touch
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  for (int i = 0; i < nrepeat; i++)
    if (spmv(c, mode, dot, xin, c->Bs, yout, nullptr, 0)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  if (ms_per_call) *ms_per_call = ms / std::max(nrepeat, 1);
  return 0;
}

extern "C" int fx_matvec_resident(fx_context *c, int nrepeat, float *ms_per_call) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->have_values) { g_fx_error = "fx_matvec_resident: no matrix resident"; return FX_ERROR_RUNTIME; }
  if (ensure_solver(c)) return FX_ERROR_RUNTIME;
  if (to_slots(c, c->A.B, c->Bs)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  for (int i = 0; i < nrepeat; i++)
    if (spmv(c, 0, 0, c->Bs, nullptr, c->W[7], nullptr, 0)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  if (ms_per_call) *ms_per_call = ms / std::max(nrepeat, 1);
  return 0;
}

extern "C" int fx_precond_apply_host(fx_context *c, const double *r, double *z) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->precond_valid) { g_fx_error = "fx_precond_apply_host: preconditioner not set up"; return FX_ERROR_RUNTIME; }
  const size_t len = (size_t)3 * c->A.NP * 8;
  KrylovState s;
  memset(&s, 0, sizeof s);
  HIP_TRY(hipMemcpyAsync(c->st, &s, sizeof s, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->W[5], r, len, hipMemcpyHostToDevice, c->stream));
  if (to_slots(c, c->W[5], c->W[6])) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemsetAsync(c->W[6] + (size_t)3 * c->ord.nslots, 0, (size_t)3 * c->ord.nhalo * 8, c->stream));  // ZP(halo) = 0
  for (int attempt = 0; attempt < 2; attempt++) {
    HIP_TRY(hipMemsetAsync(c->W[7], 0, (size_t)c->wlen * 8, c->stream));
    int np;
    if (precond_apply(c, c->W[6], c->W[7], false, &np)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!df_take_error(c)) break;  // a timed-out dataflow sweep: redone with the launch-per-level sweeps
  }
  if (from_slots(c, c->W[7], c->W[5])) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(z, c->W[5], len, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int fx_dot_host(fx_context *c, const double *x, const double *y, double *result) {
  HIP_TRY(hipSetDevice(c->device));
  const size_t len = (size_t)3 * c->A.NP * 8;
  if (ensure_solver(c)) return FX_ERROR_RUNTIME;
  HIP_TRY(hipMemcpyAsync(c->W[4], x, len, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->W[5], y, len, hipMemcpyHostToDevice, c->stream));
  if (to_slots(c, c->W[4], c->W[6]) || to_slots(c, c->W[5], c->W[7])) return FX_ERROR_RUNTIME;
  int np;
  double tmp;
  if (dot_into_partials(c, c->W[6], c->W[7], nullptr, 0, &np)) return FX_ERROR_RUNTIME;
  return host_sum(c, np, 0, result, &tmp);
}

// z = M^-1 r on resident work vectors, timed with HIP events on the solver stream.
extern "C" int fx_precond_apply_resident(fx_context *c, int nrepeat, float *ms_per_call) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->precond_valid) { g_fx_error = "fx_precond_apply_resident: preconditioner not set up"; return FX_ERROR_RUNTIME; }
  KrylovState s;
  memset(&s, 0, sizeof s);
  HIP_TRY(hipMemcpyAsync(c->st, &s, sizeof s, hipMemcpyHostToDevice, c->stream));
  int np;
  if (to_slots(c, c->A.B, c->Bs)) return FX_ERROR_RUNTIME;
  float ms = 0.f;
  for (int attempt = 0; attempt < 2; attempt++) {
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < nrepeat; i++)
      if (precond_apply(c, c->Bs, c->W[7], true, &np)) return FX_ERROR_RUNTIME;
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (!df_take_error(c)) break;  // a timed-out dataflow sweep: timed again with the launch-per-level sweeps
  }
  if (ms_per_call) *ms_per_call = ms / std::max(nrepeat, 1);
  return 0;
}

// The passes of the auto-SIGMA_DIAG / METHOD2 loop of the last solve on this context (hecmw_solver_Iterative.f90:117-157): the
// reference prints its banner before every pass, the pass's ITERLOG lines, and 'Increasing SIGMA_DIAG to <value>' before a
// SIGMA_DIAG retry; a binding replays those lines from here.  Arrays of `cap` entries; *n_attempts is the true count.
extern "C" int fx_solve_attempts(fx_context *c, int32_t cap, int32_t *n_attempts, int32_t *method, double *sigma_diag, int32_t *n_hist) {
  if (!c || !n_attempts) { g_fx_error = "fx_solve_attempts: null argument"; return FX_ERROR_RUNTIME; }
  *n_attempts = (int32_t)c->attempts.size();
  for (int32_t k = 0; k < cap && k < *n_attempts; k++) {
    if (method) method[k] = c->attempts[k].method;
    if (sigma_diag) sigma_diag[k] = c->attempts[k].sigma_diag;
    if (n_hist) n_hist[k] = (int32_t)c->attempts[k].hist.size();
  }
  return 0;
}
extern "C" int fx_solve_attempt_history(fx_context *c, int32_t attempt, double *hist, int32_t cap) {
  if (!c || attempt < 0 || attempt >= (int32_t)c->attempts.size()) { g_fx_error = "fx_solve_attempt_history: no such attempt"; return FX_ERROR_RUNTIME; }
  const std::vector<double> &h = c->attempts[attempt].hist;
  if (hist && cap > 0 && !h.empty()) memcpy(hist, h.data(), sizeof(double) * std::min<size_t>((size_t)cap, h.size()));
  return 0;
}

// Scalars of the Krylov loop as they stand on the device (diagnostics):
// out = rho rho1 beta c1 alpha omega c2 cg0 cg1 dnrm2 bnrm2 resid tol iter status need_verify
extern "C" int fx_debug_state(fx_context *c, double out[16]) {
  if (c->k_method_last >= 3) { memcpy(out, c->host_dbg, 16 * sizeof(double)); return 0; }  // host-driven recurrences (GMRES, GPBiCG)
  KrylovState s;
  if (poll_state(c, &s)) return FX_ERROR_RUNTIME;
  const double v[16] = {s.rho, s.rho1, s.beta, s.c1, s.alpha, s.omega, s.c2, s.cg0, s.cg1, s.dnrm2, s.bnrm2, s.resid, s.tol,
                        (double)s.iter, (double)s.status, (double)s.need_verify};
  memcpy(out, v, sizeof v);
  return 0;
}

// Measured read-streaming rate of this device over the resident value array of M (GB/s).
extern "C" int fx_stream_ceiling(fx_context *c, int nrepeat, double *gbs) {
  HIP_TRY(hipSetDevice(c->device));
  if (ensure_solver(c)) return FX_ERROR_RUNTIME;
  const int64_t n2 = (int64_t)c->M.npairs * 576 / 2;  // double2 words
  if (n2 <= 0) { g_fx_error = "fx_stream_ceiling: no matrix resident"; return FX_ERROR_RUNTIME; }
  const int g = std::min(256 * 32, (int)c->max_partials);  // 32 contiguous chunks per CU, one partial each
  hipLaunchKernelGGL(k_stream_read, dim3(g), dim3(FX_BLOCK), 0, c->stream, n2, (const double2 *)c->M.val2, c->partials);
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  for (int i = 0; i < nrepeat; i++)
    hipLaunchKernelGGL(k_stream_read, dim3(g), dim3(FX_BLOCK), 0, c->stream, n2, (const double2 *)c->M.val2, c->partials);
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *gbs = (double)n2 * 16.0 * nrepeat / (ms * 1e-3) / 1e9;
  return 0;
}

// Sizes of the resident structures (for the algorithmic-bytes accounting of bench.py).
// out[0] N, [1] NP, [2] NPL, [3] NPU, [4] M.npairs, [5] M.nblocks, [6] M.nslices,
// [7] ssor.ncolor, [8] L.npairs, [9] L.nblocks, [10] U.npairs, [11] U.nblocks, [12] ssor slices,
// [13] interior / [14] boundary workgroups of the SpMV (domain-decomposed systems)

extern "C" int fx_get_stats(fx_context *c, int64_t out[16]) {
  memset(out, 0, 16 * sizeof(int64_t));
  out[0] = c->A.N; out[1] = c->A.NP; out[2] = c->A.NPL; out[3] = c->A.NPU;
  out[4] = c->M.npairs; out[5] = c->M.nblocks; out[6] = c->M.nslices;
  out[7] = c->ssor.ncolor;
  out[8] = c->ssor.L.npairs; out[9] = c->ssor.L.nblocks; out[10] = c->ssor.U.npairs; out[11] = c->ssor.U.nblocks;
  out[12] = c->ssor.L.nslices;
  out[13] = c->M.n_wg_interior; out[14] = c->M.n_wg_boundary;  // SpMV workgroups overlapped with / ordered after the halo exchange
  out[15] = (c->eis_active ? 1 : 0) | (c->precond_kind == 11 ? 2 : 0) | ((int64_t)(c->df_mode & 3) << 2) | ((int64_t)std::min(c->df_fallbacks, 255) << 8) |
           ((int64_t)c->df_grid_last << 16);   // bit 0: the last Krylov loop ran in Eisenstat's form; bit 1: PRECOND = 1 runs as the natural-order SSOR
  return 0;
}

// The dataflow tail of the Eisenstat sweeps (k_eis_*_df): out[0] first tail colour of the last iteration (ncolor: none), [1] its
// slices, [2] workgroups of its backward launch, [3] tail launches enqueued or captured by this context, [4] colours, [5] the co-resident grid.
extern "C" int fx_eis_tail_stats(fx_context *c, int64_t out[6]) {
  out[0] = c->eis_tail_color0; out[1] = c->eis_tail_slices; out[2] = c->eis_tail_grid; out[3] = c->eis_tail_launches;
  out[4] = c->ssor.ncolor; out[5] = std::min(c->eis_df_grid_max[0], c->eis_df_grid_max[1]);
  return 0;
}

// The ordering the resident multicolour SSOR was built with: perm (new -> old, 1-based) and COLORindex(0:ncolor).
extern "C" int fx_get_ssor_ordering(fx_context *c, int32_t *perm, int32_t *colorindex, int32_t colorindex_cap, int32_t *ncolor) {
  const SsorDev &S = c->ssor;
  if (c->precond_kind != 1 || S.perm.empty()) { g_fx_error = "fx_get_ssor_ordering: no multicolour SSOR resident"; return FX_ERROR_RUNTIME; }
  if ((int32_t)S.colorindex.size() > colorindex_cap) { g_fx_error = "fx_get_ssor_ordering: colorindex too small"; return FX_ERROR_RUNTIME; }
  std::copy(S.perm.begin(), S.perm.end(), perm);
  std::copy(S.colorindex.begin(), S.colorindex.end(), colorindex);
  *ncolor = S.ncolor;
  return 0;
}

#include "fx_assemble_host.h"
#include "fx_update_linear.h"
#include "fx_assemble_groups.h"
#include "fx_heat.h"
#include "fx_dload.h"
#include "fx_nonlinear_host.h"
#include "fx_nodal_stress.h"
#include "fx_debug_host.h"
