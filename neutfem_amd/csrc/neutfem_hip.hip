// neutfem_hip.hip -- C-ABI implementation (include/neutfem_hip.h) over the gfx950 kernels.
//
// Host logic mirrors the reference's control flow (NeutFEM::SolveKeff / SolveCoarse /
// SchurSolver::Solve) while every vector stays resident in HBM; per outer iteration the host
// reads back 4 doubles, per CG solve one small struct every few iterations.
//
// Multi-GPU: the mesh is cut into z-slabs.  A "team" is the set of slabs of one global problem that
// live in this process (one per GPU in production; several on one GPU in the loopback used for
// testing) plus an RCCL communicator to the slabs of the other processes.  Every phase of the solve
// loops over the local slabs; the only data-path communication is (i) one plane of fp64 per slab
// interface per Schur apply (partition method for the z-line solves) and (ii) all-reduces of 1-3
// scalars, all enqueued on the team's stream -- the host never waits for them.
#include "../../include/neutfem_hip.h"
#include "nf_kernels.h"
#include "nf_assembly.h"
#include "nf_line_groups.h"
#include "nf_options.h"
#include "nf_resident_lanes.h"
#include "nf_small_eig.h"
#include "nf_xsol_ring.h"

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using namespace nf;

static thread_local std::string g_err;
static int fail(int code, const char *fmt, ...)
{
    char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf; return code;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(NF_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define NFCHK(x) do { int r_ = (x); if (r_ != NF_OK) return r_; } while (0)

static_assert(NF_OPT_RED_GRID == 1024, "nf_options.h: defaults and cap of the reduction-shaped grids follow RED_GRID");
static const int RED_GRID = 1024;          // fixed grid of the streaming/reduction kernels
static const int MAX_LOCAL_SLABS = 16;

// event-timed launches of one pass.  Launches queued behind a converged CG solve exit at once (CgScalars::done): they are no
// work and must not dilute the average, and an occasional preempted launch must not distort it either, so the figures are
// taken over the samples of at least a quarter of the MEDIAN duration.
struct ProfSlot {
    std::vector<float> samples;
    void stats(long *count, double *ms, long *skipped) const
    {
        *count = 0; *ms = 0.0; *skipped = 0;
        if (samples.empty()) return;
        std::vector<float> v(samples); std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
        const double thr = 0.25 * v[v.size() / 2];
        for (float x : samples) { if (x < thr) ++*skipped; else { ++*count; *ms += x; } }
    }
};

// ---- RCCL, resolved lazily with dlopen so that single-GPU use never loads it -------------------
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(ncclUniqueId *) = nullptr;
    int (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*CommAbort)(ncclComm_t) = nullptr;          // optional: used when a peer stops answering (comm_timeout_s)
    int (*CommCount)(const ncclComm_t, int *) = nullptr;   // optional: nf_comm_info reports what the LIVE communicator says, not what the launcher claimed
    char path[512] = { 0 };                          // file the symbols were actually resolved from (dladdr)
};
static Rccl g_rccl;
// NEUTFEM_TRACE_COMM=1: one line on stderr per collective this rank issues (debugging the order of collectives across ranks)
static bool trace_comm() { static int on = -1; if (on < 0) { const char *e = getenv("NEUTFEM_TRACE_COMM"); on = e && atoi(e) ? 1 : 0; } return on == 1; }
#define TRACE_COMM(...) do { if (trace_comm()) { fprintf(stderr, "[comm] " __VA_ARGS__); fputc('\n', stderr); } } while (0)
static const int NCCL_DOUBLE = 8, NCCL_SUM = 0, NCCL_MAX = 2;   // ncclFloat64 / ncclSum / ncclMax in rccl.h
#define NCCLCHK(x) do { int r_ = (x); if (r_ != 0) return fail(NF_ERR_HIP, "%s failed: %s", #x, g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "rccl error"); } while (0)

static int rccl_load()
{
    if (g_rccl.lib) return NF_OK;
    // the ROCm install this library was built against first; symbols are taken from THIS handle only (dlsym), so a
    // second RCCL copy that a framework may have mapped (e.g. the one bundled with PyTorch) is never mixed in
    const char *env = getenv("NEUTFEM_RCCL_LIB");
    const char *names[] = { env ? env : "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so" };
    for (const char *n : names) { g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (g_rccl.lib) break; }
    if (!g_rccl.lib) return fail(NF_ERR_HIP, "cannot load librccl.so: %s", dlerror());
#define SYM(field, name) do { *(void **)(&g_rccl.field) = dlsym(g_rccl.lib, name); if (!g_rccl.field) return fail(NF_ERR_HIP, "librccl.so lacks %s", name); } while (0)
    SYM(GetUniqueId, "ncclGetUniqueId"); SYM(CommInitRank, "ncclCommInitRank"); SYM(CommDestroy, "ncclCommDestroy");
    SYM(AllReduce, "ncclAllReduce"); SYM(Send, "ncclSend"); SYM(Recv, "ncclRecv"); SYM(GroupStart, "ncclGroupStart");
    SYM(GroupEnd, "ncclGroupEnd"); SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    *(void **)(&g_rccl.CommAbort) = dlsym(g_rccl.lib, "ncclCommAbort");
    *(void **)(&g_rccl.CommCount) = dlsym(g_rccl.lib, "ncclCommCount");
    Dl_info di;
    if (dladdr((void *)g_rccl.AllReduce, &di) && di.dli_fname) snprintf(g_rccl.path, sizeof g_rccl.path, "%s", di.dli_fname);
    return NF_OK;
}

struct nf_solver;
struct Transient;                                                 // the running transient of a handle (nf_transient_begin), defined with its code
struct nf_team {
    NfOptions opt;                       // what nf_set_option sets (nf_options.h); team_copy_options hands it to the team of a derived handle
    std::vector<nf_solver *> slabs;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;   // interface planes travel here while the x / y passes run on `stream`
    // small slabs (a rank's share at strong-scaling sizes): a pass on 2 M cells does not fill the chip, so the y pass runs BESIDE the x
    // pass on a stream of its own, into its own vector; the accumulation pass of the z lines adds the two (SlabArgs::yadd)
    hipStream_t y_stream = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_z1 = nullptr, ev_xchg = nullptr;
    int nproc = 1, rank = 0;
    ncclComm_t comm = nullptr;
    ncclComm_t comm_x = nullptr;    // option "xchg_comm": the communicator of the interface planes (created collectively in team_prepare)
    int last_cg_reductions = 0; long team_max_cells = 0;   // single-reduction CG on slab teams (option "cg_single_reduce"): all-reduces per iteration of the last solve, largest slab of the team
    int last_cg_form = 0;           // the CgForm the last cg_solve ran (nf_info "cg_form")
    int last_endpoint_w = 0;        // its endpoint pass ran as two weighted sums per line (option "endpoint_weights")
    bool rccl_reduce = false;       // scalar reductions go through ncclAllReduce (nproc > 1, or forced for testing)
    double *d_partials = nullptr; long partial_stride = 0, slab_cap = 0;
    CgScalars *d_cg = nullptr;
    double *d_ah = nullptr;                   // alpha history of the scalar-backed CG forms (cg_logic): 8 doubles
    double *d_out = nullptr;        // 4 doubles read by the host each outer
    double *d_red = nullptr;        // 8 doubles: process-local sums awaiting the all-reduce, each followed by this rank's error flag
    // A rank that fails locally inside a solve must not leave the others waiting in the next collective:
    // it raises d_errsrc (k_finalize appends it to every reduction that crosses ranks; the consumers stop every rank with
    // CgScalars::err), keeps issuing the collectives of the schedule without the compute ("poisoned"), and returns its own error
    // once the flag has come back; the other ranks return NF_ERR_REMOTE at the same iteration.
    double *d_errsrc = nullptr;     // 1 double, 0 = fine
    // Vector reduce (multi-rank, one slab per rank, equal slab shapes): the block partials of p.q and |r|^2 are all-reduced as they are
    // (a few KB: still latency-bound) into d_vec and the consuming kernels sum them, every block redundantly, like the lean CG of an
    // undivided mesh -- the two one-block k_finalize launches per CG iteration leave the critical path (7 -> 5 kernels per rank).
    double *d_vec = nullptr; long vec_stride = 0;          // 2 rows: all-reduced p.q partials, all-reduced |r|^2 partials (+ flag slot each)
    int vec_cnt_pq = 0, vec_cnt_rr = 0; bool vec_ok = false; int last_vec_reduce = 0;
    bool dead = false;              // a collective timed out (NF_ERR_COMM): the streams may hold operations that never complete -- no further solve, no stream waits at teardown
    bool poisoned = false; int poison_rc = 0; char poison_msg[256] = { 0 };
    int xchg_in_apply = 0;          // interface exchanges issued since the current Schur apply began
    long cg_iter_total = 0;         // CG iterations launched since the team was created (NEUTFEM_INJECT_FAIL=<rank>:<iteration>)
    int inject_rank = -1; long inject_iter = -1;
    int inject_outer = -1; char inject_where = 0;   // NEUTFEM_INJECT_FAIL=<rank>:o<n> / :e<n> (start / end of outer n, outside the CG loop), :a (next exchange-only collective)
    double comm_timeout_s = 120.0;  // multi-rank teams: a stream that does not drain for this long means a peer is gone (NEUTFEM_COMM_TIMEOUT_S)
    nf_progress_fn progress_fn = nullptr; void *progress_user = nullptr;   // nf_set_progress_callback
    volatile long outers_done = 0;  // completed outer iterations of the running / last SolveKeff (bench.py's watchdog polls it from another thread)
    bool linked_ready = false;      // separator diagonals exchanged
    int sep_sweeps = 0;             // Jacobi sweeps on the separator system (0: slabs thick enough for it to be diagonal to rounding)
    std::vector<int> last_its;
    // stats of the last SolveKeff
    int last_outer = 0, coarse_outer = 0; long last_cg_total = 0;
    std::vector<double> hist_k, hist_dk, hist_dphi; std::vector<int> hist_cg;
    int has_valid_keff = 0; double last_keff = 1.0;
    // profiling
    HostPub *h_pub = nullptr, *d_pub = nullptr; unsigned long long pub_seq = 0;   // low-latency scalar readback (k_publish, option "host_pub")
    bool profile = false; long prof_tick = 0;   // event-timed launches: every prof_every-th Schur apply of a profiled solve
    std::map<std::string, ProfSlot> prof;
    struct Ev { hipEvent_t a, b; int slot; };
    std::vector<Ev> ev_pending; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_free;
    OuterState *d_ost = nullptr; double *d_hist = nullptr; int hist_cap = 0;   // device-resident outer loop (diagonal path)
    int ncu = 256;                                        // compute units of the device (a staged launch of s_stage_grid 0 takes one block each)
    size_t lds_limit = 160 * 1024;                        // dynamic LDS a block may ask for (hipDeviceAttributeMaxSharedMemoryPerBlock at team creation)
    int last_xcd = 0; long xcd_solves = 0, xcd_refused = 0;   // one-XCD CG (k_cg_xcd, option "cg_xcd"): the last solve took it; solves / refused launches so far
    XcdState *d_xcd = nullptr; double *d_xpart = nullptr;
    int last_resident_serial = 0;                         // whole SolveKeff in one workgroup (k_resident_keff): the last one ran its serial variant
    int *d_hist_cg = nullptr; int hist_cg_cap = 0; ResidentOut *d_rout = nullptr;
    ResidentArgs *d_batch_args = nullptr; int batch_cap = 0; long batch_launches = 0;   // nf_solve_keff_batch with this team's handle first: one struct per workgroup (grow-only), launches so far
    int last_path = 0;                                    // 0 host-driven outer loop, 1 diagonal device loop, 2 resident kernel, 3 one-XCD kernel (nf_info "last_path")
    int last_direct = 0;                                  // the last solve used: 0 CG as configured, 1 dense S^-1, 2 CG to 1e-14 standing in
    long standin_unconverged = 0;                         // group solves of the stand-in that ended above 1e-14
    // coarse twin of the team (SolveCoarse): built on the first coarse-mesh start and kept until the cross sections, the boundary
    // conditions or the team change -- creating and factoring it costs more than solving it on the benchmark meshes
    std::vector<nf_solver *> cc; int cc_f[3] = {0, 0, 0};
};

struct nf_solver {
    int device = 0;
    nf_team *team = nullptr;
    int slab_index = 0;
    int if_lo = 0, if_hi = 0;                            // interface with the slab below / above (z)
    // mesh (of this slab)
    int dim = 1, nx = 1, ny = 1, nz = 1, ng = 1, k = 0, m = 0;
    int n1 = 1, nloc = 1, nb = 0;                        // P moments per axis, per cell; bubble moments present in P_m
    long N = 0, nphi = 0, nJ = 0, nJx = 0, nJy = 0, nJz = 0;   // nphi = nloc * N DOFs per group (device layout [p][e])
    std::vector<double> xb, yb, zb, hx, hy, hz;
    double *d_hx = nullptr, *d_hy = nullptr, *d_hz = nullptr, *d_xb = nullptr, *d_yb = nullptr, *d_zb = nullptr;
    int bc_set[8] = {0}, bc_type[8] = {0};
    // XS on device (reference layouts)
    double *d_D = nullptr, *d_SigR = nullptr, *d_NSF = nullptr, *d_Chi = nullptr;
    std::vector<double *> d_SigS;          // ng*ng blocks [g_to*ng+g_from], nullptr when all |s| <= 1e-14
    bool xs_uploaded = false, built = false, diag_valid = false;
    // nf_set_void: cells cut out of the domain (device bytes, nullptr = no mask; the host copy for nf_get_void), J.n = void_gamma phi on kept|void faces
    unsigned char *d_void = nullptr; std::vector<unsigned char> void_host; double void_gamma = 0.0; long void_cells = 0;
    // operators
    double *d_Cd = nullptr, *d_Mf = nullptr, *d_Mchi = nullptr;   // ng*nphi diagonals: C, fission, chi-weighted mass (adjoint)
    double *d_phi_adj = nullptr;                        // adjoint flux, ng*nphi (allocated by the first adjoint solve)
    double *d_modes[2] = {nullptr, nullptr}; int modes_n[2] = {0, 0}, modes_cap[2] = {0, 0};   // lambda-modes of the last nf_solve_modes (direct / adjoint), modes_n * ng*nphi
    int has_valid_adjoint = 0; double last_keff_adj = 1.0;
    // nf_solve_gpt: the generalized adjoint Gamma+ (ng*nphi; gpt_valid: it holds a finished solve or an nf_set_gamma), the two weight fields
    // (2 * ng*N, [w_a | w_b]; nullptr before the first solve) and the device scalars of the last solve (GPT_SLOTS; <w_a,phi>, <w_b,phi> first)
    double *d_gamma = nullptr, *d_gpt_w = nullptr, *d_gpt_sc = nullptr; bool gpt_valid = false;
    std::vector<double *> d_Ms;                          // ng*ng
    const double **d_Ms_tab = nullptr;                   // the same ng*ng pointers on the device (resident kernel)
    double *d_L[3] = {nullptr, nullptr, nullptr}, *d_DR[3] = {nullptr, nullptr, nullptr}, *d_D0[3] = {nullptr, nullptr, nullptr};
    long nlines[3] = {0, 0, 0};
    // tables of distinct lines, built on first need (line_dict_prepare) and dropped with the factors: ids [ng][nlines] and, per group, the
    // rows of L, 1/d (and the C diagonal, x) at ld_off[d][g] doubles into d_ltab[d]; ld_rows: distinct lines per group
    bool ld_tried = false, ld_use[3] = {false, false, false}; int ld_rejected = 0, ld_pitch[3] = {0, 0, 0};
    int *d_lid[3] = {nullptr, nullptr, nullptr}; double *d_ltab[3] = {nullptr, nullptr, nullptr};
    std::vector<long> ld_off[3]; std::vector<int> ld_rows[3]; size_t ld_bytes = 0;
    double *d_Sinv = nullptr;
    double *d_Sdense = nullptr; bool dense_valid = false;   // explicit-S branch: S^-1 per group, ng * nphi^2, column-major
    // slab interfaces (partition method for the z lines), all per z-line
    double *d_alo = nullptr, *d_ahi = nullptr, *d_hlo = nullptr, *d_hhi = nullptr, *d_gfl = nullptr;   // ng * nlines[2]
    double *d_sinv_lo = nullptr, *d_sinv_hi = nullptr;  // ng * nlines[2]
    double *d_clo = nullptr, *d_chi = nullptr, *d_rlo = nullptr, *d_rhi = nullptr, *d_ulo = nullptr, *d_uhi = nullptr;
    double *d_ctlo = nullptr, *d_cthi = nullptr, *d_elo = nullptr, *d_ehi = nullptr, *d_relo = nullptr, *d_rehi = nullptr;   // separator sweeps (thin slabs)
    double *d_Wlo = nullptr, *d_Whi = nullptr; bool w_valid = false;   // endpoint functionals of the z lines (k_endpoint_w), ng * N each
    // state
    double *d_phi = nullptr, *d_raw = nullptr;          // current iterate / raw group solutions, ng*N
    double *d_p0 = nullptr, *d_p1 = nullptr;            // Chebyshev history
    double *d_tf = nullptr, *d_rhs = nullptr, *d_r = nullptr, *d_p = nullptr, *d_q = nullptr;
    // batched x_sol update of the fused CG (CgFuse, nf_xsol_ring.h): slots 1 .. ring_m-1 of the ring of directions (slot 0 is d_p), nphi doubles each,
    // shared by all groups; ring_refused: the device had no room for them, this handle stays with one buffer
    double *d_ring = nullptr; int ring_m = 0; bool ring_refused = false;
    double *d_p2 = nullptr, *d_qy = nullptr, *d_qz = nullptr;   // fused-direction CG (k_apply3): second buffer of the p pair, y / z outputs
    bool raw_valid = false, raw_is_diag = false;
    double *d_qsrc = nullptr;                           // external source as a load vector, ng * nphi (nf_upload_source, k_source_q)
    double src_total = 0.0; bool src_any = false;       // sum of Q |e| over the slab's cells, some Q != 0
    Transient *tr = nullptr; long build_gen = 0;        // nf_transient_begin's state; nf_build calls so far (the step operator follows them)
    long tr_rebuilds = 0;                               // builds of the step operator since the handle was created (nf_info "transient_rebuilds")
    int opt_tr_rebalance = 1;                           // option "transient_rebalance"
    double *d_Jz = nullptr; bool jz_valid = false;      // slabs: z currents of the last solve, ng * nJz face DOFs (nf_get_J)
    double *d_Jzb = nullptr;                            // slabs, RT1+: z bubbles of the local cells, ng * N * ni
    // CMFD (include/NeutFEM.hpp:119-143): D~ / D^ per direction (ng * faces), PCG work vectors, scalars
    bool cmfd_init = false, cmfd_iface = false; double cmfd_relax = 1.0;
    double *d_Dt[3] = {nullptr, nullptr, nullptr}, *d_Dh[3] = {nullptr, nullptr, nullptr}; long nfc[3] = {0, 0, 0};
    double *d_cm = nullptr, *d_cmJ = nullptr; CmfdScalars *d_cmsc = nullptr;
    int cmfd_last_its = 0;
};

const char *nf_last_error(void) { return g_err.c_str(); }

static void coarse_cache_drop(nf_team *T)
{
    if (!T || T->cc.empty()) return;
    std::string keep = g_err;
    std::vector<nf_solver *> cc; cc.swap(T->cc);
    for (int i = (int)cc.size() - 1; i >= 0; --i) if (cc[i]) nf_destroy(cc[i]);
    g_err = keep;
}

int nf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

template <class T> static int dalloc(T **p, size_t n)
{
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    HIPCHK(hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T)));
    return NF_OK;
}
template <class T> static void dfree(T *&p) { if (p) { (void)hipFree(p); p = nullptr; } }
// scratch device buffer of one function call: released on every return path
template <class T> struct DevTmp { T *p = nullptr; ~DevTmp() { if (p) (void)hipFree(p); } DevTmp() = default; DevTmp(const DevTmp &) = delete; DevTmp &operator=(const DevTmp &) = delete; };

// the tables of distinct lines go with the factors they were taken from (nf_build, nf_upload_xs, nf_set_bc) and with the options that shaped them
static void line_dict_drop(nf_solver *S)
{
    if (S->team && S->team->stream && (S->d_lid[0] || S->d_lid[1] || S->d_lid[2])) (void)hipStreamSynchronize(S->team->stream);
    for (int d = 0; d < 3; ++d) { dfree(S->d_lid[d]); dfree(S->d_ltab[d]); S->ld_use[d] = false; S->ld_pitch[d] = 0; S->ld_off[d].clear(); S->ld_rows[d].clear(); }
    S->ld_tried = false; S->ld_rejected = 0; S->ld_bytes = 0;
}

static void modes_drop(nf_solver *S);
static void gpt_drop(nf_solver *S);
static void transient_drop(nf_solver *S);
static bool team_is_single(const nf_team *T);

// nf_set_void.  The vector kernels of the CG come in two instantiations: launch(std::true_type, mask) on a masked handle, else
// launch(std::false_type, {}) -- the code without a mask.
template <class F> static void with_void(const nf_solver *S, F &&launch)
{
    if (S->d_void) launch(std::true_type{}, VoidMask{ S->d_void, S->N }); else launch(std::false_type{}, VoidMask{ nullptr, 0 });
}
// The calls that form A_ff themselves or build a twin handle that would not carry the mask, and the solves whose exact twins know no mask
static int void_refuse(const nf_solver *S, const char *who)
{
    if (S) for (const nf_solver *X : S->team->slabs) if (X->d_void)
        return fail(NF_ERR_UNSUPPORTED, "%s: not supported on a handle with cut-out cells (nf_set_void); remove the mask with nf_set_void(h, NULL, 0) and build again", who);
    return NF_OK;
}
static long transient_steps(const nf_solver *S);

static const char *SLOT_NAMES[5] = { "schur_x", "schur_y", "schur_z", "schur_apply", "schur_z1" };

static Geom make_geom(const nf_solver *S)
{
    Geom G; G.dim = S->dim; G.nx = S->nx; G.ny = S->ny; G.nz = S->nz; G.k = S->k; G.hx = S->d_hx; G.hy = S->d_hy; G.hz = S->d_hz;
    G.T0 = (double)(1 << (S->dim - 1));
    // face block of the 1-D element matrix after condensing the k bubbles (exact values of the reference's Gauss
    // quadrature, src/FEM.cpp:891-924): M^FF - M^Fb (M^bb)^-1 M^bF
    if (S->k == 0) { G.aLL = 2.0 / 3.0; G.aLR = 1.0 / 3.0; }
    else if (S->k == 1) { G.aLL = 1.0 / 4.0; G.aLR = -1.0 / 12.0; }
    else { G.aLL = 2.0 / 15.0; G.aLR = 1.0 / 30.0; }
    // GetBoundaryAttribute, src/NeutFEM.cpp:2338-2347
    for (int d = 0; d < 3; ++d) {
        int lo, hi;
        if (S->dim == 1) { lo = 1; hi = 2; }
        else if (S->dim == 2) { if (d == 0) { lo = 1; hi = 2; } else { lo = 4; hi = 3; } }
        else { if (d == 0) { lo = 3; hi = 4; } else if (d == 1) { lo = 6; hi = 5; } else { lo = 1; hi = 2; } }
        G.dir_lo[d] = S->bc_set[lo] && S->bc_type[lo] == NF_BC_DIRICHLET;
        G.dir_hi[d] = S->bc_set[hi] && S->bc_type[hi] == NF_BC_DIRICHLET;
    }
    if (S->if_lo) G.dir_lo[2] = 0;             // a slab interface is not a domain boundary
    if (S->if_hi) G.dir_hi[2] = 0;
    return G;
}

static int grid_for(long n, int block = 256, int cap = RED_GRID)
{
    long g = (n + block - 1) / block; if (g < 1) g = 1; if (g > cap) g = cap; return (int)g;
}

// transverse Legendre modes of one direction that couple to phi: a in [0,m]^(dim-1)
static int n_modes(const nf_solver *S) { int n = 1; for (int t = 1; t < S->dim; ++t) n *= S->n1; return n; }
// moment index p = i_x + n1 i_y + n1^2 i_z of (along-index i, transverse mode `mode`) for direction d, and T_a
static int moment_index(const nf_solver *S, int d, int mode, int i, double *Ta)
{
    const int n1 = S->n1;
    int idx[3] = {0, 0, 0}; double ta = 1.0; int q = mode;
    for (int t = 0; t < S->dim; ++t) {
        if (t == d) { idx[t] = i; continue; }
        idx[t] = q % n1; q /= n1;
        ta *= 2.0 / (2.0 * idx[t] + 1.0);
    }
    if (Ta) *Ta = ta;
    return idx[0] + n1 * idx[1] + n1 * n1 * idx[2];
}
// per-pass constants + moment pointers (ModeArgs) for direction d, mode `mode`; xb/yb: SoA vectors of nphi doubles
static ModeArgs mode_args(const nf_solver *S, int g, int d, int mode, const double *xb, double *yb)
{
    ModeArgs ma; memset(&ma, 0, sizeof ma);
    double Ta = 1.0;
    for (int i = 0; i <= S->nb; ++i) {
        const int p = moment_index(S, d, mode, i, &Ta);
        ma.x[i] = xb + (long)p * S->N; ma.y[i] = yb + (long)p * S->N; ma.Cd[i] = S->d_Cd + (long)g * S->nphi + (long)p * S->N;
    }
    ma.Ta = Ta; ma.dir = d; ma.D = S->d_D + (long)g * S->N;
    // bubble l: eL/eR = M^Fb_{L/R,l} / M^bb_l, Gc = int P_{l+1} d/dxi[(1-xi^2) P_l], iM = 1 / M^bb_l  (src/FEM.cpp:377-620)
    ma.eL[0] = 5.0 / 8.0; ma.eR[0] = 5.0 / 8.0; ma.Gc[0] = -4.0 / 3.0; ma.iM[0] = 15.0 / 16.0;
    ma.eL[1] = -7.0 / 8.0; ma.eR[1] = 7.0 / 8.0; ma.Gc[1] = -4.0 / 5.0; ma.iM[1] = 105.0 / 16.0;
    return ma;
}
// every transverse mode of direction d relative to mode 0 (ModeTab): T_a and moment offsets
static ModeTab mode_tab(const nf_solver *S, int d)
{
    ModeTab mt; memset(&mt, 0, sizeof mt);
    mt.n = n_modes(S);
    for (int m = 0; m < mt.n; ++m)
        for (int i = 0; i <= S->nb; ++i) {
            double Ta = 1.0;
            const int p = moment_index(S, d, m, i, &Ta), p0 = moment_index(S, d, 0, i, nullptr);
            mt.Ta[m] = Ta; mt.doff[m][i] = (long)(p - p0) * S->N;
        }
    return mt;
}

// ---- team management ---------------------------------------------------------------------------
static long slab_partial_need(const nf_solver *S)
{
    // the fused-direction launch (k_apply3) writes one partial per x, y and z block of the same launch
    return (std::max<long>(RED_GRID, S->nlines[0] + (long)((S->nx + 7) / 8) * ((long)S->ny + S->nz)) + 16) * n_modes(S);
}
static int team_alloc(nf_team *T)
{
    long cap = 0;
    for (auto *S : T->slabs) cap = std::max(cap, slab_partial_need(S));
    T->slab_cap = cap; T->partial_stride = cap * (long)T->slabs.size();
    NFCHK(dalloc(&T->d_partials, (size_t)T->partial_stride * 4));
    if (!T->d_cg) NFCHK(dalloc(&T->d_cg, 1));
    if (!T->d_ah) { NFCHK(dalloc(&T->d_ah, 8)); HIPCHK(hipMemset(T->d_ah, 0, 8 * sizeof(double))); }
    if (!T->d_out) NFCHK(dalloc(&T->d_out, 8));
    if (!T->d_red) NFCHK(dalloc(&T->d_red, 8));
    if (!T->d_errsrc) { NFCHK(dalloc(&T->d_errsrc, 1)); HIPCHK(hipMemset(T->d_errsrc, 0, sizeof(double))); }
    // NEUTFEM_INJECT_FAIL=<rank>:<iteration>[:<min local DOFs per cell>] (tests): the optional third field keeps the injection away from
    // the RT0-P0 coarse twin of a higher-order team, so that the non-lean reduction route of RT1 / RT2 teams is the one that is hit
    if (const char *e = getenv("NEUTFEM_INJECT_FAIL")) {
        int r = -1, ml = 0; long it = -1; char w = 0; int on = -1;
        if (sscanf(e, "%d:%c%d", &r, &w, &on) >= 2 && (w == 'o' || w == 'e' || w == 'a')) { T->inject_rank = r; T->inject_where = w; T->inject_outer = on; }
        else {
            const int nf = sscanf(e, "%d:%ld:%d", &r, &it, &ml);
            if (nf >= 2 && (nf < 3 || T->slabs.empty() || T->slabs[0]->nloc >= ml)) { T->inject_rank = r; T->inject_iter = it; }
        }
    }
    if (const char *e = getenv("NEUTFEM_COMM_TIMEOUT_S")) { const double v = atof(e); if (v > 0) T->comm_timeout_s = v; }
    T->last_its.assign(64, 0);
    return NF_OK;
}
static void team_free(nf_team *T)
{
    if (!T) return;
    (void)hipSetDevice(T->device);
    if (T->dead) {
        // after NF_ERR_COMM the streams hold collectives whose peers are gone: waiting for them, destroying them or the communicator can
        // block for ever.  Everything of this team is left to the process exit, which the caller owes anyway (include/neutfem_hip.h).
        delete T;
        return;
    }
    if (T->stream) (void)hipStreamSynchronize(T->stream);
    for (auto &e : T->ev_pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto &e : T->ev_free) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (T->comm_x && g_rccl.CommDestroy) g_rccl.CommDestroy(T->comm_x);
    if (T->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(T->comm);
    if (T->d_xcd) (void)hipFree(T->d_xcd);
    dfree(T->d_xpart);
    dfree(T->d_partials); dfree(T->d_cg); dfree(T->d_ah); dfree(T->d_out); dfree(T->d_red); dfree(T->d_errsrc); dfree(T->d_vec); dfree(T->d_ost); dfree(T->d_hist); dfree(T->d_hist_cg); dfree(T->d_rout); dfree(T->d_batch_args);
    if (T->h_pub) (void)hipHostFree(T->h_pub);
    if (T->comm_stream) { (void)hipStreamSynchronize(T->comm_stream); (void)hipStreamDestroy(T->comm_stream); }
    if (T->y_stream) { (void)hipStreamSynchronize(T->y_stream); (void)hipStreamDestroy(T->y_stream); }
    if (T->ev_fork) (void)hipEventDestroy(T->ev_fork);
    if (T->ev_join) (void)hipEventDestroy(T->ev_join);
    if (T->ev_z1) (void)hipEventDestroy(T->ev_z1);
    if (T->ev_xchg) (void)hipEventDestroy(T->ev_xchg);
    if (T->stream) (void)hipStreamDestroy(T->stream);
    delete T;
}
static PartSegs segs_for(const nf_team *T, const std::vector<int> &counts)
{
    PartSegs ps; ps.n = (int)T->slabs.size();
    for (int i = 0; i < ps.n; ++i) { ps.off[i] = (int)(i * T->slab_cap); ps.cnt[i] = counts[i]; }
    return ps;
}

static int create_impl(int rt_order, int p_order, int ng, int nxb, const double *xb, int nyb, const double *yb, int nzb,
                       const double *zb, int if_lo, int if_hi, int device, nf_handle *out)
{
    if (!out || !xb || nxb < 2 || ng < 1 || ng > 64) return fail(NF_ERR_ARG, "nf_create: bad arguments");
    int k = std::min(rt_order, 2), m = std::min(p_order, 2);
    if (k < m) m = k;                                            // src/NeutFEM.cpp:149-169
    int ndev = nf_device_count();
    if (ndev <= 0) return fail(NF_ERR_NO_DEVICE, "nf_create: no HIP device visible (the gfx950 path has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(NF_ERR_ARG, "nf_create: device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    nf_solver *S = new nf_solver();
    S->device = device; S->k = k; S->m = m; S->ng = ng; S->if_lo = if_lo; S->if_hi = if_hi;
    S->xb.assign(xb, xb + nxb);
    if (nyb > 1) S->yb.assign(yb, yb + nyb); else S->yb.assign(1, nyb == 1 && yb ? yb[0] : 0.0);
    if (nzb > 1) S->zb.assign(zb, zb + nzb); else S->zb.assign(1, nzb == 1 && zb ? zb[0] : 0.0);
    S->nx = nxb - 1; S->ny = nyb > 1 ? nyb - 1 : 1; S->nz = nzb > 1 ? nzb - 1 : 1;
    S->dim = S->nz > 1 ? 3 : (S->ny > 1 ? 2 : 1);               // src/FEM.cpp:33-35
    if ((if_lo || if_hi) && (S->dim != 3 || S->nz < 3)) { delete S; return fail(NF_ERR_ARG, "a slab needs a 3D mesh with at least 3 z-planes"); }
    // a 3D mesh reads y_breaks(i+1) - y_breaks(i) (src/FEM.cpp:43-47): one y cell still needs its two breaks (Eigen asserts there)
    if (S->dim == 3 && (nyb < 2 || !yb)) { delete S; return fail(NF_ERR_ARG, "nf_create: a 3D mesh needs at least 2 y breaks (got %d)", nyb); }
    S->N = (long)S->nx * S->ny * S->nz;
    S->n1 = m + 1; S->nloc = 1; for (int t = 0; t < S->dim; ++t) S->nloc *= S->n1;
    S->nphi = S->N * S->nloc; S->nb = std::min(k, m);
    S->hx.resize(S->nx); S->hy.assign(S->ny, 1.0); S->hz.assign(S->nz, 1.0);
    for (int i = 0; i < S->nx; ++i) S->hx[i] = xb[i + 1] - xb[i];
    if (S->dim >= 2) for (int i = 0; i < S->ny; ++i) S->hy[i] = yb[i + 1] - yb[i];
    if (S->dim == 3) for (int i = 0; i < S->nz; ++i) S->hz[i] = zb[i + 1] - zb[i];
    for (auto *h : { &S->hx, &S->hy, &S->hz })
        for (double v : *h)
            if (!(v > 0.0) || !std::isfinite(v)) { delete S; return fail(NF_ERR_ARG, "nf_create: mesh breaks must be finite and strictly increasing (cell width %g)", v); }
    {                                                            // src/FEM.cpp:177-259
        int nf = 1, ni = k; for (int t = 1; t < S->dim; ++t) { nf *= k + 1; ni *= k + 1; }
        S->nJx = (long)(S->nx + 1) * S->ny * S->nz * nf;
        S->nJy = S->dim >= 2 ? (long)S->nx * (S->ny + 1) * S->nz * nf : 0;
        S->nJz = S->dim == 3 ? (long)S->nx * S->ny * (S->nz + 1) * nf : 0;
        S->nJ = S->nJx + S->nJy + S->nJz + S->N * S->dim * ni;
    }
    S->nlines[0] = (long)S->ny * S->nz; S->nlines[1] = (long)S->nx * S->nz; S->nlines[2] = (long)S->nx * S->ny;
    nf_team *T = new nf_team();
    T->device = device; T->slabs.push_back(S); S->team = T; S->slab_index = 0;
    {   // dynamic LDS a workgroup may ask for on this device (gfx950: 160 KiB); the LDS-resident paths plan against it and step aside when it is smaller
        int a = 0, b = 0;
        if (hipDeviceGetAttribute(&a, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) a = 0;
        if (hipDeviceGetAttribute(&b, hipDeviceAttributeSharedMemPerBlockOptin, device) != hipSuccess) b = 0;
        (void)hipGetLastError();
        T->lds_limit = (size_t)std::max(std::max(a, b), 64 * 1024);
        if (hipDeviceGetAttribute(&a, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && a > 0) T->ncu = a;
        (void)hipGetLastError();
    }
    const char *cb = getenv("NEUTFEM_CG_BATCH"); T->opt.cg_batch = cb ? atoi(cb) : 0;
    *out = S;
    int rc = NF_OK;
    // NEUTFEM_OPTS="key=value,key=value": nf_set_option on every handle at creation (A/B runs of programs that do not expose the options,
    // e.g. bench.py with slab teams); unknown keys are reported once on stderr
    if (const char *e = getenv("NEUTFEM_OPTS")) {
        std::string all(e); size_t pos = 0;
        while (pos < all.size()) {
            const size_t c = all.find(',', pos); const std::string kv = all.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
            const size_t eq = kv.find('=');
            if (eq != std::string::npos && nf_set_option(S, kv.substr(0, eq).c_str(), atol(kv.c_str() + eq + 1)) != NF_OK) fprintf(stderr, "NEUTFEM_OPTS: %s\n", nf_last_error());
            if (c == std::string::npos) break;
            pos = c + 1;
        }
    }
    auto up = [&](double **d, const std::vector<double> &h) {
        if (rc != NF_OK) return;
        rc = dalloc(d, h.size());
        if (rc == NF_OK && hipMemcpy(*d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(NF_ERR_HIP, "nf_create: upload failed");
    };
    if (hipStreamCreateWithFlags(&T->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(NF_ERR_HIP, "hipStreamCreate failed");
    if (rc == NF_OK && (if_lo || if_hi)) {
        if (hipStreamCreateWithFlags(&T->comm_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&T->ev_z1, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&T->ev_xchg, hipEventDisableTiming) != hipSuccess ||
            hipStreamCreateWithFlags(&T->y_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&T->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&T->ev_join, hipEventDisableTiming) != hipSuccess) rc = fail(NF_ERR_HIP, "comm stream / event creation failed");
    }
    up(&S->d_hx, S->hx); up(&S->d_hy, S->hy); up(&S->d_hz, S->hz); up(&S->d_xb, S->xb); up(&S->d_yb, S->yb); up(&S->d_zb, S->zb);
    const size_t NN = (size_t)S->nphi * ng;
    if (rc == NF_OK) rc = dalloc(&S->d_phi, NN);
    if (rc == NF_OK) rc = dalloc(&S->d_raw, NN);
    if (rc == NF_OK) rc = dalloc(&S->d_tf, S->nphi);
    if (rc == NF_OK) rc = dalloc(&S->d_rhs, S->nphi);
    if (rc == NF_OK) rc = dalloc(&S->d_r, S->nphi);
    if (rc == NF_OK) rc = dalloc(&S->d_p, S->nphi);
    if (rc == NF_OK) rc = dalloc(&S->d_q, S->nphi);
    if (rc == NF_OK && (if_lo || if_hi)) {
        const size_t nl = (size_t)S->nlines[2] * n_modes(S);          // exchange planes: [transverse mode][line]
        double **arrs[] = { &S->d_clo, &S->d_chi, &S->d_rlo, &S->d_rhi, &S->d_ulo, &S->d_uhi, &S->d_ctlo, &S->d_cthi, &S->d_elo, &S->d_ehi, &S->d_relo, &S->d_rehi };
        for (auto a : arrs) if (rc == NF_OK) { rc = dalloc(a, nl); if (rc == NF_OK) (void)hipMemset(*a, 0, nl * sizeof(double)); }
    }
    if (rc == NF_OK) rc = team_alloc(T);
    if (rc != NF_OK) { nf_destroy(S); *out = nullptr; return rc; }
    S->d_SigS.assign((size_t)ng * ng, nullptr); S->d_Ms.assign((size_t)ng * ng, nullptr);
    return nf_reset_flux(S);
}

int nf_create(int rt_order, int p_order, int ng, int nxb, const double *xb, int nyb, const double *yb, int nzb,
              const double *zb, int device, nf_handle *out)
{
    return create_impl(rt_order, p_order, ng, nxb, xb, nyb, yb, nzb, zb, 0, 0, device, out);
}
int nf_create_slab(int rt_order, int p_order, int ng, int nxb, const double *xb, int nyb, const double *yb, int nzb,
                   const double *zb_slab, int interface_below, int interface_above, int device, nf_handle *out)
{
    return create_impl(rt_order, p_order, ng, nxb, xb, nyb, yb, nzb, zb_slab, interface_below ? 1 : 0, interface_above ? 1 : 0, device, out);
}

int nf_destroy(nf_handle S)
{
    if (!S) return NF_OK;
    (void)hipSetDevice(S->device);
    nf_team *T = S->team;
    if (T && T->dead) {                                          // see team_free: nothing of a dead team is waited for or freed (hipFree drains the device)
        std::vector<nf_solver *> cc; cc.swap(T->cc);
        for (auto *c : cc) if (c) nf_destroy(c);
        T->slabs.erase(std::remove(T->slabs.begin(), T->slabs.end(), S), T->slabs.end());
        if (T->slabs.empty()) team_free(T);
        delete S;
        return NF_OK;
    }
    coarse_cache_drop(T);
    transient_drop(S);
    if (T && T->stream) (void)hipStreamSynchronize(T->stream);
    for (int d = 0; d < 3; ++d) { dfree(S->d_Dt[d]); dfree(S->d_Dh[d]); }
    dfree(S->d_cm); dfree(S->d_cmJ); dfree(S->d_cmsc);
    dfree(S->d_hx); dfree(S->d_hy); dfree(S->d_hz); dfree(S->d_xb); dfree(S->d_yb); dfree(S->d_zb);
    dfree(S->d_D); dfree(S->d_SigR); dfree(S->d_NSF); dfree(S->d_Chi); dfree(S->d_void);
    for (auto &p : S->d_SigS) dfree(p);
    for (auto &p : S->d_Ms) dfree(p);
    dfree(S->d_Ms_tab);
    dfree(S->d_Cd); dfree(S->d_Mf); dfree(S->d_Mchi); dfree(S->d_phi_adj); dfree(S->d_Sinv); dfree(S->d_Sdense);
    for (int d = 0; d < 3; ++d) { dfree(S->d_L[d]); dfree(S->d_DR[d]); dfree(S->d_D0[d]); dfree(S->d_lid[d]); dfree(S->d_ltab[d]); }
    dfree(S->d_alo); dfree(S->d_ahi); dfree(S->d_hlo); dfree(S->d_hhi); dfree(S->d_gfl); dfree(S->d_sinv_lo); dfree(S->d_sinv_hi);
    dfree(S->d_clo); dfree(S->d_chi); dfree(S->d_rlo); dfree(S->d_rhi); dfree(S->d_ulo); dfree(S->d_uhi);
    dfree(S->d_Wlo); dfree(S->d_Whi);
    dfree(S->d_Jz); dfree(S->d_Jzb); dfree(S->d_ctlo); dfree(S->d_cthi); dfree(S->d_elo); dfree(S->d_ehi); dfree(S->d_relo); dfree(S->d_rehi);
    dfree(S->d_phi); dfree(S->d_raw); dfree(S->d_p0); dfree(S->d_p1);
    dfree(S->d_tf); dfree(S->d_rhs); dfree(S->d_r); dfree(S->d_p); dfree(S->d_q); dfree(S->d_p2); dfree(S->d_qy); dfree(S->d_qz); dfree(S->d_ring);
    dfree(S->d_qsrc); dfree(S->d_modes[0]); dfree(S->d_modes[1]);
    dfree(S->d_gamma); dfree(S->d_gpt_w); dfree(S->d_gpt_sc);
    if (T) {
        T->slabs.erase(std::remove(T->slabs.begin(), T->slabs.end(), S), T->slabs.end());
        for (size_t i = 0; i < T->slabs.size(); ++i) T->slabs[i]->slab_index = (int)i;
        if (T->slabs.empty()) team_free(T);
    }
    delete S;
    return NF_OK;
}

// link n slabs (ordered bottom to top, same device, adjacent ones sharing an interface) into one team
int nf_link_slabs(nf_handle *handles, int n)
{
    if (!handles || n < 1 || n > MAX_LOCAL_SLABS) return fail(NF_ERR_ARG, "nf_link_slabs: 1..%d slabs", MAX_LOCAL_SLABS);
    nf_solver *S0 = handles[0];
    if (!S0) return fail(NF_ERR_ARG, "nf_link_slabs: null handle");
    HIPCHK(hipSetDevice(S0->device));
    for (int i = 0; i < n; ++i) {
        nf_solver *S = handles[i];
        if (!S || S->team->slabs.size() != 1) return fail(NF_ERR_STATE, "nf_link_slabs: handle %d is null or already linked", i);
        if (S->device != S0->device || S->nx != S0->nx || S->ny != S0->ny || S->ng != S0->ng)
            return fail(NF_ERR_ARG, "nf_link_slabs: slab %d does not match slab 0 (device, nx, ny, groups)", i);
        if (i > 0 && (!S->if_lo || !handles[i - 1]->if_hi)) return fail(NF_ERR_ARG, "nf_link_slabs: slabs %d/%d lack the shared interface flag", i - 1, i);
    }
    nf_team *T = S0->team;
    for (int i = 0; i < n; ++i) coarse_cache_drop(handles[i]->team);
    for (int i = 1; i < n; ++i) {
        nf_solver *S = handles[i];
        team_free(S->team);
        S->team = T; S->slab_index = i; T->slabs.push_back(S);
    }
    T->linked_ready = false;
    return team_alloc(T);
}

int nf_comm_unique_id(void *id128)
{
    if (!id128) return fail(NF_ERR_ARG, "nf_comm_unique_id: null buffer");
    NFCHK(rccl_load());
    ncclUniqueId id; NCCLCHK(g_rccl.GetUniqueId(&id));
    memcpy(id128, &id, sizeof id);
    return NF_OK;
}
int nf_comm_init(nf_handle S, const void *id128, int nranks, int rank)
{
    if (!S || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(NF_ERR_ARG, "nf_comm_init: bad arguments");
    nf_team *T = S->team;
    const bool force = getenv("NEUTFEM_FORCE_RCCL") != nullptr;   // 1-rank communicator: exercises the RCCL reduce path on one GPU
    if (nranks == 1 && !force) { T->nproc = 1; T->rank = 0; return NF_OK; }
    NFCHK(rccl_load());
    HIPCHK(hipSetDevice(T->device));
    ncclUniqueId id; memcpy(&id, id128, sizeof id);
    NCCLCHK(g_rccl.CommInitRank(&T->comm, nranks, id, rank));
    T->nproc = nranks; T->rank = rank; T->linked_ready = false; T->rccl_reduce = true;
    return NF_OK;
}

// What carries the data path of this team: ranks of the live communicator as the library itself counts them (ncclCommCount; 0 = no
// communicator, -1 = the library has no such entry) and the file the RCCL symbols were resolved from.
int nf_comm_info(nf_handle S, int *comm_ranks, char *lib_path, size_t len)
{
    if (!S) return fail(NF_ERR_ARG, "null handle");
    nf_team *T = S->team;
    if (comm_ranks) {
        *comm_ranks = 0;
        if (T->comm) { *comm_ranks = -1; int n = 0; if (g_rccl.CommCount && g_rccl.CommCount(T->comm, &n) == 0) *comm_ranks = n; }
    }
    if (lib_path && len) snprintf(lib_path, len, "%s", T->comm ? g_rccl.path : "");
    return NF_OK;
}

// Diagnostic: the point-to-point calls of the plane exchange against the loaded RCCL, on this rank alone -- a grouped
// ncclSend / ncclRecv pair to and from the own rank on the comm stream, ordered against the main stream with the same
// events the Schur apply uses, followed by an all-reduce(max).  Verifies the dlsym'd signatures and the stream / event
// choreography with the real library where only one GPU is available.
int nf_comm_selftest(nf_handle S)
{
    if (!S) return fail(NF_ERR_ARG, "null handle");
    nf_team *T = S->team;
    if (!T->comm) return fail(NF_ERR_STATE, "nf_comm_selftest: no communicator (call nf_comm_init first)");
    HIPCHK(hipSetDevice(T->device));
    const size_t n = 1 << 16;
    double *a = nullptr, *b = nullptr;
    NFCHK(dalloc(&a, n)); if (dalloc(&b, n) != NF_OK) { dfree(a); return NF_ERR_HIP; }
    hipStream_t cs = T->comm_stream ? T->comm_stream : T->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreateWithFlags(&e0, hipEventDisableTiming); (void)hipEventCreateWithFlags(&e1, hipEventDisableTiming);
    int rc = NF_OK;
    hipLaunchKernelGGL(k_fill_pattern, dim3(64), dim3(256), 0, T->stream, a, (long)n);
    (void)hipMemsetAsync(b, 0, n * sizeof(double), T->stream);
    (void)hipEventRecord(e0, T->stream); (void)hipStreamWaitEvent(cs, e0, 0);
    if (g_rccl.GroupStart() != 0 || g_rccl.Send(a, n, NCCL_DOUBLE, T->rank, T->comm, cs) != 0 ||
        g_rccl.Recv(b, n, NCCL_DOUBLE, T->rank, T->comm, cs) != 0 || g_rccl.GroupEnd() != 0) rc = fail(NF_ERR_HIP, "nf_comm_selftest: grouped ncclSend/ncclRecv failed");
    (void)hipEventRecord(e1, cs); (void)hipStreamWaitEvent(T->stream, e1, 0);
    double w = 3.25;
    if (rc == NF_OK) {
        (void)hipMemcpyAsync(T->d_red, &w, sizeof w, hipMemcpyHostToDevice, T->stream);
        if (g_rccl.AllReduce(T->d_red, T->d_red, 1, NCCL_DOUBLE, NCCL_MAX, T->comm, T->stream) != 0) rc = fail(NF_ERR_HIP, "nf_comm_selftest: ncclAllReduce(max) failed");
        (void)hipMemcpyAsync(&w, T->d_red, sizeof w, hipMemcpyDeviceToHost, T->stream);
    }
    // the vector reduce's call form: out-of-place sum of 1024 partials + 1 flag slot (b <- sum over ranks of a[0 .. 1025))
    const size_t nv = 1025;
    if (rc == NF_OK && g_rccl.AllReduce(a, b + n - nv, nv, NCCL_DOUBLE, NCCL_SUM, T->comm, T->stream) != 0) rc = fail(NF_ERR_HIP, "nf_comm_selftest: ncclAllReduce(sum, 1025 doubles) failed");
    std::vector<double> ha(n), hb(n);
    if (hipStreamSynchronize(T->stream) != hipSuccess) rc = fail(NF_ERR_HIP, "nf_comm_selftest: stream failed");
    if (rc == NF_OK) {
        (void)hipMemcpy(ha.data(), a, n * sizeof(double), hipMemcpyDeviceToHost); (void)hipMemcpy(hb.data(), b, n * sizeof(double), hipMemcpyDeviceToHost);
        bool vec_ok = true;                                        // every rank sends the same pattern: the sum is nproc times it
        for (size_t i = 0; i < nv && vec_ok; ++i) vec_ok = hb[n - nv + i] == (double)T->nproc * ha[i];
        if (memcmp(ha.data(), hb.data(), (n - nv) * sizeof(double)) != 0) rc = fail(NF_ERR_NUMERIC, "nf_comm_selftest: received plane differs from the sent one");
        else if (!vec_ok) rc = fail(NF_ERR_NUMERIC, "nf_comm_selftest: all-reduce(sum) of a 1025-double vector returned wrong values");
        else if (T->nproc == 1 && w != 3.25) rc = fail(NF_ERR_NUMERIC, "nf_comm_selftest: all-reduce(max) returned %g", w);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    dfree(a); dfree(b);
    return rc;
}

long nf_info(nf_handle S, const char *key)
{
    if (!S || !key) return -1;
    nf_team *T = S->team;
#define K(s, v) if (!strcmp(key, s)) return (long)(v)
    K("dim", S->dim); K("nx", S->nx); K("ny", S->ny); K("nz", S->nz); K("ne", S->N); K("ng", S->ng);
    K("n_phi", S->nphi); K("n_J", S->nJ); K("n_loc", S->nloc); K("rt_order", S->k); K("p_order", S->m); K("last_outer", T->last_outer);
    K("last_cg_total", T->last_cg_total); K("coarse_outer", T->coarse_outer); K("device", S->device);
    K("last_path", T->last_path); K("last_resident_serial", T->last_resident_serial); K("batch_launches", T->batch_launches); K("batch_capacity", T->batch_cap); K("compute_units", T->ncu); K("last_direct", T->last_direct); K("direct_standin_unconverged", T->standin_unconverged); K("n_local_slabs", T->slabs.size()); K("n_ranks", T->nproc); K("rank", T->rank); K("vec_reduce", T->last_vec_reduce); K("cg_reductions", T->last_cg_reductions); K("cg_form", T->last_cg_form); K("endpoint_weights", T->last_endpoint_w); K("xchg_comm", T->comm_x ? 1 : 0); K("last_xcd", T->last_xcd); K("xcd_solves", T->xcd_solves); K("xcd_refused", T->xcd_refused);
    K("void_cells", S->void_cells);
    K("line_dict_rejected", S->ld_rejected); K("line_dict_bytes", S->ld_bytes);
    K("transient_steps", transient_steps(S)); K("transient_rebuilds", S->tr_rebuilds);
#undef K
    return -1;
}

int nf_set_bc(nf_handle S, int attr, int bc_type)
{
    if (!S || attr < 0 || attr >= 8) return fail(NF_ERR_ARG, "nf_set_bc: bad attribute %d", attr);
    S->bc_set[attr] = 1; S->bc_type[attr] = bc_type; S->dense_valid = false;
    coarse_cache_drop(S->team); line_dict_drop(S); gpt_drop(S);
    return NF_OK;
}

int nf_set_void(nf_handle S, const unsigned char *mask, double gamma)
{
    if (!S) return fail(NF_ERR_ARG, "nf_set_void: null handle");
    if (S->if_lo || S->if_hi || !team_is_single(S->team)) return fail(NF_ERR_UNSUPPORTED, "nf_set_void: slabs and slab teams know no cut-out cells (undivided meshes only)");
    long cnt = 0;
    if (mask) {
        if (!std::isfinite(gamma) || !(gamma > 0.0)) return fail(NF_ERR_ARG, "nf_set_void: gamma must be finite and positive (got %g)", gamma);
        for (long e = 0; e < S->N; ++e) cnt += mask[e] != 0;
        if (cnt == S->N) return fail(NF_ERR_ARG, "nf_set_void: every cell is void");
    }
    HIPCHK(hipSetDevice(S->device));
    hipStream_t st = S->team->stream;
    // the operator, and whatever was derived from it, is stale until the next nf_build (as after nf_upload_xs)
    S->built = false; S->diag_valid = false; S->cmfd_init = false; S->cmfd_iface = false; S->dense_valid = false;
    coarse_cache_drop(S->team); line_dict_drop(S); modes_drop(S); gpt_drop(S);
    HIPCHK(hipStreamSynchronize(st));
    dfree(S->d_void); S->void_host.clear(); S->void_cells = 0; S->void_gamma = 0.0;
    if (cnt == 0) return NF_OK;                                   // a mask without a set byte is no mask
    S->void_host.resize((size_t)S->N);
    for (long e = 0; e < S->N; ++e) S->void_host[e] = mask[e] ? 1 : 0;
    NFCHK(dalloc(&S->d_void, (size_t)S->N));
    HIPCHK(hipMemcpyAsync(S->d_void, S->void_host.data(), (size_t)S->N, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    S->void_cells = cnt; S->void_gamma = gamma;
    return NF_OK;
}
int nf_get_void(nf_handle S, unsigned char *mask, double *gamma)
{
    if (!S) return fail(NF_ERR_ARG, "nf_get_void: null handle");
    if (!S->d_void) return fail(NF_ERR_STATE, "nf_get_void: no mask is set (nf_set_void)");
    if (mask) memcpy(mask, S->void_host.data(), (size_t)S->N);
    if (gamma) *gamma = S->void_gamma;
    return NF_OK;
}

int nf_upload_xs(nf_handle S, const double *D, const double *SigR, const double *NSF, const double *Chi, const double *SigS)
{
    if (!S || !D || !SigR || !NSF || !Chi || !SigS) return fail(NF_ERR_ARG, "nf_upload_xs: null pointer");
    HIPCHK(hipSetDevice(S->device));
    hipStream_t st = S->team->stream;
    const size_t NN = (size_t)S->N * S->ng, B = NN * sizeof(double);
    // the device copies are overwritten from here on: whatever was built from the old ones is stale until the next nf_build,
    // also when this upload is refused below (a refused upload leaves the handle un-built, never half-valid)
    S->xs_uploaded = false; S->built = false; S->diag_valid = false; S->cmfd_init = false; S->cmfd_iface = false; S->dense_valid = false;
    coarse_cache_drop(S->team); line_dict_drop(S); modes_drop(S); gpt_drop(S);
    NFCHK(dalloc(&S->d_D, NN)); NFCHK(dalloc(&S->d_SigR, NN)); NFCHK(dalloc(&S->d_NSF, NN)); NFCHK(dalloc(&S->d_Chi, NN));
    HIPCHK(hipMemcpyAsync(S->d_D, D, B, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S->d_SigR, SigR, B, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S->d_NSF, NSF, B, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S->d_Chi, Chi, B, hipMemcpyHostToDevice, st));
    const int ng = S->ng;
    for (int i = 0; i < ng * ng; ++i) {
        const double *blk = SigS + (size_t)i * S->N;
        bool nz = false;                                          // src/NeutFEM.cpp:1265 : |sigs| > 1e-14
        for (long e = 0; e < S->N; ++e) if (!(std::fabs(blk[e]) <= 1e-14)) { nz = true; break; }   // NaN counts as non-empty (flagged below)
        if (!nz) { dfree(S->d_SigS[i]); continue; }              // an empty block adds exact zeros: skipping it is equivalent (:1722)
        NFCHK(dalloc(&S->d_SigS[i], S->N));
        HIPCHK(hipMemcpyAsync(S->d_SigS[i], blk, S->N * sizeof(double), hipMemcpyHostToDevice, st));
    }
    // non-finite cross sections or D == 0 would only surface later as a NaN eigenvalue: refuse them here (checked on the device)
    int *d_flags = nullptr, flags = 0;
    NFCHK(dalloc(&d_flags, 1));
    (void)hipMemsetAsync(d_flags, 0, sizeof(int), st);
    const int gchk = grid_for((long)NN, 256, 4096);
    hipLaunchKernelGGL(k_check_xs, dim3(gchk), dim3(256), 0, st, S->d_D, (long)NN, 1, 0, d_flags);
    hipLaunchKernelGGL(k_check_xs, dim3(gchk), dim3(256), 0, st, S->d_SigR, (long)NN, 0, 1, d_flags);
    hipLaunchKernelGGL(k_check_xs, dim3(gchk), dim3(256), 0, st, S->d_NSF, (long)NN, 0, 2, d_flags);
    hipLaunchKernelGGL(k_check_xs, dim3(gchk), dim3(256), 0, st, S->d_Chi, (long)NN, 0, 3, d_flags);
    for (int i = 0; i < ng * ng; ++i)
        if (S->d_SigS[i]) hipLaunchKernelGGL(k_check_xs, dim3(grid_for(S->N, 256, 4096)), dim3(256), 0, st, S->d_SigS[i], S->N, 0, 4, d_flags);
    hipError_t ce = hipMemcpyAsync(&flags, d_flags, sizeof(int), hipMemcpyDeviceToHost, st);
    if (ce == hipSuccess) ce = hipStreamSynchronize(st);
    dfree(d_flags);
    if (ce != hipSuccess) return fail(NF_ERR_HIP, "nf_upload_xs: %s", hipGetErrorString(ce));
    if (flags) {
        static const char *names[5] = { "D (non-finite or zero)", "SigR", "NSF", "Chi", "SigS" };
        std::string which;
        for (int b = 0; b < 5; ++b) if (flags & (1 << b)) { if (!which.empty()) which += ", "; which += names[b]; }
        return fail(NF_ERR_ARG, "nf_upload_xs: invalid cross sections: %s", which.c_str());
    }
    S->xs_uploaded = true; S->built = false;
    return NF_OK;
}

int nf_build(nf_handle S)
{
    if (!S) return fail(NF_ERR_ARG, "nf_build: null handle");
    if (!S->xs_uploaded) return fail(NF_ERR_STATE, "nf_build: call nf_upload_xs first");
    if (S->d_void && !team_is_single(S->team)) return fail(NF_ERR_UNSUPPORTED, "nf_build: a slab team knows no cut-out cells (nf_set_void)");
    HIPCHK(hipSetDevice(S->device));
    coarse_cache_drop(S->team); line_dict_drop(S); modes_drop(S); gpt_drop(S);
    hipStream_t st = S->team->stream;
    const int ng = S->ng; const long N = S->N, NP = S->nphi; const size_t NN = (size_t)N * ng;
    NFCHK(dalloc(&S->d_Cd, (size_t)NP * ng)); NFCHK(dalloc(&S->d_Mf, (size_t)NP * ng)); NFCHK(dalloc(&S->d_Mchi, (size_t)NP * ng));
    for (int d = 0; d < S->dim; ++d) {
        NFCHK(dalloc(&S->d_L[d], NN)); NFCHK(dalloc(&S->d_DR[d], NN)); NFCHK(dalloc(&S->d_D0[d], (size_t)S->nlines[d] * ng));
    }
    ChatArgs ch; ch.nloc = S->nloc;                               // C-hat_pp = prod 2/(2 i_t + 1), Legendre mass (include/FEM.hpp:197-200)
    for (int p = 0; p < S->nloc; ++p) {
        int q = p; double c = 1.0;
        for (int t = 0; t < S->dim; ++t) { c *= 2.0 / (2.0 * (q % S->n1) + 1.0); q /= S->n1; }
        ch.c[p] = c;
    }
    const bool slab = S->if_lo || S->if_hi;
    if (slab) {
        const size_t nl = (size_t)S->nlines[2] * ng;
        NFCHK(dalloc(&S->d_alo, nl)); NFCHK(dalloc(&S->d_ahi, nl)); NFCHK(dalloc(&S->d_hlo, nl)); NFCHK(dalloc(&S->d_hhi, nl));
        NFCHK(dalloc(&S->d_gfl, nl)); NFCHK(dalloc(&S->d_sinv_lo, nl)); NFCHK(dalloc(&S->d_sinv_hi, nl));
    }
    Geom G = make_geom(S);
    const int gN = grid_for(N, 256, 65535);
    const unsigned char *vmask = S->d_void;
    for (int g = 0; g < ng; ++g) {
        hipLaunchKernelGGL(k_cell_coef, dim3(gN), dim3(256), 0, st, S->d_SigR + g * N, S->d_Cd + g * NP, S->d_hx, S->d_hy, S->d_hz, S->nx, S->ny, N, 0, S->dim, ch);
        // nf_set_void: the flux is zero in the void cells, so Mf, M_chi and Ms are zero there whatever was uploaded; C keeps them
        hipLaunchKernelGGL(k_cell_coef, dim3(gN), dim3(256), 0, st, S->d_NSF + g * N, S->d_Mf + g * NP, S->d_hx, S->d_hy, S->d_hz, S->nx, S->ny, N, 1, S->dim, ch, vmask);
        hipLaunchKernelGGL(k_cell_coef, dim3(gN), dim3(256), 0, st, S->d_Chi + g * N, S->d_Mchi + g * NP, S->d_hx, S->d_hy, S->d_hz, S->nx, S->ny, N, 2, S->dim, ch, vmask);   // M_chi (:432-439)
        for (int gp = 0; gp < ng; ++gp) {
            const int i = g * ng + gp;
            if (!S->d_SigS[i]) { dfree(S->d_Ms[i]); continue; }
            NFCHK(dalloc(&S->d_Ms[i], NP));
            hipLaunchKernelGGL(k_cell_coef, dim3(gN), dim3(256), 0, st, S->d_SigS[i], S->d_Ms[i], S->d_hx, S->d_hy, S->d_hz, S->nx, S->ny, N, 1, S->dim, ch, vmask);
        }
        for (int d = 0; d < S->dim; ++d) {
            const long nl = S->nlines[d];
            SlabOut so = { nullptr, nullptr, nullptr, nullptr, nullptr };
            int lo = 0, hi = 0;
            if (d == 2 && slab) {
                lo = S->if_lo; hi = S->if_hi;
                so.alo = S->d_alo + g * nl; so.ahi = S->d_ahi + g * nl; so.hlo = S->d_hlo + g * nl; so.hhi = S->d_hhi + g * nl; so.gfl = S->d_gfl + g * nl;
            }
            if (vmask) hipLaunchKernelGGL(k_factor_lines<true>, dim3((unsigned)((nl + 63) / 64)), dim3(64), 0, st, G, d, S->d_D + g * N,
                                          S->d_L[d] + g * N, S->d_DR[d] + g * N, S->d_D0[d] + g * nl, nl, lo, hi, so, VoidArgs{ vmask, 1.0 / S->void_gamma });
            else hipLaunchKernelGGL(k_factor_lines<false>, dim3((unsigned)((nl + 63) / 64)), dim3(64), 0, st, G, d, S->d_D + g * N,
                                    S->d_L[d] + g * N, S->d_DR[d] + g * N, S->d_D0[d] + g * nl, nl, lo, hi, so, VoidArgs{ nullptr, 0.0 });
        }
    }
    {
        std::vector<const double *> tab(S->d_Ms.begin(), S->d_Ms.end());
        NFCHK(dalloc(&S->d_Ms_tab, tab.size()));
        HIPCHK(hipMemcpyAsync(S->d_Ms_tab, tab.data(), tab.size() * sizeof(double *), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));                         // `tab` is host stack memory
    }
    // Chebyshev history of the power iteration (two multigroup vectors): allocated here, not inside the outer loop
    if (!S->d_p0) { NFCHK(dalloc(&S->d_p0, (size_t)NP * ng)); NFCHK(dalloc(&S->d_p1, (size_t)NP * ng)); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    S->built = true; S->diag_valid = false; S->cmfd_init = false; S->cmfd_iface = false; S->dense_valid = false;   // src/NeutFEM.cpp:454-456
    ++S->build_gen;
    S->team->linked_ready = false;
    return NF_OK;
}

// Host wait for a stream with low wake-up latency: hipStreamSynchronize sleeps on an interrupt, which costs 20-30 us per wait -- as much
// as two CG iterations of a 27 k-cell mesh, once per group solve and once per outer iteration.  Poll for a while first; long waits
// (big meshes) fall through to the blocking call, which also reports errors.
static hipError_t stream_wait(hipStream_t st)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0;; ++i) {
        const hipError_t q = hipStreamQuery(st);
        if (q != hipErrorNotReady) return q == hipSuccess ? hipSuccess : hipStreamSynchronize(st);
        if ((i & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    return hipStreamSynchronize(st);
}

// Wait for the solver's stream.  On a multi-rank team the stream holds collectives: if it does not drain within comm_timeout_s a peer
// is gone or stuck, and blocking for ever would pin this rank (and, under torchrun, the whole node) -- abort the communicator and
// return NF_ERR_COMM instead.
static int team_stream_wait(nf_team *T, hipStream_t st)
{
    if (T->nproc <= 1) { HIPCHK(stream_wait(st)); return NF_OK; }
    const auto t0 = std::chrono::steady_clock::now();
    for (long i = 0;; ++i) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) return NF_OK;
        if (q != hipErrorNotReady) { HIPCHK(q); }
        if (i > 2000) usleep(i > 20000 ? 200 : 20);
        if ((i & 1023) == 1023 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > T->comm_timeout_s) {
            if (g_rccl.CommAbort && T->comm_x) { (void)g_rccl.CommAbort(T->comm_x); }
            if (g_rccl.CommAbort && T->comm) { (void)g_rccl.CommAbort(T->comm); }
            T->comm = nullptr; T->comm_x = nullptr; T->dead = true;   // with or without ncclCommAbort the queued collectives may never finish: the team is unusable from here on
            for (auto *c : T->cc) if (c && c->team) { c->team->comm = nullptr; c->team->comm_x = nullptr; c->team->dead = true; }   // the coarse twin borrowed the same communicator
            return fail(NF_ERR_COMM, "rank %d: a collective did not complete within %.0f s (NEUTFEM_COMM_TIMEOUT_S): a peer rank is gone or stuck", T->rank, T->comm_timeout_s);
        }
    }
}

// Read the CG scalars and / or nout doubles of `out` back to the host: through the mapped page when available, else D2H copy + wait.
static bool pub_ready(nf_team *T)                                 // the mapped page exists (created on first use)
{
    if (T->opt.host_pub && !T->h_pub) {
        void *hp = nullptr;
        if (hipHostMalloc(&hp, sizeof(HostPub), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
            void *dp = nullptr;
            if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) { T->h_pub = (HostPub *)hp; T->d_pub = (HostPub *)dp; memset(hp, 0, sizeof(HostPub)); }
            else (void)hipHostFree(hp);
        }
        if (!T->h_pub) { (void)hipGetLastError(); T->opt.host_pub = 0; }
    }
    return T->opt.host_pub && T->h_pub;
}
static int pub_wait(nf_team *T, unsigned long long seq, CgScalars *h_cg, double *h_out, int nout)   // a kernel of the stream publishes `seq`
{
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (int i = 0;; ++i) {
        if (__atomic_load_n(&T->h_pub->seq, __ATOMIC_ACQUIRE) == seq) { seen = true; break; }
        if ((i & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    if (!seen) {                                                  // long wait (big mesh) or an error: block, then look again
        NFCHK(team_stream_wait(T, T->stream));
        if (__atomic_load_n(&T->h_pub->seq, __ATOMIC_ACQUIRE) != seq) return fail(NF_ERR_HIP, "scalar readback: the device never published sequence %llu", seq);
    }
    if (h_cg) *h_cg = T->h_pub->cg;
    for (int i = 0; i < nout; ++i) h_out[i] = T->h_pub->out[i];
    return NF_OK;
}
static int readback(nf_team *T, const CgScalars *d_cg, CgScalars *h_cg, const double *d_out, double *h_out, int nout)
{
    hipStream_t st = T->stream;
    if (pub_ready(T)) {
        const unsigned long long seq = ++T->pub_seq;
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, d_cg, d_out, nout, T->d_pub, seq);
        return pub_wait(T, seq, h_cg, h_out, nout);
    }
    if (h_cg) HIPCHK(hipMemcpyAsync(h_cg, d_cg, sizeof *h_cg, hipMemcpyDeviceToHost, st));
    if (nout > 0) HIPCHK(hipMemcpyAsync(h_out, d_out, nout * sizeof(double), hipMemcpyDeviceToHost, st));
    NFCHK(team_stream_wait(T, st));
    return NF_OK;
}

// ---- profiling helpers -----------------------------------------------------------------------
static void prof_begin(nf_team *T, int slot, hipEvent_t *a, hipEvent_t *b)
{
    if (T->ev_free.empty()) {
        hipEvent_t x, y; (void)hipEventCreate(&x); (void)hipEventCreate(&y); T->ev_free.push_back({x, y});
    }
    auto pr = T->ev_free.back(); T->ev_free.pop_back();
    *a = pr.first; *b = pr.second;
    (void)hipEventRecord(*a, T->stream);
    T->ev_pending.push_back({*a, *b, slot});
}
static void prof_collect(nf_team *T)
{
    for (auto &e : T->ev_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) T->prof[SLOT_NAMES[e.slot]].samples.push_back(ms);
        T->ev_free.push_back({e.a, e.b});
    }
    T->ev_pending.clear();
}

// ---- communication between slabs -----------------------------------------------------------------
// exchange one plane per interface: own c_hi goes up (becomes the upper slab's r_lo), own c_lo goes down.
// which = 0: the per-apply contributions (d_clo/d_chi -> d_rlo/d_rhi); which = 2: the separator-sweep couplings
// (d_elo/d_ehi -> d_relo/d_rehi); which = 1: the separator-diagonal halves of
// group g (d_hlo/d_hhi -> d_rlo/d_rhi, build time).
static int exchange_planes(nf_team *T, int which, int g, hipStream_t st)
{
    const int ns = (int)T->slabs.size();
    ++T->xchg_in_apply;
    auto send_lo = [&](nf_solver *S) { return which == 0 ? S->d_clo : which == 2 ? S->d_elo : S->d_hlo + (size_t)g * S->nlines[2]; };
    auto send_hi = [&](nf_solver *S) { return which == 0 ? S->d_chi : which == 2 ? S->d_ehi : S->d_hhi + (size_t)g * S->nlines[2]; };
    auto recv_lo = [&](nf_solver *S) { return which == 2 ? S->d_relo : S->d_rlo; };
    auto recv_hi = [&](nf_solver *S) { return which == 2 ? S->d_rehi : S->d_rhi; };
    for (int i = 0; i + 1 < ns; ++i) {                            // interfaces between local slabs
        nf_solver *A = T->slabs[i], *B = T->slabs[i + 1];
        const size_t bytes = (size_t)A->nlines[2] * (which == 1 ? 1 : n_modes(A)) * sizeof(double);
        HIPCHK(hipMemcpyAsync(recv_lo(B), send_hi(A), bytes, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(recv_hi(A), send_lo(B), bytes, hipMemcpyDeviceToDevice, st));
    }
    nf_solver *bot = T->slabs.front(), *top = T->slabs.back();
    if (T->nproc > 1 && (bot->if_lo || top->if_hi)) {
        const size_t cnt = (size_t)bot->nlines[2] * (which == 1 ? 1 : n_modes(bot));
        TRACE_COMM("rank %d exchange which=%d count=%zu lo=%d hi=%d poisoned=%d", T->rank, which, cnt, bot->if_lo, top->if_hi, (int)T->poisoned);
        ncclComm_t cx = T->comm_x ? T->comm_x : T->comm;
        NCCLCHK(g_rccl.GroupStart());
        if (bot->if_lo) {
            NCCLCHK(g_rccl.Send(send_lo(bot), cnt, NCCL_DOUBLE, T->rank - 1, cx, st));
            NCCLCHK(g_rccl.Recv(recv_lo(bot), cnt, NCCL_DOUBLE, T->rank - 1, cx, st));
        }
        if (top->if_hi) {
            NCCLCHK(g_rccl.Send(send_hi(top), cnt, NCCL_DOUBLE, T->rank + 1, cx, st));
            NCCLCHK(g_rccl.Recv(recv_hi(top), cnt, NCCL_DOUBLE, T->rank + 1, cx, st));
        }
        NCCLCHK(g_rccl.GroupEnd());
    } else if (bot->if_lo || top->if_hi) {
        return fail(NF_ERR_STATE, "slab %s has an interface but no neighbour: link the slabs (nf_link_slabs) or init the communicator (nf_comm_init)",
                    bot->if_lo ? "bottom" : "top");
    }
    return NF_OK;
}

// What a CG iteration hands to the kernels of a Schur apply.  The launch functions are pure in their arguments: these two values are the
// only way the state of a solve reaches a kernel, and a default-constructed one means "a plain apply outside CG".
struct ApplyCg {                                        // per apply: cg_solve -> team_schur_apply / team_endpoint_phase
    const CgScalars *cg = nullptr;
    bool fused = false; const std::vector<double *> *xsol = nullptr;   // fused CG: CgFuse of slab i = { d_p, d_r, (*xsol)[i] } (k_schur_x / k_schur_s mode 1)
    CgLean lean = {};                                   // lean CG, undivided mesh: the x pass consumes the |r|^2 partials
    CgLean lean_z1 = {};                                // lean CG, slab teams: the endpoint pass of the z lines consumes the all-reduced |r|^2
    Cg1 cg1 = {};                                       // slab teams, single-reduction CG: the z passes take their SR instantiations
    // batched x_sol update (undivided RT0-P0 mesh, CgPlan::xsol_batch > 1): the x pass's CgFuse with the ring slots of this iteration and which
    // k_schur_x<..., XB> takes it; pnew = the slot the x pass writes, which the y / z passes read
    bool ring = false; CgFuse ringfz = {}; int xb = XB_NOW; const double *pnew = nullptr;
};
struct PassCg {                                         // per launch: team_schur_apply / team_endpoint_phase -> launch_x / launch_s
    const CgScalars *cg = nullptr; CgFuse fuse = {}; CgLean lean = {}, lean_z1 = {}; Cg1 cg1 = {};   // of the apply, for this slab
    bool zw_dot = false;                                // the y / z passes emit T_a sum z_f w_f as their share of x.y (team_schur_apply, split)
    hipStream_t stream = nullptr;                       // another stream than the team's (x || y on small slabs)
    bool noacc = false; const double *yadd = nullptr;   // SlabArgs::noacc / yadd
    int xb = XB_NOW;                                    // the x pass's template argument XB (ApplyCg::xb)
};
static PassCg pass_cg(const ApplyCg &A, const nf_solver *S, int i)   // slab i
{
    PassCg P = { A.cg, A.fused ? CgFuse{ S->d_p, S->d_r, (*A.xsol)[i] } : CgFuse{}, A.lean, A.lean_z1, A.cg1 };
    if (A.ring) { P.fuse = A.ringfz; P.xb = A.xb; }
    return P;
}
// launch shape of the one-chunk line kernel (k_schur_s); rc != NF_OK: the line length is refused
struct SegPlan { int rc = NF_OK, SEG = 0, NSEG = 0, TX = 0, nparts = 0; dim3 grid, block; size_t lds = 0; };
static SegPlan seg_plan(const nf_solver *S, int d, int zmode);
static int launch_s(const nf_solver *S, int d, int g, const ModeArgs &ma, const Geom &G, int last, double *partials, const PassCg &P, int *nparts, int zmode);
// build-time: S_red = own half + neighbour's half for every separator; checks that separators decouple
static int line_dict_prepare(nf_team *T);
static int team_prepare(nf_team *T)
{
    NFCHK(line_dict_prepare(T));                                 // once per build too, but on its own flag: options may drop the tables alone
    if (T->linked_ready) return NF_OK;
    if (T->opt.xchg_comm && T->nproc > 1 && T->comm && !T->comm_x) {
        // collective: rank 0 draws a second unique id and hands it to the others through the first communicator (an all-reduce(sum) of
        // its 128 bytes as doubles, zeros from everyone else)
        ncclUniqueId id2; memset(&id2, 0, sizeof id2);
        double v[128]; for (double &x : v) x = 0.0;
        if (T->rank == 0) { NCCLCHK(g_rccl.GetUniqueId(&id2)); for (int i = 0; i < 128; ++i) v[i] = (double)(unsigned char)id2.internal[i]; }
        DevTmp<double> d; NFCHK(dalloc(&d.p, 128));
        HIPCHK(hipMemcpyAsync(d.p, v, sizeof v, hipMemcpyHostToDevice, T->stream));
        NCCLCHK(g_rccl.AllReduce(d.p, d.p, 128, NCCL_DOUBLE, NCCL_SUM, T->comm, T->stream));
        HIPCHK(hipMemcpyAsync(v, d.p, sizeof v, hipMemcpyDeviceToHost, T->stream));
        NFCHK(team_stream_wait(T, T->stream));
        for (int i = 0; i < 128; ++i) id2.internal[i] = (char)(unsigned char)v[i];
        NCCLCHK(g_rccl.CommInitRank(&T->comm_x, T->nproc, id2, T->rank));
        TRACE_COMM("rank %d: second communicator for the plane exchange", T->rank);
    }
    bool any = false;
    for (auto *S : T->slabs) { if (!S->built) return fail(NF_ERR_STATE, "every slab must be built (nf_build) before solving"); any |= S->if_lo || S->if_hi; }
    if (any) {
        const int ng = T->slabs[0]->ng;
        for (int g = 0; g < ng; ++g) {
            NFCHK(exchange_planes(T, 1, g, T->stream));
            for (auto *S : T->slabs) {
                const long nl = S->nlines[2];
                const unsigned gr = (unsigned)((nl + 255) / 256);
                if (S->if_lo) hipLaunchKernelGGL(k_sred_inv, dim3(gr), dim3(256), 0, T->stream, S->d_hlo + g * nl, S->d_rlo, S->d_sinv_lo + g * nl, nl, 0);
                if (S->if_hi) hipLaunchKernelGGL(k_sred_inv, dim3(gr), dim3(256), 0, T->stream, S->d_hhi + g * nl, S->d_rhi, S->d_sinv_hi + g * nl, nl, 1);
            }
            NFCHK(team_stream_wait(T, T->stream));
        }
        // separators must decouple through a slab: |a_lo a_hi (T_II^-1)[first,last]| * sqrt(sinv_lo sinv_hi) <= 1e-15.
        // The verdict is taken on the maximum over ALL ranks, so that every process of a decomposed run refuses together
        // (a single refusing rank would leave the others blocked in their next collective).
        double worst = 0.0; int worst_nz = 0;
        for (auto *S : T->slabs) {
            if (!(S->if_lo && S->if_hi)) continue;
            const size_t nl = (size_t)S->nlines[2] * ng;
            std::vector<double> gfl(nl), slo(nl), shi(nl);
            HIPCHK(hipMemcpy(gfl.data(), S->d_gfl, nl * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(slo.data(), S->d_sinv_lo, nl * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(shi.data(), S->d_sinv_hi, nl * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < nl; ++i) {
                const double w = std::fabs(gfl[i]) * std::sqrt(std::fabs(slo[i] * shi[i]));
                if (w > worst) { worst = w; worst_nz = S->nz; }
            }
        }
        if (T->rccl_reduce && T->nproc > 1) {
            HIPCHK(hipMemcpyAsync(T->d_red, &worst, sizeof(double), hipMemcpyHostToDevice, T->stream));
            NCCLCHK(g_rccl.AllReduce(T->d_red, T->d_red, 1, NCCL_DOUBLE, NCCL_MAX, T->comm, T->stream));
            HIPCHK(hipMemcpyAsync(&worst, T->d_red, sizeof(double), hipMemcpyDeviceToHost, T->stream));
            NFCHK(team_stream_wait(T, T->stream));                      // a collective sits on the stream: bounded wait (NEUTFEM_COMM_TIMEOUT_S)
        }
        // Jacobi on the separator system contracts by <= 2 * worst per sweep (two neighbours): sweeps until the neglected term is
        // below 1e-16 of the solution; none for thick slabs (>= ~30 planes), refused beyond 8 (slabs of fewer than ~4 planes)
        T->sep_sweeps = 0;
        if (worst > 1e-15) {
            const double rho = 2.0 * worst;
            int m = rho < 1.0 ? (int)std::ceil(std::log(1e-16) / std::log(rho)) - 1 : 99;
            if (m < 1) m = 1;
            if (m > 8) {
                if (worst_nz) return fail(NF_ERR_UNSUPPORTED, "slab of %d z-planes is too thin: separator coupling %.2e needs %d sweeps (limit 8; use slabs of >= 4 planes)", worst_nz, worst, m);
                return fail(NF_ERR_UNSUPPORTED, "a slab on another rank is too thin: separator coupling %.2e needs %d sweeps (limit 8; use slabs of >= 4 planes)", worst, m);
            }
            T->sep_sweeps = m;
        }
    }
    // vector reduce: partial counts of the accumulation pass (z lines, mode 2) and of k_cg_rupdate, equal on every rank?  EVERY rank of a
    // multi-rank team takes part in this all-reduce, eligible or not (an ineligible rank contributes zeros, which makes max != -min
    // and switches the path off everywhere): a collective behind a rank-local condition would be a hang.
    T->vec_ok = false;
    T->team_max_cells = 0; for (auto *X : T->slabs) T->team_max_cells = std::max(T->team_max_cells, X->N);
    if (T->rccl_reduce && T->nproc > 1) {
        nf_solver *S = T->slabs[0];
        const bool eligible = T->slabs.size() == 1 && S->nloc == 1 && S->dim == 3 && (S->if_lo || S->if_hi);
        int np = 0;
        if (eligible) {
            const SegPlan sp = seg_plan(S, 2, 2);
            np = sp.rc == NF_OK ? sp.nparts : 0;                  // a refused plan is not an error here: the scalar route serves
        }
        const int nr = eligible ? grid_for(S->nphi) : 0;
        double v[5] = { (double)np, -(double)np, (double)nr, -(double)nr, (double)T->team_max_cells };
        HIPCHK(hipMemcpyAsync(T->d_red, v, sizeof v, hipMemcpyHostToDevice, T->stream));
        NCCLCHK(g_rccl.AllReduce(T->d_red, T->d_red, 5, NCCL_DOUBLE, NCCL_MAX, T->comm, T->stream));
        HIPCHK(hipMemcpyAsync(v, T->d_red, sizeof v, hipMemcpyDeviceToHost, T->stream));
        NFCHK(team_stream_wait(T, T->stream));                      // a collective sits on the stream: bounded wait (NEUTFEM_COMM_TIMEOUT_S)
        T->team_max_cells = (long)v[4];                              // every rank takes the same decision about the CG form (cg_solve)
        T->vec_cnt_pq = np; T->vec_cnt_rr = nr;
        T->vec_stride = T->slab_cap + 2;
        T->vec_ok = eligible && v[0] == -v[1] && v[2] == -v[3] && np > 0 && np < T->slab_cap && nr > 0 && nr < T->slab_cap;
        if (T->vec_ok && !T->d_vec) { NFCHK(dalloc(&T->d_vec, (size_t)T->vec_stride * 2)); HIPCHK(hipMemset(T->d_vec, 0, (size_t)T->vec_stride * 2 * sizeof(double))); }
    }
    // endpoint functionals for the single-reduction CG (k_endpoint_w): the response of c_lo / c_hi to the unit vector of every plane, measured with
    // the endpoint pass itself -- nz launches per group, once per BuildMatrices
    for (auto *S : T->slabs) S->w_valid = false;
    if (T->opt.endpoint_weights && T->opt.cg_single_reduce != 0 && (T->opt.cg_single_reduce > 0 || T->team_max_cells <= T->opt.cg_single_reduce_max_cells))
        for (auto *S : T->slabs) {
            if (!(S->if_lo || S->if_hi) || S->nb != 0 || S->dim != 3 || S->nloc != 1) continue;
            const size_t NG = (size_t)S->N * S->ng; const long nxy = S->nlines[2];
            if (!S->d_Wlo) { NFCHK(dalloc(&S->d_Wlo, NG)); NFCHK(dalloc(&S->d_Whi, NG)); }
            HIPCHK(hipMemsetAsync(S->d_Wlo, 0, NG * sizeof(double), T->stream)); HIPCHK(hipMemsetAsync(S->d_Whi, 0, NG * sizeof(double), T->stream));
            HIPCHK(hipMemsetAsync(S->d_p, 0, (size_t)S->N * sizeof(double), T->stream));
            const Geom G = make_geom(S);
            const unsigned gf = (unsigned)grid_for(nxy);
            for (int g = 0; g < S->ng; ++g)
                for (int k = 0; k < S->nz; ++k) {
                    double *plane = S->d_p + (size_t)k * nxy;
                    hipLaunchKernelGGL(k_fill_const, dim3(gf), dim3(256), 0, T->stream, plane, nxy, 1.0);
                    NFCHK(launch_s(S, 2, g, mode_args(S, g, 2, 0, S->d_p, S->d_q), G, 0, nullptr, PassCg(), nullptr, 1));
                    if (S->if_lo) HIPCHK(hipMemcpyAsync(S->d_Wlo + (size_t)g * S->N + (size_t)k * nxy, S->d_clo, (size_t)nxy * sizeof(double), hipMemcpyDeviceToDevice, T->stream));
                    if (S->if_hi) HIPCHK(hipMemcpyAsync(S->d_Whi + (size_t)g * S->N + (size_t)k * nxy, S->d_chi, (size_t)nxy * sizeof(double), hipMemcpyDeviceToDevice, T->stream));
                    hipLaunchKernelGGL(k_fill_const, dim3(gf), dim3(256), 0, T->stream, plane, nxy, 0.0);
                }
            HIPCHK(hipStreamSynchronize(T->stream));
            HIPCHK(hipGetLastError());
            S->w_valid = true;
        }
    T->linked_ready = true;
    return NF_OK;
}

// process-local sum of the partials (+ all-reduce over ranks) + the scalar logic of `op`
// want_flag (FIN_SUM on a multi-rank team): the all-reduced error flags of the ranks land in out[nq], next to the sums (0 elsewhere)
static int team_finalize(nf_team *T, int op, const std::vector<int> &counts, int nq, double *out, double tol, int maxit, bool want_flag = false)
{
    PartSegs ps = segs_for(T, counts);
    if (!T->rccl_reduce) {
        hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, T->stream, op, T->d_partials, ps, T->partial_stride, nq, T->d_cg, out, tol, maxit, 0, T->d_red, (const double *)nullptr, T->d_ah);
    } else {
        // the sums of this rank followed by its error flag: one all-reduce of nq + 1 doubles (CgScalars::err)
        hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, T->stream, op, T->d_partials, ps, T->partial_stride, nq, T->d_cg, out, tol, maxit, 1, T->d_red, (const double *)T->d_errsrc);
        TRACE_COMM("rank %d allreduce finalize op=%d count=%d poisoned=%d", T->rank, op, nq + 1, (int)T->poisoned);
        NCCLCHK(g_rccl.AllReduce(T->d_red, T->d_red, (size_t)nq + 1, NCCL_DOUBLE, NCCL_SUM, T->comm, T->stream));
        hipLaunchKernelGGL(k_cg_logic, dim3(1), dim3(1), 0, T->stream, op, T->d_red, nq, T->d_cg, out, tol, maxit, want_flag ? 2 : 1, T->d_ah);
    }
    return NF_OK;
}

// A rank-local failure on a multi-rank team OUTSIDE the CG loop (an allocation, a refused launch between two collectives of the outer
// iteration): the rank raises its flag and carries on with the schedule instead of returning -- its peers are about to enter the next
// collective.  The flag travels in the reductions that exist anyway: the next CG solve ends on every rank at its first reduction
// (cg_logic, FIN_RHS), the per-outer reduction hands the flags to the host (team_finalize, want_flag).  Returns true when the caller
// must return `code` at once (single process).  Inside the CG loop (cg_solve) the rank likewise keeps issuing the collectives of the schedule
// without the compute; vec_slots (the vector-reduce form): also the flag slots of the two partial vectors it sends from now on.
static bool team_poison(nf_team *T, int code, bool vec_slots = false)
{
    if (code == NF_OK) return false;
    if (T->nproc <= 1) return true;
    if (!T->poisoned) {
        T->poisoned = true; T->poison_rc = code; snprintf(T->poison_msg, sizeof T->poison_msg, "%s", nf_last_error());
        const double one = 1.0;
        (void)hipMemcpyAsync(T->d_errsrc, &one, sizeof one, hipMemcpyHostToDevice, T->stream);
        if (vec_slots) for (double *slot : { T->d_partials + T->vec_cnt_pq, T->d_partials + T->partial_stride + T->vec_cnt_rr }) (void)hipMemcpyAsync(slot, &one, sizeof one, hipMemcpyHostToDevice, T->stream);
        (void)hipStreamSynchronize(T->stream);                   // `one` lives on this stack frame; the stream may also have to recover from the failed call
        (void)hipGetLastError();
    }
    return false;
}
static int team_poison_result(nf_team *T)                         // the poisoned rank's own error, once every rank has stopped
{
    const int code = T->poison_rc; char msg[256]; snprintf(msg, sizeof msg, "%s", T->poison_msg);
    T->poisoned = false;
    (void)hipMemsetAsync(T->d_errsrc, 0, sizeof(double), T->stream);
    return fail(code, "%s", msg);
}
// Exchange-only collectives (nf_build_diagonal_cache, nf_get_J, nf_initialize_cmfd: planes travel, nothing is reduced): every rank does
// its fallible local work first (allocations), then the verdicts are all-reduced, and only if every rank is fine is the first plane
// posted -- a rank that failed would otherwise return while its neighbours wait in ncclRecv until the timeout.
static int team_verdict(nf_team *T, int local_rc, const char *what)
{
    if (T->nproc > 1 && T->rank == T->inject_rank && T->inject_where == 'a') { T->inject_where = 0; local_rc = fail(NF_ERR_HIP, "injected failure on rank %d before %s (NEUTFEM_INJECT_FAIL)", T->rank, what); }
    if (!(T->rccl_reduce && T->nproc > 1)) return local_rc;
    std::string keep = local_rc != NF_OK ? g_err : std::string();
    double v = local_rc != NF_OK ? 1.0 : 0.0;
    HIPCHK(hipMemcpyAsync(T->d_red, &v, sizeof v, hipMemcpyHostToDevice, T->stream));
    TRACE_COMM("rank %d allreduce verdict before %s", T->rank, what);
    NCCLCHK(g_rccl.AllReduce(T->d_red, T->d_red, 1, NCCL_DOUBLE, NCCL_MAX, T->comm, T->stream));
    HIPCHK(hipMemcpyAsync(&v, T->d_red, sizeof v, hipMemcpyDeviceToHost, T->stream));
    NFCHK(team_stream_wait(T, T->stream));
    if (local_rc != NF_OK) { g_err = keep; return local_rc; }
    if (v != 0.0) return fail(NF_ERR_REMOTE, "another rank of the team reported an error before %s; no rank started it", what);
    return NF_OK;
}

// lean CG on slab teams: process-local sum of the partials into red[0] (+ all-reduce over ranks); the kernels that consume the
// total derive the CG scalars themselves (CgLean with count < 0), so no k_cg_logic launch follows
static int team_reduce(nf_team *T, const std::vector<int> &counts, double *red)
{
    PartSegs ps = segs_for(T, counts);
    // red[0] = the sum, red[1] = this rank's error flag: both travel in the one all-reduce (the consumers read red[1], CgLean count < 0)
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, T->stream, (int)FIN_SUM, T->d_partials, ps, T->partial_stride, 1, T->d_cg, red, 0.0, 0, 1, red, (const double *)T->d_errsrc);
    if (T->rccl_reduce) { TRACE_COMM("rank %d allreduce reduce count=2 poisoned=%d", T->rank, (int)T->poisoned); NCCLCHK(g_rccl.AllReduce(red, red, 2, NCCL_DOUBLE, NCCL_SUM, T->comm, T->stream)); }
    return NF_OK;
}

// single-reduction CG: the four rows of block partials (p.q, q.q, r.q from the accumulation pass, |r|^2 from the endpoint pass; the same
// count per slab in every row) -> red[0..3], this rank's error flag -> red[4], one all-reduce of five doubles
static int team_reduce_sr(nf_team *T, const std::vector<int> &counts, const std::vector<int> &cnt3)
{
    PartSegs ps = segs_for(T, counts);
    std::vector<int> c3(counts);                                 // row 3: the endpoint pass's own block count where k_endpoint_w ran (0 on a poisoned rank)
    for (size_t i = 0; i < c3.size(); ++i) if (cnt3[i] > 0 && counts[i] > 0) c3[i] = cnt3[i];
    PartSegs ps3 = segs_for(T, c3);
    hipLaunchKernelGGL(k_reduce_rows, dim3(1), dim3(256), 0, T->stream, (const double *)T->d_partials, ps, ps3, T->partial_stride, T->d_red, (const double *)T->d_errsrc);
    if (T->rccl_reduce) { TRACE_COMM("rank %d allreduce single-reduction count=5 poisoned=%d", T->rank, (int)T->poisoned); NCCLCHK(g_rccl.AllReduce(T->d_red, T->d_red, 5, NCCL_DOUBLE, NCCL_SUM, T->comm, T->stream)); }
    return NF_OK;
}

// Opt a kernel in to `lds` bytes of dynamic LDS (above the 64 KiB a launch gets by default).  Asked once per kernel and size class,
// not on every solve; a refusal (a device or driver with less LDS than planned for) is not an error of the solve: the caller steps
// back to the host-driven path.
static bool lds_opt_in(const void *fn, size_t lds)
{
    if (lds <= 64 * 1024) return true;
    // the attribute belongs to the CURRENT device's copy of the function: a process that holds handles on two devices must ask on each
    static std::map<std::pair<int, const void *>, size_t> granted;
    static std::mutex mu;
    int dev = 0; (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    auto it = granted.find({ dev, fn });
    if (it != granted.end() && it->second >= lds) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return false; }
    granted[{ dev, fn }] = lds;
    return true;
}
// ---- Schur apply -----------------------------------------------------------------------------
// The choices of the launch functions below as small predicates: the launches and nf_apply_plan (the read-only report) both call them.
static bool nt_regime(const nf_solver *S) { return S->team->opt.nt_loads && S->N > S->team->opt.nt_min_cells; }   // streaming loads beyond the caches (per slab on teams)
static bool x_nt(const nf_solver *S, int NB) { return NB == 0 && S->nx % 2 == 0 && nt_regime(S); }
// Table of distinct lines instead of the line's own factors (LineDict): where the streaming instantiation is taken and line_dict_prepare
// found the direction's lines repeating and verified them.  x_dict / c_dict / s_dict sit next to x_nt / c_nt / s_nt in the launches.
static bool dict_dir(const nf_solver *S, int d) { return S->ld_use[d]; }
static const int X_DICT_MAX_NCH = 16;                            // 32 chunks per lane (x lines beyond 2048 cells) spill with or without a table: not instantiated
static bool x_dict(const nf_solver *S, int NB, int NCH, bool nt) { return nt && NB == 0 && NCH <= X_DICT_MAX_NCH && dict_dir(S, 0); }
struct DictArgs { bool on = false; const double *L = nullptr, *DR = nullptr, *C = nullptr; LineDict ld; };   // what a table launch passes in place of L, DR (and Cd)
static DictArgs dict_args(const nf_solver *S, int d, int g, bool on)
{
    DictArgs A; A.on = on;
    if (!on) return A;
    const long rows = (long)S->ld_rows[d][g] * S->ld_pitch[d];
    A.L = S->d_ltab[d] + S->ld_off[d][g]; A.DR = A.L + rows; A.C = d == 0 ? A.DR + rows : nullptr;
    A.ld.id = S->d_lid[d] + (long)g * S->nlines[d]; A.ld.pitch = S->ld_pitch[d];
    return A;
}
static bool x_xcd(const nf_solver *S, bool nt) { return nt && S->team->opt.xcd >= 0 && (S->team->opt.xcd & 4); }   // bit 1 of k_schur_x's `first`: the streaming instantiations only
static bool x_fuses(const nf_solver *S) { return !(S->if_lo || S->if_hi); }                                       // slabs fuse in their endpoint pass instead
// f(std::integral_constant<unsigned, key>()), key < N: how a launch function gets from runtime values to an instantiation.  f decodes its index,
// returns false under `if constexpr` where the combination is not legal and launches otherwise: exactly the legal ones are instantiated.
template <class F, unsigned I> static bool call_index(F &f) { return f(std::integral_constant<unsigned, I>()); }
template <class F, unsigned... I> static bool with_index(unsigned key, F &f, std::integer_sequence<unsigned, I...>)
{
    static constexpr bool (*tab[])(F &) = { &call_index<F, I>... };   // one indexed call, however many instantiations there are
    return key < sizeof...(I) && tab[key](f);
}
template <unsigned N, class F> static bool with_index(unsigned key, F &&f) { return with_index(key, f, std::make_integer_sequence<unsigned, N>()); }

// The instantiations of k_schur_x<2, NCH, VEC, NB, NT, DICT>: up to 32 chunks per lane (16, 32: RT0-P0 only), streaming loads for RT0-P0 lines
// of even length, the table next to the streaming loads only
static const int X_BATCH_MAX_NCH = 8;                            // the batched x_sol update (XB_SKIP, XB_APPLY): x lines of up to 1024 cells
constexpr bool schur_x_legal(int NCH, bool VEC, int NB, bool NT, bool DICT, int XB = XB_NOW)
{
    return NCH >= 1 && NCH <= (NB == 0 ? 32 : 8) && (NCH & (NCH - 1)) == 0 && NB >= 0 && NB <= 2
        && (!NT || (VEC && NB == 0)) && (!DICT || (NT && NCH <= X_DICT_MAX_NCH))
        && XB >= XB_NOW && XB <= XB_APPLY && (XB == XB_NOW || (NB == 0 && NCH <= X_BATCH_MAX_NCH));
}
// the x pass: launch shape, NCH = the instantiation's chunks per lane (0: the line is refused), and what else picks the instantiation
struct XPlan { int lpl_log2 = 0, NCH = 0; unsigned grid = 0; bool vec = false, nt = false, xcd = false, dict = false; };
static XPlan x_plan(const nf_solver *S)
{
    XPlan P; const int K = 2;
    const int lanes = (S->nx + K - 1) / K;
    while ((1 << P.lpl_log2) < lanes && P.lpl_log2 < 6) ++P.lpl_log2;
    const int LPL = 1 << P.lpl_log2, LPW = 64 / LPL;
    const int nch = (S->nx + LPL * K - 1) / (LPL * K);
    P.grid = (unsigned)((S->nlines[0] + 4 * LPW - 1) / (4 * LPW));
    for (int c = 1; c <= (S->nb == 0 ? 32 : 8); c *= 2) if (nch <= c) { P.NCH = c; break; }   // long lines (16, 32: RT0-P0 only): more registers per lane, lower occupancy
    P.vec = S->nx % 2 == 0; P.nt = x_nt(S, S->nb);
    P.xcd = x_xcd(S, P.nt); P.dict = x_dict(S, S->nb, P.NCH, P.nt);
    return P;
}
static int launch_x(const nf_solver *S, int g, const ModeArgs &ma0, const Geom &G, int last, double *partials, const PassCg &P, int *nparts)
{
    const XPlan xp = x_plan(S);
    if (!xp.NCH) return fail(NF_ERR_UNSUPPORTED, "nx = %d exceeds the x-line kernel limit (%d cells)", S->nx, S->nb == 0 ? 4096 : 1024);
    if (nparts) *nparts = (int)xp.grid * n_modes(S);
    const CgFuse fz = x_fuses(S) ? P.fuse : CgFuse{ nullptr, nullptr, nullptr };
    const ModeTab mt = mode_tab(S, 0);
    const dim3 gr(xp.grid, (unsigned)mt.n);                       // all transverse modes in one launch
    const int first = 1 | (xp.xcd ? 2 : 0);
    const DictArgs da = dict_args(S, 0, g, xp.dict);              // the line's row of the table instead of its own L, 1/d and C diagonal
    ModeArgs ma = ma0; if (da.on) ma.Cd[0] = da.C;
    const double *L = da.on ? da.L : S->d_L[0] + g * S->N, *DR = da.on ? da.DR : S->d_DR[0] + g * S->N, *D0 = S->d_D0[0] + g * S->nlines[0];
    int lg = 0; while ((1 << lg) < xp.NCH) ++lg;
    const unsigned key = (((((unsigned)P.xb * 6 + (unsigned)lg) * 3 + (unsigned)S->nb) * 2 + xp.vec) * 2 + xp.nt) * 2 + xp.dict;
    const bool hit = with_index<3 * 6 * 3 * 8>(key, [&](auto i) {
        constexpr unsigned I = decltype(i)::value;
        constexpr int XB = I / 144, NCH = 1 << (I / 24 % 6), NB = I / 8 % 3; constexpr bool VEC = I & 4, NT = I & 2, DICT = I & 1;
        if constexpr (!schur_x_legal(NCH, VEC, NB, NT, DICT, XB)) return false;
        else hipLaunchKernelGGL((k_schur_x<2, NCH, VEC, NB, NT, DICT, XB>), gr, dim3(256), 0, S->team->stream, ma, mt, G, L, DR, D0, S->nx, S->ny, S->nlines[0], xp.lpl_log2,
                                first, last, partials, P.cg, fz, P.lean, da.ld);
        return true;
    });
    return hit ? NF_OK : fail(NF_ERR_ARG, "k_schur_x: no instantiation for NCH = %d, NB = %d, vec %d, nt %d, dict %d, xb %d", xp.NCH, S->nb, xp.vec, xp.nt, xp.dict, P.xb);
}

// Does direction d (1 = y, 2 = z) of this mesh take the chunked long-line kernel (k_schur_c)?  Plain lines of RT0-P0 meshes beyond
// s_long_min cells (s_long: -1 = from 257 cells per line, where k_schur_s would drop below 32 columns; 0 = never; 1 = whenever the
// shape allows), one group's array below 4 GiB (32-bit byte offsets inside), at most 1024 threads and the device's LDS.
struct ChunkPlan { bool ok = false; int NS = 0, TX = 0; size_t lds = 0; };
static ChunkPlan chunk_plan(const nf_solver *S, int d)
{
    ChunkPlan P; const nf_team *T = S->team;
    const int n = d == 1 ? S->ny : S->nz;
    if (S->nb != 0 || d < 1 || d >= S->dim || (d == 2 && (S->if_lo || S->if_hi)) || !((T->opt.s_long_dirs >> (d - 1)) & 1)) return P;
    // y lines already from 256 cells (32 columns x 512 threads, two blocks per CU: y 128 -> 120 us inside CG at 256^3, 510 -> 502 us per
    // iteration; nothing at 192^3, a loss at 128^3); z lines from 257: the last pass would need the split dot product, which eats its
    // 6 us at 256^3 (profiles/r03_i_ab_cg_chunked_y.txt)
    const int nmin = d == 1 ? T->opt.s_long_min_y : T->opt.s_long_min;
    if (!(T->opt.s_long == 1 || (T->opt.s_long < 0 && n > nmin)) || (size_t)S->N * sizeof(double) >= (1ull << 32)) return P;
    P.NS = (n + 15) / 16;                                        // segments of 8 cells per chunk, two chunks
    // 32 columns: 512-thread blocks at 256-cell lines (two per CU: one block's load phase overlaps the other's scans) beat 64 columns
    // x 1024 threads there (y 113 vs 117 us, z 116 vs 127 at 256^3, profiles/r03_h_ab_256.txt); at 512 cells 32 columns need the full 1024
    P.TX = T->opt.s_tx ? T->opt.s_tx : 32;
    while (P.TX > 8 && P.TX * P.NS > 1024) P.TX >>= 1;
    while (P.TX > 8 && P.TX / 2 >= S->nx) P.TX >>= 1;
    P.lds = (size_t)(3 * P.TX * P.NS + 2 * P.TX + 16 + 2 * 8 * P.NS * P.TX) * sizeof(double);
    P.ok = P.TX * P.NS <= 1024 && P.lds <= T->lds_limit;
    // up to 256 cells per line the one-chunk kernel has 32 columns too, and the chunked one only wins through two blocks per CU
    // overlapping: that needs tiles to overlap with.  A 256 x 256 x 32 slab has 256 of them -- one per CU -- and loses (y 22.8 vs 20.8 us,
    // 8-slab loopback 983 vs 971 us per CG iteration, profiles/r03_n_thin_slab_tiles.txt); 256^3 has 2048 and wins.
    if (P.ok && n <= 256 && T->opt.s_long < 1) {
        const long tiles = (long)((S->nx + P.TX - 1) / P.TX) * (d == 1 ? S->nz : S->ny);
        if (tiles < 1024) P.ok = false;
    }
    return P;
}

// launch shape and load / order flags of the chunked kernel
static dim3 c_grid(const nf_solver *S, int d, const ChunkPlan &cp) { return dim3((unsigned)((S->nx + cp.TX - 1) / cp.TX), (unsigned)(d == 1 ? S->nz : S->ny)); }
static unsigned c_block(const ChunkPlan &cp) { return (unsigned)((cp.TX * cp.NS + 63) / 64 * 64); }   // whole wavefronts, as in seg_plan
static const int C_SEG = 8, C_NCH = 2;                           // k_schur_c: segments of 8 cells, two chunks per block (chunk_plan's NS counts 16 cells)
static bool c_nt(const nf_solver *S) { return nt_regime(S); }
static bool c_dict(const nf_solver *S, int d, bool nt) { return nt && dict_dir(S, d); }
static const int C_EARLY_AUTO = 2;                               // what c_early = -1 resolves to
// early vector loads of the chunked kernel (k_schur_c EARLY): the table-backed passes only, 0 for every other pass
static int c_early(const nf_solver *S, bool dict) { const int e = S->team->opt.c_early; return dict ? (e < 0 ? C_EARLY_AUTO : e) : 0; }
static int c_xcd(const nf_solver *S, int d, bool nt) { const nf_team *T = S->team; return T->opt.xcd >= 0 ? (T->opt.xcd >> (d - 1)) & 1 : (d == 1 && nt); }
// one-chunk kernel (k_schur_s).  XCD-contiguous tile order: bit 0 = y passes, bit 1 = z passes; -1 (default) = the y passes of meshes in the streaming
// regime -- the 8 x tiles of a row set then run on one XCD back to back (256^3: y 133 -> 123 us, 501 -> 493 us per CG iteration;
// z passes lose 10 us with it; neutral to -0.5 % at 96^3 ... 192^3)
// z passes of SMALL slabs (at most 6 Mi cells): the XCD-contiguous order by default too (8-slab loopback at 256^3: accumulation pass 33.3 -> 30.7 us,
// 848 -> 835 us per CG iteration; 4 slabs 800 -> 773; on 8.4 M / 16.8 M-cell slabs it loses: 93 -> 101 / 191 -> 201 us; profiles/r04_o_slab_options.txt)
static int s_xcd(const nf_solver *S, int d, int zmode)
{
    const nf_team *T = S->team;
    return T->opt.xcd >= 0 ? (T->opt.xcd >> (d - 1)) & 1 : ((d == 1 && nt_regime(S)) || ((zmode == 1 || zmode == 2) && S->N <= (6L << 20)));
}
// undivided meshes beyond the caches (the classic path's sizes): the variant with streaming loads (SV_NT)
static bool s_nt(const nf_solver *S, int zmode, int SEG) { return zmode != 3 && S->nb == 0 && SEG == 8 && nt_regime(S); }   // plain lines and the z passes of a slab
static bool s_dict(const nf_solver *S, int d, int zmode, int SEG) { return zmode == 0 && s_nt(S, zmode, SEG) && dict_dir(S, d); }
static bool s_zw(const nf_solver *S, int zmode, bool zw_dot, bool want_dot) { return zmode == 0 && S->nb == 0 && zw_dot && want_dot; }     // z.w form of the pass's share of x.y
// Staged form (SV_STAGE): plain table-backed lines in full-width tiles (16-byte aligned rows of TX doubles, a whole number of them per
// 1-KiB copy instruction), the staged tile next to the summaries within the device's LDS.  Automatic: the directions that measurably
// gain, and only where a block has a next tile to fetch (tiles >= 2 blocks).
static const int S_STAGE_AUTO_DIRS = 2;                          // bit 0 = y, bit 1 = z
static size_t s_stage_bytes(int n, int TX) { const int rpp = 1024 / (8 * TX); return (size_t)((n + rpp - 1) / rpp) * 1024; }
static unsigned s_stage_blocks(const nf_solver *S, const SegPlan &sp)
{
    const unsigned tiles = sp.grid.x * sp.grid.y, want = (unsigned)(S->team->opt.s_stage_grid > 0 ? S->team->opt.s_stage_grid : S->team->ncu);
    return std::min(tiles, want);
}
static bool s_stage(const nf_solver *S, int d, int zmode, const SegPlan &sp, unsigned V)
{
    const nf_team *T = S->team;
    if (zmode != 0 || T->opt.s_stage == 0 || !(V & SV_NT) || !(V & SV_DICT) || (V & ~(SV_NT | SV_DICT | SV_ZW))) return false;
    if (sp.TX < 8 || sp.TX > 64 || (sp.TX & (sp.TX - 1)) || S->nx % sp.TX != 0) return false;
    if (sp.lds + s_stage_bytes(d == 1 ? S->ny : S->nz, sp.TX) > T->lds_limit) return false;
    if (T->opt.s_stage > 0) return true;
    return ((S_STAGE_AUTO_DIRS >> (d - 1)) & 1) && sp.grid.x * sp.grid.y >= 2 * s_stage_blocks(S, sp);
}
// Whole-tile form (FULL) of the staged pass and of the table-backed early-load chunked pass: the grid has no partial tile -- the tile width divides
// nx, the line is a whole number of segments (of chunks), the block has one thread per (column, segment) and the summaries are not scanned by whole
// wavefronts.  The bodies then drop the per-access predicates and address the vectors by 32-bit byte offsets (one group's array below 4 GiB).
static bool s_full(const nf_solver *S, int d, const SegPlan &sp, unsigned V)
{
    const nf_team *T = S->team; const int n = d == 1 ? S->ny : S->nz;
    if (T->opt.tile_full == 0 || !(V & SV_STAGE)) return false;
    const int wsmin = T->opt.s_wsmin > 0 ? T->opt.s_wsmin : 64, nt = sp.TX * sp.NSEG;
    const bool wscan = sp.NSEG >= wsmin && sp.NSEG <= 64 && (nt & 63) == 0;   // schur_s_tile's test
    return S->nx % sp.TX == 0 && n == sp.SEG * sp.NSEG && (unsigned)nt == sp.block.x && !wscan && (size_t)S->N * sizeof(double) < (1ull << 32);
}
static bool c_full(const nf_solver *S, int d, const ChunkPlan &cp, bool dict, int early)
{
    const int n = d == 1 ? S->ny : S->nz;
    return S->team->opt.tile_full != 0 && dict && early == 2 && S->nx % cp.TX == 0 && n == C_NCH * C_SEG * cp.NS && (unsigned)(cp.TX * cp.NS) == c_block(cp);
}
static bool s_fold(const nf_team *T, int zmode) { return zmode == 2 && T->sep_sweeps == 0 && T->opt.sep_fold; }   // thick slabs: the accumulation pass forms the separator values itself
// tiles of a (gx, gy) launch move under the XCD-contiguous order only when their count is a multiple of 8 (the kernels' own test) beyond 8 (the identity)
static bool xcd_permutes(bool order, unsigned tiles) { return order && tiles % 8 == 0 && tiles > 8; }
// 8-cell segments up to 1024 cells per line (16 / 32 cells spill to scratch: 1.4x slower even though TX drops to 8 at 1024)
// higher orders: 4-cell segments up to 256 cells per line; beyond, RT1 keeps 8 (148 B / lane of scratch and still faster: y 97 vs 122 us on
// 48 x 512 x 48), RT2 takes 4 up to 512 cells (8 columns per block, no scratch: y 352 vs 383 us, z 412 vs 431; profiles/r04_g_higher_orders.txt)
static SegPlan seg_plan(const nf_solver *S, int d, int zmode)     // direction d (1 = y, 2 = z); zmode as in launch_s
{
    SegPlan P; const nf_team *T = S->team;
    const int n = d == 1 ? S->ny : S->nz, nouter = d == 1 ? S->nz : S->ny;
    P.SEG = T->opt.s_seg ? T->opt.s_seg : (S->nb > 0 ? ((n <= 256 || (S->nb == 2 && n <= 512)) ? 4 : 8) : (n <= 1024 ? 8 : (n <= 2048 ? 16 : 32)));
    P.NSEG = (n + P.SEG - 1) / P.SEG;
    if (P.NSEG > 128) { P.rc = fail(NF_ERR_UNSUPPORTED, "line length %d exceeds the segmented kernel limit", n); return P; }
    P.TX = T->opt.s_tx ? T->opt.s_tx : 64;
    const int tmax = zmode != 0 ? 512 : 1024;                     // slab variants: 512 threads (register budget, see k_schur_s)
    while (P.TX > 8 && P.TX * P.NSEG > tmax) P.TX >>= 1;
    if (P.TX * P.NSEG > tmax) { P.rc = fail(NF_ERR_UNSUPPORTED, "line length %d needs more than %d threads per block", n, tmax); return P; }
    while (P.TX > 8 && P.TX / 2 >= S->nx) P.TX >>= 1;             // narrow meshes
    // whole wavefronts: the reductions use data-parallel-primitive moves and read lane 63 (threads beyond TX * NSEG only keep the barriers company)
    P.grid = dim3((unsigned)((S->nx + P.TX - 1) / P.TX), (unsigned)nouter, (unsigned)n_modes(S)); P.block = dim3((unsigned)((P.TX * P.NSEG + 63) / 64 * 64));
    P.nparts = (int)(P.grid.x * P.grid.y * P.grid.z);
    P.lds = (size_t)(4 * P.TX * (P.NSEG + 1) + P.TX + 32) * sizeof(double);   // + reduction scratch (block_sum: 8, block_sum3: 24 doubles at 512 threads)
    return P;
}
// Directions that take their table under line_dict = -1: those whose pass measurably gains at the benchmark size
static const int LINE_DICT_AUTO_DIRS = 7;
// would direction d stream its factors today, and do the options allow a table for it?  (undivided RT0-P0 meshes only)
static bool line_dict_eligible(const nf_solver *S, int d)
{
    const nf_team *T = S->team;
    if (T->opt.line_dict == 0 || d >= S->dim || T->slabs.size() != 1 || S->if_lo || S->if_hi || S->k != 0 || S->nb != 0 || S->nloc != 1 || !nt_regime(S)) return false;
    const int dirs = T->opt.line_dict_dirs & (T->opt.line_dict < 0 ? LINE_DICT_AUTO_DIRS : 7);
    if (!((dirs >> d) & 1)) return false;
    if (d == 0) { const int nch = x_plan(S).NCH; return x_nt(S, 0) && nch >= 1 && nch <= X_DICT_MAX_NCH; }
    if (chunk_plan(S, d).ok && c_nt(S)) return true;
    const SegPlan sp = seg_plan(S, d, 0);
    return sp.rc == NF_OK && s_nt(S, 0, sp.SEG);
}
// Once per build, on the first apply or solve that could use them: fingerprints of every line's stored factors, grouped on the host, verified
// bit for bit against the group's representative, the representatives' rows gathered.  A direction uses its table only if EVERY group
// verified, repeats at least fourfold (a core without repeats keeps the streaming path) and fits line_dict_max_bytes.
static int line_dict_prepare(nf_team *T)
{
    static_assert(sizeof(LineFp) == sizeof(nf_fp128), "fingerprints travel as they are");
    for (auto *S : T->slabs) {
        if (S->ld_tried || !S->built) continue;
        S->ld_tried = true;
        hipStream_t st = T->stream;
        const int ng = S->ng;
        for (int d = 0; d < S->dim; ++d) {
            if (!line_dict_eligible(S, d)) continue;
            const long nl = S->nlines[d], N = S->N;
            const int n = d == 0 ? S->nx : d == 1 ? S->ny : S->nz, pitch = (n + 15) / 16 * 16, narr = d == 0 ? 3 : 2;
            const unsigned gl = (unsigned)((nl + 63) / 64);
            auto Cd = [&](int g) { return d == 0 ? (const double *)(S->d_Cd + (size_t)g * S->nphi) : (const double *)nullptr; };
            DevTmp<LineFp> fp; NFCHK(dalloc(&fp.p, (size_t)nl * ng));
            for (int g = 0; g < ng; ++g)
                hipLaunchKernelGGL(k_line_fp, dim3(gl), dim3(64), 0, st, d, S->nx, S->ny, S->nz, (const double *)(S->d_L[d] + g * N), (const double *)(S->d_DR[d] + g * N),
                                   (const double *)(S->d_D0[d] + g * nl), Cd(g), nl, T->opt.line_dict_fp_bits, fp.p + (size_t)g * nl);
            std::vector<nf_fp128> h((size_t)nl * ng);
            HIPCHK(hipMemcpyAsync(h.data(), fp.p, h.size() * sizeof(nf_fp128), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            std::vector<int> ids((size_t)nl * ng), reps, rows(ng), idg, repg;
            std::vector<long> off(ng);
            bool fits = true; long total = 0;
            for (int g = 0; g < ng; ++g) {
                rows[g] = nf_group_lines(h.data() + (size_t)g * nl, nl, idg, repg);
                std::copy(idg.begin(), idg.end(), ids.begin() + (size_t)g * nl);
                reps.insert(reps.end(), repg.begin(), repg.end());
                off[g] = total; total += (long)rows[g] * pitch * narr;
                fits = fits && (long)rows[g] * 4 <= nl && (long)rows[g] * pitch * narr * (long)sizeof(double) <= T->opt.line_dict_max_bytes;
            }
            if (!fits) continue;
            DevTmp<int> drep, dmis; int mism = 0;
            NFCHK(dalloc(&drep.p, reps.size())); NFCHK(dalloc(&dmis.p, 1));
            NFCHK(dalloc(&S->d_lid[d], ids.size())); NFCHK(dalloc(&S->d_ltab[d], (size_t)total));
            HIPCHK(hipMemcpyAsync(S->d_lid[d], ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(drep.p, reps.data(), reps.size() * sizeof(int), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemsetAsync(dmis.p, 0, sizeof(int), st));
            long roff = 0;
            for (int g = 0; g < ng; ++g) {
                const double *L = S->d_L[d] + g * N, *DR = S->d_DR[d] + g * N;
                double *tL = S->d_ltab[d] + off[g], *tR = tL + (long)rows[g] * pitch, *tC = d == 0 ? tR + (long)rows[g] * pitch : nullptr;
                hipLaunchKernelGGL(k_line_verify, dim3(gl), dim3(64), 0, st, d, S->nx, S->ny, S->nz, L, DR, (const double *)(S->d_D0[d] + g * nl), Cd(g), nl,
                                   (const int *)(S->d_lid[d] + (size_t)g * nl), (const int *)(drep.p + roff), dmis.p);
                hipLaunchKernelGGL(k_line_gather, dim3((unsigned)(((long)rows[g] * pitch + 255) / 256)), dim3(256), 0, st, d, S->nx, S->ny, S->nz, L, DR, Cd(g),
                                   (const int *)(drep.p + roff), rows[g], pitch, tL, tR, tC);
                roff += rows[g];
            }
            HIPCHK(hipMemcpyAsync(&mism, dmis.p, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
            if (mism) { S->ld_rejected |= 1 << d; dfree(S->d_lid[d]); dfree(S->d_ltab[d]); continue; }   // fingerprints collided: this direction keeps streaming
            S->ld_use[d] = true; S->ld_pitch[d] = pitch; S->ld_off[d] = off; S->ld_rows[d] = rows;
            S->ld_bytes += (size_t)total * sizeof(double) + ids.size() * sizeof(int);
        }
    }
    return NF_OK;
}
// One y / z pass, chosen: launch_s executes this, plan_s prints it, and neither derives a flag of its own.
// V: the k_schur_s variant (SV_* of nf_kernels.h); for the chunked kernel SV_NT and SV_DICT are its template flags and SV_ZW says that it forms a dot product.
struct SPass { int rc = NF_OK; bool chunked = false; ChunkPlan cp; SegPlan seg; unsigned V = 0; int xcd = 0, early = 0, full = 0; bool fold = false, fuse = false; };
static std::string variant_name(unsigned V)                      // "fuse+nt+sr"; "" for the base kernel
{
    static const char *const bit[] = { "fuse", "nt", "zw", "sr", "dict", "stage" };
    std::string r;
    for (int i = 0; i < 6; ++i) if (V >> i & 1) r += (r.empty() ? "" : "+") + std::string(bit[i]);
    return r;
}
// want_dot: the pass leaves its share of x.y (zw_dot: in the z.w form); fuse / cg1: a fused CG update / the single-reduction state (Cg1) ride along;
// chunks = false: the device refused the chunked kernel's LDS
static SPass s_pass(const nf_solver *S, int d, int zmode, bool want_dot, bool zw_dot, bool fuse, bool cg1, bool chunks = true)
{
    SPass R;
    // long plain lines of RT0-P0 meshes: two chunks per block, twice the tile width (k_schur_c).  Its share of x.y comes in the z.w
    // form only: inside CG it needs the split dot product of team_schur_apply
    if (chunks && zmode == 0) R.cp = chunk_plan(S, d);            // the slab chain passes never take it
    if (R.cp.ok && (!want_dot || zw_dot)) {
        const bool nt = c_nt(S), dict = c_dict(S, d, nt);
        R.chunked = true; R.V = (nt ? SV_NT : 0) | (want_dot ? SV_ZW : 0) | (dict ? SV_DICT : 0);
        R.xcd = c_xcd(S, d, nt); R.early = c_early(S, dict); R.full = c_full(S, d, R.cp, dict, R.early);
        return R;
    }
    R.seg = seg_plan(S, d, zmode);
    if ((R.rc = R.seg.rc) != NF_OK) return R;
    const int SEG = R.seg.SEG; const bool p0 = S->nb == 0;
    R.fuse = fuse && zmode == 1 && S->nloc == 1;                  // the endpoint pass of a slab carries the update
    // single-reduction CG (Cg1): the endpoint pass (mode 1) consumes the reduction of the previous iteration and carries r -= alpha q, the
    // accumulation pass (mode 2) leaves p.q, q.q, r.q; |r|^2 comes from the endpoint pass (row 3 of the partial buffer)
    const bool sr = cg1 && p0 && SEG == 8 && d == 2 && ((zmode == 1 && R.fuse) || (zmode == 2 && want_dot));
    R.V = (R.fuse && p0 ? SV_FUSE : 0) | (s_nt(S, zmode, SEG) ? SV_NT : 0) | (s_zw(S, zmode, zw_dot, want_dot) ? SV_ZW : 0)
        | (sr ? SV_SR : 0) | (s_dict(S, d, zmode, SEG) ? SV_DICT : 0);
    if (s_stage(S, d, zmode, R.seg, R.V)) R.V |= SV_STAGE;
    R.xcd = s_xcd(S, d, zmode); R.fold = s_fold(S->team, zmode);
    R.full = s_full(S, d, R.seg, R.V);
    return R;
}
// zmode: 0 = plain line kernel (y lines, or z lines of an undivided mesh); 1 / 2 = slab chain passes (z lines)
static int launch_s(const nf_solver *S, int d, int g, const ModeArgs &ma, const Geom &G, int last, double *partials, const PassCg &P, int *nparts, int zmode)
{
    const nf_team *T = S->team; const CgScalars *cg = P.cg;
    const long N = S->N;
    const int n = d == 1 ? S->ny : S->nz;
    const long nxy = (long)S->nx * S->ny;
    const long sl = d == 1 ? S->nx : nxy, ostride = d == 1 ? nxy : S->nx;
    const double *L = S->d_L[d] + g * N, *DR = S->d_DR[d] + g * N, *D0 = S->d_D0[d] + g * S->nlines[d];
    auto pick = [&](bool chunks) { return s_pass(S, d, zmode, last && partials, P.zw_dot, P.fuse.p != nullptr, P.cg1.red != nullptr, chunks); };
    SPass ps = pick(true);
    if (ps.chunked) {
        const ChunkPlan &cp = ps.cp;
        const dim3 grid = c_grid(S, d, cp), block(c_block(cp));
        const DictArgs da = dict_args(S, d, g, (ps.V & SV_DICT) != 0);
        const unsigned key = (((unsigned)ps.full * 3 + (unsigned)ps.early) * 2 + da.on) * 4 + ((ps.V & SV_NT) ? 2 : 0) + (unsigned)(d - 1);
        bool launched = false;                                    // false: the device refused the LDS, or the launch (LDS, block size) -> the one-chunk kernel below
        const bool hit = with_index<2 * 3 * 2 * 2 * 2>(key, [&](auto i) {
            constexpr unsigned I = decltype(i)::value;
            constexpr int DIR = 1 + (I & 1), EARLY = I / 8 % 3, FULL = I / 24; constexpr bool NT = I & 2, DICT = I & 4;
            if constexpr (!schur_c_legal(DIR, NT, DICT, EARLY, FULL)) return false;
            else if (lds_opt_in((const void *)k_schur_c<DIR, NT, DICT, EARLY, FULL>, cp.lds)) {
                hipLaunchKernelGGL((k_schur_c<DIR, NT, DICT, EARLY, FULL>), grid, block, cp.lds, T->stream, ma.x[0], ma.y[0], ma.Ta, da.on ? da.L : L, da.on ? da.DR : DR, D0, n, sl, ostride,
                                   S->nx, cp.TX, cp.NS, last, partials, cg, ps.xcd, da.ld);
                launched = hipGetLastError() == hipSuccess;
            }
            return true;
        });
        if (!hit) return fail(NF_ERR_ARG, "k_schur_c: no instantiation for direction %d, nt %d, dict %d, early %d, full %d", d, (ps.V & SV_NT) ? 1 : 0, da.on ? 1 : 0, ps.early, ps.full);
        if (launched) { if (nparts) *nparts = (int)(grid.x * grid.y); return NF_OK; }
        ps = pick(false);
    }
    if (ps.rc != NF_OK) return ps.rc;
    const ModeTab mt = mode_tab(S, d);
    if (nparts) *nparts = ps.seg.nparts;
    hipStream_t st = P.stream ? P.stream : T->stream;
    SlabArgs sa; memset(&sa, 0, sizeof sa);
    sa.noacc = P.noacc ? 1 : 0; sa.yadd = P.yadd;
    sa.xcd = ps.xcd;
    sa.wsmin = T->opt.s_wsmin;
    const CgFuse fz = ps.fuse ? P.fuse : CgFuse{ nullptr, nullptr, nullptr };
    const CgLean lz = fz.p ? P.lean_z1 : CgLean{ nullptr, nullptr, 0, 0, 0 };
    if (ps.V & SV_SR) {
        sa.sr = P.cg1; sa.sr_r = S->d_r; sa.sr_q = S->d_q; sa.sr_stride = T->partial_stride;
        sa.sr_part = T->d_partials + 3 * T->partial_stride + (long)S->slab_index * T->slab_cap;
    }
    const DictArgs da = dict_args(S, d, g, (ps.V & SV_DICT) != 0);   // the column's row of the table instead of its own L, 1/d
    if (zmode != 0) {
        const long nl = S->nlines[2];
        sa.if_lo = S->if_lo; sa.if_hi = S->if_hi; sa.mode = zmode;
        sa.alo = S->d_alo + g * nl; sa.ahi = S->d_ahi + g * nl; sa.ulo = S->d_ulo; sa.uhi = S->d_uhi; sa.clo = S->d_clo; sa.chi = S->d_chi;
        if (zmode == 3) {                                           // current reconstruction: face DOFs and bubbles of every transverse mode
            int nfa = 1, ni = S->k; for (int t = 1; t < S->dim; ++t) { nfa *= S->k + 1; ni *= S->k + 1; }
            sa.nfa = nfa; sa.ni = ni;
            sa.jz = S->d_Jz + (size_t)g * S->nJz; sa.jzb = S->d_Jzb ? S->d_Jzb + (size_t)g * S->N * ni : nullptr;
            for (int m = 0; m < mt.n && m < 9; ++m) {                // RT transverse index of P mode m: a = sum a_t (k+1)^t (src/FEM.cpp:364-374)
                int amode = 0, q = m, mul = 1;
                for (int t = 0; t < S->dim; ++t) { if (t == d) continue; amode += (q % S->n1) * mul; q /= S->n1; mul *= S->k + 1; }
                sa.amode[m] = amode;
            }
        }
        if (ps.fold) {                                              // separators formed inside the pass (no k_separators launch)
            sa.fold = 1; sa.rlo = S->d_rlo; sa.rhi = S->d_rhi; sa.sinv_lo = S->d_sinv_lo + g * nl; sa.sinv_hi = S->d_sinv_hi + g * nl;
        }
    }
    // staged form: persistent blocks over the same tile grid, the staged tile behind the summaries.  A vector that is not 16-byte aligned, a
    // refused LDS opt-in or a refused launch leave the pass to the unstaged variant (as the chunked kernel steps back above)
    if ((ps.V & SV_STAGE) && ((uintptr_t)ma.x[0] & 15)) { ps.V &= ~SV_STAGE; ps.full = 0; }
    int lg = 0; while ((4 << lg) < ps.seg.SEG) ++lg;
    for (;;) {
        bool staged = true;
        const unsigned key = (4 << lg) == ps.seg.SEG ? ((((unsigned)ps.full * (SV_ALL + 1) + ps.V) * 3 + (zmode != 0 ? 2u : d - 1u)) * 3 + (unsigned)S->nb) * 4 + (unsigned)lg : ~0u;   // shapes: y lines, z lines, z lines of a slab
        const bool hit = with_index<2 * (SV_ALL + 1) * 3 * 3 * 4>(key, [&](auto i) {
            constexpr unsigned I = decltype(i)::value, V = I / 36 % (SV_ALL + 1); constexpr int FULL = I / (36 * (SV_ALL + 1));
            constexpr int SEG = 4 << (I & 3), NB = I / 4 % 3, DIR = I / 12 % 3 == 0 ? 1 : 2; constexpr bool SLAB = I / 12 % 3 == 2;
            if constexpr (!schur_s_legal(SEG, DIR, SLAB, NB, V) || (FULL && !(V & SV_STAGE))) return false;
            else if constexpr ((V & SV_STAGE) != 0) {
                const size_t lds = ps.seg.lds + s_stage_bytes(n, ps.seg.TX);
                const StageGrid sgr{ ps.seg.grid.x, ps.seg.grid.y };
                staged = false;
                if (lds_opt_in((const void *)k_schur_s<SEG, DIR, SLAB, NB, V, FULL>, lds)) {
                    hipLaunchKernelGGL((k_schur_s<SEG, DIR, SLAB, NB, V, FULL>), dim3(s_stage_blocks(S, ps.seg), 1, ps.seg.grid.z), ps.seg.block, lds, st, ma, mt, G, da.on ? da.L : L, da.on ? da.DR : DR,
                                       D0, n, sl, ostride, S->nx, ps.seg.TX, ps.seg.NSEG, last, partials, cg, sa, fz, lz, da.ld, sgr);
                    staged = hipGetLastError() == hipSuccess;
                }
            }
            else hipLaunchKernelGGL((k_schur_s<SEG, DIR, SLAB, NB, V, FULL>), ps.seg.grid, ps.seg.block, ps.seg.lds, st, ma, mt, G, da.on ? da.L : L, da.on ? da.DR : DR, D0, n, sl, ostride, S->nx,
                                    ps.seg.TX, ps.seg.NSEG, last, partials, cg, sa, fz, lz, da.ld);
            return true;
        });
        if (hit && (ps.V & SV_STAGE) && !staged) { ps.V &= ~SV_STAGE; ps.full = 0; continue; }   // refused: the unstaged variant
        return hit ? NF_OK : fail(NF_ERR_ARG, "k_schur_s: no instantiation for SEG = %d (s_seg), direction %d, zmode %d, NB = %d, variant \"%s\", full %d", ps.seg.SEG, d, zmode, S->nb, variant_name(ps.V).c_str(), ps.full);
    }
}

// the endpoint pass of a slab as weighted sums (k_endpoint_w) instead of a chain solve: inside the single-reduction CG (sr), weights measured,
// the fused update reading the vector the pass is applied to, and its |r|^2 partials fitting the slab's share of the partial buffer
static dim3 endpoint_w_grid(const nf_solver *S) { return dim3((unsigned)((S->nx + 63) / 64), (unsigned)S->ny); }
static bool endpoint_w_taken(const nf_team *T, const nf_solver *S, bool sr, bool fuse_reads_x)
{
    const dim3 gr = endpoint_w_grid(S);
    return sr && S->w_valid && T->opt.endpoint_weights && fuse_reads_x && (long)gr.x * gr.y <= T->slab_cap;
}
// Partition method, first half (slab teams): the endpoint pass of every slab (mode 1), the plane exchange and the separator
// values (+ Jacobi sweeps for thin slabs).  The exchange and the separator kernels run on the comm stream; ev_xchg marks
// their end -- the caller's z pass (or current reconstruction) waits for it, the x / y passes do not.
// cnt3 (if given): per slab, the |r|^2 partials that k_endpoint_w left in row 3 of the partial buffer (0 where the chain solve ran).
static int team_endpoint_phase(nf_team *T, int g, const std::vector<const double *> &xs, const std::vector<double *> &ys, const ApplyCg &A,
                               hipEvent_t after_z1, bool need_u = false, std::vector<int> *cnt3 = nullptr)
{
    const int ns = (int)T->slabs.size(); const CgScalars *cg = A.cg;
    for (int i = 0; i < ns; ++i) {
        const nf_solver *S = T->slabs[i];
        if (cnt3) (*cnt3)[i] = 0;
        if (!(S->if_lo || S->if_hi)) continue;
        const PassCg P = pass_cg(A, S, i);
        if (endpoint_w_taken(T, S, P.cg1.red != nullptr, P.fuse.p == xs[i])) {
            // single-reduction CG: the chain-end responses as weighted sums of the line's cells + the deferred CG update (k_endpoint_w)
            const dim3 gr = endpoint_w_grid(S);
            {
                hipLaunchKernelGGL(k_endpoint_w, gr, dim3(256), 0, T->stream, P.fuse.p, const_cast<double *>(P.fuse.r), (const double *)S->d_q, P.fuse.xsol,
                                   (const double *)(S->d_Wlo + (size_t)g * S->N), (const double *)(S->d_Whi + (size_t)g * S->N), S->d_clo, S->d_chi,
                                   S->nx, S->ny, S->nz, S->if_lo, S->if_hi, 40, P.cg1, cg, T->d_partials + 3 * T->partial_stride + (long)S->slab_index * T->slab_cap);
                if (cnt3) (*cnt3)[i] = (int)(gr.x * gr.y);
                T->last_endpoint_w = 1;
                continue;
            }
        }
        NFCHK(launch_s(S, 2, g, mode_args(S, g, 2, 0, xs[i], ys[i]), make_geom(S), 0, nullptr, P, nullptr, 1));
    }
    if (after_z1) (void)hipEventRecord(after_z1, T->stream);
    HIPCHK(hipEventRecord(T->ev_z1, T->stream));
    HIPCHK(hipStreamWaitEvent(T->comm_stream, T->ev_z1, 0));
    NFCHK(exchange_planes(T, 0, 0, T->comm_stream));
    auto each_slab = [&](auto &&launch) {
        for (int i = 0; i < ns; ++i) {
            nf_solver *S = T->slabs[i];
            if (S->if_lo || S->if_hi) launch(S, S->nlines[2], dim3((unsigned)((S->nlines[2] * n_modes(S) + 255) / 256)));
        }
    };
    // thick slabs (no separator sweeps): the accumulation pass forms u = (c_below + c_above) S_red^-1 itself (SlabArgs::fold)
    if (need_u || !s_fold(T, 2))
        each_slab([&](nf_solver *S, long nl, dim3 gr) {
            hipLaunchKernelGGL(k_separators, gr, dim3(256), 0, T->comm_stream, S->d_clo, S->d_chi, S->d_rlo, S->d_rhi, S->d_sinv_lo + g * nl, S->d_sinv_hi + g * nl,
                               S->d_ulo, S->d_uhi, S->d_ctlo, S->d_cthi, nl, nl * n_modes(S), S->if_lo, S->if_hi, cg); });
    for (int sweep = 0; sweep < T->sep_sweeps; ++sweep) {
        each_slab([&](nf_solver *S, long nl, dim3 gr) {
            hipLaunchKernelGGL(k_sep_couple, gr, dim3(256), 0, T->comm_stream, S->d_gfl + g * nl, S->d_ulo, S->d_uhi, S->d_elo, S->d_ehi, nl, nl * n_modes(S), S->if_lo, S->if_hi, cg); });
        NFCHK(exchange_planes(T, 2, 0, T->comm_stream));
        each_slab([&](nf_solver *S, long nl, dim3 gr) {
            hipLaunchKernelGGL(k_sep_update, gr, dim3(256), 0, T->comm_stream, S->d_ctlo, S->d_cthi, S->d_elo, S->d_ehi, S->d_relo, S->d_rehi,
                               S->d_sinv_lo + g * nl, S->d_sinv_hi + g * nl, S->d_ulo, S->d_uhi, nl, nl * n_modes(S), S->if_lo, S->if_hi, cg); });
    }
    HIPCHK(hipEventRecord(T->ev_xchg, T->comm_stream));
    return NF_OK;
}

static bool team_is_single(const nf_team *T) { return T->slabs.size() == 1 && !T->slabs[0]->if_lo && !T->slabs[0]->if_hi; }
// Split dot product of an apply inside CG (see team_schur_apply): on undivided RT0-P0 meshes outside the lean path, where a chunked long-line
// pass forms the last share (only the LAST pass forms the dot product otherwise) or on request (split_dot = 2)
static bool split_dot(const nf_team *T, bool want_dot, bool lean)
{
    const int dim = T->slabs[0]->dim;
    bool split = want_dot && dim >= 2 && team_is_single(T) && T->slabs[0]->nb == 0 && !lean && T->opt.split_dot;
    if (split && T->opt.split_dot < 2) split = chunk_plan(T->slabs[0], dim - 1).ok;
    return split;
}
// x || y (slab teams, RT0-P0, slabs small enough not to fill the chip)
static bool xy_overlap(const nf_team *T, bool any_if, bool prof)
{
    const bool xy = T->slabs[0]->dim == 3 && any_if && T->opt.xy_overlap && T->slabs[0]->nb == 0 && T->y_stream && !prof;
    bool xy_all = xy; if (xy) for (auto *X : T->slabs) xy_all = xy_all && X->N <= T->opt.xy_overlap_max_cells && !chunk_plan(X, 1).ok;
    return xy_all;
}

// y = S_g x on every local slab.  xs / ys: per-slab device pointers (nphi doubles, layout [p][e]).  With `want_dot` the
// passes of the last direction leave the block partials of x.y in the team buffer and counts[] receives the number per slab (cnt3[]: team_endpoint_phase).
static int team_schur_apply(nf_team *T, int g, const std::vector<const double *> &xs, const std::vector<double *> &ys, bool want_dot,
                            const ApplyCg &A, std::vector<int> *counts = nullptr, std::vector<int> *cnt3 = nullptr)
{
    const int ns = (int)T->slabs.size();
    const int dim = T->slabs[0]->dim;
    bool any_if = false; for (auto *S : T->slabs) any_if |= S->if_lo || S->if_hi;
    hipEvent_t a, b, ta = nullptr, tb = nullptr;
    // event-timed: every prof_every-th apply (an event record keeps the launches around it from being dispatched back to back:
    // eight records per apply cost 36 us per CG iteration at 256^3, 6 % of the iteration they are meant to measure)
    const bool prof = T->profile && (T->prof_tick++ % T->opt.prof_every == 0);
    if (prof) prof_begin(T, 3, &ta, &tb);
    if (any_if) {                                                 // partition method step 1 + interface exchange
        if (prof) prof_begin(T, 4, &a, &b);
        NFCHK(team_endpoint_phase(T, g, xs, ys, A, prof ? b : nullptr, false, cnt3));
    }
    // Split dot product (undivided RT0-P0 meshes outside the lean path, i.e. the big ones): every pass leaves the partials of ITS share
    // of x.y -- the x pass x.(C x + S_x x), the y / z passes T_a sum z_f w_f from their forward sweeps (schur_s_tile, ZW) -- one after
    // the other in the slab's segment of the partial buffer; the consumer (k_finalize) sums them all.  The last pass then needs x only
    // for its forward sweep.
    // Taken where a chunked long-line pass runs (it has no x left when its parked chunk comes back) or on request (split_dot = 2: tests);
    // elsewhere the last pass sums x_i y_i with x still in its registers, which is cheaper than three sets of partials (256^3: 504 vs
    // 531 us per CG iteration, profiles/r03_e_ab_cg.txt).
    const bool split = split_dot(T, want_dot, A.lean.st != nullptr);
    std::vector<int> totals(ns, 0);
    for (int d = 0; d < dim; ++d) {
        const int last = d == dim - 1;
        if (d == 2 && any_if) HIPCHK(hipStreamWaitEvent(T->stream, T->ev_xchg, 0));
        if (prof) prof_begin(T, d, &a, &b);
        // x || y (slab teams, RT0-P0, slabs small enough not to fill the chip): fork after the endpoint pass -- the new p is complete --,
        // the y pass of every local slab on y_stream into d_qy, join before the accumulation pass, which adds d_qy
        const bool xy_all = xy_overlap(T, any_if, prof);
        if (d == 0 && xy_all) { HIPCHK(hipEventRecord(T->ev_fork, T->stream)); HIPCHK(hipStreamWaitEvent(T->y_stream, T->ev_fork, 0)); }
        if (d == 2 && xy_all) { HIPCHK(hipEventRecord(T->ev_join, T->y_stream)); HIPCHK(hipStreamWaitEvent(T->stream, T->ev_join, 0)); }
        for (int i = 0; i < ns; ++i) {
            nf_solver *S = T->slabs[i];
            const Geom G = make_geom(S);
            if (xy_all && !S->d_qy) NFCHK(dalloc(&S->d_qy, S->nphi));
            {
                double *part = (want_dot && (last || split)) ? T->d_partials + i * T->slab_cap + totals[i] : nullptr;
                const double *xin = d > 0 && A.pnew ? A.pnew : xs[i];       // batched x_sol update: the x pass left the new direction in another slot
                const ModeArgs ma = mode_args(S, g, d, 0, xin, ys[i]);      // mode 0; the kernels derive the others (ModeTab)
                int np = 0;
                PassCg P = pass_cg(A, S, i); P.zw_dot = split;
                if (d == 0) NFCHK(launch_x(S, g, ma, G, last || split, part, P, &np));
                else if (d == 2 && (S->if_lo || S->if_hi)) {
                    P.yadd = xy_all ? S->d_qy : nullptr;
                    NFCHK(launch_s(S, 2, g, ma, G, last, part, P, &np, 2));
                } else if (d == 1 && xy_all) {
                    P.stream = T->y_stream; P.noacc = true;
                    NFCHK(launch_s(S, 1, g, mode_args(S, g, 1, 0, xin, S->d_qy), G, 0, nullptr, P, &np, 0));
                } else NFCHK(launch_s(S, d, g, ma, G, last || split, part, P, &np, 0));
                if (part) totals[i] += np;
            }
            if (counts && last) (*counts)[i] = totals[i];
        }
        if (prof) (void)hipEventRecord(b, T->stream);
    }
    if (prof) (void)hipEventRecord(tb, T->stream);
    return NF_OK;
}


int nf_schur_apply(nf_handle S, int g, const double *x_dev, double *y_dev)
{
    if (!S || !x_dev || !y_dev || g < 0 || g >= S->ng) return fail(NF_ERR_ARG, "nf_schur_apply: bad arguments");
    if (!S->built) return fail(NF_ERR_STATE, "nf_schur_apply: call nf_build first");
    nf_team *T = S->team;
    if (!team_is_single(T)) return fail(NF_ERR_STATE, "nf_schur_apply works on an undivided mesh; use nf_team_schur_apply for slabs");
    HIPCHK(hipSetDevice(S->device));
    NFCHK(line_dict_prepare(T));                                 // an undivided mesh needs nothing else of team_prepare
    NFCHK(team_schur_apply(T, g, { x_dev }, { y_dev }, false, ApplyCg()));
    // nf_set_void: the passes know no mask; the void cells' own entries are set to what the masked operator gives there, C x
    if (S->d_void) hipLaunchKernelGGL(k_void_apply_fix, dim3(grid_for(S->nphi)), dim3(256), 0, T->stream, x_dev, y_dev, (const double *)(S->d_Cd + (size_t)g * S->nphi), S->nphi, VoidMask{ S->d_void, S->N });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(T->stream));
    if (T->profile) prof_collect(T);
    return NF_OK;
}

// team variant: x/y pointer arrays with one entry per local slab (N_slab doubles each, device)
int nf_team_schur_apply(nf_handle S, int g, const double *const *x_dev, double *const *y_dev)
{
    if (!S || !x_dev || !y_dev || g < 0 || g >= S->ng) return fail(NF_ERR_ARG, "nf_team_schur_apply: bad arguments");
    if (S->team->dead) return fail(NF_ERR_COMM, "this team lost a collective (NF_ERR_COMM) and is unusable: destroy the handles and end the process with a non-zero code (never re-exec)");
    nf_team *T = S->team;
    HIPCHK(hipSetDevice(T->device));
    NFCHK(team_prepare(T));
    std::vector<const double *> xs(x_dev, x_dev + T->slabs.size()); std::vector<double *> ys(y_dev, y_dev + T->slabs.size());
    NFCHK(team_schur_apply(T, g, xs, ys, false, ApplyCg()));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(T->stream));
    if (T->profile) prof_collect(T);
    return NF_OK;
}

#ifdef NF_STAMPS
static long long *g_stamps = nullptr;
extern "C" int nf_debug_stamps(long long *out48) { if (!g_stamps) return -1; return hipMemcpy(out48, g_stamps, 48 * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2; }
#endif
// ---- fused-direction apply (k_apply3): geometry of the launch ------------------------------------
struct Fuse3Plan { bool ok = false; int nch = 1, vec = 1, seg = 8, B = 256, nblocks = 0; size_t lds = 0; Apply3 A; };
static Fuse3Plan fuse3_plan(const nf_solver *S)
{
    Fuse3Plan P; memset(&P.A, 0, sizeof P.A);
    const int K = 2, modes = n_modes(S);
    int lanes = (S->nx + K - 1) / K, lpl_log2 = 0;
    while ((1 << lpl_log2) < lanes && lpl_log2 < 6) ++lpl_log2;
    const int LPL = 1 << lpl_log2, LPW = 64 / LPL;
    const int nch = (S->nx + LPL * K - 1) / (LPL * K);
    if (nch > 4) return P;                                       // x lines beyond 512 cells: registers of a 512-thread block
    P.nch = nch <= 1 ? 1 : nch <= 2 ? 2 : 4; P.vec = S->nx % 2 == 0;
    const int nmax = std::max(S->dim >= 2 ? S->ny : 1, S->dim == 3 ? S->nz : 1);
    P.seg = S->nb > 0 ? (nmax <= 256 ? 4 : 8) : 8;
    int B = 256;
    for (int r = 0; r < 2; ++r) {
        if (S->dim < r + 2) continue;
        const int n = r == 0 ? S->ny : S->nz;
        const int NSEG = (n + P.seg - 1) / P.seg;
        if (NSEG > 64) return P;
        // small meshes: narrow tiles, so that the launch spreads over many CUs (one CU pulls ~10 B/cycle; measured with in-kernel
        // stamps at 38x38x19: 64-column tiles spent 4 us of a 6 us block in their load phase); big ones: wide rows for HBM
        int TX = S->N <= (1L << 16) ? 8 : S->N <= (1L << 18) ? 16 : S->N <= (1L << 20) ? 32 : 64;
        while (TX > 8 && TX * NSEG > 512) TX >>= 1;
        while (TX > 8 && TX / 2 >= S->nx) TX >>= 1;
        const long nxy = (long)S->nx * S->ny;
        P.A.n[r] = n; P.A.TX[r] = TX; P.A.NSEG[r] = NSEG; P.A.gx[r] = (S->nx + TX - 1) / TX; P.A.gy[r] = r == 0 ? S->nz : S->ny;
        P.A.sl[r] = r == 0 ? S->nx : nxy; P.A.ostride[r] = r == 0 ? nxy : S->nx;
        B = std::max(B, (TX * NSEG + 63) / 64 * 64);
    }
    P.B = B;
    const int nw = B / 64;
    P.A.ntask_x = (int)((S->nlines[0] + LPW - 1) / LPW); P.A.lpl_log2 = lpl_log2;
    P.A.nbx = (int)(((long)P.A.ntask_x * modes + nw - 1) / nw);
    P.A.nby = S->dim >= 2 ? P.A.gx[0] * P.A.gy[0] * modes : 0;
    P.A.nbz = S->dim == 3 ? P.A.gx[1] * P.A.gy[1] * modes : 0;
    P.nblocks = P.A.nbx + P.A.nby + P.A.nbz;
    P.lds = (size_t)(4 * B + 320 + 16) * sizeof(double);
    P.A.stamps = nullptr;
#ifdef NF_STAMPS
    { static long long *d_st = nullptr; if (!d_st) (void)hipMalloc((void **)&d_st, 48 * sizeof(long long)); P.A.stamps = d_st; g_stamps = d_st; }
#endif
    P.ok = true;
    return P;
}
// The instantiations of k_apply3<NCH, VEC, NB, SEG>: up to four chunks per lane; 8-cell segments, and 4-cell ones for the bubble moments
constexpr bool apply3_legal(int NCH, int NB, int SEG) { return NCH >= 1 && NCH <= 4 && NB >= 0 && NB <= 2 && (SEG == 8 || (SEG == 4 && NB > 0)); }
// one k_apply3 launch: q_d = S_d p for every direction; pin = the vector the iteration reads, pout = where the new p goes
static int launch_apply3(nf_solver *S, int g, const Fuse3Plan &P, const double *pin, double *pout, double *xsol, const CgLean &lean)
{
    nf_team *T = S->team; hipStream_t st = T->stream;
    const long N = S->N;
    const Geom G = make_geom(S);
    ModeArgs ma[3]; ModeTab mt[3]; const double *L[3], *DR[3], *D0[3];
    double *qd[3] = { S->d_q, S->d_qy, S->d_qz };
    for (int d = 0; d < 3; ++d) {
        const int dd = d < S->dim ? d : 0;
        ma[d] = mode_args(S, g, dd, 0, pin, qd[dd]); mt[d] = mode_tab(S, dd);
        L[d] = S->d_L[dd] + g * N; DR[d] = S->d_DR[dd] + g * N; D0[d] = S->d_D0[dd] + g * S->nlines[dd];
    }
    const CgFuse fz = { const_cast<double *>(pin), S->d_r, xsol, pout };
    int lg = 0; while ((1 << lg) < P.nch) ++lg;
    const unsigned key = (P.seg == 4 || P.seg == 8) ? ((((unsigned)lg * 2 + (P.vec ? 1u : 0u)) * 3 + (unsigned)S->nb) * 2 + (P.seg == 8 ? 1u : 0u)) : ~0u;
    const bool hit = with_index<3 * 2 * 3 * 2>(key, [&](auto i) {
        constexpr unsigned I = decltype(i)::value;
        constexpr int NCH = 1 << (I / 12), NB = I / 2 % 3, SEG = (I & 1) ? 8 : 4; constexpr bool VEC = I / 6 % 2;
        if constexpr (!apply3_legal(NCH, NB, SEG)) return false;
        else hipLaunchKernelGGL((k_apply3<NCH, VEC, NB, SEG>), dim3((unsigned)P.nblocks), dim3((unsigned)P.B), P.lds, st, ma[0], ma[1], ma[2], mt[0], mt[1], mt[2], G,
                                L[0], DR[0], D0[0], L[1], DR[1], D0[1], L[2], DR[2], D0[2], S->nx, S->ny, S->nlines[0], P.A, T->d_partials, T->d_cg, fz, lean);
        return true;
    });
    if (!hit) return fail(NF_ERR_ARG, "k_apply3: no instantiation for NCH = %d, vec %d, NB = %d, SEG = %d", P.nch, P.vec, S->nb, P.seg);
    return NF_OK;
}

// ---- whole CG solve on one XCD (k_cg_xcd) ---------------------------------------------------------
// CgScalars hold the outcome of FIN_RHS, r = p = rhs, x = 0.  One launch; the kernel publishes the final scalars to the host itself.
static bool xcd_eligible(const nf_team *T, const nf_solver *S, const Fuse3Plan &P)
{
    if (!T->opt.cg_xcd || !P.ok || T->profile || S->d_void) return false;   // nf_set_void: the one-launch kernels keep their CG vectors to themselves and know no mask
    if (S->nb == 0 ? (S->nloc != 1 || n_modes(S) != 1) : (P.seg != 4 || n_modes(S) > 9 || S->nb > 2)) return false;   // P0 flux: one unknown per cell; bubble moments: the SEG = 4 tiles
    if (S->nphi < T->opt.cg_xcd_min_cells || S->nphi > T->opt.cg_xcd_max_cells) return false;                                      // the window counts unknowns per group
    for (int r = 0; r < 2; ++r) if (S->dim >= r + 2 && (P.A.NSEG[r] >= 64 || P.A.TX[r] * P.A.NSEG[r] > 448)) return false;   // no wavefront scan in the packed tiles; a tile fits beside the other roles
    return S->nx <= 128;                                          // x lines: at most two chunks per lane (128 VGPRs at 1024 threads)
}
// geometry, factors (of group g) and CG vectors of a k_cg_xcd / k_keff_xcd launch; *nch_out: chunks per lane of the x lines
static int xcd_fill(nf_solver *S, int g, const Fuse3Plan &P, XcdArgs &A, int *nch_out)
{
    nf_team *T = S->team;
    const long N = S->N;
    if (!T->d_xcd) { HIPCHK(hipMalloc((void **)&T->d_xcd, sizeof(XcdState))); NFCHK(dalloc(&T->d_xpart, 512)); HIPCHK(hipMemset(T->d_xpart, 0, 512 * sizeof(double))); }
    HIPCHK(hipMemsetAsync(T->d_xcd, 0, sizeof(XcdState), T->stream));
    memset(&A, 0, sizeof A);
    A.G = make_geom(S);
    double *qd[3] = { S->d_q, S->d_qy, S->d_qz };
    for (int d = 0; d < 3; ++d) {
        const int dd = d < S->dim ? d : 0;
        A.ma[d] = mode_args(S, g, dd, 0, S->d_p, qd[dd]);
        A.L[d] = S->d_L[dd] + g * N; A.DR[d] = S->d_DR[dd] + g * N; A.D0[d] = S->d_D0[dd] + g * S->nlines[dd]; A.q[d] = qd[dd];
    }
    A.nx = S->nx; A.ny = S->ny; A.dim = S->dim; A.nlines_x = S->nlines[0]; A.N = S->nphi;
    A.nmodes = n_modes(S);
    for (int d = 0; d < 3; ++d) A.mt[d] = mode_tab(S, d < S->dim ? d : 0);
    // x lines: few wavefronts matter more here than short scans (the roles share the 12 wavefronts of a workgroup, and a second round
    // costs a whole memory round trip): two chunks per lane from 33 cells on -- 38 cells = 16 lanes x 2 cells x 2 chunks, four lines
    // per wavefront, where the launch path takes 32 lanes and two lines
    int lanes = (S->nx + 1) / 2, lpl_log2 = 0;
    while ((1 << lpl_log2) < lanes && lpl_log2 < 5) ++lpl_log2;
    int nch = (lanes + (1 << lpl_log2) - 1) >> lpl_log2;
    if (nch == 1 && lpl_log2 == 5) {
        // 32 lanes, one chunk (the shorter chain) if the three roles of a workgroup still fit its wavefronts in one round
        const int Pn = T->opt.cg_xcd_groups, tasks = (int)((S->nlines[0] + 1) / 2) * A.nmodes;
        int waves = (tasks + Pn - 1) / Pn;
        for (int r = 0; r < 2; ++r) if (S->dim >= r + 2) waves += (((P.A.gx[r] * P.A.gy[r] * A.nmodes + Pn - 1) / Pn) * P.A.TX[r] * P.A.NSEG[r] + 63) / 64;
        if (waves > XCD_THREADS / 64) { lpl_log2 = 4; nch = 2; }
    }
    if (nch > 2) return fail(NF_ERR_STATE, "k_cg_xcd: x lines of %d cells", S->nx);
    A.lpl_log2 = lpl_log2; A.ntask_x = (int)((S->nlines[0] + (64 >> lpl_log2) - 1) / (64 >> lpl_log2));
    for (int r = 0; r < 2; ++r) { A.n[r] = P.A.n[r]; A.TX[r] = P.A.TX[r]; A.NSEG[r] = P.A.NSEG[r]; A.gx[r] = P.A.gx[r]; A.gy[r] = P.A.gy[r]; A.sl[r] = P.A.sl[r]; A.ostride[r] = P.A.ostride[r]; }
    if (S->dim < 2) { A.TX[0] = A.NSEG[0] = 1; } if (S->dim < 3) { A.TX[1] = A.NSEG[1] = 1; }
    A.pA = S->d_p; A.pB = S->d_p2; A.r = S->d_r;
    A.part = T->d_xpart; A.st = T->d_xcd; A.xcc = T->opt.cg_xcd_id;
    *nch_out = nch;
    return NF_OK;
}
// The instantiations of k_cg_xcd / k_keff_xcd<NCH, VEC, NB, SEG>: one or two chunks per lane; 8-cell segments for the P0 flux, 4-cell ones
// for the bubble moments (xcd_eligible).  launch(XcdInst) opts the kernel of its family in to the LDS and launches it.
constexpr bool xcd_legal(int NCH, int NB, int SEG) { return NCH >= 1 && NCH <= 2 && NB >= 0 && NB <= 2 && SEG == (NB == 0 ? 8 : 4); }
template <int NCH_, bool VEC_, int NB_, int SEG_> struct XcdInst { static constexpr int NCH = NCH_, NB = NB_, SEG = SEG_; static constexpr bool VEC = VEC_; };
template <class F> static int xcd_select(const char *name, const nf_solver *S, const Fuse3Plan &P, int nch, F &&launch)
{
    int rc = NF_OK;
    const unsigned key = (P.seg == 4 || P.seg == 8) ? ((((unsigned)(nch - 1) * 2 + (P.vec ? 1u : 0u)) * 3 + (unsigned)S->nb) * 2 + (P.seg == 8 ? 1u : 0u)) : ~0u;
    const bool hit = with_index<2 * 2 * 3 * 2>(key, [&](auto i) {
        constexpr unsigned I = decltype(i)::value;
        constexpr int NCH = 1 + I / 12, NB = I / 2 % 3, SEG = (I & 1) ? 8 : 4; constexpr bool VEC = I / 6 % 2;
        if constexpr (!xcd_legal(NCH, NB, SEG)) return false;
        else { rc = launch(XcdInst<NCH, VEC, NB, SEG>()); return true; }
    });
    return hit ? rc : fail(NF_ERR_ARG, "%s: no instantiation for NCH = %d, vec %d, NB = %d, SEG = %d", name, nch, P.vec, S->nb, P.seg);
}
static const size_t XCD_LDS = (size_t)(5 * 1024 + 64 + 32) * sizeof(double);
static int launch_cg_xcd(nf_solver *S, int g, const Fuse3Plan &P, double *xsol, unsigned long long seq)
{
    nf_team *T = S->team; hipStream_t st = T->stream;
    XcdArgs A; int nch = 1;
    NFCHK(xcd_fill(S, g, P, A, &nch));
    A.xsol = xsol; A.cg = T->d_cg; A.hp = T->d_pub; A.seq = seq;
    const size_t lds = XCD_LDS; const unsigned G = 8u * (unsigned)T->opt.cg_xcd_groups;
    NFCHK(xcd_select("k_cg_xcd", S, P, nch, [&](auto t) -> int { using I = decltype(t);
        if (!lds_opt_in((const void *)k_cg_xcd<I::NCH, I::VEC, I::NB, I::SEG>, lds)) return fail(NF_ERR_HIP, "k_cg_xcd: %zu bytes of LDS refused", lds);
        hipLaunchKernelGGL((k_cg_xcd<I::NCH, I::VEC, I::NB, I::SEG>), dim3(G), dim3(XCD_THREADS), lds, st, A);
        return NF_OK;
    }));
    HIPCHK(hipGetLastError());
    return NF_OK;
}
// ---- the forms of the CG iteration: cg_plan is the only place that chooses one.  cg_solve runs the plan, nf_apply_plan and nf_info report it, solve_keff_impl asks it whether
// the one-XCD kernels apply.  What an iteration of each form launches: the table of DESIGN.md 3 and the cg_step functions.  fused: x_sol / p
// updates ride in the next x pass (RT0-P0 undivided mesh; k_schur_x, CgFuse) or in the endpoint pass of the z lines, the first pass to read
// p (slab teams, P0).  The order is nf_info "cg_form".
enum CgForm { CG_XCD, CG_FUSE3, CG_LEAN, CG_FUSED, CG_CLASSIC, CG_TEAM_LEAN, CG_TEAM_VEC, CG_TEAM_SR };
static const char *const CG_FORM_NAME[] = { "xcd", "fuse3", "lean", "fused", "classic", "team_lean", "team_vec", "team_sr" };
struct CgPlan {
    CgForm form = CG_CLASSIC; Fuse3Plan f3; int gru = 0;         // f3: xcd, fuse3; gru: those and lean (blocks of k_cg_rupdate / k_cg_rupdate3)
    bool fused = false; int reductions = 0;                      // ApplyCg::fused (every form but classic); cross-rank reductions per iteration (nf_info "cg_reductions")
    bool lean() const { return form == CG_XCD || form == CG_FUSE3 || form == CG_LEAN; }   // ApplyCg::lean is set
    int xsol_batch = 1;                                          // fused: x_sol is updated in every M-th x pass (nf_xsol_ring.h); 1 = in every pass
};
// What xsol_batch = -1 resolves to beyond cg_lean_max_cells.
static const int XSOL_BATCH_AUTO = 4;
static CgPlan cg_plan_form(const nf_team *T);
static CgPlan cg_plan(const nf_team *T)
{
    CgPlan P = cg_plan_form(T); const nf_solver *S0 = T->slabs[0];
    // the ring of directions: the fused form (scalars behind k_finalize: its alpha history) on an undivided RT0-P0 mesh whose x pass has the
    // instantiations; a handle whose ring the device refused stays with one buffer
    if (P.form != CG_FUSED || !team_is_single(T) || !x_fuses(S0) || S0->nb != 0 || S0->ring_refused) return P;
    const int nch = x_plan(S0).NCH;
    if (nch < 1 || nch > X_BATCH_MAX_NCH) return P;
    const long o = T->opt.xsol_batch;
    P.xsol_batch = o < 0 ? (S0->N > T->opt.cg_lean_max_cells ? XSOL_BATCH_AUTO : 1) : (int)std::min<long>(std::max<long>(o, 1), NF_XSOL_RING_MAX);
    return P;
}
static CgPlan cg_plan_form(const nf_team *T)
{
    CgPlan P; const nf_solver *S0 = T->slabs[0]; const bool single = team_is_single(T);
    P.fused = T->opt.cg_fuse != 0 && (single || S0->nloc == 1);
    P.reductions = single ? 0 : 2;
    P.form = P.fused ? CG_FUSED : CG_CLASSIC;
    if (!P.fused || !T->opt.cg_lean) return P;
    if (!single) {
        bool sr = T->opt.cg_single_reduce > 0 || (T->opt.cg_single_reduce < 0 && T->team_max_cells <= T->opt.cg_single_reduce_max_cells);
        for (auto *S : T->slabs) sr = sr && S->dim == 3 && S->nb == 0 && (T->opt.s_seg == 0 || T->opt.s_seg == 8) && S->nz <= 1024;
        const bool vec = T->nproc > 1 && T->slabs.size() == 1 && T->vec_ok && T->opt.vec_reduce;
        P.form = sr ? CG_TEAM_SR : vec ? CG_TEAM_VEC : CG_TEAM_LEAN; P.reductions = sr ? 1 : 2;
        return P;
    }
    if (T->rccl_reduce || S0->N > T->opt.cg_lean_max_cells) return P;
    P.form = CG_LEAN;
    // every block of the next x pass sums the |r|^2 partials; fewer partials (cg_lean_grid) cost k_cg_rupdate more than they save (measured)
    P.gru = grid_for(S0->nphi, 256, T->opt.cg_lean_grid);
    if (!T->opt.cg_fuse3 || S0->N > T->opt.cg_fuse3_max_cells) return P;
    P.f3 = fuse3_plan(S0);
    if (P.f3.ok && P.f3.nblocks > T->slab_cap) P.f3.ok = false;  // cannot decide: slab_partial_need counts a partial per block of this launch
    if (P.f3.ok) P.form = xcd_eligible(T, S0, P.f3) ? CG_XCD : CG_FUSE3;
    return P;
}

// ---- read-only report of the launch plan -------------------------------------------------------
// What the next Schur apply on this handle's mesh (or slab) would launch, per direction, as one JSON object.  It prints what
// the launch functions execute (x_plan for the x pass, s_pass for a y / z pass) and calls the predicates they call (endpoint_w_taken, cg_plan,
// split_dot, xy_overlap); apart from building the tables of distinct lines where the next
// apply would (line_dict_prepare) it launches nothing and writes no state.  The one thing it cannot know is a device
// that refuses the chunked kernel's LDS at launch time (launch_s then falls back to the one-chunk kernel).
struct PlanPass { const char *dir, *family; int mode, SEG, NCH, TX, NSEG; dim3 grid; unsigned block; bool nt, zw, order; unsigned tiles; bool fold = false, dict = false; int early = 0; unsigned V = 0, blocks = 0; int full = 0; };
static void plan_emit(std::string &js, const PlanPass &p)
{
    char tmp[416];
    snprintf(tmp, sizeof tmp, "%s{\"dir\": \"%s\", \"mode\": %d, \"family\": \"%s\", \"SEG\": %d, \"NCH\": %d, \"TX\": %d, \"NSEG\": %d, \"grid\": [%u, %u, %u], "
             "\"block\": %u, \"nt\": %d, \"zw\": %d, \"xcd_order\": %d, \"xcd_permutes\": %d, \"fold\": %d, \"dict\": %d, \"early\": %d", js.back() == '[' ? "" : ", ", p.dir, p.mode, p.family,
             p.SEG, p.NCH, p.TX, p.NSEG, p.grid.x, p.grid.y, p.grid.z, p.block, p.nt ? 1 : 0, p.zw ? 1 : 0, p.order ? 1 : 0, xcd_permutes(p.order, p.tiles) ? 1 : 0, p.fold ? 1 : 0, p.dict ? 1 : 0, p.early);
    js += tmp;
    if (!strcmp(p.family, "s")) js += ", \"variant\": \"" + variant_name(p.V) + "\"";   // which k_schur_s
    if (p.dir[0] != 'x') js += ", \"stage\": " + std::to_string((p.V & SV_STAGE) && !strcmp(p.family, "s") ? 1 : 0) + ", \"blocks\": " + std::to_string(p.blocks)   // launched blocks (staged: persistent)
                            + ", \"full\": " + std::to_string(p.full);
    js += "}";
}
static int plan_s(std::string &js, const nf_solver *S, int d, int zmode, bool want_dot, bool zw_dot, bool fuse, bool cg1)   // a launch_s call
{
    const SPass ps = s_pass(S, d, zmode, want_dot, zw_dot, fuse, cg1);
    if (ps.rc != NF_OK) return ps.rc;
    const dim3 gr = ps.chunked ? c_grid(S, d, ps.cp) : ps.seg.grid;
    plan_emit(js, { d == 1 ? "y" : "z", ps.chunked ? "c" : "s", zmode, ps.chunked ? C_SEG : ps.seg.SEG, ps.chunked ? C_NCH : 1, ps.chunked ? ps.cp.TX : ps.seg.TX, ps.chunked ? ps.cp.NS : ps.seg.NSEG,
                    gr, ps.chunked ? c_block(ps.cp) : ps.seg.block.x, (ps.V & SV_NT) != 0, (ps.V & SV_ZW) != 0, ps.xcd != 0, gr.x * gr.y, ps.fold, (ps.V & SV_DICT) != 0, ps.early, ps.V,
                    !ps.chunked && (ps.V & SV_STAGE) ? s_stage_blocks(S, ps.seg) * gr.z : gr.x * gr.y * gr.z, ps.full });
    return NF_OK;
}
int nf_apply_plan(nf_handle S, int in_cg, char *json_buf, size_t len)
{
    if (!S || !json_buf || len < 2) return fail(NF_ERR_ARG, "nf_apply_plan: bad arguments");
    if (!S->built) return fail(NF_ERR_STATE, "nf_apply_plan: call nf_build first");
    // the tables of distinct lines are part of what the next apply does: it would build them first, so the report does (its only side effect)
    HIPCHK(hipSetDevice(S->team->device));
    NFCHK(line_dict_prepare(S->team));
    const nf_team *T = S->team;
    const bool slab = S->if_lo || S->if_hi;
    // a team settles the separator sweeps, the endpoint weights and its largest slab when it is prepared (the first team apply or solve)
    if (!team_is_single(T) && !T->linked_ready) return fail(NF_ERR_STATE, "nf_apply_plan: run a team apply or solve first (the team has not been prepared since its options changed)");
    // cg_solve applies S to d_p with CgFuse::p = d_p when fused (`P.fuse.p == xs[i]` of team_endpoint_phase) and asks for the dot product of every
    // apply: the last pass, and every pass under the split dot product, gets a partial buffer.  xcd and fuse3 launch no Schur pass: theirs
    // are the passes of the launch path (lean) such a solve would fall back to.
    const CgPlan cp = cg_plan(T);
    const bool cg = in_cg != 0, fused = cg && cp.fused, lean = cg && cp.lean(), sr = cg && cp.form == CG_TEAM_SR;
    const bool split = split_dot(T, cg, lean);
    bool any_if = false; for (auto *X : T->slabs) any_if |= X->if_lo || X->if_hi;
    const bool xy_all = xy_overlap(T, any_if, false);
    char tmp[320];
    snprintf(tmp, sizeof tmp, "{\"in_cg\": %d, \"form\": \"%s\", \"xsol_batch\": %d, \"slab\": %d, \"fused\": %d, \"lean\": %d, \"single_reduce\": %d, \"split_dot\": %d, \"xy_overlap\": %d, \"passes\": [",
             cg ? 1 : 0, cg ? CG_FORM_NAME[cp.form] : "", cg ? cp.xsol_batch : 1, slab ? 1 : 0, fused ? 1 : 0, lean ? 1 : 0, sr ? 1 : 0, split ? 1 : 0, xy_all ? 1 : 0);
    std::string js = tmp;
    for (int d = 0; d < S->dim; ++d) {
        const bool last = d == S->dim - 1, want_dot = cg && (last || split);
        if (d == 0) {
            const XPlan xp = x_plan(S);
            if (!xp.NCH) return fail(NF_ERR_UNSUPPORTED, "nx = %d exceeds the x-line kernel limit (%d cells)", S->nx, S->nb == 0 ? 4096 : 1024);
            plan_emit(js, { "x", "x", 0, 0, xp.NCH, 1 << xp.lpl_log2, 0, dim3(xp.grid, (unsigned)n_modes(S)), 256u, xp.nt, false, xp.xcd, xp.grid, false, xp.dict });
        } else if (d == 2 && slab) {
            // endpoint pass: inside the fused CG the update reads the vector the pass is applied to (cg_solve applies to d_p)
            if (endpoint_w_taken(T, S, sr, fused)) { const dim3 gr = endpoint_w_grid(S); plan_emit(js, { "z", "endpoint_w", 1, 0, 0, 64, 0, gr, 256u, false, false, false, gr.x * gr.y }); }
            else NFCHK(plan_s(js, S, 2, 1, false, false, fused, sr));
            NFCHK(plan_s(js, S, 2, 2, want_dot, split, fused, sr));
        } else if (d == 1 && xy_all) NFCHK(plan_s(js, S, 1, 0, false, split, fused, sr));
        else NFCHK(plan_s(js, S, d, 0, want_dot, split, fused, sr));
    }
    {   // distinct lines of the largest group per direction, 0 where the direction does not use its table
        int nd[3] = { 0, 0, 0 };
        for (int d = 0; d < S->dim; ++d) if (dict_dir(S, d)) nd[d] = *std::max_element(S->ld_rows[d].begin(), S->ld_rows[d].end());
        snprintf(tmp, sizeof tmp, "], \"line_dict\": {\"x\": %d, \"y\": %d, \"z\": %d}}", nd[0], nd[1], nd[2]);
        js += tmp;
    }
    if (js.size() + 1 > len) return fail(NF_ERR_ARG, "nf_apply_plan: buffer of %zu bytes is too small (%zu needed)", len, js.size() + 1);
    memcpy(json_buf, js.c_str(), js.size() + 1);
    return NF_OK;
}

// ---- CG (SchurSolver::SolveSchurImplicit, src/solvers.cpp:577-636) -----------------------------
// What the pieces of one cg_solve share.  form: the plan's, or fuse3 after a one-XCD start that was not to be (no mapped page, refused, timed out).
// Lean, vector reduce: row 0 of the partial buffer holds the p.q partials of the last direction pass, row 1 the |r|^2 partials of k_cg_rupdate
// (vector reduce: + a flag slot each; d_vec: the two rows all-reduced).
struct CgRun {
    nf_team *T; int g; const CgPlan &P; CgForm form; const std::vector<double *> &x;   // x: the solution, per slab
    std::vector<const double *> ps; std::vector<double *> qs;     // p and q = S p, per slab
    std::vector<int> gcnt, acnt, cnt3;                             // per slab: blocks of the vector kernels, p.q partials of the apply, |r|^2 partials of k_endpoint_w
    bool any_if = false;                                           // some local slab has an interface
    int M = 1;                                                     // the plan's xsol_batch, or 1 where the ring could not be allocated
    double *slot(int s) const { nf_solver *S = T->slabs[0]; return s == 0 ? S->d_p : S->d_ring + (size_t)(s - 1) * S->nphi; }   // of the ring of directions
    double *row1() const { return T->d_partials + T->partial_stride; }
    double *vec_rr() const { return T->d_vec + T->vec_stride; }
    // a failed call inside the iteration: NF_OK if the rank is poisoned and carries on with the schedule, the code if it must leave at once
    int chk(int rc) const { return team_poison(T, rc, form == CG_TEAM_VEC) ? rc : NF_OK; }
    template <class F> void each_slab(F &&launch) const { if (!T->poisoned) for (size_t i = 0; i < T->slabs.size(); ++i) launch(T->slabs[i], (int)i); }   // a poisoned rank launches no compute
};
// The CG state an apply of iteration `index` consumes, and with index = the iterations launched so far what the batch-end stop test reads
static ApplyCg cg_apply_args(const CgRun &R, int index)
{
    nf_team *T = R.T; const int first = index == 0 ? 1 : 0;
    ApplyCg A; A.cg = T->d_cg; A.fused = R.P.fused; A.xsol = &R.x;
    if (R.form == CG_FUSE3 || R.form == CG_LEAN) A.lean = CgLean{ T->d_cg, R.row1(), R.P.gru, index & 1, first };
    if (R.form == CG_TEAM_SR) A.cg1 = Cg1{ T->d_red, T->d_cg, index };
    if (R.form == CG_TEAM_VEC) A.lean_z1 = CgLean{ T->d_cg, R.vec_rr(), T->vec_cnt_rr, index & 1, first, T->vec_cnt_rr };
    if (R.form == CG_TEAM_LEAN) A.lean_z1 = CgLean{ T->d_cg, T->d_red + 2, -1, index & 1, first };
    if (R.M > 1) {                                                // the slots of iteration `index` (nf_xsol_ring.h)
        const int rd = nf_ring_read(index, R.M), wr = nf_ring_write(index, R.M);
        const NfRingBatch B = nf_ring_apply(index, R.M);
        A.ring = true; A.xb = index == 0 ? XB_NOW : B.n ? XB_APPLY : XB_SKIP; A.pnew = R.slot(wr);
        A.ringfz = CgFuse{ R.slot(rd), T->slabs[0]->d_r, R.x[0], wr == rd ? nullptr : R.slot(wr) };
        if (B.n) {                                                // all but the last, which is the direction the pass reads
            A.ringfz.nold = B.n - 1; A.ringfz.a0 = B.u[0].alpha; A.ringfz.ah = T->d_ah;
            for (int i = 0; i + 1 < B.n; ++i) A.ringfz.old[i] = R.slot(B.u[i].slot);
        }
    }
    return A;
}
// fuse3: two launches.  p lives in a pair of buffers: iteration 0 reads A = d_p as k_cg_init left it; iteration i >= 1 reads the p of
// iteration i-1 (A for odd i, B for even i) and writes r + beta p into the other one
static int cg_step_fuse3(CgRun &R, int index)
{
    nf_team *T = R.T; nf_solver *S0 = T->slabs[0];
    double *A = S0->d_p, *B = S0->d_p2;
    double *pin = (index == 0 || (index & 1)) ? A : B, *pout = pin == A ? B : A;
    hipEvent_t ta = nullptr, tb = nullptr;
    const bool prof = T->profile && (T->prof_tick++ % T->opt.prof_every == 0);
    if (prof) prof_begin(T, 3, &ta, &tb);
    const int rc = launch_apply3(S0, R.g, R.P.f3, pin, pout, R.x[0], cg_apply_args(R, index).lean);
    if (prof) (void)hipEventRecord(tb, T->stream);
    with_void(S0, [&](auto M, VoidMask vm) {
        hipLaunchKernelGGL(k_cg_rupdate3<decltype(M)::value>, dim3(R.P.gru), dim3(256), 0, T->stream, S0->d_r, (const double *)S0->d_q, (const double *)(S0->dim >= 2 ? S0->d_qy : nullptr),
                           (const double *)(S0->dim == 3 ? S0->d_qz : nullptr), S0->nphi, T->d_cg, R.row1(), CgLean{ T->d_cg, T->d_partials, R.P.f3.nblocks, index & 1, 0 }, vm); });
    return rc;
}
// every other form: q = S p with the form's CG state; on a poisoned rank, what the apply owes its neighbours instead
static int cg_step_apply(CgRun &R, int index, long global_it)
{
    nf_team *T = R.T;
    T->xchg_in_apply = 0;
    int ra = NF_OK;
    if (T->nproc > 1 && T->rank == T->inject_rank && global_it == T->inject_iter)
        { ra = fail(NF_ERR_HIP, "injected failure on rank %d at CG iteration %ld (NEUTFEM_INJECT_FAIL)", T->rank, global_it); TRACE_COMM("rank %d INJECT at %ld", T->rank, global_it); }
    else if (!T->poisoned) {
        const ApplyCg A = cg_apply_args(R, index);
        if (A.ring) R.ps[0] = A.ringfz.p;                         // the x pass reads the direction of the iteration before from its slot
        ra = team_schur_apply(T, R.g, R.ps, R.qs, true, A, &R.acnt, &R.cnt3);
    }
    NFCHK(R.chk(ra));
    if (T->poisoned && R.any_if) {
        // the interface exchanges this apply still owes its neighbours: one per apply + one per separator sweep (team_endpoint_phase)
        // with the stream dependencies of team_endpoint_phase: the exchange waits for the solver's stream (ev_z1), the reductions
        // wait for the exchange (ev_xchg).  Without the first one the comm stream runs iterations ahead, and a transport whose
        // operations of one process share a progress thread (the stand-in does; RCCL's proxy has the same shape) deadlocks: this
        // rank blocks in the NEXT iteration's receive while its peers still wait for it in THIS iteration's all-reduce.
        if (T->xchg_in_apply == 0) { (void)hipEventRecord(T->ev_z1, T->stream); (void)hipStreamWaitEvent(T->comm_stream, T->ev_z1, 0); }
        for (int k = T->xchg_in_apply; k < 1 + T->sep_sweeps; ++k) (void)exchange_planes(T, k == 0 ? 0 : 2, 0, T->comm_stream);
        (void)hipEventRecord(T->ev_xchg, T->comm_stream); (void)hipStreamWaitEvent(T->stream, T->ev_xchg, 0);
        // a poisoned rank skips the apply, so cnt3 still holds the counts of its last one: cleared with acnt.  team_reduce_sr reads
        // cnt3[i] only where acnt[i] > 0, so the reduction sees no partials of this rank in any row either way
        for (size_t i = 0; i < R.acnt.size(); ++i) R.acnt[i] = R.cnt3[i] = 0;
    }
    return NF_OK;
}
// what follows the apply, per form
static int cg_step_team_sr(CgRun &R, int) { return R.chk(team_reduce_sr(R.T, R.acnt, R.cnt3)); }   // the one reduction of the iteration; its consumer is the next endpoint pass
static int cg_step_team_vec(CgRun &R, int index)                   // the partial vectors themselves cross the ranks; their consumers sum them (CgLean with a count and a flag slot)
{
    nf_team *T = R.T; double *send_pq = T->d_partials, *send_rr = R.row1(), *vec_pq = T->d_vec;
    auto allred = [&](double *send, double *recv, int cnt) -> int { NCCLCHK(g_rccl.AllReduce(send, recv, (size_t)cnt + 1, NCCL_DOUBLE, NCCL_SUM, T->comm, T->stream)); return NF_OK; };
    if (!T->poisoned && R.acnt[0] != T->vec_cnt_pq) NFCHK(R.chk(fail(NF_ERR_STATE, "vector reduce: the accumulation pass left %d partials, %d were agreed", R.acnt[0], T->vec_cnt_pq)));
    NFCHK(R.chk(allred(send_pq, vec_pq, T->vec_cnt_pq)));
    R.each_slab([&](nf_solver *S, int i) { hipLaunchKernelGGL(k_cg_rupdate<false>, dim3(R.gcnt[i]), dim3(256), 0, T->stream, S->d_r, S->d_q, S->nphi, T->d_cg, send_rr, CgLean{ T->d_cg, vec_pq, T->vec_cnt_pq, index & 1, 0, T->vec_cnt_pq }, VoidMask{ nullptr, 0 }); });
    return R.chk(allred(send_rr, R.vec_rr(), T->vec_cnt_rr));
}
static int cg_step_team_lean(CgRun &R, int index)
{
    nf_team *T = R.T;
    NFCHK(R.chk(team_reduce(T, R.acnt, T->d_red)));               // d_red[0] = p.q, d_red[1] = error flags
    R.each_slab([&](nf_solver *S, int i) { hipLaunchKernelGGL(k_cg_rupdate<false>, dim3(R.gcnt[i]), dim3(256), 0, T->stream, S->d_r, S->d_q, S->nphi, T->d_cg, T->d_partials + i * T->slab_cap, CgLean{ T->d_cg, T->d_red, -1, index & 1, 0 }, VoidMask{ nullptr, 0 }); });
    return R.chk(team_reduce(T, R.gcnt, T->d_red + 2));           // d_red[2] = |r|^2, d_red[3] = error flags
}
static int cg_step_lean(CgRun &R, int index)
{
    R.each_slab([&](nf_solver *S, int) { with_void(S, [&](auto M, VoidMask vm) {
        hipLaunchKernelGGL(k_cg_rupdate<decltype(M)::value>, dim3(R.P.gru), dim3(256), 0, R.T->stream, S->d_r, S->d_q, S->nphi, R.T->d_cg, R.row1(), CgLean{ R.T->d_cg, R.T->d_partials, R.acnt[0], index & 1, 0 }, vm); }); });
    return NF_OK;
}
static int cg_step_scalar(CgRun &R, int)                           // fused, classic: the scalars behind k_finalize
{
    nf_team *T = R.T; const bool fused = R.form == CG_FUSED;
    NFCHK(R.chk(team_finalize(T, FIN_PAP, R.acnt, 1, T->d_out, 0.0, 0)));
    R.each_slab([&](nf_solver *S, int i) { with_void(S, [&](auto M, VoidMask vm) {
        if (fused) hipLaunchKernelGGL(k_cg_rupdate<decltype(M)::value>, dim3(R.gcnt[i]), dim3(256), 0, T->stream, S->d_r, S->d_q, S->nphi, T->d_cg, T->d_partials + i * T->slab_cap, CgLean{}, vm);
        else hipLaunchKernelGGL(k_cg_update<decltype(M)::value>, dim3(R.gcnt[i]), dim3(256), 0, T->stream, R.x[i], S->d_r, S->d_p, S->d_q, S->nphi, T->d_cg, T->d_partials + i * T->slab_cap, vm); }); });
    NFCHK(R.chk(team_finalize(T, FIN_RR, R.gcnt, 1, T->d_out, 0.0, 0)));
    if (!fused) R.each_slab([&](nf_solver *S, int i) { hipLaunchKernelGGL(k_cg_pupdate, dim3(R.gcnt[i]), dim3(256), 0, T->stream, S->d_p, S->d_r, S->nphi, T->d_cg); });
    return NF_OK;
}
static int cg_step(CgRun &R, int index, long global_it)           // iteration `index` of the solve in the run's form
{
    static int (*const after_apply[])(CgRun &, int) = { nullptr, nullptr, cg_step_lean, cg_step_scalar, cg_step_scalar, cg_step_team_lean, cg_step_team_vec, cg_step_team_sr };   // by CgForm
    if (R.form == CG_FUSE3) return cg_step_fuse3(R, index);
    NFCHK(cg_step_apply(R, index, global_it));
    return after_apply[R.form](R, index);
}
// The stop test of a batch's last iteration where the form leaves it to the next pass that consumes |r|^2, and the scalars to the host
static int cg_stop_test(CgRun &R, int launched, CgScalars *sc)
{
    nf_team *T = R.T; const ApplyCg A = cg_apply_args(R, launched);
    if ((R.form == CG_FUSE3 || R.form == CG_LEAN) && pub_ready(T)) {
        const unsigned long long seq = ++T->pub_seq;
        hipLaunchKernelGGL(k_cg_lean_rr, dim3(1), dim3(256), 0, T->stream, A.lean, T->d_pub, seq);
        return pub_wait(T, seq, sc, nullptr, 0);
    }
    if (R.form == CG_FUSE3 || R.form == CG_LEAN) hipLaunchKernelGGL(k_cg_lean_rr, dim3(1), dim3(256), 0, T->stream, A.lean, (HostPub *)nullptr, 0ULL);
    if (R.form == CG_TEAM_SR) hipLaunchKernelGGL(k_cg1_logic, dim3(1), dim3(64), 0, T->stream, A.cg1, (HostPub *)nullptr, 0ULL);
    if (R.form == CG_TEAM_VEC || R.form == CG_TEAM_LEAN) hipLaunchKernelGGL(k_cg_lean_rr, dim3(1), dim3(256), 0, T->stream, A.lean_z1, (HostPub *)nullptr, 0ULL);
    return readback(T, T->d_cg, sc, nullptr, nullptr, 0);
}
static int cg_result(nf_team *T, int g, CgForm form, const CgScalars &sc, int *its_out, double *res_out)   // what a finished solve reports
{
    T->last_cg_form = form;
    if (!std::isfinite(sc.rr)) return fail(NF_ERR_NUMERIC, "CG produced a non-finite residual (group %d)", g);
    T->last_its[g] = sc.its;
    if (its_out) *its_out = sc.its;
    if (res_out) *res_out = sc.rhs_norm > 0 ? std::sqrt(sc.rr) / sc.rhs_norm : 0.0;
    return NF_OK;
}
// rhs / x: per-slab pointers
// inited: k_group_rhs has already written x = 0, r = p = rhs and the |rhs|^2 partials (one launch less per group solve)
static int cg_solve(nf_team *T, int g, const std::vector<const double *> &rhs, const std::vector<double *> &x, double tol, int maxit,
                    int *its_out, double *res_out, bool inited = false)
{
    const int ns = (int)T->slabs.size(); nf_solver *S0 = T->slabs[0];
    const CgPlan P = cg_plan(T);
    CgRun R{ T, g, P, P.form, x };
    R.ps.resize(ns); R.qs.resize(ns); R.gcnt.resize(ns); R.acnt.resize(ns); R.cnt3.assign(ns, 0);
    auto init = [&] { for (int i = 0; i < ns; ++i) with_void(T->slabs[i], [&](auto M, VoidMask vm) {
        hipLaunchKernelGGL(k_cg_init<decltype(M)::value>, dim3(R.gcnt[i]), dim3(256), 0, T->stream, rhs[i], x[i], T->slabs[i]->d_r, T->slabs[i]->d_p, T->slabs[i]->nphi, T->d_partials + i * T->slab_cap, vm); }); };
    for (int i = 0; i < ns; ++i) { nf_solver *S = T->slabs[i]; R.gcnt[i] = grid_for(S->nphi); R.ps[i] = S->d_p; R.qs[i] = S->d_q; R.any_if |= S->if_lo || S->if_hi; }
    if (!inited) init();
    NFCHK(team_finalize(T, FIN_RHS, R.gcnt, 1, T->d_out, tol, maxit));
    CgScalars sc; memset(&sc, 0, sizeof sc);
    T->last_cg_reductions = P.reductions; T->last_endpoint_w = 0; T->last_vec_reduce = P.form == CG_TEAM_VEC ? 1 : 0; T->last_xcd = 0;
    if (P.f3.ok) {
        if (!S0->d_p2) NFCHK(dalloc(&S0->d_p2, S0->nphi));
        if (S0->dim >= 2 && !S0->d_qy) NFCHK(dalloc(&S0->d_qy, S0->nphi));
        if (S0->dim == 3 && !S0->d_qz) NFCHK(dalloc(&S0->d_qz, S0->nphi));
    }
    if (P.xsol_batch > 1) {                                       // M - 1 more direction buffers; a refusal is not an error: this handle carries on with one
        if (S0->ring_m != P.xsol_batch) {
            dfree(S0->d_ring); S0->ring_m = 0;
            if (hipMalloc((void **)&S0->d_ring, (size_t)(P.xsol_batch - 1) * S0->nphi * sizeof(double)) == hipSuccess) S0->ring_m = P.xsol_batch;
            else { (void)hipGetLastError(); S0->d_ring = nullptr; S0->ring_refused = true; }
        }
        if (S0->ring_m == P.xsol_batch) R.M = P.xsol_batch;
    }
    if (R.form == CG_XCD && !pub_ready(T)) R.form = CG_FUSE3;    // the kernel hands the final scalars to the host itself: no mapped page, no one-XCD solve
    if (R.form == CG_XCD) {                                       // the whole solve in one launch on one XCD (k_cg_xcd)
        const unsigned long long seq = ++T->pub_seq;
        NFCHK(launch_cg_xcd(S0, g, P.f3, x[0], seq));
        NFCHK(pub_wait(T, seq, &sc, nullptr, 0));
        if (sc.err != 3 && sc.err != 4) { T->last_xcd = 1; ++T->xcd_solves; HIPCHK(hipGetLastError()); return cg_result(T, g, CG_XCD, sc, its_out, res_out); }
        // err 3: the workgroups did not assemble (nothing placed on the XCD, or it is busy): no vector has been touched.  err 4: a grid
        // barrier timed out in the middle of the solve (a participant stalled for longer than the bound: another process on the GPU, a
        // debugger): x, r and p are half-way, but the right-hand side is intact (the kernels have all left by now: the flag that ended
        // one ended the others).  Either way this solve starts again on the launch path, and so do the following ones of this solver
        T->opt.cg_xcd = 0; ++T->xcd_refused; R.form = CG_FUSE3;
        if (sc.err == 4) { HIPCHK(hipStreamSynchronize(T->stream)); init(); }
        NFCHK(team_finalize(T, FIN_RHS, R.gcnt, 1, T->d_out, tol, maxit));
        memset(&sc, 0, sizeof sc);
    }
    if (R.form == CG_TEAM_VEC)                                    // other kernels use these rows between solves: clear the two flag slots
        for (double *slot : { T->d_partials + T->vec_cnt_pq, R.row1() + T->vec_cnt_rr }) HIPCHK(hipMemsetAsync(slot, 0, sizeof(double), T->stream));
    int launched = 0, rc = NF_OK;
    // first batch: what the previous solve of this group needed, plus two (an iteration launched past convergence costs five
    // early-exit kernels, ~10 us; a second host check costs a D2H copy and a stream drain, ~50 us)
    int batch = T->opt.cg_batch > 0 ? T->opt.cg_batch : (T->last_its[g] > 0 ? T->last_its[g] + 2 : 1), grow = 2;
    while (launched < maxit && rc == NF_OK) {
        const int nb = std::min(batch, maxit - launched);
        for (int it = 0; it < nb && rc == NF_OK; ++it) rc = cg_step(R, launched + it, T->cg_iter_total++);
        if (rc != NF_OK) break;
        launched += nb;
        rc = cg_stop_test(R, launched, &sc);
        if (rc != NF_OK || sc.done) break;
        // after the first (predicted) batch grow geometrically: an iteration launched past convergence is five early-exit
        // kernels (~10 us), a host check is a D2H copy + stream drain (~50 us)
        batch = T->opt.cg_batch > 0 ? T->opt.cg_batch : (launched < 8 ? 1 : grow);
        if (launched >= 8) grow = std::min(64, 2 * grow);
    }
    NFCHK(rc);
    if (T->poisoned) return team_poison_result(T);               // the flag has stopped every rank (or maxit did): this rank reports what hit it
    if (sc.err == 2) return fail(NF_ERR_REMOTE, "another rank of the team reported an error during the CG solve of group %d; every rank stopped at iteration %d", g, sc.its);
    if (launched == 0) {
        HIPCHK(hipMemcpyAsync(&sc, T->d_cg, sizeof sc, hipMemcpyDeviceToHost, T->stream));
        HIPCHK(hipStreamSynchronize(T->stream));
    }
    if (P.fused && R.M > 1) {                                     // what the x passes of this solve left in the ring, from the final scalars
        const NfRingBatch B = nf_ring_pending(sc.its, sc.pend, R.M);
        FlushRing fr; memset(&fr, 0, sizeof fr); fr.n = B.n; fr.ah = T->d_ah;
        for (int j = 0; j < B.n; ++j) { fr.alpha[j] = B.u[j].alpha; fr.p[j] = R.slot(B.u[j].slot); }
        if (B.n > 0) hipLaunchKernelGGL(k_cg_flush, dim3(R.gcnt[0]), dim3(256), 0, T->stream, x[0], (const double *)nullptr, S0->nphi, T->d_cg, fr);
    } else if (P.fused)
        for (int i = 0; i < ns; ++i) {
            const double *plast = T->slabs[i]->d_p;
            if (R.form == CG_FUSE3 && sc.its >= 2 && ((sc.its - 1) & 1)) plast = T->slabs[i]->d_p2;   // the direction of the last iteration (see cg_step_fuse3)
            FlushRing fr; memset(&fr, 0, sizeof fr); fr.n = -1;
            hipLaunchKernelGGL(k_cg_flush, dim3(R.gcnt[i]), dim3(256), 0, T->stream, x[i], plast, T->slabs[i]->nphi, T->d_cg, fr);
        }
    HIPCHK(hipGetLastError());
    if (T->profile) prof_collect(T);
    return cg_result(T, g, R.form, sc, its_out, res_out);
}

int nf_solve_group(nf_handle S, int g, const double *rhs_dev, double *phi_dev, double tol, int maxit, int *its, double *res)
{
    if (!S || !rhs_dev || !phi_dev || g < 0 || g >= S->ng) return fail(NF_ERR_ARG, "nf_solve_group: bad arguments");
    if (!S->built) return fail(NF_ERR_STATE, "nf_solve_group: call nf_build first");
    if (!team_is_single(S->team)) return fail(NF_ERR_STATE, "nf_solve_group works on an undivided mesh");
    HIPCHK(hipSetDevice(S->device));
    NFCHK(line_dict_prepare(S->team));
    return cg_solve(S->team, g, { rhs_dev }, { phi_dev }, tol, maxit, its, res);
}

// ---- diagonal cache ----------------------------------------------------------------------------
// Whole team at once: on slabs the interface faces need the neighbour's edge-cell a2 (one plane per group, exchanged here).
int nf_build_diagonal_cache(nf_handle S)
{
    if (!S) return fail(NF_ERR_ARG, "null handle");
    nf_team *T = S->team;
    for (auto *X : T->slabs) if (!X->built) return fail(NF_ERR_STATE, "nf_build_diagonal_cache: call nf_build first");
    NFCHK(void_refuse(S, "nf_build_diagonal_cache"));
    if (S->k != 0 || S->m != 0) return NF_OK;                     // "non applicable (ordre > 0)", src/NeutFEM.cpp:484-487
    bool valid = true, any_if = false;
    for (auto *X : T->slabs) { valid &= X->diag_valid; any_if |= X->if_lo || X->if_hi; }
    if (valid) return NF_OK;
    HIPCHK(hipSetDevice(S->device));
    {
        int lrc = NF_OK;
        for (auto *X : T->slabs) if (lrc == NF_OK && !X->d_Sinv) lrc = dalloc(&X->d_Sinv, (size_t)X->N * X->ng);
        NFCHK(team_verdict(T, lrc, "the edge-plane exchange of nf_build_diagonal_cache"));
    }
    for (int g = 0; g < S->ng; ++g) {
        if (any_if) {
            for (auto *X : T->slabs) {
                const long nl = X->nlines[2];
                hipLaunchKernelGGL(k_edge_a2, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, T->stream, make_geom(X), X->d_D + g * X->N, X->d_clo, X->d_chi, nl);
            }
            NFCHK(exchange_planes(T, 0, 0, T->stream));
        }
        for (auto *X : T->slabs) {
            const long N = X->N;
            hipLaunchKernelGGL(k_diag_cache, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, T->stream, make_geom(X), X->d_D + g * N, X->d_Cd + g * N,
                               X->d_Sinv + g * N, N, X->if_lo ? X->d_rlo : (const double *)nullptr, X->if_hi ? X->d_rhi : (const double *)nullptr);
        }
        NFCHK(team_stream_wait(T, T->stream));                  // the exchange buffers are reused by the next group
    }
    HIPCHK(hipGetLastError());
    for (auto *X : T->slabs) X->diag_valid = true;
    return NF_OK;
}
int nf_get_diagonal_cache(nf_handle S, int g, double *sinv_host)
{
    if (!S || g < 0 || g >= S->ng || !sinv_host) return fail(NF_ERR_ARG, "nf_get_diagonal_cache: bad arguments");
    NFCHK(nf_build_diagonal_cache(S));
    if (!S->diag_valid) return fail(NF_ERR_UNSUPPORTED, "the diagonal cache exists for RT0-P0 only");
    HIPCHK(hipMemcpy(sinv_host, S->d_Sinv + g * S->N, S->N * sizeof(double), hipMemcpyDeviceToHost));
    return NF_OK;
}

// ---- state -------------------------------------------------------------------------------------
// host layout [g][e*nloc + p] (reference, src/FEM.cpp:321-334) <-> device layout [g][p][e]
static int phi_transfer(nf_solver *S, double *host, bool to_device, double *dev = nullptr)
{
    if (!dev) dev = S->d_phi;
    HIPCHK(hipSetDevice(S->device));
    hipStream_t st = S->team->stream;
    HIPCHK(hipStreamSynchronize(st));
    const size_t NN = (size_t)S->nphi * S->ng;
    if (S->nloc == 1) {
        if (to_device) HIPCHK(hipMemcpy(dev, host, NN * sizeof(double), hipMemcpyHostToDevice));
        else HIPCHK(hipMemcpy(host, dev, NN * sizeof(double), hipMemcpyDeviceToHost));
        return NF_OK;
    }
    DevTmp<double> tmp_; NFCHK(dalloc(&tmp_.p, NN)); double *tmp = tmp_.p;
    if (to_device) HIPCHK(hipMemcpy(tmp, host, NN * sizeof(double), hipMemcpyHostToDevice));
    for (int g = 0; g < S->ng; ++g) {
        const double *src = (to_device ? tmp : dev) + (size_t)g * S->nphi;
        double *dst = (to_device ? dev : tmp) + (size_t)g * S->nphi;
        hipLaunchKernelGGL(k_transpose_dofs, dim3(grid_for(S->nphi)), dim3(256), 0, st, src, dst, S->N, S->nloc, to_device ? 1 : 0);
    }
    HIPCHK(hipStreamSynchronize(st));
    if (!to_device) HIPCHK(hipMemcpy(host, tmp, NN * sizeof(double), hipMemcpyDeviceToHost));
    return NF_OK;
}
int nf_set_phi(nf_handle S, const double *phi)
{
    if (!S || !phi) return fail(NF_ERR_ARG, "nf_set_phi: bad arguments");
    return phi_transfer(S, const_cast<double *>(phi), true);
}
int nf_get_phi(nf_handle S, double *phi)
{
    if (!S || !phi) return fail(NF_ERR_ARG, "nf_get_phi: bad arguments");
    return phi_transfer(S, phi, false);
}
int nf_reset_flux(nf_handle S)
{
    if (!S) return fail(NF_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(S->device));
    std::vector<double> ones((size_t)S->nphi * S->ng, 1.0);     // Sol_Phi_ = 1 on every DOF, src/NeutFEM.cpp:347-354
    HIPCHK(hipMemcpy(S->d_phi, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
    S->team->has_valid_keff = 0; S->raw_valid = false;
    return NF_OK;
}
int nf_set_warm_state(nf_handle S, int v, double k) { if (!S) return fail(NF_ERR_ARG, "null handle"); S->team->has_valid_keff = v; S->team->last_keff = k; return NF_OK; }
int nf_get_warm_state(nf_handle S, int *v, double *k) { if (!S) return fail(NF_ERR_ARG, "null handle"); if (v) *v = S->team->has_valid_keff; if (k) *k = S->team->last_keff; return NF_OK; }

// z currents of every local slab from the raw group fluxes of the last solve: endpoint pass, exchange, separators, then the
// chain solve in "emit" mode (k_schur_s mode 3).  Cached until the next solve.
static int team_reconstruct_Jz(nf_team *T)
{
    bool all = true; for (auto *S : T->slabs) all &= S->jz_valid;
    if (all) return NF_OK;
    NFCHK(team_prepare(T));
    const int ns = (int)T->slabs.size(), ng = T->slabs[0]->ng;
    {
        int lrc = NF_OK;
        for (auto *S : T->slabs) {
            if (lrc == NF_OK && !S->d_Jz) lrc = dalloc(&S->d_Jz, (size_t)S->nJz * ng);
            if (lrc == NF_OK && S->k > 0 && !S->d_Jzb) { int ni = S->k; for (int t = 1; t < S->dim; ++t) ni *= S->k + 1; lrc = dalloc(&S->d_Jzb, (size_t)S->N * ni * ng); }
        }
        NFCHK(team_verdict(T, lrc, "the partition-method solve of nf_get_J"));
    }
    for (auto *S : T->slabs) {
        HIPCHK(hipMemsetAsync(S->d_Jz, 0, (size_t)S->nJz * ng * sizeof(double), T->stream));         // RT modes that see no phi moment stay 0
        if (S->k > 0) {
            int ni = S->k; for (int t = 1; t < S->dim; ++t) ni *= S->k + 1;
            HIPCHK(hipMemsetAsync(S->d_Jzb, 0, (size_t)S->N * ni * ng * sizeof(double), T->stream));
        }
    }
    std::vector<const double *> xs(ns); std::vector<double *> ys(ns);
    for (int g = 0; g < ng; ++g) {
        for (int i = 0; i < ns; ++i) { xs[i] = T->slabs[i]->d_raw + (size_t)g * T->slabs[i]->nphi; ys[i] = T->slabs[i]->d_q; }
        NFCHK(team_endpoint_phase(T, g, xs, ys, ApplyCg(), nullptr, true));
        HIPCHK(hipStreamWaitEvent(T->stream, T->ev_xchg, 0));
        for (int i = 0; i < ns; ++i) {
            nf_solver *S = T->slabs[i];
            NFCHK(launch_s(S, 2, g, mode_args(S, g, 2, 0, xs[i], ys[i]), make_geom(S), 0, nullptr, PassCg(), nullptr, 3));
        }
        NFCHK(team_stream_wait(T, T->stream));                  // the exchange buffers are reused by the next group
    }
    HIPCHK(hipGetLastError());
    for (auto *S : T->slabs) S->jz_valid = true;
    return NF_OK;
}

// z currents of every local slab after a diagonal-Schur solve (J_f = +(B^T phi)_f / A_ff, src/NeutFEM.cpp:620-633): per group
// one plane of edge-cell a2 and one of edge-cell phi per interface go to the neighbour; collective like team_reconstruct_Jz.
static int team_reconstruct_Jz_diag(nf_team *T)
{
    bool all = true; for (auto *S : T->slabs) all &= S->jz_valid;
    if (all) return NF_OK;
    NFCHK(team_prepare(T));
    const int ng = T->slabs[0]->ng;
    hipStream_t st = T->stream;
    {
        int lrc = NF_OK;
        for (auto *S : T->slabs) if (lrc == NF_OK && !S->d_Jz) lrc = dalloc(&S->d_Jz, (size_t)S->nJz * ng);
        NFCHK(team_verdict(T, lrc, "the edge-plane exchanges of nf_get_J (diagonal path)"));
    }
    for (int g = 0; g < ng; ++g) {
        // (1) a2 of the edge cells -> d_rlo / d_rhi ; kept in d_ctlo / d_cthi while the planes are reused for phi
        for (auto *S : T->slabs) {
            const long nl = S->nlines[2];
            hipLaunchKernelGGL(k_edge_a2, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, make_geom(S), S->d_D + g * S->N, S->d_clo, S->d_chi, nl);
        }
        NFCHK(exchange_planes(T, 0, 0, st));
        for (auto *S : T->slabs) {
            const size_t b = (size_t)S->nlines[2] * sizeof(double);
            HIPCHK(hipMemcpyAsync(S->d_ctlo, S->d_rlo, b, hipMemcpyDeviceToDevice, st)); HIPCHK(hipMemcpyAsync(S->d_cthi, S->d_rhi, b, hipMemcpyDeviceToDevice, st));
        }
        // (2) phi of the edge cells (first and last plane of the raw group flux)
        for (auto *S : T->slabs) {
            const size_t b = (size_t)S->nlines[2] * sizeof(double);
            const double *raw = S->d_raw + (size_t)g * S->nphi;
            HIPCHK(hipMemcpyAsync(S->d_clo, raw, b, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(S->d_chi, raw + (size_t)(S->nz - 1) * S->nlines[2], b, hipMemcpyDeviceToDevice, st));
        }
        NFCHK(exchange_planes(T, 0, 0, st));
        for (auto *S : T->slabs) {
            const long nl = S->nlines[2];
            hipLaunchKernelGGL(k_diag_Jz_slab, dim3((unsigned)((nl + 63) / 64)), dim3(64), 0, st, make_geom(S), S->d_D + g * S->N, S->d_raw + (size_t)g * S->nphi,
                               S->d_Jz + (size_t)g * S->nJz, nl, S->if_lo, S->if_hi, (const double *)S->d_rlo, (const double *)S->d_ctlo,
                               (const double *)S->d_rhi, (const double *)S->d_cthi);
        }
        NFCHK(team_stream_wait(T, st));                         // the exchange buffers are reused by the next group
    }
    HIPCHK(hipGetLastError());
    for (auto *S : T->slabs) S->jz_valid = true;
    return NF_OK;
}

// The current of one group's field into dJ (nJ doubles, the reference DOF order): dJ zeroed, then one k_flux_to_J launch per direction
// d < ndirs and transverse mode that sees a phi moment.  field_g: nphi doubles in the device layout (the raw flux of the last solve for
// nf_get_J, any field for nf_sensitivity); diag: the diagonal-path formula
static int flux_to_J(nf_solver *S, int g, const double *field_g, double *dJ, int ndirs, int diag, hipStream_t st)
{
    const long N = S->N, nJ = S->nJ;
    Geom G = make_geom(S);
    int nfa = 1, ni = S->k; for (int t = 1; t < S->dim; ++t) { nfa *= S->k + 1; ni *= S->k + 1; }
    const long nJface = S->nJx + S->nJy + S->nJz;
    const long foff[3] = { 0, S->nJx, S->nJx + S->nJy };
    HIPCHK(hipMemsetAsync(dJ, 0, (size_t)nJ * sizeof(double), st));                         // modes that see no phi moment stay 0
    for (int d = 0; d < ndirs; ++d)
        for (int mode = 0; mode < n_modes(S); ++mode) {
            ModeArgs ma = mode_args(S, g, d, mode, field_g, const_cast<double *>(field_g));
            // transverse mode index in the RT numbering: a = sum a_t (k+1)^t over the transverse axes (FEM.cpp:364-374)
            int amode = 0, q = mode, mul = 1;
            for (int t = 0; t < S->dim; ++t) { if (t == d) continue; amode += (q % S->n1) * mul; q /= S->n1; mul *= S->k + 1; }
            hipLaunchKernelGGL(k_flux_to_J, dim3((unsigned)((S->nlines[d] + 63) / 64)), dim3(64), 0, st, G, ma, S->nb, amode, nfa, ni,
                               S->d_D + g * N, S->d_L[d] + g * N, S->d_DR[d] + g * N, S->d_D0[d] + g * S->nlines[d],
                               dJ + foff[d], dJ + nJface + (long)d * N * ni, S->nlines[d], diag, (const unsigned char *)S->d_void);
        }
    return NF_OK;
}

int nf_get_J(nf_handle S, double *J_host)
{
    if (!S || !J_host) return fail(NF_ERR_ARG, "nf_get_J: bad arguments");
    if (S->team->dead) return fail(NF_ERR_COMM, "this team lost a collective (NF_ERR_COMM) and is unusable: destroy the handles and end the process with a non-zero code (never re-exec)");
    HIPCHK(hipSetDevice(S->device));
    hipStream_t st = S->team->stream;
    const long N = S->N, nJ = S->nJ;
    if (!S->raw_valid) { memset(J_host, 0, sizeof(double) * nJ * S->ng); return NF_OK; }   // Sol_J_ = 0 before any solve
    const bool slab = S->if_lo || S->if_hi;
    if (slab) {
        // z currents cross slabs: one partition-method solve per group on the raw group fluxes, for the whole team (collective:
        // every rank calls nf_get_J on its slabs in the same order; the first call after a solve does the work for all local slabs)
        if (S->raw_is_diag) NFCHK(team_reconstruct_Jz_diag(S->team));       // RT0-P0 by construction (the diagonal path exists for that order only)
        else NFCHK(team_reconstruct_Jz(S->team));
    }
    DevTmp<double> dJ_; NFCHK(dalloc(&dJ_.p, (size_t)nJ)); double *dJ = dJ_.p;
    int ni = S->k; for (int t = 1; t < S->dim; ++t) ni *= S->k + 1;
    const long nJface = S->nJx + S->nJy + S->nJz;
    const long foff[3] = { 0, S->nJx, S->nJx + S->nJy };
    for (int g = 0; g < S->ng; ++g) {
        NFCHK(flux_to_J(S, g, S->d_raw + (size_t)g * S->nphi, dJ, slab ? 2 : S->dim, S->raw_is_diag ? 1 : 0, st));
        if (slab) {
            HIPCHK(hipMemcpyAsync(dJ + foff[2], S->d_Jz + (size_t)g * S->nJz, S->nJz * sizeof(double), hipMemcpyDeviceToDevice, st));
            if (ni > 0 && !S->raw_is_diag && S->d_Jzb)
                HIPCHK(hipMemcpyAsync(dJ + nJface + 2L * N * ni, S->d_Jzb + (size_t)g * N * ni, (size_t)N * ni * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(hipMemcpyAsync(J_host + (size_t)g * nJ, dJ, nJ * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipGetLastError());
    return NF_OK;
}

// phi = Chebyshev(raw / norm) on one slab with the step of cheb_next (nf_outer.h): p0 / p1 on first use, the launch, the swap after a
// three-term step.  Shared by the host-driven direct and adjoint iterations; each keeps its own handling of the code returned.
static int normalize_cheb(nf_solver *S, hipStream_t st, double *cur, double norm, bool do_norm, const ChebStep &cs)
{
    const long NT = S->nphi * S->ng;
    if (cs.mode && !S->d_p0) { NFCHK(dalloc(&S->d_p0, (size_t)NT)); NFCHK(dalloc(&S->d_p1, (size_t)NT)); }
    hipLaunchKernelGGL(k_normalize_cheb, dim3(grid_for(NT)), dim3(256), 0, st, S->d_raw, cur, S->d_p0, S->d_p1, NT, norm, do_norm ? 1 : 0, cs.mode, cs.a, cs.b);
    if (cs.mode == 3) std::swap(S->d_p0, S->d_p1);
    return NF_OK;
}

// ---- explicit-S branch (src/solvers.cpp:114-124, 259-509) ----------------------------------------
// FormSchurComplement + PrepareSolver once per BuildMatrices: column j of S = S e_j through the matrix-free apply (the
// reference solves A x = B^T e_j and multiplies by B: the same numbers up to its 1e-14 drop threshold), then S^-1 by n
// Gauss-Jordan steps on the whole chip.  Undivided meshes of at most direct_max_dofs unknowns per group.
static int dense_prepare(nf_team *T)
{
    nf_solver *S = T->slabs[0];
    if (S->dense_valid) return NF_OK;
    const int n = (int)S->nphi, ng = S->ng; const size_t nn = (size_t)n * n;
    hipStream_t st = T->stream;
    NFCHK(dalloc(&S->d_Sdense, nn * ng));
    DevTmp<double> work; NFCHK(dalloc(&work.p, nn));
    for (int g = 0; g < ng; ++g) {
        double *M = S->d_Sdense + (size_t)g * nn;
        for (int j = 0; j < n; ++j) {
            hipLaunchKernelGGL(k_unit_vector, dim3(grid_for(n)), dim3(256), 0, st, S->d_p, (long)n, (long)j);
            NFCHK(team_schur_apply(T, g, { S->d_p }, { M + (size_t)j * n }, false, ApplyCg()));
        }
        double *a = M, *b = work.p;
        const unsigned gr = (unsigned)((nn + 255) / 256);
        for (int k = 0; k < n; ++k) { hipLaunchKernelGGL(k_gj_step, dim3(gr), dim3(256), 0, st, (const double *)a, b, n, k); std::swap(a, b); }
        if (a != M) HIPCHK(hipMemcpyAsync(M, a, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipGetLastError());
    S->dense_valid = true;
    return NF_OK;
}
static void dense_solve(nf_team *T, int g, const double *rhs, double *sol)
{
    nf_solver *S = T->slabs[0];
    const int n = (int)S->nphi;
    hipLaunchKernelGGL(k_dense_matvec, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T->stream, (const double *)(S->d_Sdense + (size_t)g * n * n), rhs, sol, n);
}

// ---- twin handles take the caller's options (nf_set_option) --------------------------------------
// The one place that hands a team's options to the team of a handle the library derives from it.  Every twin gets what chooses its solve:
// the form of the CG iteration (cg_plan, xcd_eligible), the group solver (inner_plan), the SolveKeff path, cg_batch.  same_mesh_kind: the
// twin has the caller's orders and runs its passes at the caller's scale (the step operator of a transient, nf_refine's fine handle), so
// it also gets what the launch plans of an apply and the scalar readback (pub_ready) read.  The coarse twin of SolveCoarse is RT0-P0 on a
// mesh many times smaller: pass tuning meant for the caller's mesh stays off it.
// what a changed option invalidates on the slabs of a team (NF_FX_DICT / NF_FX_REGIME of nf_options.h; DICT covers REGIME)
static int team_apply_table_effects(nf_team *T, unsigned fx)
{
    if (fx & NF_FX_DICT) { HIPCHK(hipSetDevice(T->device)); for (auto *X : T->slabs) line_dict_drop(X); }
    else if (fx & NF_FX_REGIME) for (auto *X : T->slabs) if (!X->d_lid[0] && !X->d_lid[1] && !X->d_lid[2]) X->ld_tried = false;
    return NF_OK;
}
// a cached twin whose values change drops its tables or looks again, as nf_set_option has it
static void team_copy_options(nf_team *C, const nf_team *T, bool same_mesh_kind) { (void)team_apply_table_effects(C, nf_options_copy(C->opt, T->opt, same_mesh_kind)); }

// ---- SolveCoarse (src/NeutFEM.cpp:2380-2611) ---------------------------------------------------
static int solve_keff_impl(nf_team *T, const nf_keff_opts *o, double *keff, int *n_outer);

// coarse twin of one slab (src/NeutFEM.cpp:2409-2556): every (rx, ry, rz) block of cells becomes one RT0-P0 cell, cross sections
// are arithmetic volume-weighted block means, boundary conditions and interface flags carry over; returned built.
static int coarsen_slab(nf_solver *S, int rx, int ry, int rz, nf_handle *out)
{
    const int dim = S->dim, ng = S->ng;
    hipStream_t st = S->team->stream;
    const int nxc = S->nx / rx, nyc = S->ny / ry, nzc = S->nz / rz;
    std::vector<double> xc(nxc + 1), yc(dim >= 2 ? nyc + 1 : 1), zc(dim >= 3 ? nzc + 1 : 1);
    for (int a = 0; a <= nxc; ++a) xc[a] = S->xb[a * rx];
    if (dim >= 2) for (int j = 0; j <= nyc; ++j) yc[j] = S->yb[j * ry]; else yc[0] = 0.0;
    if (dim >= 3) for (int kk = 0; kk <= nzc; ++kk) zc[kk] = S->zb[kk * rz]; else zc[0] = 0.0;
    nf_handle C = nullptr;
    NFCHK(create_impl(0, 0, ng, nxc + 1, xc.data(), (int)yc.size(), yc.data(), (int)zc.size(), zc.data(), S->if_lo, S->if_hi, S->device, &C));
    *out = C;
    for (int a = 0; a < 8; ++a) if (S->bc_set[a]) nf_set_bc(C, a, S->bc_type[a]);
    const long Nc = C->N;
    auto coarsen = [&](const double *fine, double **coarse, int nfields) -> int {
        NFCHK(dalloc(coarse, (size_t)Nc * nfields));
        hipLaunchKernelGGL(k_coarsen, dim3((unsigned)((Nc + 127) / 128)), dim3(128), 0, st, fine, *coarse, S->d_xb, S->d_yb, S->d_zb,
                           dim, S->nx, S->ny, S->nz, rx, ry, rz, nfields);
        return NF_OK;
    };
    NFCHK(coarsen(S->d_D, &C->d_D, ng)); NFCHK(coarsen(S->d_SigR, &C->d_SigR, ng));
    NFCHK(coarsen(S->d_NSF, &C->d_NSF, ng)); NFCHK(coarsen(S->d_Chi, &C->d_Chi, ng));
    for (int b = 0; b < ng * ng; ++b)
        if (S->d_SigS[b]) NFCHK(coarsen(S->d_SigS[b], &C->d_SigS[b], 1));        // mean of an all-zero block is zero
    HIPCHK(hipStreamSynchronize(st));
    C->xs_uploaded = true;
    return nf_build(C);
}

// Builds + solves the coarse problem on the device (every local slab coarsens its own planes; the coarse slabs form a
// team that shares the fine team's communicator); the prolonged flux of slab i is written to dsts[i] (ng*nphi).
static int coarse_init(nf_team *T, const nf_keff_opts *o, double *k_coarse, const std::vector<double *> &dsts, bool *done)
{
    *done = false;
    const int ns = (int)T->slabs.size();
    nf_solver *S0 = T->slabs[0];
    const int dim = S0->dim, ng = S0->ng;
    const int nf = o->n_coarse_factors;
    int rx = nf > 0 ? std::max(o->coarse_factors[0], 1) : 1;
    int ry = (nf > 1 && dim >= 2) ? std::max(o->coarse_factors[1], 1) : 1;
    int rz = (nf > 2 && dim >= 3) ? std::max(o->coarse_factors[2], 1) : 1;
    // :2402-2407 -> (1.0, Sol_Phi_).  On a decomposed mesh every slab must be divisible (a global decision is needed,
    // so indivisible local slabs are an error rather than a silent fallback on some ranks only).
    double bad = 0.0; const nf_solver *Sbad = nullptr;
    for (auto *S : T->slabs)
        if (S->nx % rx || S->ny % ry || S->nz % rz) { bad = 1.0; Sbad = S; }
    if (T->rccl_reduce && T->nproc > 1) {                         // one verdict for all ranks (a lone refusal would block the others)
        HIPCHK(hipMemcpyAsync(T->d_red, &bad, sizeof(double), hipMemcpyHostToDevice, T->stream));
        NCCLCHK(g_rccl.AllReduce(T->d_red, T->d_red, 1, NCCL_DOUBLE, NCCL_MAX, T->comm, T->stream));
        HIPCHK(hipMemcpyAsync(&bad, T->d_red, sizeof(double), hipMemcpyDeviceToHost, T->stream));
        NFCHK(team_stream_wait(T, T->stream));                      // a collective sits on the stream: bounded wait (NEUTFEM_COMM_TIMEOUT_S)
    }
    if (bad != 0.0) {
        if (ns == 1 && T->nproc == 1) return NF_OK;
        if (Sbad) return fail(NF_ERR_ARG, "coarse factors (%d,%d,%d) do not divide slab %d x %d x %d", rx, ry, rz, Sbad->nx, Sbad->ny, Sbad->nz);
        return fail(NF_ERR_ARG, "coarse factors (%d,%d,%d) do not divide a slab on another rank", rx, ry, rz);
    }
    std::vector<nf_handle> C(ns, nullptr);
    int rc = NF_OK;
    const bool reuse = (int)T->cc.size() == ns && T->cc_f[0] == rx && T->cc_f[1] == ry && T->cc_f[2] == rz;
    if (reuse) {
        for (int i = 0; i < ns && rc == NF_OK; ++i) { C[i] = T->cc[i]; rc = nf_reset_flux(C[i]); }   // a fresh coarse solver starts from phi = 1, k = 1 (:2458)
    } else {
        coarse_cache_drop(T);
        for (int i = 0; i < ns && rc == NF_OK; ++i) rc = coarsen_slab(T->slabs[i], rx, ry, rz, &C[i]);
        if (rc == NF_OK && ns > 1) rc = nf_link_slabs(C.data(), ns);
        if (rc == NF_OK) { T->cc = C; T->cc_f[0] = rx; T->cc_f[1] = ry; T->cc_f[2] = rz; }
        else { std::string keep = g_err; for (int i = ns - 1; i >= 0; --i) if (C[i]) nf_destroy(C[i]); g_err = keep; return rc; }
    }
    nf_team *CT = rc == NF_OK ? C[0]->team : nullptr;
    if (CT) {
        CT->comm = T->comm; CT->nproc = T->nproc; CT->rank = T->rank; CT->rccl_reduce = T->rccl_reduce; CT->linked_ready = false;
        // tuning options (nf_set_option) apply to the coarse solve as well
        CT->comm_x = T->comm_x; team_copy_options(CT, T, false);
    }
    double kc = 1.0; int nout = 0;
    if (rc == NF_OK) {
        nf_keff_opts co = *o;                                    // :2460-2467
        co.tol_keff = o->tol_keff * 10.0; co.tol_flux = o->tol_flux * 10.0; co.max_outer = o->max_outer / 2;
        co.use_coarse_init = 0; co.n_coarse_factors = 0; co.use_diagonal_solver = 0; co.solver_type_pushed = 1; co.profile = 0; co.use_cmfd = 0;
        rc = solve_keff_impl(CT, &co, &kc, &nout);
    }
    if (rc == NF_OK) {
        T->coarse_outer = nout;
        for (int i = 0; i < ns; ++i) {
            nf_solver *S = T->slabs[i];
            (void)hipMemsetAsync(dsts[i], 0, (size_t)S->nphi * ng * sizeof(double), CT->stream);   // higher moments 0 (:2585-2606)
            hipLaunchKernelGGL(k_prolong, dim3((unsigned)((S->N + 255) / 256)), dim3(256), 0, CT->stream, C[i]->d_phi, dsts[i], S->nx, S->ny, S->nz, rx, ry, rz, ng, S->nphi);
        }
        if (hipStreamSynchronize(CT->stream) != hipSuccess) rc = fail(NF_ERR_HIP, "prolong failed");
    }
    if (CT && CT->dead) { T->dead = true; T->comm = nullptr; T->comm_x = nullptr; }   // a collective of the coarse solve timed out on the BORROWED communicator: the fine team lost it too
    if (CT) { CT->comm = nullptr; CT->comm_x = nullptr; CT->nproc = 1; CT->rccl_reduce = false; }   // borrowed for the solve only: never destroyed with the coarse team
    if (rc != NF_OK) { coarse_cache_drop(T); return rc; }
    *k_coarse = kc; *done = true;
    return NF_OK;
}

int nf_solve_coarse(nf_handle S, const nf_keff_opts *o, double *k_coarse, double *phi_host)
{
    if (!S || !o || !k_coarse || !phi_host) return fail(NF_ERR_ARG, "nf_solve_coarse: bad arguments");
    NFCHK(void_refuse(S, "nf_solve_coarse"));
    if (!S->built) return fail(NF_ERR_STATE, "nf_solve_coarse: call nf_build first");
    if (!team_is_single(S->team)) return fail(NF_ERR_UNSUPPORTED, "coarse-mesh initialisation is not available on a slab-decomposed mesh");
    HIPCHK(hipSetDevice(S->device));
    bool done = false; double kc = 1.0;
    if (o->n_coarse_factors > 0) NFCHK(coarse_init(S->team, o, &kc, { S->d_raw }, &done));
    S->raw_valid = false;
    if (done) std::swap(S->d_raw, S->d_phi);                     // reuse the layout-converting download
    int rc = phi_transfer(S, phi_host, false);
    if (done) std::swap(S->d_raw, S->d_phi);
    NFCHK(rc);
    *k_coarse = done ? kc : 1.0;
    return NF_OK;
}

// ---- CMFD (src/NeutFEM.cpp:662-1017) -------------------------------------------------------------
// InitializeCMFD: D~ for every direction, D^ = 0.  Idempotent until the next nf_build (is_initialized, :663).
static int cmfd_initialize(nf_solver *S)
{
    if (S->cmfd_init) return NF_OK;
    hipStream_t st = S->team->stream;
    const int ng = S->ng; const long N = S->N;
    S->nfc[0] = (long)(S->nx + 1) * S->ny * S->nz; S->nfc[1] = (long)S->nx * (S->ny + 1) * S->nz; S->nfc[2] = (long)S->nx * S->ny * (S->nz + 1);
    Geom G = make_geom(S);
    for (int d = 0; d < 3; ++d) {
        NFCHK(dalloc(&S->d_Dt[d], (size_t)S->nfc[d] * ng)); NFCHK(dalloc(&S->d_Dh[d], (size_t)S->nfc[d] * ng));
        HIPCHK(hipMemsetAsync(S->d_Dt[d], 0, (size_t)S->nfc[d] * ng * sizeof(double), st));
        HIPCHK(hipMemsetAsync(S->d_Dh[d], 0, (size_t)S->nfc[d] * ng * sizeof(double), st));
        if (d >= S->dim) continue;
        for (int g = 0; g < ng; ++g)
            hipLaunchKernelGGL(k_cmfd_dtilde, dim3((unsigned)((S->nfc[d] + 255) / 256)), dim3(256), 0, st, G, d, S->d_D + g * N, S->d_Dt[d] + g * S->nfc[d], S->nfc[d]);
    }
    if (!S->d_cm) NFCHK(dalloc(&S->d_cm, (size_t)N * 6));
    if (!S->d_cmJ) NFCHK(dalloc(&S->d_cmJ, (size_t)S->nJ));
    if (!S->d_cmsc) NFCHK(dalloc(&S->d_cmsc, 1));
    HIPCHK(hipGetLastError());
    S->cmfd_init = true;
    return NF_OK;
}
static int cmfd_initialize_team(nf_team *T);
int nf_initialize_cmfd(nf_handle S)
{
    if (!S) return fail(NF_ERR_ARG, "null handle");
    if (!S->built) return fail(NF_ERR_STATE, "nf_initialize_cmfd: call nf_build first");
    NFCHK(void_refuse(S, "nf_initialize_cmfd"));
    HIPCHK(hipSetDevice(S->device));
    for (auto *X : S->team->slabs) if (!X->built) return fail(NF_ERR_STATE, "nf_initialize_cmfd: every slab of the team must be built first");
    NFCHK(cmfd_initialize_team(S->team));                        // collective on a multi-rank team (interface D-tilde)
    HIPCHK(hipStreamSynchronize(S->team->stream));
    return NF_OK;
}
// team-wide: every slab of the handle's team applies the same omega in k_cmfd_correct (on a multi-rank run every rank must set the same value)
int nf_set_cmfd_relaxation(nf_handle S, double omega) { if (!S) return fail(NF_ERR_ARG, "null handle"); for (auto *X : S->team->slabs) X->cmfd_relax = omega; return NF_OK; }
int nf_get_cmfd_coefficients(nf_handle S, int g, int dir, double *dtilde_host, double *dhat_host)
{
    if (!S || g < 0 || g >= S->ng || dir < 0 || dir > 2) return fail(NF_ERR_ARG, "nf_get_cmfd_coefficients: bad arguments");
    if (!S->cmfd_init) return fail(NF_ERR_STATE, "CMFD is not initialised");
    HIPCHK(hipSetDevice(S->device));
    HIPCHK(hipStreamSynchronize(S->team->stream));
    if (dtilde_host) HIPCHK(hipMemcpy(dtilde_host, S->d_Dt[dir] + g * S->nfc[dir], S->nfc[dir] * sizeof(double), hipMemcpyDeviceToHost));
    if (dhat_host) HIPCHK(hipMemcpy(dhat_host, S->d_Dh[dir] + g * S->nfc[dir], S->nfc[dir] * sizeof(double), hipMemcpyDeviceToHost));
    return NF_OK;
}

// UpdateDhatCoefficients for every group, then phi_g *= ApplyCMFDCorrection(g, phi_g, total_fiss, keff) (:1750-1761).
// phi = post-sweep group fluxes (d_raw), tf = d_tf of this outer, diag_sign = the J convention of the group solver.
static int cmfd_step(nf_solver *S, double keff, int use_diag)
{
    nf_team *T = S->team; hipStream_t st = T->stream;
    const int ng = S->ng; const long N = S->N, NP = S->nphi;
    Geom G = make_geom(S);
    int nfa = 1, ni = S->k; for (int t = 1; t < S->dim; ++t) { nfa *= S->k + 1; ni *= S->k + 1; }
    const long nJface = S->nJx + S->nJy + S->nJz;
    for (int g = 0; g < ng; ++g) {
        // Sol_J_ x-face mode 0 of group g (the only current D^ reads)
        ModeArgs ma = mode_args(S, g, 0, 0, S->d_raw + (size_t)g * NP, S->d_raw + (size_t)g * NP);
        hipLaunchKernelGGL(k_flux_to_J, dim3((unsigned)((S->nlines[0] + 63) / 64)), dim3(64), 0, st, G, ma, S->nb, 0, nfa, ni,
                           S->d_D + g * N, S->d_L[0] + g * N, S->d_DR[0] + g * N, S->d_D0[0] + g * S->nlines[0],
                           S->d_cmJ, S->d_cmJ + nJface, S->nlines[0], use_diag);
        hipLaunchKernelGGL(k_cmfd_dhat, dim3((unsigned)((S->nfc[0] + 255) / 256)), dim3(256), 0, st, G, S->d_raw + (size_t)g * NP, S->d_cmJ, nfa,
                           S->d_Dt[0] + g * S->nfc[0], S->d_Dh[0] + g * S->nfc[0], S->nfc[0]);
    }
    double *diag = S->d_cm, *x = diag + N, *r = x + N, *pp = r + N, *q = pp + N, *z = q + N;
    const int gN = grid_for(N);
    const long stride = T->partial_stride;
    S->cmfd_last_its = 0;
    for (int g = 0; g < ng; ++g) {
        CmfdFaces F;
        for (int d = 0; d < 3; ++d) { F.Dt[d] = S->d_Dt[d] + g * S->nfc[d]; F.Dh[d] = S->d_Dh[d] + g * S->nfc[d]; }
        hipLaunchKernelGGL(k_cmfd_setup, dim3(gN), dim3(256), 0, st, G, F, S->d_Cd + (size_t)g * NP, S->d_Chi + g * N, S->d_tf, 1.0 / keff,
                           diag, x, r, pp, N, T->d_partials, stride);
        hipLaunchKernelGGL(k_cmfd_logic, dim3(1), dim3(256), 0, st, 0, T->d_partials, gN, stride, S->d_cmsc);
        CmfdScalars hs; hs.done = 0; hs.its = 0;
        for (int base = 0; base < 100 && !hs.done; base += 10) {
            for (int i = 0; i < 10; ++i) {
                hipLaunchKernelGGL(k_cmfd_matvec, dim3(gN), dim3(256), 0, st, G, F, diag, pp, q, N, S->d_cmsc, T->d_partials, (const double *)nullptr, (const double *)nullptr);
                hipLaunchKernelGGL(k_cmfd_logic, dim3(1), dim3(256), 0, st, 1, T->d_partials, gN, stride, S->d_cmsc);
                hipLaunchKernelGGL(k_cmfd_update, dim3(gN), dim3(256), 0, st, diag, pp, q, x, r, z, N, S->d_cmsc, T->d_partials, stride);
                hipLaunchKernelGGL(k_cmfd_logic, dim3(1), dim3(256), 0, st, 2, T->d_partials, gN, stride, S->d_cmsc);
                hipLaunchKernelGGL(k_cmfd_pupdate, dim3(gN), dim3(256), 0, st, z, pp, N, S->d_cmsc);
            }
            HIPCHK(hipMemcpyAsync(&hs, S->d_cmsc, sizeof(hs), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        S->cmfd_last_its += hs.its;
        hipLaunchKernelGGL(k_cmfd_correct, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, x, S->d_raw + (size_t)g * NP, N, S->nloc, S->cmfd_relax);
    }
    HIPCHK(hipGetLastError());
    return NF_OK;
}

// CMFD on a slab team: every slab initialises its own faces; the D-tilde of an interface z face couples the edge cells of two slabs
// (one plane of D per group and the edge cell height travel to the neighbour, once per BuildMatrices).
static int cmfd_initialize_team(nf_team *T)
{
    bool done = true, any_if = false;
    for (auto *S : T->slabs) { done &= S->cmfd_init && S->cmfd_iface; any_if |= S->if_lo || S->if_hi; }
    if (done) return NF_OK;
    {
        int lrc = NF_OK;
        for (auto *S : T->slabs) if (lrc == NF_OK) lrc = cmfd_initialize(S);     // allocations + the slab-local D-tilde
        if (any_if) NFCHK(team_verdict(T, lrc, "the interface exchange of nf_initialize_cmfd")); else NFCHK(lrc);
    }
    if (any_if) {
        NFCHK(team_prepare(T));
        hipStream_t st = T->stream;
        const int ng = T->slabs[0]->ng;
        for (int g = 0; g < ng; ++g) {
            for (auto *S : T->slabs) {                            // edge planes of D
                const size_t b = (size_t)S->nlines[2] * sizeof(double);
                HIPCHK(hipMemcpyAsync(S->d_clo, S->d_D + (size_t)g * S->N, b, hipMemcpyDeviceToDevice, st));
                HIPCHK(hipMemcpyAsync(S->d_chi, S->d_D + (size_t)g * S->N + (size_t)(S->nz - 1) * S->nlines[2], b, hipMemcpyDeviceToDevice, st));
            }
            NFCHK(exchange_planes(T, 0, 0, st));
            for (auto *S : T->slabs) {
                const size_t b = (size_t)S->nlines[2] * sizeof(double);
                HIPCHK(hipMemcpyAsync(S->d_ctlo, S->d_rlo, b, hipMemcpyDeviceToDevice, st)); HIPCHK(hipMemcpyAsync(S->d_cthi, S->d_rhi, b, hipMemcpyDeviceToDevice, st));
                const int gr = grid_for(S->nlines[2]);
                hipLaunchKernelGGL(k_fill_const, dim3(gr), dim3(256), 0, st, S->d_clo, S->nlines[2], S->hz.front());   // edge cell heights
                hipLaunchKernelGGL(k_fill_const, dim3(gr), dim3(256), 0, st, S->d_chi, S->nlines[2], S->hz.back());
            }
            NFCHK(exchange_planes(T, 0, 0, st));
            for (auto *S : T->slabs) {
                const long nl = S->nlines[2]; const unsigned gr = (unsigned)((nl + 255) / 256);
                double *Dt = S->d_Dt[2] + (size_t)g * S->nfc[2];
                if (S->if_lo) hipLaunchKernelGGL(k_cmfd_dtilde_iface, dim3(gr), dim3(256), 0, st, (const double *)(S->d_D + (size_t)g * S->N), (const double *)S->d_ctlo,
                                                 (const double *)S->d_rlo, S->hz.front(), Dt, nl, 1);
                if (S->if_hi) hipLaunchKernelGGL(k_cmfd_dtilde_iface, dim3(gr), dim3(256), 0, st, (const double *)(S->d_D + (size_t)g * S->N + (size_t)(S->nz - 1) * nl),
                                                 (const double *)S->d_cthi, (const double *)S->d_rhi, S->hz.back(), Dt + (size_t)S->nz * nl, nl, 0);
            }
            NFCHK(team_stream_wait(T, st));                     // the exchange planes are reused by the next group
        }
        HIPCHK(hipGetLastError());
    }
    for (auto *S : T->slabs) S->cmfd_iface = true;
    return NF_OK;
}

// UpdateDhat + ApplyCMFDCorrection on a slab team (:1750-1761): the PCG of cmfd_step with one plane of p per interface and
// iteration (7-point stencil across the cut) and team-wide dot products (process-local sums + all-reduce over ranks); the CG
// scalars live in the first local slab's CmfdScalars.  Same arithmetic per cell as the undivided solve.
static int cmfd_step_team(nf_team *T, double keff, int use_diag)
{
    hipStream_t st = T->stream;
    const int ns = (int)T->slabs.size(), ng = T->slabs[0]->ng;
    CmfdScalars *sc = T->slabs[0]->d_cmsc;
    std::vector<int> gN(ns);
    for (int i = 0; i < ns; ++i) gN[i] = grid_for(T->slabs[i]->N);
    auto reduce_logic = [&](int op, int nq) -> int {
        PartSegs ps = segs_for(T, gN);
        hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, st, (int)FIN_SUM, T->d_partials, ps, T->partial_stride, nq, T->d_cg, T->d_red, 0.0, 0, 1, T->d_red, (const double *)nullptr);
        if (T->rccl_reduce) NCCLCHK(g_rccl.AllReduce(T->d_red, T->d_red, (size_t)nq, NCCL_DOUBLE, NCCL_SUM, T->comm, st));
        hipLaunchKernelGGL(k_cmfd_logic_tot, dim3(1), dim3(1), 0, st, op, (const double *)T->d_red, sc);
        return NF_OK;
    };
    for (auto *S : T->slabs) {                                    // D-hat: x faces only, slab-local (x lines do not cross slabs)
        const long N = S->N, NP = S->nphi;
        Geom G = make_geom(S);
        int nfa = 1, ni = S->k; for (int t = 1; t < S->dim; ++t) { nfa *= S->k + 1; ni *= S->k + 1; }
        const long nJface = S->nJx + S->nJy + S->nJz;
        for (int g = 0; g < ng; ++g) {
            ModeArgs ma = mode_args(S, g, 0, 0, S->d_raw + (size_t)g * NP, S->d_raw + (size_t)g * NP);
            hipLaunchKernelGGL(k_flux_to_J, dim3((unsigned)((S->nlines[0] + 63) / 64)), dim3(64), 0, st, G, ma, S->nb, 0, nfa, ni,
                               S->d_D + g * N, S->d_L[0] + g * N, S->d_DR[0] + g * N, S->d_D0[0] + g * S->nlines[0],
                               S->d_cmJ, S->d_cmJ + nJface, S->nlines[0], use_diag);
            hipLaunchKernelGGL(k_cmfd_dhat, dim3((unsigned)((S->nfc[0] + 255) / 256)), dim3(256), 0, st, G, S->d_raw + (size_t)g * NP, S->d_cmJ, nfa,
                               S->d_Dt[0] + g * S->nfc[0], S->d_Dh[0] + g * S->nfc[0], S->nfc[0]);
        }
        S->cmfd_last_its = 0;
    }
    for (int g = 0; g < ng; ++g) {
        for (int i = 0; i < ns; ++i) {
            nf_solver *S = T->slabs[i]; const long N = S->N;
            CmfdFaces F; for (int d = 0; d < 3; ++d) { F.Dt[d] = S->d_Dt[d] + g * S->nfc[d]; F.Dh[d] = S->d_Dh[d] + g * S->nfc[d]; }
            double *diag = S->d_cm, *x = diag + N, *r = x + N, *pp = r + N;
            hipLaunchKernelGGL(k_cmfd_setup, dim3(gN[i]), dim3(256), 0, st, make_geom(S), F, S->d_Cd + (size_t)g * S->nphi, S->d_Chi + g * N, S->d_tf, 1.0 / keff,
                               diag, x, r, pp, N, T->d_partials + i * T->slab_cap, T->partial_stride);
        }
        NFCHK(reduce_logic(0, 2));
        CmfdScalars hs; hs.done = 0; hs.its = 0;
        for (int base = 0; base < 100 && !hs.done; base += 10) {
            for (int it = 0; it < 10; ++it) {
                for (auto *S : T->slabs) {                        // edge planes of p to the neighbours
                    const size_t b = (size_t)S->nlines[2] * sizeof(double); const double *pp = S->d_cm + 3 * S->N;
                    HIPCHK(hipMemcpyAsync(S->d_clo, pp, b, hipMemcpyDeviceToDevice, st));
                    HIPCHK(hipMemcpyAsync(S->d_chi, pp + (size_t)(S->nz - 1) * S->nlines[2], b, hipMemcpyDeviceToDevice, st));
                }
                NFCHK(exchange_planes(T, 0, 0, st));
                for (int i = 0; i < ns; ++i) {
                    nf_solver *S = T->slabs[i]; const long N = S->N;
                    CmfdFaces F; for (int d = 0; d < 3; ++d) { F.Dt[d] = S->d_Dt[d] + g * S->nfc[d]; F.Dh[d] = S->d_Dh[d] + g * S->nfc[d]; }
                    double *diag = S->d_cm, *pp = diag + 3 * N, *q = diag + 4 * N;
                    hipLaunchKernelGGL(k_cmfd_matvec, dim3(gN[i]), dim3(256), 0, st, make_geom(S), F, (const double *)diag, (const double *)pp, q, N, (const CmfdScalars *)sc,
                                       T->d_partials + i * T->slab_cap, S->if_lo ? (const double *)S->d_rlo : (const double *)nullptr,
                                       S->if_hi ? (const double *)S->d_rhi : (const double *)nullptr);
                }
                NFCHK(reduce_logic(1, 1));
                for (int i = 0; i < ns; ++i) {
                    nf_solver *S = T->slabs[i]; const long N = S->N;
                    double *diag = S->d_cm, *x = diag + N, *r = x + N, *pp = r + N, *q = pp + N, *z = q + N;
                    hipLaunchKernelGGL(k_cmfd_update, dim3(gN[i]), dim3(256), 0, st, (const double *)diag, (const double *)pp, (const double *)q, x, r, z, N, (const CmfdScalars *)sc,
                                       T->d_partials + i * T->slab_cap, T->partial_stride);
                }
                NFCHK(reduce_logic(2, 2));
                for (int i = 0; i < ns; ++i) {
                    nf_solver *S = T->slabs[i]; const long N = S->N;
                    hipLaunchKernelGGL(k_cmfd_pupdate, dim3(gN[i]), dim3(256), 0, st, (const double *)(S->d_cm + 5 * N), S->d_cm + 3 * N, N, (const CmfdScalars *)sc);
                }
            }
            HIPCHK(hipMemcpyAsync(&hs, sc, sizeof(hs), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        for (auto *S : T->slabs) {
            S->cmfd_last_its += hs.its;
            hipLaunchKernelGGL(k_cmfd_correct, dim3((unsigned)((S->N + 255) / 256)), dim3(256), 0, st, (const double *)(S->d_cm + S->N), S->d_raw + (size_t)g * S->nphi, S->N, S->nloc, S->cmfd_relax);
        }
    }
    HIPCHK(hipGetLastError());
    return NF_OK;
}

// the two halves of SolveCoarse as separate entry points (undivided meshes): a built coarse handle, and the injection of its
// flux into the fine handle's current flux (piecewise constant, higher moments zero, :2585-2606)
int nf_coarsen(nf_handle S, int rx, int ry, int rz, nf_handle *coarse)
{
    if (!S || !coarse || rx < 1 || ry < 1 || rz < 1) return fail(NF_ERR_ARG, "nf_coarsen: bad arguments");
    NFCHK(void_refuse(S, "nf_coarsen"));
    if (!S->xs_uploaded) return fail(NF_ERR_STATE, "nf_coarsen: call nf_upload_xs first");
    if (!team_is_single(S->team)) return fail(NF_ERR_UNSUPPORTED, "nf_coarsen works on an undivided mesh (slab teams coarsen inside nf_solve_keff)");
    if (S->dim < 2) ry = 1;
    if (S->dim < 3) rz = 1;
    if (S->nx % rx || S->ny % ry || S->nz % rz) return fail(NF_ERR_ARG, "coarse factors (%d,%d,%d) do not divide the mesh %d x %d x %d", rx, ry, rz, S->nx, S->ny, S->nz);
    HIPCHK(hipSetDevice(S->device));
    *coarse = nullptr;
    int rc = coarsen_slab(S, rx, ry, rz, coarse);
    if (rc != NF_OK && *coarse) { std::string keep = g_err; nf_destroy(*coarse); *coarse = nullptr; g_err = keep; }
    return rc;
}
int nf_prolong(nf_handle C, nf_handle S)
{
    if (!C || !S) return fail(NF_ERR_ARG, "nf_prolong: null handle");
    if (C->ng != S->ng || C->dim != S->dim || C->nloc != 1 || C->nx < 1 || S->nx % C->nx || S->ny % C->ny || S->nz % C->nz || C->device != S->device)
        return fail(NF_ERR_ARG, "nf_prolong: %d x %d x %d is not a coarsening of %d x %d x %d (same device, groups, dimension; RT0-P0 coarse mesh)", C->nx, C->ny, C->nz, S->nx, S->ny, S->nz);
    HIPCHK(hipSetDevice(S->device));
    hipStream_t st = S->team->stream;
    HIPCHK(hipStreamSynchronize(C->team->stream));
    HIPCHK(hipMemsetAsync(S->d_phi, 0, (size_t)S->nphi * S->ng * sizeof(double), st));
    hipLaunchKernelGGL(k_prolong, dim3((unsigned)((S->N + 255) / 256)), dim3(256), 0, st, C->d_phi, S->d_phi, S->nx, S->ny, S->nz,
                       S->nx / C->nx, S->ny / C->ny, S->nz / C->nz, S->ng, S->nphi);
    HIPCHK(hipStreamSynchronize(st));
    return NF_OK;
}
// counters and timers of the last solve as one JSON object (profiling slots of nf_profile_get, iteration counts)
int nf_timers(nf_handle S, char *buf, size_t len)
{
    if (!S || !buf || len < 2) return fail(NF_ERR_ARG, "nf_timers: bad arguments");
    nf_team *T = S->team;
    std::string js = "{";
    char tmp[160];
    for (const char *nm : SLOT_NAMES) {
        long c = 0, sk = 0; double msum = 0.0;
        T->prof[nm].stats(&c, &msum, &sk);
        snprintf(tmp, sizeof tmp, "\"%s\": {\"count\": %ld, \"ms\": %.6f, \"skipped_noop\": %ld}, ", nm, c, msum, sk);
        js += tmp;
    }
    snprintf(tmp, sizeof tmp, "\"last_outer\": %d, \"coarse_outer\": %d, \"last_cg_total\": %ld, \"separator_sweeps\": %d}", T->last_outer, T->coarse_outer, T->last_cg_total, T->sep_sweeps);
    js += tmp;
    if (js.size() + 1 > len) return fail(NF_ERR_ARG, "nf_timers: buffer of %zu bytes is too small (%zu needed)", len, js.size() + 1);
    memcpy(buf, js.c_str(), js.size() + 1);
    return NF_OK;
}

// The scatter blocks k_group_rhs / k_diag_group read for group g: Ms[g <- g'], or Ms[g' <- g] when transposed (adjoint); nullptr beyond ng.
static ScatterArgs scatter_args(const nf_solver *S, int g, bool transposed)
{
    ScatterArgs sa; sa.ng = S->ng;
    for (int gp = 0; gp < 64; ++gp) sa.M[gp] = gp < S->ng ? S->d_Ms[transposed ? gp * S->ng + g : g * S->ng + gp] : nullptr;
    return sa;
}

// ---- the history of a solve whose outer loop ran on the device ----------------------------------------------------
// d_hist: three rows (k, dk, dphi) of max_outer entries (+ 8 for NF_STAMPS); with CG counts (cg: the one-launch solves) d_hist_cg and d_rout
static int hist_reserve(nf_team *T, int max_outer, bool cg)
{
    const int ng = T->slabs[0]->ng;
    if (T->hist_cap < max_outer) { NFCHK(dalloc(&T->d_hist, (size_t)3 * max_outer + 8)); T->hist_cap = max_outer; }
    if (cg && T->hist_cg_cap < max_outer * ng) { NFCHK(dalloc(&T->d_hist_cg, (size_t)max_outer * ng)); T->hist_cg_cap = max_outer * ng; }
    if (cg && !T->d_rout) NFCHK(dalloc(&T->d_rout, 1));
    return NF_OK;
}
// n outers of it into hist_k / dk / dphi / cg (`row`: the row length the kernels wrote d_hist with), last_its, last_outer, last_cg_total;
// status 2 of the device loop is the divergence the host-driven loop reports
static int hist_fetch(nf_team *T, int n, size_t row, bool cg, long cg_total, int status)
{
    const int ng = T->slabs[0]->ng;
    T->hist_k.resize(n); T->hist_dk.resize(n); T->hist_dphi.resize(n); T->hist_cg.assign((size_t)n * ng, 0);
    if (n > 0) {
        HIPCHK(hipMemcpy(T->hist_k.data(), T->d_hist, n * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(T->hist_dk.data(), T->d_hist + row, n * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(T->hist_dphi.data(), T->d_hist + 2 * row, n * sizeof(double), hipMemcpyDeviceToHost));
        if (cg) {
            HIPCHK(hipMemcpy(T->hist_cg.data(), T->d_hist_cg, (size_t)n * ng * sizeof(int), hipMemcpyDeviceToHost));
            for (int g = 0; g < ng; ++g) T->last_its[g] = T->hist_cg[(size_t)(n - 1) * ng + g];
        }
    }
    T->last_outer = n; T->last_cg_total = cg_total;
    if (status == 2) return fail(NF_ERR_NUMERIC, "power iteration diverged (outer %d: k=%g dphi=%g)", n - 1, n > 0 ? T->hist_k[n - 1] : 0.0, n > 0 ? T->hist_dphi[n - 1] : 0.0);
    return NF_OK;
}

// ---- diagonal path, outer loop on the device (undivided mesh, no CMFD) --------------------------------------------
static int solve_keff_diag_device(nf_team *T, const nf_keff_opts *o, double keff0, const ChebTable &cheb, double *keff_out)
{
    nf_solver *S = T->slabs[0];
    const int ng = S->ng; const long N = S->N, NP = S->nphi, NT = NP * ng;
    hipStream_t st = T->stream;
    if (!S->d_p0) { NFCHK(dalloc(&S->d_p0, (size_t)NT)); NFCHK(dalloc(&S->d_p1, (size_t)NT)); }
    if (!T->d_ost) NFCHK(dalloc(&T->d_ost, 1));
    NFCHK(hist_reserve(T, o->max_outer, false));
    double *hk = T->d_hist, *hdk = hk + T->hist_cap, *hdp = hdk + T->hist_cap;   // the row length here is hist_cap
    OuterState h; memset(&h, 0, sizeof h);
    h.keff = keff0; h.tol_keff = o->tol_keff; h.tol_flux = o->tol_flux; h.max_outer = o->max_outer; h.cheb = cheb;
    HIPCHK(hipMemcpyAsync(T->d_ost, &h, sizeof h, hipMemcpyHostToDevice, st));
    const int gN = grid_for(NP);
    const long stride = T->partial_stride;
    hipLaunchKernelGGL(k_fission, dim3(gN), dim3(256), 0, st, S->d_Mf, S->d_phi, ng, NP, S->d_tf, T->d_partials, (const double *)nullptr, 0L);
    OuterState hs = h;
    int queued = 0;
    while (queued < o->max_outer) {
        const int nb = std::min(queued == 0 ? 8 : 32, o->max_outer - queued);
        for (int b = 0; b < nb; ++b) {
            for (int g = 0; g < ng; ++g) {
                hipLaunchKernelGGL(k_diag_group, dim3(gN), dim3(256), 0, st, scatter_args(S, g, false), g, S->d_Chi + g * N, S->d_tf, S->d_raw, S->d_phi, S->d_Sinv + g * N,
                                   S->d_Mf + (size_t)g * NP, S->d_raw + (size_t)g * NP, NP, T->d_ost, T->d_partials, stride);
            }
            hipLaunchKernelGGL(k_outer_logic, dim3(1), dim3(256), 0, st, T->d_partials, gN, gN, stride, T->d_ost, hk, hdk, hdp);
            hipLaunchKernelGGL(k_normalize_fission, dim3(gN), dim3(256), 0, st, S->d_raw, S->d_phi, S->d_p0, S->d_p1, S->d_Mf, ng, NP, T->d_ost, S->d_tf, T->d_partials);
        }
        queued += nb;
        HIPCHK(hipMemcpyAsync(&hs, T->d_ost, sizeof hs, hipMemcpyDeviceToHost, st));
        HIPCHK(stream_wait(st));
        if (hs.done || hs.done_next) break;
    }
    HIPCHK(hipGetLastError());
    NFCHK(hist_fetch(T, hs.it, (size_t)T->hist_cap, false, 0, hs.done));
    *keff_out = hs.keff;
    return NF_OK;
}

// ---- resident solve (k_resident_keff): whole power iteration of a small undivided mesh in one launch ------------------
static bool resident_plan(const nf_solver *S, ResidentArgs *A)
{
    const int K = 2;
    int lanes = (S->nx + K - 1) / K, lpl_log2 = 0;
    while ((1 << lpl_log2) < lanes && lpl_log2 < 6) ++lpl_log2;
    const int LPL = 1 << lpl_log2, LPW = 64 / LPL;
    if (S->nx > LPL * K) return false;                           // one chunk per x line (nx <= 128)
    const int seg = S->nb > 0 ? 4 : 8;
    for (int r = 0; r < 2; ++r) {
        if (S->dim < r + 2) { A->n[r] = 1; A->TX[r] = 8; A->NSEG[r] = 1; A->gx[r] = A->gy[r] = 0; A->sl[r] = A->ostride[r] = 0; continue; }
        const int n = r == 0 ? S->ny : S->nz;
        const int NSEG = (n + seg - 1) / seg;
        if (NSEG > 64) return false;
        int TX = 64;
        while (TX > 8 && TX * NSEG > 512) TX >>= 1;
        while (TX > 8 && TX / 2 >= S->nx) TX >>= 1;
        const long nxy = (long)S->nx * S->ny;
        A->n[r] = n; A->TX[r] = TX; A->NSEG[r] = NSEG; A->gx[r] = (S->nx + TX - 1) / TX; A->gy[r] = r == 0 ? S->nz : S->ny;
        A->sl[r] = r == 0 ? S->nx : nxy; A->ostride[r] = r == 0 ? nxy : S->nx;
    }
    A->lpl_log2 = lpl_log2; A->ntask_x = (int)((S->nlines[0] + LPW - 1) / LPW);
    return true;
}
// the plan of the line-per-lane variants for this mesh (nf_resident_lanes.h), and whether one of them takes it
static long resident_lds_cap(const nf_team *T) { return (long)T->lds_limit / 8 - 32; }
static LanePlan resident_lane_plan(const nf_team *T, const nf_solver *S)
{
    return lane_plan(S->dim, S->nx, S->ny, S->nz, S->nlines, S->nb, S->nloc, n_modes(S), T->opt.resident_two_sided != 0, resident_lds_cap(T));
}
static bool resident_serial_fits(const nf_team *T, const nf_solver *S, LanePlan *plan = nullptr)
{
    const LanePlan lp = resident_lane_plan(T, S);
    if (plan) *plan = lp;
    return T->opt.resident_serial && T->opt.resident_lds && lp.fits;
}
static const int NF_RESIDENT_UNAVAILABLE = 1;                     // positive: not an error code of the C ABI
// The instantiation a mesh takes (nf_batch_result::variant), its two entries -- one mesh per launch, one mesh per workgroup -- and the dynamic LDS
struct ResidentKernels { void (*one)(ResidentArgs); void (*batch)(ResidentArgsConst *, int); };
static ResidentKernels resident_kernels(int variant)
{
#define NF_RES_K(...) ResidentKernels{ k_resident_keff<__VA_ARGS__>, k_resident_keff_batch<__VA_ARGS__> }
    switch (variant) {
    case 1: return NF_RES_K(false, 0, 1536);
    case 2: return NF_RES_K(false, 0, 2560);
    case 3: return NF_RES_K(false, 1, -1);
    case 4: return NF_RES_K(false, 2, -1);
    case 5: return NF_RES_K(false, 0);
    case 6: return NF_RES_K(true, 0);
    case 7: return NF_RES_K(false, 1);
    case 8: return NF_RES_K(true, 1);
    case 9: return NF_RES_K(false, 2);
    case 10: return NF_RES_K(true, 2);
    default: return ResidentKernels{ nullptr, nullptr };              // 0: no plan (resident_choose refused the mesh)
    }
#undef NF_RES_K
}
static const int NF_RESIDENT_BLOCK = 512;
// What depends on the mesh and the options alone: the plan fields of A, the instantiation and its LDS.  Changes nothing; false: not eligible.
struct ResidentLaunch { ResidentArgs A; int variant = 0; size_t lds = 0; bool serial = false; };
static bool resident_choose(const nf_team *T, ResidentLaunch *R)
{
    const nf_solver *S = T->slabs[0];
    ResidentArgs &A = R->A; memset(&A, 0, sizeof A);
    const bool planned = resident_plan(S, &A);
    LanePlan lp;
    const bool lanes_fit = resident_serial_fits(T, S, &lp);
    if (!planned && !lanes_fit) return false;
    // LDS plan: 160 KiB per workgroup; behind the scratch of the direction passes the CG vectors and this group's factors, in
    // priority order, as far as they fit (ResidentArgs::lds_mask)
    A.lds_mask = 0;
    // the line-per-lane variants, when everything their sweeps touch fits in LDS (p, the contribution of every direction, the factors and
    // the per-line values): RT0-P0 at a compile-time block pitch; RT_k-P_m with bubble moments, DOF = moment * PC + padded cell
    const long cap = resident_lds_cap(T);
    R->serial = S->nphi <= T->opt.resident_serial_max_dofs && lanes_fit;
    if (R->serial) {
        for (int d = 0; d < 3; ++d) A.tw[d] = lp.tw[d];
        for (int d = 0; d < 4; ++d) A.slot0[d] = lp.slot0[d];
        R->lds = (size_t)lp.need * sizeof(double);
        if (S->nb == 0) R->variant = lp.pitch == 1536 ? 1 : 2;
        else {
            R->variant = S->nb == 1 ? 3 : 4;
            A.PC = (int)lp.PC;
            const int nm = n_modes(S);
            const ModeArgs c = mode_args(S, 0, 0, 0, S->d_p, S->d_q);
            for (int d = 0; d < S->dim; ++d)
                for (int m = 0; m < nm; ++m) {
                    double Ta = 1.0;
                    for (int i = 0; i <= S->nb; ++i) A.mom[d][m][i] = moment_index(S, d, m, i, &Ta);
                    for (int l = 0; l < S->nb; ++l) A.diagc[A.mom[d][m][l + 1]][d] = Ta * c.Gc[l] * c.Gc[l] * c.iM[l];
                }
        }
        return true;
    }
    if (!planned) return false;
    long used = 5 * NF_RESIDENT_BLOCK + 64 + 16;
    if (T->opt.resident_lds) {
        const long NP2 = (S->nphi + 1) & ~1L, N2 = (S->N + 1) & ~1L;
        const int bits[11] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10 };
        for (int b : bits) {
            if ((b == 6 || b == 7) && S->dim < 2) continue;
            if ((b == 8 || b == 9) && S->dim < 3) continue;
            const long need = (b <= 3 || b == 10) ? NP2 : N2;
            if (used + need <= cap) { used += need; A.lds_mask |= 1 << b; }
        }
    }
    R->lds = (size_t)used * sizeof(double);
    R->variant = 5 + 2 * S->nb + (S->nx % 2 == 0 ? 1 : 0);
    return true;
}
// fill: on top of a plan (resident_choose) everything else k_resident_keff reads for this solve, the history buffers included.  Launches nothing.
static int resident_fill(nf_team *T, const nf_keff_opts *o, double keff0, const ChebTable &cheb, double cg_tol, int cg_max, ResidentLaunch *R)
{
    nf_solver *S = T->slabs[0];
    const int ng = S->ng;
    ResidentArgs &A = R->A;
    A.G = make_geom(S); A.ng = ng; A.dim = S->dim; A.nmodes = n_modes(S); A.N = S->N; A.nphi = S->nphi;
    for (int d = 0; d < 3; ++d) {
        const int dd = d < S->dim ? d : 0;
        A.ma[d] = mode_args(S, 0, dd, 0, S->d_p, S->d_q); A.mt[d] = mode_tab(S, dd);
        A.L[d] = S->d_L[dd]; A.DR[d] = S->d_DR[dd]; A.D0[d] = S->d_D0[dd]; A.nlines[d] = S->nlines[dd];
    }
    A.Mf = S->d_Mf; A.Chi = S->d_Chi; A.Ms = S->d_Ms_tab;
    A.phi = S->d_phi; A.raw = S->d_raw; A.p0 = S->d_p0; A.p1 = S->d_p1; A.tf = S->d_tf; A.r = S->d_r; A.p = S->d_p; A.q = S->d_q;
    A.keff0 = keff0; A.tol_keff = o->tol_keff; A.tol_flux = o->tol_flux; A.cg_tol = cg_tol; A.cg_max = cg_max; A.max_outer = o->max_outer;
    A.cheb = cheb;
    NFCHK(hist_reserve(T, o->max_outer, true));
#ifdef NF_STAMPS
    (void)hipMemsetAsync(T->d_hist + 3 * (size_t)o->max_outer, 0, 8 * sizeof(double), T->stream);
#endif
    A.hist = T->d_hist; A.hist_cg = T->d_hist_cg; A.out = T->d_rout;   // the kernel indexes its history with max_outer as the row length
    A.Cd0 = S->d_Cd;
    return NF_OK;
}
// fetch: what the kernel left for this team -- ResidentOut and the history -- once its launch is queued on `st` (or has finished)
static int resident_fetch(nf_team *T, const nf_keff_opts *o, hipStream_t st, double *keff_out)
{
    ResidentOut ro;
    HIPCHK(hipMemcpyAsync(&ro, T->d_rout, sizeof ro, hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(st));
    NFCHK(hist_fetch(T, ro.n_outer, (size_t)o->max_outer, true, ro.cg_total, ro.status));
#ifdef NF_STAMPS
    { long long acc[5]; (void)hipMemcpy(acc, T->d_hist + 3 * (size_t)o->max_outer, sizeof acc, hipMemcpyDeviceToHost);
      if (acc[4] > 0) fprintf(stderr, "[resident stamps] %lld CG iterations: x pass %.0f, y/z passes %.0f, p.q reduction %.0f, r update + |r|^2 reduction %.0f cycles per iteration\n",
                              acc[4], (double)acc[0] / acc[4], (double)acc[1] / acc[4], (double)acc[2] / acc[4], (double)acc[3] / acc[4]); }
#endif
    *keff_out = ro.keff;
    return NF_OK;
}
static int solve_keff_resident(nf_team *T, const nf_keff_opts *o, double keff0, const ChebTable &cheb, double cg_tol, int cg_max, double *keff_out)
{
    ResidentLaunch R;
    if (!resident_choose(T, &R)) return fail(NF_ERR_STATE, "resident solve: mesh not eligible");
    NFCHK(resident_fill(T, o, keff0, cheb, cg_tol, cg_max, &R));
    const ResidentKernels K = resident_kernels(R.variant);
    if (!K.one) return fail(NF_ERR_STATE, "resident solve: no kernel for this plan");
    if (!lds_opt_in((const void *)K.one, R.lds)) { if (!R.serial) T->last_resident_serial = 0; return NF_RESIDENT_UNAVAILABLE; }
    hipLaunchKernelGGL(K.one, dim3(1), dim3(NF_RESIDENT_BLOCK), R.lds, T->stream, R.A);
    T->last_resident_serial = R.serial ? 1 : 0;
    HIPCHK(hipGetLastError());
    return resident_fetch(T, o, T->stream, keff_out);
}

// ---- whole SolveKeff on one XCD (k_keff_xcd): the meshes of k_cg_xcd, iterative full-Schur path ------------------------
// returns NF_RESIDENT_UNAVAILABLE when the workgroups did not assemble (nothing has been touched: the host-driven path takes over)
static int solve_keff_xcd(nf_team *T, const nf_keff_opts *o, const Fuse3Plan &P, double keff0, const ChebTable &cheb, double cg_tol, int cg_max,
                          double *keff_out)
{
    nf_solver *S = T->slabs[0];
    const int ng = S->ng; hipStream_t st = T->stream;
    if (!S->d_p2) NFCHK(dalloc(&S->d_p2, S->nphi));
    if (S->dim >= 2 && !S->d_qy) NFCHK(dalloc(&S->d_qy, S->nphi));
    if (S->dim == 3 && !S->d_qz) NFCHK(dalloc(&S->d_qz, S->nphi));
    XcdArgs A; int nch = 1;
    NFCHK(xcd_fill(S, 0, P, A, &nch));
    XcdOuter O; memset(&O, 0, sizeof O);
    O.ng = ng; O.NP = S->nphi; O.N = S->N;
    O.Mf = S->d_Mf; O.Chi = S->d_Chi; O.Ms = S->d_Ms_tab;
    O.phi = S->d_phi; O.raw = S->d_raw; O.p0 = S->d_p0; O.p1 = S->d_p1; O.tf = S->d_tf;
    for (int d = 0; d < 3; ++d) O.nl[d] = S->nlines[d < S->dim ? d : 0];
    O.keff0 = keff0; O.tol_keff = o->tol_keff; O.tol_flux = o->tol_flux; O.cg_tol = cg_tol; O.cg_max = cg_max; O.max_outer = o->max_outer;
    O.cheb = cheb;
    NFCHK(hist_reserve(T, o->max_outer, true));
    O.hist = T->d_hist; O.hist_cg = T->d_hist_cg; O.out = T->d_rout;
    const size_t lds = XCD_LDS; const unsigned G = 8u * (unsigned)T->opt.cg_xcd_groups;
    NFCHK(xcd_select("k_keff_xcd", S, P, nch, [&](auto t) -> int { using I = decltype(t);
        if (!lds_opt_in((const void *)k_keff_xcd<I::NCH, I::VEC, I::NB, I::SEG>, lds)) return NF_RESIDENT_UNAVAILABLE;
        hipLaunchKernelGGL((k_keff_xcd<I::NCH, I::VEC, I::NB, I::SEG>), dim3(G), dim3(XCD_THREADS), lds, st, A, O);
        return NF_OK;
    }));
    HIPCHK(hipGetLastError());
    ResidentOut ro;
    HIPCHK(hipMemcpyAsync(&ro, T->d_rout, sizeof ro, hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(st));
    if (ro.status == 3) { T->opt.keff_xcd = 0; T->opt.cg_xcd = 0; ++T->xcd_refused; return NF_RESIDENT_UNAVAILABLE; }
    if (ro.status == 4) { T->opt.keff_xcd = 0; T->opt.cg_xcd = 0; return fail(NF_ERR_HIP, "XCD-local SolveKeff (k_keff_xcd): a grid barrier timed out in outer iteration %d (a participant was lost); the path is now off for this solver", ro.n_outer); }
    T->xcd_solves += (long)ro.n_outer * ng; T->last_xcd = 1;
    NFCHK(hist_fetch(T, ro.n_outer, (size_t)o->max_outer, true, ro.cg_total, ro.status));
    *keff_out = ro.keff;
    return NF_OK;
}

// ---- SolveKeff (src/NeutFEM.cpp:1627-1815) -----------------------------------------------------
// The group solver of the host-driven outer loops (SolveKeff, SolveSubcritical).
// SchurSolver type: DIRECT_* or n_phi < 200 -> "exact" solve (CG to 1e-14 stands in)
// SchurSolver::NeedsExplicitSchur (src/solvers.cpp:114-124): direct types, a type that was never pushed (quirk 11), n_phi < 200.
// Undivided meshes up to direct_max_dofs get the real thing (dense S^-1, dense_prepare); beyond that and on slab teams CG to
// 1e-14 stands in, bounded so that an ill-conditioned S (IAEA-3D: cond ~1e17) cannot run away; such solves are counted.
struct InnerPlan { bool direct, dense; double cg_tol; int cg_max; };
static InnerPlan inner_plan(const nf_team *T, const nf_keff_opts *o)
{
    const bool single = team_is_single(T);
    long Ntot = 0; for (auto *S : T->slabs) Ntot += S->nphi;
    InnerPlan p;
    p.direct = !o->solver_type_pushed || o->solver_type <= 2 || (single && Ntot < 200);
    p.dense = p.direct && single && !T->rccl_reduce && Ntot <= T->opt.direct_max_dofs && !T->slabs[0]->d_void;   // nf_set_void: the dense S^-1 is formed without the mask; CG to 1e-14 stands in
    p.cg_tol = p.direct ? 1e-14 : o->tol_flux;                    // SetTolerance forwards tol_flux (:334)
    p.cg_max = p.direct ? (int)std::min<long>(20 * Ntot + 50, 200000L) : o->max_inner;   // CG ends in <= n steps in exact arithmetic
    return p;
}

// What the host-driven drivers do before their first sweep: team_prepare, the diagonal S^-1 where the driver allows it (flag dropped for
// order > 0, :1640-1644; whole team, slabs exchange one edge plane per group), `between` (SolveKeff: CMFD and the coarse start), then the
// group solver of inner_plan, last_direct, and the dense S^-1 where inner_plan picks it.  DIAG_LEAN (SolveModes) is DIAG_OK without the
// dense S^-1 the diagonal path never reads; SolveKeff and SolveSubcritical have always formed it.
enum DiagUse { DIAG_NEVER, DIAG_OK, DIAG_LEAN };
static bool diag_wanted(const nf_solver *S0, const nf_keff_opts *o) { return o->use_diagonal_solver && S0->k == 0 && S0->m == 0; }   // :1640-1644
struct Inner { InnerPlan ip; int use_diag; };
template <class Between>
static int inner_begin(nf_team *T, const nf_keff_opts *o, DiagUse diag, Inner *in, Between between)
{
    nf_solver *S0 = T->slabs[0];
    NFCHK(team_prepare(T));
    in->use_diag = (diag != DIAG_NEVER && diag_wanted(S0, o)) ? 1 : 0;
    if (in->use_diag) NFCHK(nf_build_diagonal_cache(S0));
    NFCHK(between());
    in->ip = inner_plan(T, o);
    T->last_direct = in->ip.dense ? 1 : in->ip.direct ? 2 : 0;
    if (in->ip.dense && !(diag == DIAG_LEAN && in->use_diag)) NFCHK(dense_prepare(T));
    return NF_OK;
}
static int inner_begin(nf_team *T, const nf_keff_opts *o, DiagUse diag, Inner *in) { return inner_begin(T, o, diag, in, [] { return NF_OK; }); }

// ---- the group sweep (src/NeutFEM.cpp:1716-1726) -------------------------------------------------------------------
// One Gauss-Seidel sweep over the energy groups of a team, the one rule every host-driven driver shares: for group g the right-hand side
// fscale * emis_g * tf + scatter_g (+ q_g), the groups this sweep has already solved read from `phi_new`, the others from `phi_old`
// (k_group_rhs: gp < g new, gp > g old -- a descending sweep therefore passes the one array as both), then the group solver: the diagonal
// S^-1 fused into k_group_rhs, the dense S^-1, or CG.  GroupSweep states what the drivers differ in; a driver fills it once per solve
// (sweep_for, then its own fields) and changes per sweep only what its iteration changes (fscale, a column's arrays).
struct SweepSlab {
    const double *emis = nullptr;                         // emission coefficient, group g at + g * N: d_Chi, d_NSF (adjoint)
    const double *phi_new = nullptr, *phi_old = nullptr;  // all groups
    double *sol = nullptr;                                // the solution, group g at + g * nphi
    const double *q = nullptr;                            // external source, group g at + g * nphi; nullptr: k_group_rhs<false>
};
struct GroupSweep {
    bool transposed = false, descending = false;
    double fscale = 1.0;                                  // 1/k, or the fission scale of a fixed-source solve
    bool ride_start = true;                               // CG: x = 0, r = p = rhs and the |rhs|^2 partials ride in k_group_rhs (cg_solve(..., inited))
    bool skip_poisoned = false;                           // SolveKeff: a poisoned rank launches nothing of its own but stays in cg_solve's collectives
    nf_team *count_team = nullptr;                        // whose standin_unconverged counts a stand-in solve that ended above 1e-14; nullptr: not counted
    std::vector<SweepSlab> slab;
    std::vector<int> grid;                                // grid_for(nphi) per slab
    std::vector<const double *> rhs; std::vector<double *> sol;   // cg_solve's per-slab operands of the current group
};
static GroupSweep sweep_for(nf_team *T)
{
    const size_t ns = T->slabs.size();
    GroupSweep w; w.count_team = T;
    w.slab.resize(ns); w.grid.resize(ns); w.rhs.resize(ns); w.sol.resize(ns);
    for (size_t i = 0; i < ns; ++i) w.grid[i] = grid_for(T->slabs[i]->nphi);
    return w;
}
// formed(g): after the right-hand side of group g is in d_rhs, before its solve.  solved(g, its): after the solve.
static void sweep_no_hook(int) { }
template <class Formed, class Solved>
static int group_sweep(nf_team *T, const InnerPlan &ip, int use_diag, GroupSweep &w, Formed formed, Solved solved)
{
    const int ns = (int)T->slabs.size(), ng = T->slabs[0]->ng;
    const bool cgi = w.ride_start && !use_diag && !ip.dense;
    const auto rhs_kernel = !w.slab[0].q ? k_group_rhs<false> : k_group_rhs<true>;
    for (int s = 0; s < ng; ++s) {
        const int g = w.descending ? ng - 1 - s : s;
        for (int i = 0; i < ns; ++i) {
            nf_solver *S = T->slabs[i]; const SweepSlab &b = w.slab[i]; const long N = S->N, NP = S->nphi;
            double *sol = b.sol + g * NP;
            w.rhs[i] = S->d_rhs; w.sol[i] = sol;
            if (w.skip_poisoned && T->poisoned) continue;
            hipLaunchKernelGGL(rhs_kernel, dim3(w.grid[i]), dim3(256), 0, T->stream, scatter_args(S, g, w.transposed), g,
                               b.emis + g * N, (const double *)S->d_tf, w.fscale, b.phi_new, b.phi_old,
                               use_diag ? S->d_Sinv + g * N : (const double *)nullptr, use_diag ? sol : S->d_rhs, NP, N,
                               cgi ? sol : (double *)nullptr, cgi ? S->d_r : (double *)nullptr, cgi ? S->d_p : (double *)nullptr,
                               cgi ? T->d_partials + i * T->slab_cap : (double *)nullptr, b.q ? b.q + g * NP : (const double *)nullptr);
        }
        formed(g);
        int its = 0; double res = 0.0;
        if (use_diag) { }
        else if (ip.dense) { dense_solve(T, g, w.rhs[0], w.sol[0]); its = 1; }          // last_iterations_ = 1 (src/solvers.cpp:447)
        else {
            NFCHK(cg_solve(T, g, w.rhs, w.sol, ip.cg_tol, ip.cg_max, &its, w.count_team ? &res : nullptr, cgi));
            if (w.count_team && ip.direct && !(res <= 1e-14)) ++w.count_team->standin_unconverged;
        }
        solved(g, its);
    }
    return NF_OK;
}

// Whether SolveKeff of this team with these options runs in one workgroup (k_resident_keff); nf_solve_keff_batch asks the same question
// before it touches anything.  Reads the team, the options and the group solver they pick, changes nothing.
static bool keff_takes_resident(const nf_team *T, const nf_keff_opts *o, const InnerPlan &ip, int use_diag)
{
    const nf_solver *S0 = T->slabs[0];
    ResidentArgs probe;
    return team_is_single(T) && !use_diag && !o->use_cmfd && !ip.direct && !T->rccl_reduce && T->opt.resident && o->max_outer > 0 && !S0->d_void &&   // nf_set_void: the resident kernel knows no mask
           ((S0->nphi <= T->opt.resident_max_dofs && resident_plan(S0, &probe)) || (S0->nphi <= T->opt.resident_serial_max_dofs && resident_serial_fits(T, S0)));
}
// What SolveKeff does before its first outer: inner_begin with CMFD and the coarse start in between, the start value of k, the reset of
// the history.  And every exit of a finished solve (:1808-1809).  jz_valid is read by nf_get_J on slabs with an interface only, which the
// exits of the undivided paths never see (team_is_single): clearing it there too changes nothing
static int keff_begin(nf_team *T, const nf_keff_opts *o, Inner *in, double *keff0)
{
    double keff = 1.0;
    auto cmfd_and_coarse_start = [&]() -> int {
        if (o->use_cmfd) NFCHK(cmfd_initialize_team(T));          // :1655-1658
        keff = T->has_valid_keff ? T->last_keff : 1.0;            // :1662
        T->coarse_outer = 0;
        if (o->use_coarse_init && o->n_coarse_factors > 0) {      // :1665-1670
            bool done = false; double kc = 1.0;
            std::vector<double *> dsts; for (auto *S : T->slabs) dsts.push_back(S->d_phi);
            NFCHK(coarse_init(T, o, &kc, dsts, &done));
            keff = done ? kc : 1.0;
        }
        return NF_OK;
    };
    NFCHK(inner_begin(T, o, DIAG_OK, in, cmfd_and_coarse_start));
    T->hist_k.clear(); T->hist_dk.clear(); T->hist_dphi.clear(); T->hist_cg.clear();
    T->last_outer = 0; T->last_cg_total = 0;
    T->profile = o->profile != 0;
    *keff0 = keff;
    return NF_OK;
}
static int keff_finish(nf_team *T, double keff, bool is_diag, double *keff_out, int *n_outer)
{
    for (auto *S : T->slabs) { S->raw_valid = T->last_outer > 0; S->raw_is_diag = is_diag; S->jz_valid = false; }
    T->has_valid_keff = 1; T->last_keff = keff;
    if (keff_out) *keff_out = keff;
    if (n_outer) *n_outer = T->last_outer;
    return NF_OK;
}

static int solve_keff_impl(nf_team *T, const nf_keff_opts *o, double *keff_out, int *n_outer)
{
    const int ns = (int)T->slabs.size();
    nf_solver *S0 = T->slabs[0];
    const int ng = S0->ng;
    const bool single = team_is_single(T);
    const bool use_cmfd = o->use_cmfd != 0;
    double keff = 1.0;
    Inner in;
    NFCHK(keff_begin(T, o, &in, &keff));
    const InnerPlan &ip = in.ip; const int use_diag = in.use_diag;
    const ChebTable cheb = cheb_table();                          // ChebyshevAccel(15, 0.98), src/solvers.cpp:664-700
    int cheb_it = 0;
    auto finish = [&](bool is_diag) { return keff_finish(T, keff, is_diag, keff_out, n_outer); };
    if (use_diag && single && !use_cmfd && !T->rccl_reduce && T->opt.outer_dev && o->max_outer > 0) {
        NFCHK(solve_keff_diag_device(T, o, keff, cheb, &keff));
        HIPCHK(hipStreamSynchronize(T->stream));
        T->profile = false; T->last_path = 1;
        return finish(true);
    }
    T->last_path = 0;
    if (keff_takes_resident(T, o, ip, use_diag)) {
        const bool prof_req = T->profile;
        T->last_path = 2; T->profile = false;
        const int rr = solve_keff_resident(T, o, keff, cheb, ip.cg_tol, ip.cg_max, &keff);
        if (rr != NF_RESIDENT_UNAVAILABLE) { NFCHK(rr); return finish(false); }
        T->last_path = 0; T->profile = prof_req;                  // the device refused the LDS the resident kernel plans with: host-driven path
    }
    // mid-size meshes (2 k - 28 k unknowns per group, every order): the whole power iteration in one launch on one XCD (k_keff_xcd),
    // where the group solves would take the one-XCD form of CG
    const CgPlan cp = cg_plan(T);
    if (!use_diag && !use_cmfd && !ip.direct && o->max_outer > 0 && T->opt.keff_xcd && cp.form == CG_XCD) {
        T->last_path = 3;
        const int rx = solve_keff_xcd(T, o, cp.f3, keff, cheb, ip.cg_tol, ip.cg_max, &keff);
        if (rx != NF_RESIDENT_UNAVAILABLE) { NFCHK(rx); return finish(false); }
        T->last_path = 0;
    }
    double hout[5] = { 0, 0, 0, 0, 0 };
    std::vector<int> gN(ns), gT(ns);
    for (int i = 0; i < ns; ++i) { gN[i] = grid_for(T->slabs[i]->nphi); gT[i] = grid_for(T->slabs[i]->nphi * ng); }
    GroupSweep sw = sweep_for(T);
    sw.skip_poisoned = true;
    for (int i = 0; i < ns; ++i) { nf_solver *S = T->slabs[i]; sw.slab[i].emis = S->d_Chi; sw.slab[i].phi_new = S->d_raw; sw.slab[i].phi_old = S->d_phi; sw.slab[i].sol = S->d_raw; }
    const bool multi = T->nproc > 1;
    // multi-rank teams: a rank-local failure between two collectives of the outer iteration poisons the rank instead of ending its part
    // of the schedule (team_poison); every rank then leaves at the same point -- the first reduction of the next CG solve, or the
    // per-outer reduction, whichever comes first
#define NF_OUTER_CHK(x) do { const int r_ = (x); if (team_poison(T, r_)) return r_; } while (0)
    for (int it = 0; it < o->max_outer; ++it) {
        if (multi && T->rank == T->inject_rank && T->inject_where == 'o' && it == T->inject_outer)
            NF_OUTER_CHK(fail(NF_ERR_HIP, "injected failure on rank %d at the start of outer iteration %d (NEUTFEM_INJECT_FAIL)", T->rank, it));
        // total_fiss and prod_old (:1700-1707)
        for (int i = 0; i < ns && !T->poisoned; ++i) {
            nf_solver *S = T->slabs[i];
            hipLaunchKernelGGL(k_fission, dim3(gN[i]), dim3(256), 0, T->stream, S->d_Mf, S->d_phi, ng, S->nphi, S->d_tf, T->d_partials + i * T->slab_cap, (const double *)nullptr, 0L);
        }
        NF_OUTER_CHK(team_finalize(T, FIN_SUM, gN, 1, T->d_out, 0.0, 0));
        sw.fscale = 1.0 / keff;
        NFCHK(group_sweep(T, ip, use_diag, sw, sweep_no_hook, [&](int, int its) { T->hist_cg.push_back(its); T->last_cg_total += its; }));
        if (use_cmfd && it >= 2 && !T->poisoned) { if (single) NFCHK(cmfd_step(S0, keff, use_diag)); else NFCHK(cmfd_step_team(T, keff, use_diag)); }   // :1750-1761
        if (multi && T->rank == T->inject_rank && T->inject_where == 'e' && it == T->inject_outer)
            NF_OUTER_CHK(fail(NF_ERR_HIP, "injected failure on rank %d at the end of outer iteration %d (NEUTFEM_INJECT_FAIL)", T->rank, it));
        // prod_new, norms (:1766-1779)
        for (int i = 0; i < ns && !T->poisoned; ++i) {
            nf_solver *S = T->slabs[i];
            hipLaunchKernelGGL(k_outer_reduce, dim3(gT[i]), dim3(256), 0, T->stream, S->d_Mf, S->d_raw, S->d_phi, S->nphi * ng, T->d_partials + i * T->slab_cap, T->partial_stride);
        }
        NF_OUTER_CHK(team_finalize(T, FIN_SUM, gT, 3, T->d_out + 1, 0.0, 0, true));
        NFCHK(readback(T, nullptr, nullptr, T->d_out, hout, multi ? 5 : 4));
        if (multi && (T->poisoned || hout[4] != 0.0)) {            // the ranks' error flags came with the sums: every rank is here, at the same outer
            if (T->poisoned) return team_poison_result(T);
            return fail(NF_ERR_REMOTE, "another rank of the team reported an error during outer iteration %d; every rank stopped there", it);
        }
        const OuterStep os = outer_step(keff, it, hout[0], hout[1], hout[2], hout[3]);
        keff = os.keff;
        if (!os.finite) return fail(NF_ERR_NUMERIC, "power iteration diverged (outer %d: k=%g dphi=%g)", it, os.keff_new, os.dphi);
        // normalise + Chebyshev (:1780-1788, src/solvers.cpp:720-756)
        const ChebStep cs = cheb_next(cheb_it, cheb, it >= 2 && !use_cmfd);       // :1786-1788
        for (int i = 0; i < ns && !T->poisoned; ++i)              // a failed allocation poisons a rank of a team
            NF_OUTER_CHK(normalize_cheb(T->slabs[i], T->stream, T->slabs[i]->d_phi, os.norm, os.do_norm, cs));
        T->hist_k.push_back(keff); T->hist_dk.push_back(os.dk); T->hist_dphi.push_back(os.dphi);
        T->last_outer = it + 1;
        __atomic_store_n(&T->outers_done, (long)(it + 1), __ATOMIC_RELEASE);
        if (T->progress_fn) T->progress_fn(T->progress_user, it, keff, os.dk, os.dphi);
        if (outer_converged(os.dk, os.dphi, o->tol_keff, o->tol_flux) && !T->poisoned) break;   // :1799-1802 (a poisoned rank stays in the schedule until the flag has gone round)
    }
#undef NF_OUTER_CHK
    if (T->poisoned) {                                            // poisoned in the last outer the loop ran: one more reduction takes the flag to everybody
        (void)team_finalize(T, FIN_SUM, gN, 1, T->d_out, 0.0, 0, true);
        (void)team_stream_wait(T, T->stream);
        return team_poison_result(T);
    }
    HIPCHK(hipStreamSynchronize(T->stream));
    HIPCHK(hipGetLastError());
    if (T->profile) prof_collect(T);
    T->profile = false;
    return finish(use_diag != 0);
}

int nf_solve_keff(nf_handle S, const nf_keff_opts *o, double *keff, int *n_outer)
{
    if (!S || !o) return fail(NF_ERR_ARG, "nf_solve_keff: bad arguments");
    if ((o->use_diagonal_solver && S->k == 0 && S->m == 0) || o->use_cmfd || o->use_coarse_init) NFCHK(void_refuse(S, "nf_solve_keff with use_diagonal_solver, use_cmfd or use_coarse_init"));
    if (S->team->dead) return fail(NF_ERR_COMM, "this team lost a collective (NF_ERR_COMM) and is unusable: destroy the handles and end the process with a non-zero code (never re-exec)");
    for (auto *X : S->team->slabs) if (!X->built) return fail(NF_ERR_STATE, "nf_solve_keff: call nf_build first");
    HIPCHK(hipSetDevice(S->device));
    __atomic_store_n(&S->team->outers_done, 0L, __ATOMIC_RELEASE);
    return solve_keff_impl(S->team, o, keff, n_outer);
}

// ---- nf_solve_keff_batch: n independent small meshes, one workgroup each, in one launch (k_resident_keff_batch) ----------
// Batched route or not: decided from the handles, the options and the plans alone, before anything is touched.  On the batched route every
// handle runs keff_begin, resident_fill, resident_fetch and keff_finish -- the functions solve_keff_impl runs around its own launch -- so that
// what a handle holds afterwards is what nf_solve_keff leaves; the one thing the handles share is the launch.
int nf_solve_keff_batch(nf_handle *h, int n, const nf_keff_opts *opts, int n_opts, double *keff, int *n_outer, int *status, nf_batch_result *res)
{
    if (!h || !opts || n < 1 || (n_opts != 1 && n_opts != n)) return fail(NF_ERR_ARG, "nf_solve_keff_batch: n >= 1 handles and 1 or n option sets");
    for (int i = 0; i < n; ++i) {
        if (!h[i]) return fail(NF_ERR_ARG, "nf_solve_keff_batch: handle %d is NULL", i);
        if (h[i]->device != h[0]->device) return fail(NF_ERR_ARG, "nf_solve_keff_batch: handle %d is on device %d, handle 0 on device %d", i, h[i]->device, h[0]->device);
    }
    { std::vector<nf_solver *> sorted(h, h + n); std::sort(sorted.begin(), sorted.end());
      if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(NF_ERR_ARG, "nf_solve_keff_batch: the same handle twice (two workgroups would write the same vectors)"); }
    for (int i = 0; i < n; ++i) {
        const nf_team *T = h[i]->team;
        if (T->dead) return fail(NF_ERR_COMM, "nf_solve_keff_batch: the team of handle %d lost a collective (NF_ERR_COMM) and is unusable", i);
        if (!team_is_single(T)) return fail(NF_ERR_UNSUPPORTED, "nf_solve_keff_batch: handle %d is a slab (nf_create_slab / nf_link_slabs); a batch takes undivided meshes only", i);
        if (T->nproc > 1 || T->comm || T->rccl_reduce) return fail(NF_ERR_UNSUPPORTED, "nf_solve_keff_batch: handle %d has a communicator (nf_comm_init); a batch must not reorder collectives", i);
        if (!h[i]->built) return fail(NF_ERR_STATE, "nf_solve_keff_batch: handle %d: call nf_build first", i);
    }
    auto opt_of = [&](int i) { return &opts[n_opts == 1 ? 0 : i]; };
    if (res) { res->n_batched = res->n_sequential = res->n_launches = res->variant = 0; }
    HIPCHK(hipSetDevice(h[0]->device));
    nf_team *T0 = h[0]->team;
    // ---- the route
    std::vector<ResidentLaunch> R(n);
    bool batched = true;
    for (int i = 0; i < n && batched; ++i) {
        const nf_solver *S = h[i], *S0 = h[0]; const nf_team *T = S->team; const nf_keff_opts *o = opt_of(i);
        const NfOptions &a = T->opt, &b = T0->opt;
        batched = S->k == S0->k && S->m == S0->m && S->ng == S0->ng && S->dim == S0->dim && S->nx == S0->nx && S->ny == S0->ny && S->nz == S0->nz &&
                  a.resident_serial == b.resident_serial && a.resident_lds == b.resident_lds && a.resident_two_sided == b.resident_two_sided &&
                  a.resident_serial_max_dofs == b.resident_serial_max_dofs && a.resident_max_dofs == b.resident_max_dofs && T->lds_limit == T0->lds_limit &&
                  !o->use_coarse_init && keff_takes_resident(T, o, inner_plan(T, o), diag_wanted(S, o) ? 1 : 0) && resident_choose(T, &R[i]) &&
                  R[i].variant == R[0].variant && R[i].lds == R[0].lds;
    }
    const ResidentKernels K = resident_kernels(batched ? R[0].variant : 0);
    if (batched && (!K.batch || !lds_opt_in((const void *)K.batch, R[0].lds))) batched = false;   // the device refuses the LDS the plan asks for: nothing touched yet
    int first = NF_OK;
    if (!batched) {
        for (int i = 0; i < n; ++i) {
            double k = 0.0; int no = 0;
            const int rc = nf_solve_keff(h[i], opt_of(i), &k, &no);
            if (keff) keff[i] = k;
            if (n_outer) n_outer[i] = no;
            if (status) status[i] = rc;
            if (first == NF_OK) first = rc;
        }
        if (res) res->n_sequential = n;
        return first;
    }
    // ---- per handle: the preamble of SolveKeff and the arguments of its workgroup
    std::vector<ResidentArgs> args; args.reserve(n);
    std::vector<int> live, st(n, NF_OK);
    const ChebTable cheb = cheb_table();
    for (int i = 0; i < n; ++i) {
        nf_team *T = h[i]->team; const nf_keff_opts *o = opt_of(i);
        __atomic_store_n(&T->outers_done, 0L, __ATOMIC_RELEASE);
        Inner in; double k0 = 1.0;
        st[i] = keff_begin(T, o, &in, &k0);
        if (st[i] == NF_OK) { T->last_path = 2; T->profile = false; st[i] = resident_fill(T, o, k0, cheb, in.ip.cg_tol, in.ip.cg_max, &R[i]); }
        if (st[i] == NF_OK) { live.push_back(i); args.push_back(R[i].A); }
    }
    // ---- one launch: the structs into the grow-only array of the first team, every handle's stream drained, one workgroup per handle
    const int nl = (int)live.size();
    int launch_rc = NF_OK;
    auto launch = [&]() -> int {
        if (nl == 0) return NF_OK;
        if (T0->batch_cap < nl) { T0->batch_cap = 0; NFCHK(dalloc(&T0->d_batch_args, (size_t)nl)); T0->batch_cap = nl; }
        HIPCHK(hipMemcpyAsync(T0->d_batch_args, args.data(), (size_t)nl * sizeof(ResidentArgs), hipMemcpyHostToDevice, T0->stream));
        for (int i : live) if (h[i]->team != T0) HIPCHK(stream_wait(h[i]->team->stream));
        hipLaunchKernelGGL(K.batch, dim3(nl), dim3(NF_RESIDENT_BLOCK), R[0].lds, T0->stream, (ResidentArgsConst *)T0->d_batch_args, nl);
        HIPCHK(hipGetLastError());
        ++T0->batch_launches;
        HIPCHK(stream_wait(T0->stream));
        return NF_OK;
    };
    launch_rc = launch();
    // ---- per handle: what solve_keff_resident does after its launch, and the exit of a finished solve
    for (int i = 0; i < n; ++i) {
        nf_team *T = h[i]->team;
        double k = 0.0; int no = 0;
        if (st[i] == NF_OK && launch_rc != NF_OK) st[i] = launch_rc;
        if (st[i] == NF_OK) {
            T->last_resident_serial = R[i].serial ? 1 : 0;
            st[i] = resident_fetch(T, opt_of(i), T->stream, &k);
            if (st[i] == NF_OK) st[i] = keff_finish(T, k, false, &k, &no);
        }
        if (keff) keff[i] = k;
        if (n_outer) n_outer[i] = no;
        if (status) status[i] = st[i];
        if (first == NF_OK) first = st[i];
    }
    if (res) { res->n_batched = nl; res->n_launches = nl > 0 && launch_rc == NF_OK ? 1 : 0; res->variant = R[0].variant; }
    return first;
}

int nf_set_progress_callback(nf_handle S, nf_progress_fn fn, void *user)
{
    if (!S) return fail(NF_ERR_ARG, "null handle");
    S->team->progress_fn = fn; S->team->progress_user = user;
    return NF_OK;
}

// Outer iterations the running (or last) nf_solve_keff has completed on the host-driven path.  Safe to call from another thread
// while the solve runs: a watchdog (bench.py) uses it to tell a slow solve from one whose peers are gone.
int nf_progress(nf_handle S, long *outers_done)
{
    if (!S || !outers_done) return fail(NF_ERR_ARG, "nf_progress: bad arguments");
    *outers_done = __atomic_load_n(&S->team->outers_done, __ATOMIC_ACQUIRE);
    return NF_OK;
}

// ---- SolveSubcritical (declared include/NeutFEM.hpp:275-279, src/wrapper.cpp:699-715; never defined there) ----------------------
// -div(D grad phi) + Sigma_r phi = F phi + Q: per group S_g phi_g = chi_g tf(phi) + scatter_g(phi) + q_g, solved by source iteration
// (DESIGN.md 11).  SRC is piecewise constant per cell: q_g[e, dof 0] = Q_g(e) |e|, higher moments 0.
int nf_upload_source(nf_handle S, const double *src)
{
    if (!S || !src) return fail(NF_ERR_ARG, "nf_upload_source: bad arguments");
    HIPCHK(hipSetDevice(S->device));
    hipStream_t st = S->team->stream;
    const long N = S->N, NT = S->nphi * S->ng;
    double tot = 0.0; bool any = false;
    for (int g = 0; g < S->ng; ++g)
        for (long e = 0; e < N; ++e) {
            const double v = src[g * N + e];
            if (!std::isfinite(v)) return fail(NF_ERR_ARG, "nf_upload_source: non-finite source in group %d, cell %ld", g, e);
            const long r = e / S->nx;
            tot += v * (S->hx[e % S->nx] * S->hy[r % S->ny] * S->hz[r / S->ny]);
            any |= v != 0.0;
        }
    if (!S->d_qsrc) NFCHK(dalloc(&S->d_qsrc, (size_t)NT));
    DevTmp<double> d_src; NFCHK(dalloc(&d_src.p, (size_t)N * S->ng));
    HIPCHK(hipMemcpyAsync(d_src.p, src, (size_t)N * S->ng * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_source_q, dim3(grid_for(NT)), dim3(256), 0, st, (const double *)d_src.p, S->d_qsrc, S->d_hx, S->d_hy, S->d_hz,
                       S->nx, S->ny, N, S->nphi, NT);
    HIPCHK(hipStreamSynchronize(st));                             // d_src is freed on return
    HIPCHK(hipGetLastError());
    S->src_total = tot; S->src_any = any;
    return NF_OK;
}

// The sweep of the fixed-source drivers: raw from raw / phi with the external source d_qsrc.  transposed: the scatter blocks Ms[g' <- g] in
// place of Ms[g <- g'] (adjoint zoom), the sweep stays in forward order as nf_solve_adjoint has it.
static GroupSweep source_sweep(nf_team *T, bool transposed)
{
    GroupSweep sw = sweep_for(T);
    sw.transposed = transposed;
    for (size_t i = 0; i < T->slabs.size(); ++i) {
        nf_solver *S = T->slabs[i];
        sw.slab[i].emis = S->d_Chi; sw.slab[i].phi_new = S->d_raw; sw.slab[i].phi_old = S->d_phi; sw.slab[i].sol = S->d_raw; sw.slab[i].q = S->d_qsrc;
    }
    return sw;
}

// One outer of the fixed-source iteration on every slab of the team: tf from the previous outer's flux, Gauss-Seidel group sweep with the
// group solver of `ip` (or the diagonal S^-1), then one streaming pass (k_subcrit_reduce) for Phi, P, the norms and the copy raw -> phi;
// hout = { Phi, P, ||phi||^2, ||dphi||^2 }.  fscale scales the fission term (0: off, 1: on, no eigenvalue).  sw: source_sweep of the team.
static int source_outer(nf_team *T, const InnerPlan &ip, int use_diag, GroupSweep &sw, double fscale, int *cg_total, double *hout)
{
    const int ns = (int)T->slabs.size();
    const int ng = T->slabs[0]->ng;
    std::vector<int> gT(ns);
    for (int i = 0; i < ns; ++i) gT[i] = grid_for(T->slabs[i]->nphi * ng);
    for (int i = 0; i < ns; ++i) {                                // tf = sum_g Mf_g phi_g of the previous outer (finite, also when scaled by 0)
        nf_solver *S = T->slabs[i];
        hipLaunchKernelGGL(k_fission, dim3(sw.grid[i]), dim3(256), 0, T->stream, S->d_Mf, S->d_phi, ng, S->nphi, S->d_tf, T->d_partials + i * T->slab_cap, (const double *)nullptr, 0L);
    }
    sw.fscale = fscale;
    NFCHK(group_sweep(T, ip, use_diag, sw, sweep_no_hook, [&](int, int its) { *cg_total += its; }));
    for (int i = 0; i < ns; ++i) {
        nf_solver *S = T->slabs[i];
        hipLaunchKernelGGL(k_subcrit_reduce, dim3(gT[i]), dim3(256), 0, T->stream, S->d_Mf, (const double *)S->d_raw, S->d_phi, S->d_hx, S->d_hy, S->d_hz,
                           S->nx, S->ny, S->N, S->nphi, S->nphi * ng, T->d_partials + i * T->slab_cap, T->partial_stride);
    }
    NFCHK(team_finalize(T, FIN_SUM, gT, 4, T->d_out, 0.0, 0));
    return readback(T, nullptr, nullptr, T->d_out, hout, 4);
}

// The fixed-source iteration with the fission term off, from phi = 0 (so the result does not depend on the flux the handles held before):
// per group S_g phi_g = q_g + scatter_g(phi) with q = d_qsrc.  Stops when |Phi_n - Phi_{n-1}| / Phi_n < tol_keff and
// ||phi_n - phi_{n-1}|| / ||phi_n|| < tol_flux (*conv = true) or after max_outer outers.  Shared by nf_solve_subcritical (its phase 0)
// and nf_zoom_resolved (the whole solve; adjoint: a transposed source_sweep).  *n outers are added to *outers and published through nf_progress.
static int nofission_phase(nf_team *T, const nf_keff_opts *o, const InnerPlan &ip, int use_diag, GroupSweep &sw, const char *who,
                           double *phi_int, double *production, int *n, int *cg_total, bool *conv, long *outers)
{
    for (auto *S : T->slabs) HIPCHK(hipMemsetAsync(S->d_phi, 0, (size_t)S->nphi * S->ng * sizeof(double), T->stream));
    double q_old = 0.0, hout[4] = { 0, 0, 0, 0 };
    *conv = false; *n = 0;
    for (int it = 0; it < o->max_outer; ++it) {
        NFCHK(source_outer(T, ip, use_diag, sw, 0.0, cg_total, hout));
        const double Phi = hout[0], P = hout[1], nsq = hout[2], dsq = hout[3];
        const double dq = Phi - q_old, dphi = std::sqrt(dsq / nsq);
        const double rel = dq == 0.0 ? 0.0 : std::fabs(dq) / std::fabs(Phi);
        *n = it + 1; ++*outers;
        __atomic_store_n(&T->outers_done, *outers, __ATOMIC_RELEASE);
        if (!std::isfinite(Phi) || !std::isfinite(P) || !std::isfinite(dphi))
            return fail(NF_ERR_NUMERIC, "%s: the source iteration without fission produced non-finite sums (outer %d: Phi=%g P=%g)", who, it, Phi, P);
        *phi_int = Phi; *production = P;
        q_old = Phi;
        if (rel < o->tol_keff && dphi < o->tol_flux) { *conv = true; break; }
    }
    return NF_OK;
}

// Two phases of the host-driven loop of solve_keff_impl: phase 0 with the fission term off (the flux without fission, phi0:
// nofission_phase), phase 1 from phi0 with fission at scale 1 (no eigenvalue).  Each outer is one source_outer with the same group
// solver SolveKeff picks (inner_plan / diagonal S^-1).  No normalisation, no acceleration.
static int solve_subcritical_impl(nf_team *T, const nf_keff_opts *o, nf_subcrit_result *res)
{
    if (T->nproc > 1) return fail(NF_ERR_UNSUPPORTED, "nf_solve_subcritical: multi-rank teams are not supported (one process, undivided mesh or linked slabs)");
    if (o->use_coarse_init || o->use_cmfd) return fail(NF_ERR_ARG, "nf_solve_subcritical: coarse start and CMFD do not apply to the fixed-source iteration");
    if (o->max_outer < 1) return fail(NF_ERR_ARG, "nf_solve_subcritical: max_outer must be at least 1");
    const int ns = (int)T->slabs.size();
    nf_solver *S0 = T->slabs[0];
    const int ng = S0->ng;
    double src_total = 0.0; bool src_any = false;
    for (auto *S : T->slabs) {
        if (!S->d_qsrc) return fail(NF_ERR_STATE, "nf_solve_subcritical: call nf_upload_source first (every slab)");
        src_total += S->src_total; src_any |= S->src_any;
    }
    if (!src_any) return fail(NF_ERR_ARG, "nf_solve_subcritical: the external source is zero on every cell");
    Inner in;
    NFCHK(inner_begin(T, o, DIAG_OK, &in));
    const InnerPlan &ip = in.ip; const int use_diag = in.use_diag;
    GroupSweep sw = source_sweep(T, false);
    T->last_path = 0; T->profile = false;
    std::vector<int> gT(ns);
    for (int i = 0; i < ns; ++i) gT[i] = grid_for(T->slabs[i]->nphi * ng);
    nf_subcrit_result r; memset(&r, 0, sizeof r);
    r.source = src_total; r.ratio = 0.0;
    double hout[4] = { 0, 0, 0, 0 };
    long outers = 0;
    bool conv[2] = { false, false };
    int rc = nofission_phase(T, o, ip, use_diag, sw, "nf_solve_subcritical", &r.phi_int, &r.production, &r.n_outer_nofission, &r.cg_total, &conv[0], &outers);
    r.phi_int_nofission = r.phi_int;
    if (rc == NF_OK) {
        double q_old = r.production, dq_old = 0.0;                // P of phi0 and its change at the previous outer
        int streak = 0, n = 0;
        for (int it = 0; it < o->max_outer; ++it) {
            if ((rc = source_outer(T, ip, use_diag, sw, 1.0, &r.cg_total, hout)) != NF_OK) break;
            const double Phi = hout[0], P = hout[1], nsq = hout[2], dsq = hout[3];
            const double dq = P - q_old, dphi = std::sqrt(dsq / nsq);
            const double rel = dq == 0.0 ? 0.0 : std::fabs(dq) / std::fabs(P);
            n = it + 1; ++outers;
            __atomic_store_n(&T->outers_done, outers, __ATOMIC_RELEASE);
            if (!std::isfinite(Phi) || !std::isfinite(P) || !std::isfinite(dphi)) {
                rc = fail(NF_ERR_NUMERIC, "nf_solve_subcritical: the system is not subcritical: the source iteration diverged (outer %d: Phi=%g P=%g; contraction estimate %g)",
                          it, Phi, P, r.ratio);
                break;
            }
            // contraction of the iteration dP_n / dP_{n-1}; below 1e-6 P the differences are inner-solve noise
            const bool meaningful = dq != 0.0 && std::fabs(dq) >= 1e-6 * std::fabs(P) && dq_old != 0.0;
            if (meaningful) r.ratio = dq / dq_old;
            streak = (it >= 4 && meaningful && dq / dq_old >= 1.0) ? streak + 1 : 0;
            if (streak >= 5) {
                rc = fail(NF_ERR_NUMERIC, "nf_solve_subcritical: the system is not subcritical: the source iteration does not contract "
                          "(estimate %.6f >= 1 over 5 consecutive outers, outer %d; k-eff of the core is about that value or above)", r.ratio, it);
                break;
            }
            r.phi_int = Phi; r.production = P;
            dq_old = dq; q_old = P;
            if (rel < o->tol_keff && dphi < o->tol_flux) { conv[1] = true; break; }
        }
        r.n_outer = n;
    }
    HIPCHK(hipStreamSynchronize(T->stream));
    HIPCHK(hipGetLastError());
    if (rc != NF_OK) {                                            // the handle stays usable: current flux back to ResetFlux's 1, warm state untouched
        for (int i = 0; i < ns; ++i) {
            nf_solver *S = T->slabs[i];
            hipLaunchKernelGGL(k_fill_const, dim3(gT[i]), dim3(256), 0, T->stream, S->d_phi, S->nphi * ng, 1.0);
            S->raw_valid = false; S->jz_valid = false;
        }
        (void)hipStreamSynchronize(T->stream);
        return rc;
    }
    for (auto *S : T->slabs) { S->raw_valid = true; S->raw_is_diag = use_diag != 0; S->jz_valid = false; }
    r.M = r.phi_int / r.phi_int_nofission;
    r.k_source = r.production / (r.production + r.source);
    r.converged = conv[0] && conv[1] ? 1 : 0;
    if (res) *res = r;
    return NF_OK;
}

int nf_solve_subcritical(nf_handle S, const nf_keff_opts *o, nf_subcrit_result *res)
{
    if (!S || !o) return fail(NF_ERR_ARG, "nf_solve_subcritical: bad arguments");
    NFCHK(void_refuse(S, "nf_solve_subcritical"));
    if (S->team->dead) return fail(NF_ERR_COMM, "this team lost a collective (NF_ERR_COMM) and is unusable: destroy the handles and end the process with a non-zero code (never re-exec)");
    for (auto *X : S->team->slabs) if (!X->built) return fail(NF_ERR_STATE, "nf_solve_subcritical: call nf_build first");
    HIPCHK(hipSetDevice(S->device));
    __atomic_store_n(&S->team->outers_done, 0L, __ATOMIC_RELEASE);
    return solve_subcritical_impl(S->team, o, res);
}

// ---- space-time kinetics (no counterpart in the reference) -------------------------------------------------------------
// Implicit Euler on the system of nf_solve_subcritical: a step is a fixed-source solve with fission on the operator whose removal cross
// section is shifted by 1 / (v dt) -- a built twin of the handle, made the way refine_impl makes one.  Host-driven like
// solve_subcritical_impl, with one scalar rebalance per outer (without it the iteration contracts like 1 - beta).
struct Transient {
    int nfam = 0; double beta[NF_PRECURSORS_MAX], lambda[NF_PRECURSORS_MAX];
    std::vector<double> v, chid; bool has_chid = false;          // ng velocities; ng values of the delayed spectrum (else the handle's Chi)
    double k0 = 1.0, P0 = 0.0;
    double time = 0.0, production = 0.0, phi_int = 0.0, precursors = 0.0, rebalance = 1.0; long n_steps = 0;   // after the last completed step
    nf_solver *twin = nullptr; double twin_dt = 0.0; long twin_gen = -1;   // the step operator and what it was built for
    double *d_phi = nullptr;        // the transient's own flux, ng * nphi: other solves on the handle change the handle's, not this one
    double *d_c = nullptr;          // precursors, nfam * nphi (tf-space, device DOF order)
    double *d_q = nullptr, *d_W = nullptr;                        // the step's source, ng * nphi; mass weights, nphi
    double *d_part = nullptr, *d_sums = nullptr;                  // TR_ROWS rows of RED_GRID block partials; their sums (layout below)
};
static const int TR_ROWS = 8, TR_ROW_U = 4, TR_ROW_E = 5, TR_ROW_Q = 6;   // rows 0..3: the balance pass (the precursor pass: 0, 1)
enum { TR_U = 0, TR_E = 1, TR_Q = 2, TR_F = 3, TR_PHI = 4, TR_P = 5, TR_NSQ = 6, TR_DSQ = 7, TR_C = 8, TR_P0 = 9, TR_NSUMS = 10 };   // d_sums: 0..7 are read back every outer

static void transient_drop(nf_solver *S)
{
    Transient *R = S->tr;
    if (!R) return;
    std::string keep = g_err;
    if (R->twin) nf_destroy(R->twin);
    (void)hipSetDevice(S->device);
    if (S->team && S->team->stream) (void)hipStreamSynchronize(S->team->stream);
    dfree(R->d_phi); dfree(R->d_c); dfree(R->d_q); dfree(R->d_W); dfree(R->d_part); dfree(R->d_sums);
    delete R; S->tr = nullptr;
    g_err = keep;
}
static long transient_steps(const nf_solver *S) { return S->tr ? S->tr->n_steps : 0; }

// sums of nq rows of block partials (cnt per row, stride RED_GRID) into out, on the team's stream: k_finalize as team_finalize launches it
static void tr_finalize(nf_team *T, const double *part, int cnt, int nq, double *out)
{
    PartSegs ps; memset(&ps, 0, sizeof ps); ps.n = 1; ps.cnt[0] = cnt;
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, T->stream, (int)FIN_SUM, part, ps, (long)RED_GRID, nq, T->d_cg, out, 0.0, 0, 0, T->d_red, (const double *)nullptr);
}
static TrGroups tr_chid(const Transient *R) { TrGroups c; memset(&c, 0, sizeof c); for (size_t g = 0; g < R->chid.size(); ++g) c.v[g] = R->chid[g]; return c; }

int nf_transient_end(nf_handle S)
{
    if (!S) return fail(NF_ERR_ARG, "null handle");
    transient_drop(S);
    return NF_OK;
}

// the kinetics data of nf_transient_begin, nf_kinetics_params: one set of rules, `who` names the caller in the text
static int kinetics_check(const nf_solver *S, const nf_kinetics *kin, double keff, const char *who)
{
    const int ng = S->ng, I = kin->n_families;
    if (!(keff > 0.0) || !std::isfinite(keff)) return fail(NF_ERR_ARG, "%s: keff must be finite and > 0 (got %g)", who, keff);
    if (I < 0 || I > NF_PRECURSORS_MAX) return fail(NF_ERR_ARG, "%s: n_families must be 0 .. %d (got %d)", who, NF_PRECURSORS_MAX, I);
    if (!kin->velocity_host) return fail(NF_ERR_ARG, "%s: velocity_host is NULL", who);
    for (int g = 0; g < ng; ++g) {
        if (!(kin->velocity_host[g] > 0.0) || !std::isfinite(kin->velocity_host[g])) return fail(NF_ERR_ARG, "%s: velocity of group %d must be finite and > 0 (got %g)", who, g, kin->velocity_host[g]);
        if (kin->chi_delayed_host && !std::isfinite(kin->chi_delayed_host[g])) return fail(NF_ERR_ARG, "%s: non-finite delayed spectrum in group %d", who, g);
    }
    double bsum = 0.0;
    for (int i = 0; i < I; ++i) {
        if (!(kin->beta[i] >= 0.0) || !std::isfinite(kin->beta[i])) return fail(NF_ERR_ARG, "%s: beta of family %d must be finite and >= 0 (got %g)", who, i, kin->beta[i]);
        if (!(kin->lambda[i] > 0.0) || !std::isfinite(kin->lambda[i])) return fail(NF_ERR_ARG, "%s: lambda of family %d must be finite and > 0 (got %g)", who, i, kin->lambda[i]);
        bsum += kin->beta[i];
    }
    if (!(bsum < 1.0)) return fail(NF_ERR_ARG, "%s: the delayed fractions sum to %g (must be < 1)", who, bsum);
    return NF_OK;
}

int nf_transient_begin(nf_handle S, const nf_kinetics *kin, double keff)
{
    if (!S || !kin) return fail(NF_ERR_ARG, "nf_transient_begin: bad arguments");
    NFCHK(void_refuse(S, "nf_transient_begin"));
    nf_team *T = S->team;
    if (T->nproc > 1 || !team_is_single(T)) return fail(NF_ERR_UNSUPPORTED, "nf_transient_begin works on an undivided mesh of one process (not on slab or multi-rank teams)");
    if (!S->built) return fail(NF_ERR_STATE, "nf_transient_begin: call nf_build first");
    const int ng = S->ng, I = kin->n_families;
    NFCHK(kinetics_check(S, kin, keff, "nf_transient_begin"));
    HIPCHK(hipSetDevice(S->device));
    transient_drop(S);
    Transient *R = new Transient();
    S->tr = R; S->tr_rebuilds = 0;
    R->nfam = I; R->k0 = keff;
    for (int i = 0; i < I; ++i) { R->beta[i] = kin->beta[i]; R->lambda[i] = kin->lambda[i]; }
    R->v.assign(kin->velocity_host, kin->velocity_host + ng);
    R->has_chid = kin->chi_delayed_host != nullptr;
    if (R->has_chid) R->chid.assign(kin->chi_delayed_host, kin->chi_delayed_host + ng);
    const long N = S->N, NP = S->nphi; const size_t NN = (size_t)NP * ng;
    hipStream_t st = T->stream;
    auto body = [&]() -> int {
        NFCHK(dalloc(&R->d_phi, NN)); NFCHK(dalloc(&R->d_c, (size_t)NP * I)); NFCHK(dalloc(&R->d_q, NN)); NFCHK(dalloc(&R->d_W, (size_t)NP));
        NFCHK(dalloc(&R->d_part, (size_t)TR_ROWS * RED_GRID)); NFCHK(dalloc(&R->d_sums, (size_t)TR_NSUMS));
        HIPCHK(hipMemsetAsync(R->d_sums, 0, TR_NSUMS * sizeof(double), st));
        HIPCHK(hipMemcpyAsync(R->d_phi, S->d_phi, NN * sizeof(double), hipMemcpyDeviceToDevice, st));
        ChatArgs ch; ch.nloc = S->nloc;                           // C-hat_pp as nf_build forms it
        for (int p = 0; p < S->nloc; ++p) {
            int q = p; double c = 1.0;
            for (int t = 0; t < S->dim; ++t) { c *= 2.0 / (2.0 * (q % S->n1) + 1.0); q /= S->n1; }
            ch.c[p] = c;
        }
        hipLaunchKernelGGL(k_tr_weights, dim3(grid_for(N)), dim3(256), 0, st, R->d_W, S->d_hx, S->d_hy, S->d_hz, S->nx, S->ny, N, S->dim, ch);
        TrFamilies fam; memset(&fam, 0, sizeof fam); fam.n = I;   // equilibrium: c_i = beta_i tf / (lambda_i k0)
        for (int i = 0; i < I; ++i) fam.b[i] = R->beta[i] / (R->lambda[i] * keff);
        const int gP = grid_for(NP);
        hipLaunchKernelGGL(k_tr_precursors, dim3(gP), dim3(256), 0, st, S->d_Mf, (const double *)R->d_phi, R->d_c, N, NP, ng, fam, 1, R->d_part, (long)RED_GRID);
        tr_finalize(T, R->d_part, gP, 2, R->d_sums + TR_C);
        double h[2] = { 0, 0 };
        NFCHK(readback(T, nullptr, nullptr, R->d_sums + TR_C, h, 2));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        if (!(h[1] > 0.0) || !std::isfinite(h[1]) || !std::isfinite(h[0]))
            return fail(NF_ERR_ARG, "nf_transient_begin: the production of the current flux, P(0) = %g, must be finite and > 0 (precursor population %g)", h[1], h[0]);
        R->precursors = h[0]; R->P0 = R->production = h[1];
        return NF_OK;
    };
    const int rc = body();
    if (rc != NF_OK) transient_drop(S);
    return rc;
}

// the step operator for dt: a built twin with SigR_g + 1 / (v_g dt) and chi~ in the place of Chi, kept until dt or the handle's build changes
static int transient_twin(nf_solver *S, double dt)
{
    Transient *R = S->tr;
    if (R->twin && R->twin_dt == dt && R->twin_gen == S->build_gen) return NF_OK;
    if (R->twin) { nf_destroy(R->twin); R->twin = nullptr; }
    const int ng = S->ng; const long N = S->N; const size_t NN = (size_t)N * ng;
    nf_handle F = nullptr;
    NFCHK(create_impl(S->k, S->m, ng, (int)S->xb.size(), S->xb.data(), (int)S->yb.size(), S->yb.data(), (int)S->zb.size(), S->zb.data(), 0, 0, S->device, &F));
    auto body = [&]() -> int {
        if (F->dim != S->dim || F->N != N || F->nphi != S->nphi) return fail(NF_ERR_ARG, "nf_transient_step: the step operator's mesh differs from the handle's");
        for (int a = 0; a < 8; ++a) if (S->bc_set[a]) nf_set_bc(F, a, S->bc_type[a]);
        team_copy_options(F->team, S->team, true);
        hipStream_t st = S->team->stream;
        NFCHK(dalloc(&F->d_D, NN)); NFCHK(dalloc(&F->d_SigR, NN)); NFCHK(dalloc(&F->d_NSF, NN)); NFCHK(dalloc(&F->d_Chi, NN));
        HIPCHK(hipMemcpyAsync(F->d_D, S->d_D, NN * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(F->d_NSF, S->d_NSF, NN * sizeof(double), hipMemcpyDeviceToDevice, st));
        TrGroups shift; memset(&shift, 0, sizeof shift);
        double a = 0.0;
        for (int g = 0; g < ng; ++g) shift.v[g] = 1.0 / (R->v[g] * dt);
        for (int i = 0; i < R->nfam; ++i) a += R->beta[i] / (1.0 + R->lambda[i] * dt);
        const int gN = grid_for((long)NN);
        hipLaunchKernelGGL(k_tr_shift, dim3(gN), dim3(256), 0, st, (const double *)S->d_SigR, F->d_SigR, N, (long)NN, shift);
        hipLaunchKernelGGL(k_tr_chi, dim3(gN), dim3(256), 0, st, (const double *)S->d_Chi, F->d_Chi, N, (long)NN, tr_chid(R), R->has_chid ? 0 : 1, a);
        for (int b = 0; b < ng * ng; ++b)
            if (S->d_SigS[b]) {
                NFCHK(dalloc(&F->d_SigS[b], (size_t)N));
                HIPCHK(hipMemcpyAsync(F->d_SigS[b], S->d_SigS[b], (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
            }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));                         // the copies ran on the handle's stream; nf_build uses the twin's
        F->xs_uploaded = true;
        return nf_build(F);
    };
    const int rc = body();
    if (rc != NF_OK) { std::string keep = g_err; nf_destroy(F); g_err = keep; (void)hipGetLastError(); return rc; }
    R->twin = F; R->twin_dt = dt; R->twin_gen = S->build_gen; ++S->tr_rebuilds;
    return NF_OK;
}

// one step on the twin F: the rebalanced source iteration from the transient's flux.  hout = the sums of the last outer (d_sums 0..7)
static int transient_iterate(nf_solver *S, nf_solver *F, const nf_keff_opts *o, const InnerPlan &ip, double dt, nf_transient_result *r,
                             long *outers, bool *conv, double *hout)
{
    Transient *R = S->tr; nf_team *TT = F->team; hipStream_t st = TT->stream;
    const int ng = S->ng; const long N = S->N, NP = S->nphi, NT = NP * ng;
    const int gP = grid_for(NP), gC = grid_for(N), gT = grid_for(NT);
    double *part = R->d_part, *sums = R->d_sums;
    HIPCHK(hipMemcpyAsync(F->d_phi, R->d_phi, (size_t)NT * sizeof(double), hipMemcpyDeviceToDevice, st));
    TrGroups ivdt; memset(&ivdt, 0, sizeof ivdt);
    for (int g = 0; g < ng; ++g) ivdt.v[g] = 1.0 / (R->v[g] * dt);
    TrFamilies fam; memset(&fam, 0, sizeof fam); fam.n = R->nfam;
    for (int i = 0; i < R->nfam; ++i) fam.a[i] = R->lambda[i] / (1.0 + R->lambda[i] * dt);
    hipLaunchKernelGGL(k_tr_source, dim3(gP), dim3(256), 0, st, (const double *)R->d_phi, (const double *)R->d_c, (const double *)R->d_W,
                       (const double *)S->d_Chi, R->d_q, N, NP, ng, ivdt, tr_chid(R), R->has_chid ? 0 : 1, fam, part + TR_ROW_Q * RED_GRID);
    tr_finalize(TT, part + TR_ROW_Q * RED_GRID, gP, 1, sums + TR_Q);
    const double inv_k = 1.0 / R->k0;
    // the sweep runs on the twin (emission chi~, source q of this step) and counts its stand-in solves on the caller's team
    GroupSweep sw = sweep_for(TT);
    sw.fscale = inv_k; sw.count_team = S->team;
    sw.slab[0].emis = F->d_Chi; sw.slab[0].phi_new = F->d_raw; sw.slab[0].phi_old = F->d_phi; sw.slab[0].sol = F->d_raw; sw.slab[0].q = R->d_q;
    double P_old = R->production;
    int n = 0;
    *conv = false;
    for (int it = 0; it < o->max_outer; ++it) {
        hipLaunchKernelGGL(k_fission, dim3(gP), dim3(256), 0, st, F->d_Mf, F->d_phi, ng, NP, F->d_tf, TT->d_partials, (const double *)nullptr, 0L);
        NFCHK(group_sweep(TT, ip, 0, sw,
                          [&](int g) { hipLaunchKernelGGL(k_tr_rhs_sum, dim3(gC), dim3(256), 0, st, (const double *)F->d_rhs, N, part + TR_ROW_U * RED_GRID, g == 0 ? 1 : 0); },
                          [&](int, int its) { r->cg_total += its; }));
        tr_finalize(TT, part + TR_ROW_U * RED_GRID, gC, 1, sums + TR_U);
        hipLaunchKernelGGL(k_tr_emission, dim3(gC), dim3(256), 0, st, F->d_Mf, (const double *)F->d_raw, (const double *)F->d_Chi,
                           (const double *const *)F->d_Ms_tab, inv_k, N, NP, ng, part + TR_ROW_E * RED_GRID);
        tr_finalize(TT, part + TR_ROW_E * RED_GRID, gC, 1, sums + TR_E);
        hipLaunchKernelGGL(k_tr_balance, dim3(gT), dim3(256), 0, st, F->d_Mf, (const double *)F->d_raw, F->d_phi, F->d_hx, F->d_hy, F->d_hz,
                           F->nx, F->ny, N, NP, NT, sums, S->opt_tr_rebalance, part, (long)RED_GRID);
        tr_finalize(TT, part, gT, 4, sums + TR_PHI);
        NFCHK(readback(TT, nullptr, nullptr, sums, hout, 8));
        n = it + 1; ++r->n_outer; ++*outers;
        __atomic_store_n(&S->team->outers_done, *outers, __ATOMIC_RELEASE);
        const double Phi = hout[TR_PHI], P = hout[TR_P], dphi = std::sqrt(hout[TR_DSQ] / hout[TR_NSQ]);
        if (!std::isfinite(hout[TR_U]) || !std::isfinite(hout[TR_E]) || !std::isfinite(hout[TR_Q]) || !std::isfinite(Phi) || !std::isfinite(P) || !std::isfinite(dphi))
            return fail(NF_ERR_NUMERIC, "nf_transient_step: the step's source iteration produced non-finite sums (step %ld, outer %d: U=%g E=%g Q=%g Phi=%g P=%g)",
                        R->n_steps + 1, it, hout[TR_U], hout[TR_E], hout[TR_Q], Phi, P);
        const double dq = P - P_old;
        const double rel = dq == 0.0 ? 0.0 : std::fabs(dq) / std::fabs(P);
        P_old = P;
        if (rel < o->tol_keff && dphi < o->tol_flux) { *conv = true; break; }
    }
    r->n_outer_max = std::max(r->n_outer_max, n);
    return NF_OK;
}

int nf_transient_step(nf_handle S, const nf_keff_opts *o, double dt, int n_steps, double *power_host, nf_transient_result *res)
{
    if (!S || !o) return fail(NF_ERR_ARG, "nf_transient_step: bad arguments");
    NFCHK(void_refuse(S, "nf_transient_step"));
    nf_team *T = S->team;
    if (T->nproc > 1 || !team_is_single(T)) return fail(NF_ERR_UNSUPPORTED, "nf_transient_step works on an undivided mesh of one process (not on slab or multi-rank teams)");
    if (o->use_coarse_init || o->use_cmfd || o->use_diagonal_solver) return fail(NF_ERR_ARG, "nf_transient_step: coarse start, CMFD and the diagonal solver do not apply to a time step");
    if (!(dt > 0.0) || !std::isfinite(dt)) return fail(NF_ERR_ARG, "nf_transient_step: dt must be finite and > 0 (got %g)", dt);
    if (n_steps < 1) return fail(NF_ERR_ARG, "nf_transient_step: n_steps must be at least 1 (got %d)", n_steps);
    if (o->max_outer < 1) return fail(NF_ERR_ARG, "nf_transient_step: max_outer must be at least 1");
    Transient *R = S->tr;
    if (!R) return fail(NF_ERR_STATE, "nf_transient_step: call nf_transient_begin first");
    if (!S->built) return fail(NF_ERR_STATE, "nf_transient_step: call nf_build first (the cross sections were uploaded again)");
    HIPCHK(hipSetDevice(S->device));
    HIPCHK(hipStreamSynchronize(T->stream));                      // the twin's stream reads what the handle's wrote
    __atomic_store_n(&T->outers_done, 0L, __ATOMIC_RELEASE);
    nf_transient_result r; memset(&r, 0, sizeof r);
    auto report = [&] {
        r.time = R->time; r.production = R->production; r.power = R->production / R->P0; r.phi_int = R->phi_int; r.precursors = R->precursors;
        r.rebalance = R->rebalance; r.n_steps = R->n_steps;
        if (res) *res = r;
    };
    const int ng = S->ng; const long N = S->N, NP = S->nphi; const size_t B = (size_t)NP * ng * sizeof(double);
    long outers = 0;
    auto body = [&]() -> int {
        NFCHK(transient_twin(S, dt));
        nf_solver *F = R->twin; nf_team *TT = F->team; hipStream_t st = TT->stream;
        team_copy_options(TT, T, true);                           // the twin is kept across steps: an option set since the last one holds for this one
        const long xcd0 = TT->xcd_solves, refused0 = TT->xcd_refused;
        Inner in;
        NFCHK(inner_begin(TT, o, DIAG_NEVER, &in));
        const InnerPlan &ip = in.ip;
        T->last_direct = TT->last_direct;
        TT->last_path = 0; TT->profile = false;
        TrFamilies fam; memset(&fam, 0, sizeof fam); fam.n = R->nfam;   // c_i <- (c_i + dt beta_i tf / k0) / (1 + lambda_i dt)
        for (int i = 0; i < R->nfam; ++i) { fam.a[i] = 1.0 / (1.0 + R->lambda[i] * dt); fam.b[i] = dt * R->beta[i] / (R->k0 * (1.0 + R->lambda[i] * dt)); }
        const int gP = grid_for(NP);
        int rc = NF_OK;
        for (int s = 0; s < n_steps && rc == NF_OK; ++s) {
            double hout[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }; bool conv = false;
            if ((rc = transient_iterate(S, F, o, ip, dt, &r, &outers, &conv, hout)) != NF_OK) break;
            // completion: precursors from tf(phi^{n+1}), the new flux becomes the transient's and the handle's, time advances
            hipLaunchKernelGGL(k_tr_precursors, dim3(gP), dim3(256), 0, st, F->d_Mf, (const double *)F->d_phi, R->d_c, N, NP, ng, fam, 0, R->d_part, (long)RED_GRID);
            tr_finalize(TT, R->d_part, gP, 2, R->d_sums + TR_C);
            double hc[2] = { 0, 0 };
            if ((rc = readback(TT, nullptr, nullptr, R->d_sums + TR_C, hc, 2)) != NF_OK) break;
            for (double *dst : { R->d_phi, S->d_phi, S->d_raw })
                if (hipMemcpyAsync(dst, F->d_phi, B, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = fail(NF_ERR_HIP, "nf_transient_step: copy of the new flux failed");
            if (rc == NF_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(NF_ERR_HIP, "nf_transient_step: %s", hipGetErrorString(hipGetLastError()));
            if (rc != NF_OK) break;
            S->raw_valid = true; S->raw_is_diag = false; S->jz_valid = false;
            R->time += dt; ++R->n_steps;
            R->phi_int = hout[TR_PHI]; R->production = hout[TR_P]; R->rebalance = hout[TR_F]; R->precursors = hc[0];
            if (!conv) ++r.n_unconverged;
            if (power_host) power_host[s] = R->production / R->P0;
        }
        // nf_info on the handle reports the step's solves; a one-XCD start the device refused switches the path off for the handle as well
        T->xcd_solves += TT->xcd_solves - xcd0; T->xcd_refused += TT->xcd_refused - refused0;
        if (TT->xcd_refused != refused0) { T->opt.cg_xcd = TT->opt.cg_xcd; T->opt.keff_xcd = TT->opt.keff_xcd; }
        if (!ip.dense && r.n_outer > 0) { T->last_cg_form = TT->last_cg_form; T->last_cg_reductions = TT->last_cg_reductions; T->last_xcd = TT->last_xcd; }
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        return rc;
    };
    const int rc = body();
    if (rc != NF_OK && R->twin) {                                 // the twin may hold a half-done solve: the next step builds a fresh one
        std::string keep = g_err; nf_destroy(R->twin); R->twin = nullptr; g_err = keep; (void)hipGetLastError();
    }
    report();
    return rc;
}

int nf_get_precursors(nf_handle S, int family, double *c_host)
{
    if (!S || !c_host) return fail(NF_ERR_ARG, "nf_get_precursors: bad arguments");
    Transient *R = S->tr;
    if (!R) return fail(NF_ERR_STATE, "nf_get_precursors: call nf_transient_begin first");
    if (family < 0 || family >= R->nfam) return fail(NF_ERR_ARG, "nf_get_precursors: family %d out of range (%d families)", family, R->nfam);
    HIPCHK(hipSetDevice(S->device));
    hipStream_t st = S->team->stream;
    const double *src = R->d_c + (size_t)family * S->nphi;
    DevTmp<double> tmp;
    if (S->nloc > 1) {
        NFCHK(dalloc(&tmp.p, (size_t)S->nphi));
        hipLaunchKernelGGL(k_transpose_dofs, dim3(grid_for(S->nphi)), dim3(256), 0, st, src, tmp.p, S->N, S->nloc, 0);
        src = tmp.p;
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(c_host, src, (size_t)S->nphi * sizeof(double), hipMemcpyDeviceToHost));
    return NF_OK;
}

// ---- adjoint-weighted kinetics parameters and dynamic reactivity (no counterpart in the reference) ----------------------
// The bilinear forms of the point-kinetics balance on (w = the handle's adjoint flux, phi, c): y_g = S_g phi_g by the launch functions of
// the plain nf_schur_apply on the BUILT operator of the handle (never the dt-shifted twin), then one k_kin_forms pass and k_finalize.
struct KinData {                                                  // what both fronts hand to pk_body
    int nfam; const double *beta, *lambda, *v, *chid;             // chid: ng values of the delayed spectrum, nullptr = the handle's Chi per cell
    const double *d_c, *d_W;                                      // the precursors (nullptr: no transient, c_amp = 0) and the transient's mass weights (nullptr: built here)
    double time; int from_transient;
};
static const int KIN_ROWS = 5 + NF_PRECURSORS_MAX;
// the state both fronts need, judged before any launch
static int pk_args(nf_handle S, nf_pk_result *res, const char *who)
{
    if (!S || !res) return fail(NF_ERR_ARG, "%s: bad arguments", who);
    NFCHK(void_refuse(S, who));
    nf_team *T = S->team;
    if (T->nproc > 1 || !team_is_single(T)) return fail(NF_ERR_UNSUPPORTED, "%s works on an undivided mesh of one process (not on slab or multi-rank teams)", who);
    if (S->N > 0xFFFFFFFFL) return fail(NF_ERR_UNSUPPORTED, "%s: %ld cells (meshes of 2^32 cells or more are not supported)", who, S->N);
    if (!S->built) return fail(NF_ERR_STATE, "%s: call nf_build first", who);
    if (!S->d_phi_adj) return fail(NF_ERR_STATE, "%s: no adjoint flux (nf_solve_adjoint or nf_set_phi_adj first)", who);
    return NF_OK;
}
static int pk_body(nf_solver *S, const char *who, const double *phi, const KinData &K, double k0, nf_pk_result *res)
{
    nf_team *T = S->team; hipStream_t st = T->stream;
    const int ng = S->ng, I = K.nfam; const long N = S->N, NP = S->nphi;
    memset(res, 0, sizeof *res);
    res->keff = k0; res->time = K.time; res->n_families = I; res->from_transient = K.from_transient;
    HIPCHK(hipSetDevice(S->device));
    (void)hipGetLastError();
    DevTmp<double> y, part, W;
    NFCHK(dalloc(&y.p, (size_t)NP * ng)); NFCHK(dalloc(&part.p, (size_t)KIN_ROWS * RED_GRID + KIN_ROWS));
    double *sums = part.p + (size_t)KIN_ROWS * RED_GRID;
    const double *dW = K.d_W;
    if (!dW) {
        NFCHK(dalloc(&W.p, (size_t)NP));
        ChatArgs ch; ch.nloc = S->nloc;                           // C-hat_pp as nf_build forms it
        for (int p = 0; p < S->nloc; ++p) {
            int q = p; double c = 1.0;
            for (int t = 0; t < S->dim; ++t) { c *= 2.0 / (2.0 * (q % S->n1) + 1.0); q /= S->n1; }
            ch.c[p] = c;
        }
        hipLaunchKernelGGL(k_tr_weights, dim3(grid_for(N)), dim3(256), 0, st, W.p, S->d_hx, S->d_hy, S->d_hz, S->nx, S->ny, N, S->dim, ch);
        dW = W.p;
    }
    NFCHK(line_dict_prepare(T));                                  // as nf_schur_apply
    const bool prof = T->profile; T->profile = false;             // no event brackets: the timers stay as they are
    int rc = NF_OK;
    for (int g = 0; g < ng && rc == NF_OK; ++g) rc = team_schur_apply(T, g, { phi + (size_t)g * NP }, { y.p + (size_t)g * NP }, false, ApplyCg());
    T->profile = prof;
    if (rc != NF_OK) { (void)hipStreamSynchronize(st); return rc; }
    TrGroups ivel, chid; memset(&ivel, 0, sizeof ivel); memset(&chid, 0, sizeof chid);
    for (int g = 0; g < ng; ++g) { ivel.v[g] = 1.0 / K.v[g]; if (K.chid) chid.v[g] = K.chid[g]; }
    const int grid = grid_for(NP, 256, T->opt.kin_grid), nfam = K.d_c ? I : 0, rows = 5 + nfam;   // without precursors no c_amp row is formed
    hipLaunchKernelGGL(k_kin_forms, dim3(grid), dim3(256), 0, st, (const double *)S->d_phi_adj, phi, (const double *)y.p, (const double *)S->d_Mf,
                       (const double *)S->d_Chi, dW, (const double *const *)S->d_Ms_tab, K.d_c, N, NP, ng, ivel, chid, K.chid ? 0 : 1, nfam,
                       part.p, (long)RED_GRID);
    for (int r0 = 0; r0 < rows; r0 += 4) tr_finalize(T, part.p + (size_t)r0 * RED_GRID, grid, std::min(4, rows - r0), sums + r0);   // k_finalize takes four rows
    double h[KIN_ROWS]; memset(h, 0, sizeof h);
    HIPCHK(hipMemcpyAsync(h, sums, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                             // the temporaries are freed on return
    HIPCHK(hipGetLastError());
    res->production = h[0]; res->delayed_production = h[1]; res->removal_leakage = h[2]; res->scatter = h[3]; res->amplitude = h[4];
    bool finite = true;
    for (int r = 0; r < 5; ++r) finite = finite && std::isfinite(h[r]);
    for (int i = 0; i < nfam; ++i) { res->c_amp[i] = h[5 + i]; finite = finite && std::isfinite(res->c_amp[i]); }
    if (!finite || res->production == 0.0)
        return fail(NF_ERR_NUMERIC, "%s: the forms are not usable: production phi+^T F phi = %g, delayed %g, removal + leakage %g, scatter %g, amplitude %g "
                    "(orthogonal, zero or non-finite fields, or no fission)", who, h[0], h[1], h[2], h[3], h[4]);
    res->fw = res->production / k0;
    res->rho = (res->production / k0 - res->removal_leakage + res->scatter) / res->fw;
    for (int i = 0; i < I; ++i) { res->beta_eff_i[i] = K.beta[i] * res->delayed_production / res->production; res->beta_eff += res->beta_eff_i[i]; }
    res->gen_time = res->amplitude / res->fw;
    res->rho_dollars = res->beta_eff == 0.0 ? 0.0 : res->rho / res->beta_eff;
    return NF_OK;
}

int nf_kinetics_params(nf_handle S, const nf_kinetics *kin, double keff, nf_pk_result *res)
{
    NFCHK(pk_args(S, res, "nf_kinetics_params"));
    if (!kin) return fail(NF_ERR_ARG, "nf_kinetics_params: bad arguments");
    NFCHK(kinetics_check(S, kin, keff, "nf_kinetics_params"));
    KinData K = { kin->n_families, kin->beta, kin->lambda, kin->velocity_host, kin->chi_delayed_host, nullptr, S->tr ? S->tr->d_W : nullptr, 0.0, 0 };
    return pk_body(S, "nf_kinetics_params", S->d_phi, K, keff, res);
}

int nf_transient_kinetics(nf_handle S, nf_pk_result *res)
{
    NFCHK(pk_args(S, res, "nf_transient_kinetics"));
    const Transient *R = S->tr;
    if (!R) return fail(NF_ERR_STATE, "nf_transient_kinetics: call nf_transient_begin first");
    KinData K = { R->nfam, R->beta, R->lambda, R->v.data(), R->has_chid ? R->chid.data() : nullptr, R->d_c, R->d_W, R->time, 1 };
    return pk_body(S, "nf_transient_kinetics", R->d_phi, K, R->k0, res);
}

// ---- SolveAdjoint (src/NeutFEM.cpp:1877-2082) -----------------------------------------------------
// Literal control flow of the reference, including what makes it fragile (forward-ordered sweep on the transposed scatter,
// Chebyshev from outer 5 when k is free).  Works on slab teams (collective).
int nf_solve_adjoint(nf_handle S, const nf_keff_opts *o, int normalize_to_direct, int use_direct_keff, double *keff_adj, int *n_outer)
{
    if (!S || !o) return fail(NF_ERR_ARG, "nf_solve_adjoint: bad arguments");
    if ((o->use_diagonal_solver && S->k == 0 && S->m == 0) || o->use_cmfd || o->use_coarse_init) NFCHK(void_refuse(S, "nf_solve_adjoint with use_diagonal_solver, use_cmfd or use_coarse_init"));
    if (S->team->dead) return fail(NF_ERR_COMM, "this team lost a collective (NF_ERR_COMM) and is unusable: destroy the handles and end the process with a non-zero code (never re-exec)");
    nf_team *T = S->team;
    for (auto *X : T->slabs) if (!X->built) return fail(NF_ERR_STATE, "nf_solve_adjoint: call nf_build first");
    HIPCHK(hipSetDevice(T->device));
    Inner in;
    NFCHK(inner_begin(T, o, DIAG_NEVER, &in));                    // S is symmetric: the same group solver, the same S^-1
    const InnerPlan &ip = in.ip;
    const int ns = (int)T->slabs.size();
    nf_solver *S0 = T->slabs[0];
    const int ng = S0->ng;
    hipStream_t st = T->stream;
    double keff = 1.0;
    if (use_direct_keff && T->has_valid_keff) keff = T->last_keff;          // :1885-1889
    // global number of flux DOFs (the start vector is 1 / ||1||, :1891-1892): local sum, all-reduced on a multi-rank team
    double ntot = 0.0;
    for (auto *X : T->slabs) ntot += (double)X->nphi * ng;
    if (T->rccl_reduce && T->nproc > 1) {
        HIPCHK(hipMemcpyAsync(T->d_red, &ntot, sizeof(double), hipMemcpyHostToDevice, st));
        NCCLCHK(g_rccl.AllReduce(T->d_red, T->d_red, 1, NCCL_DOUBLE, NCCL_SUM, T->comm, st));
        HIPCHK(hipMemcpyAsync(&ntot, T->d_red, sizeof(double), hipMemcpyDeviceToHost, st));
        NFCHK(team_stream_wait(T, st));
    }
    std::vector<DevTmp<double>> nsft(ns);
    std::vector<int> gN(ns), gT(ns);
    for (int i = 0; i < ns; ++i) {
        nf_solver *X = T->slabs[i];
        const long NT = X->nphi * ng;
        gN[i] = grid_for(X->nphi); gT[i] = grid_for(NT);
        if (!X->d_phi_adj) NFCHK(dalloc(&X->d_phi_adj, (size_t)NT));
        hipLaunchKernelGGL(k_fill_const, dim3(gT[i]), dim3(256), 0, st, X->d_phi_adj, NT, 1.0 / std::sqrt(ntot));
        NFCHK(dalloc(&nsft[i].p, (size_t)X->N));
        hipLaunchKernelGGL(k_sum_groups, dim3(grid_for(X->N)), dim3(256), 0, st, X->d_NSF, nsft[i].p, X->N, ng);    // :1898-1905
    }
    const ChebTable cheb = cheb_table();
    int cheb_it = 0;
    T->hist_k.clear(); T->hist_dk.clear(); T->hist_dphi.clear(); T->hist_cg.clear();
    T->last_outer = 0; T->last_cg_total = 0;
    // forward-ordered sweep on the transposed blocks (:1944-1950), emission nu Sigma_f; the reference starts this CG plainly and counts no
    // stand-in solve here: both kept as they are
    GroupSweep sw = sweep_for(T);
    sw.transposed = true; sw.ride_start = false; sw.count_team = nullptr;
    for (int i = 0; i < ns; ++i) { nf_solver *X = T->slabs[i]; sw.slab[i].emis = X->d_NSF; sw.slab[i].phi_new = X->d_raw; sw.slab[i].phi_old = X->d_phi_adj; sw.slab[i].sol = X->d_raw; }
    double hout[4];
    int rc = NF_OK;
    // sum_e nsf_tot[e] * (M_chi v)[e, dof 0] over the team, result in `out` (:1912-1936)
    auto chi_product = [&](bool of_raw, double *out) -> int {
        for (int i = 0; i < ns; ++i) {
            nf_solver *X = T->slabs[i];
            hipLaunchKernelGGL(k_fission, dim3(gN[i]), dim3(256), 0, st, X->d_Mchi, of_raw ? X->d_raw : X->d_phi_adj, ng, X->nphi, X->d_tf,
                               T->d_partials + i * T->slab_cap, (const double *)nsft[i].p, X->N);
        }
        return team_finalize(T, FIN_SUM, gN, 1, out, 0.0, 0);
    };
    for (int it = 0; it < o->max_outer && rc == NF_OK; ++it) {
        if ((rc = chi_product(false, T->d_out)) != NF_OK) break;
        sw.fscale = 1.0 / keff;
        if ((rc = group_sweep(T, ip, 0, sw, sweep_no_hook, [&](int, int its) { T->hist_cg.push_back(its); T->last_cg_total += its; })) != NF_OK) break;
        // NB: chi_product(true) overwrites d_tf with M_chi raw; the next outer recomputes it from phi_adj first
        if ((rc = chi_product(true, T->d_out + 1)) != NF_OK) break;
        for (int i = 0; i < ns; ++i) {
            nf_solver *X = T->slabs[i];
            hipLaunchKernelGGL(k_outer_reduce, dim3(gT[i]), dim3(256), 0, st, X->d_Mchi, X->d_raw, X->d_phi_adj, X->nphi * ng, T->d_partials + i * T->slab_cap, T->partial_stride);
        }
        if ((rc = team_finalize(T, FIN_SUM, gT, 3, T->d_out + 2, 0.0, 0)) != NF_OK) break;     // d_out[2..4]: { unused, ||phi||^2, ||dphi||^2 }
        double h5[5];
        if (hipMemcpyAsync(h5, T->d_out, 5 * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            rc = fail(NF_ERR_HIP, "adjoint: read-back failed"); break;
        }
        hout[0] = h5[0]; hout[1] = h5[1];
        const double prod_old = hout[0], prod_new = hout[1], nsq = h5[3], dsq = h5[4];
        // not outer_step: the reference's adjoint guards the quotient (|prod_old| > 1e-14, from outer 1), takes sqrt(dsq) / sqrt(nsq), and freezes k
        double keff_new = keff, dk;
        if (!use_direct_keff || !T->has_valid_keff) {                          // :1966-1975
            if (std::fabs(prod_old) > 1e-14 && it > 0) keff_new = keff * (prod_new / prod_old);
            dk = std::fabs(keff_new - keff); keff = keff_new;
        } else dk = 0.0;
        const double dphi = std::sqrt(dsq) / std::sqrt(nsq), norm = std::sqrt(nsq);
        if (!std::isfinite(keff) || !std::isfinite(dphi)) { rc = fail(NF_ERR_NUMERIC, "adjoint iteration diverged (outer %d: k=%g dphi=%g)", it, keff, dphi); break; }
        const ChebStep cs = cheb_next(cheb_it, cheb, !use_direct_keff && it >= 5);   // :1990-1992
        for (int i = 0; i < ns && rc == NF_OK; ++i) rc = normalize_cheb(T->slabs[i], st, T->slabs[i]->d_phi_adj, norm, norm > 1e-14, cs);
        if (rc != NF_OK) break;
        T->hist_k.push_back(keff); T->hist_dk.push_back(dk); T->hist_dphi.push_back(dphi);
        T->last_outer = it + 1;
        bool conv = dphi < o->tol_flux;
        if (!use_direct_keff) conv = conv && dk < o->tol_keff;
        if (conv) break;
    }
    if (rc == NF_OK && normalize_to_direct && T->has_valid_keff) {            // <phi, phi+> = 1 with vol * w = detJ * C-hat_pp (:2020-2066)
        std::vector<DevTmp<double>> mass(ns), one(ns);
        for (int i = 0; i < ns && rc == NF_OK; ++i) {
            nf_solver *X = T->slabs[i];
            rc = dalloc(&mass[i].p, (size_t)X->nphi); if (rc == NF_OK) rc = dalloc(&one[i].p, (size_t)X->N);
            if (rc != NF_OK) break;
            ChatArgs ch; ch.nloc = X->nloc;
            for (int p = 0; p < X->nloc; ++p) { int q = p; double c = 1.0; for (int t = 0; t < X->dim; ++t) { c *= 2.0 / (2.0 * (q % X->n1) + 1.0); q /= X->n1; } ch.c[p] = c; }
            hipLaunchKernelGGL(k_fill_const, dim3(grid_for(X->N)), dim3(256), 0, st, one[i].p, X->N, 1.0);
            hipLaunchKernelGGL(k_cell_coef, dim3(grid_for(X->N, 256, 65535)), dim3(256), 0, st, one[i].p, mass[i].p, X->d_hx, X->d_hy, X->d_hz, X->nx, X->ny, X->N, 2, X->dim, ch);
            hipLaunchKernelGGL(k_dot3, dim3(gT[i]), dim3(256), 0, st, X->d_phi, X->d_phi_adj, mass[i].p, X->nphi, ng, T->d_partials + i * T->slab_cap);
        }
        if (rc == NF_OK) rc = team_finalize(T, FIN_SUM, gT, 1, T->d_out, 0.0, 0);
        double ip = 0.0;
        if (rc == NF_OK && (hipMemcpyAsync(&ip, T->d_out, sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
            rc = fail(NF_ERR_HIP, "adjoint: read-back failed");
        if (rc == NF_OK && std::fabs(ip) > 1e-14)
            for (int i = 0; i < ns; ++i) hipLaunchKernelGGL(k_scale, dim3(gT[i]), dim3(256), 0, st, T->slabs[i]->d_phi_adj, T->slabs[i]->nphi * ng, ip);
        (void)hipStreamSynchronize(st);
    }
    (void)hipStreamSynchronize(st);
    if (rc != NF_OK) return rc;
    HIPCHK(hipGetLastError());
    for (auto *X : T->slabs) { X->raw_valid = false; X->has_valid_adjoint = 1; X->last_keff_adj = keff; }
    if (keff_adj) *keff_adj = keff;
    if (n_outer) *n_outer = T->last_outer;
    return NF_OK;
}
int nf_get_phi_adj(nf_handle S, double *phi_host)
{
    if (!S || !phi_host) return fail(NF_ERR_ARG, "nf_get_phi_adj: bad arguments");
    if (!S->d_phi_adj) { for (long i = 0; i < S->nphi * S->ng; ++i) phi_host[i] = 1.0; return NF_OK; }   // Sol_Phi_adj_ = 1 (:226-235)
    return phi_transfer(S, phi_host, false, S->d_phi_adj);
}

// ---- ProjectFluxRefined / ProjectPowerRefined (declared include/NeutFEM.hpp:303-313, bound src/wrapper.cpp:1003-1043; never defined
// there): the mean of every cell's flux polynomial over rx x ry x rz equal sub-cells, k_project_refined
template <int DIM, int M>
static void launch_project_dm(bool power, int grid, hipStream_t st, const double *phi, const double *ksf, double *out, const nf_solver *S,
                              int rx, int ry, int rz, int NX, int NY, int crows, int npairs, int vec, int step_rows, int step_pairs)
{
    if (power)
        hipLaunchKernelGGL((k_project_refined<DIM, M, true>), dim3(grid), dim3(256), 0, st, phi, ksf, out, S->nx, S->ny, S->N, S->nphi, S->ng,
                           rx, ry, rz, NX, NY, crows, npairs, vec, step_rows, step_pairs);
    else
        hipLaunchKernelGGL((k_project_refined<DIM, M, false>), dim3(grid), dim3(256), 0, st, phi, ksf, out, S->nx, S->ny, S->N, S->nphi, S->ng,
                           rx, ry, rz, NX, NY, crows, npairs, vec, step_rows, step_pairs);
}
template <int DIM>
static void launch_project_d(int m, bool power, int grid, hipStream_t st, const double *phi, const double *ksf, double *out, const nf_solver *S,
                             int rx, int ry, int rz, int NX, int NY, int crows, int npairs, int vec, int step_rows, int step_pairs)
{
    if (m == 0) launch_project_dm<DIM, 0>(power, grid, st, phi, ksf, out, S, rx, ry, rz, NX, NY, crows, npairs, vec, step_rows, step_pairs);
    else if (m == 1) launch_project_dm<DIM, 1>(power, grid, st, phi, ksf, out, S, rx, ry, rz, NX, NY, crows, npairs, vec, step_rows, step_pairs);
    else launch_project_dm<DIM, 2>(power, grid, st, phi, ksf, out, S, rx, ry, rz, NX, NY, crows, npairs, vec, step_rows, step_pairs);
}

// launch shape of the kernels that walk the mesh refined by (rx, ry, rz) (k_project_refined, k_zoom_source): a thread owns one pair of
// fine columns of one coarse row, all its ry rz fine rows; 32 waves per CU, then grid-stride by step_rows rows + step_pairs pairs
struct RefinePlan { int NX, NY, crows, npairs, grid, step_rows, step_pairs; long NE; };
static int refine_plan(const nf_solver *S, int rx, int ry, int rz, const char *who, RefinePlan *P)
{
    const long NXl = (long)S->nx * rx, rowsl = (long)S->ny * ry * S->nz * rz;
    if (NXl >= INT_MAX || rowsl > INT_MAX / 2) return fail(NF_ERR_ARG, "%s: refined mesh of %ld x %ld cells is too large", who, NXl, rowsl);
    P->NX = (int)NXl; P->NY = S->ny * ry; P->crows = S->ny * S->nz; P->npairs = (P->NX + 1) / 2;
    P->NE = (long)S->N * rx * ry * rz;
    int ncu = 256; (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, S->device);
    const long items = (long)P->crows * P->npairs;
    P->grid = (int)std::max<long>(1, std::min<long>((items + 255) / 256, 8L * ncu));
    const long stride = (long)P->grid * 256;
    P->step_rows = (int)(stride / P->npairs); P->step_pairs = (int)(stride % P->npairs);
    return NF_OK;
}

// flux (ksf == nullptr): group g >= 0, or every group (g = -1) into consecutive N R blocks; power: sum over the groups weighted by ksf
static int project_impl(nf_solver *S, int rx, int ry, int rz, int adjoint, int g, const double *ksf_host, double *out, const char *who)
{
    const bool power = ksf_host != nullptr;
    if (!S || !out) return fail(NF_ERR_ARG, "%s: bad arguments", who);
    if (!power && (g < -1 || g >= S->ng)) return fail(NF_ERR_ARG, "%s: group %d outside -1 .. %d", who, g, S->ng - 1);
    if (rx < 1 || ry < 1 || rz < 1) return fail(NF_ERR_ARG, "%s: refine factors must be >= 1 (got %d, %d, %d)", who, rx, ry, rz);
    if ((S->dim < 2 && ry > 1) || (S->dim < 3 && rz > 1))
        return fail(NF_ERR_ARG, "%s: refine factor > 1 on an axis the %dD mesh does not have (%d, %d, %d)", who, S->dim, rx, ry, rz);
    if (!S->built) return fail(NF_ERR_STATE, "%s: call nf_build first", who);
    RefinePlan P;
    NFCHK(refine_plan(S, rx, ry, rz, who, &P));
    const int NX = P.NX, NY = P.NY, crows = P.crows, npairs = P.npairs;
    const long NE = P.NE;
    const long N = S->N;
    if (power)
        for (int gg = 0; gg < S->ng; ++gg)
            for (long e = 0; e < N; ++e)
                if (!std::isfinite(ksf_host[gg * N + e])) return fail(NF_ERR_ARG, "%s: non-finite kappa Sigma_f in group %d, cell %ld", who, gg, e);
    HIPCHK(hipSetDevice(S->device));
    hipStream_t st = S->team->stream;
    (void)hipGetLastError();                                      // a failed allocation of an earlier call must not be reported here
    DevTmp<double> ones, ksf;
    const double *src = adjoint ? S->d_phi_adj : S->d_phi;
    if (!src) {                                                   // no adjoint solve yet: Sol_Phi_adj_ = 1 on every DOF (nf_get_phi_adj)
        const long n = power ? S->nphi * S->ng : S->nphi;
        NFCHK(dalloc(&ones.p, (size_t)n));
        hipLaunchKernelGGL(k_fill_const, dim3(grid_for(n)), dim3(256), 0, st, ones.p, n, 1.0);
        src = ones.p;
    }
    if (power) {
        NFCHK(dalloc(&ksf.p, (size_t)N * S->ng));
        HIPCHK(hipMemcpyAsync(ksf.p, ksf_host, (size_t)N * S->ng * sizeof(double), hipMemcpyHostToDevice, st));
    }
    const int grid = P.grid, step_rows = P.step_rows, step_pairs = P.step_pairs;
    const int vec = (NX % 2 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    const int g0 = power ? 0 : (g < 0 ? 0 : g), g1 = power ? 1 : (g < 0 ? S->ng : g + 1);
    for (int gg = g0; gg < g1; ++gg) {
        const double *phi = src == ones.p || power ? src : src + (size_t)gg * S->nphi;
        double *o = out + (g < 0 && !power ? (size_t)gg * NE : 0);
        const int v = vec && ((uintptr_t)o & 15) == 0;
        if (S->dim == 1) launch_project_d<1>(S->m, power, grid, st, phi, ksf.p, o, S, rx, ry, rz, NX, NY, crows, npairs, v, step_rows, step_pairs);
        else if (S->dim == 2) launch_project_d<2>(S->m, power, grid, st, phi, ksf.p, o, S, rx, ry, rz, NX, NY, crows, npairs, v, step_rows, step_pairs);
        else launch_project_d<3>(S->m, power, grid, st, phi, ksf.p, o, S, rx, ry, rz, NX, NY, crows, npairs, v, step_rows, step_pairs);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));                             // the temporaries are freed on return
    return NF_OK;
}
int nf_project_flux(nf_handle S, int rx, int ry, int rz, int adjoint, int g, double *out_dev)
{
    return project_impl(S, rx, ry, rz, adjoint, g, nullptr, out_dev, "nf_project_flux");
}
int nf_project_power(nf_handle S, int rx, int ry, int rz, int adjoint, const double *ksf_host, double *out_dev)
{
    if (!ksf_host) return fail(NF_ERR_ARG, "nf_project_power: bad arguments");
    return project_impl(S, rx, ry, rz, adjoint, 0, ksf_host, out_dev, "nf_project_power");
}

// ---- zoom_resolved (NeutFEM::ZoomResolved, include/NeutFEM.hpp:311, bound src/wrapper.cpp:1045-1065; declared, never defined there):
// the problem is solved again on the mesh refined by (rx, ry, rz) with the fission source of the coarse solution frozen

// a per-cell array of `nfields` fields [f*N + e] replicated onto the refined mesh [f*NE + E] (injection of the cross sections): the P0
// instantiation of k_project_refined copies DOF 0 of the parent into every sub-cell
static void refine_replicate(const nf_solver *S, const RefinePlan &P, int rx, int ry, int rz, const double *src, double *dst, int nfields)
{
    hipStream_t st = S->team->stream;
    const int vec = P.NX % 2 == 0 ? 1 : 0;                        // hipMalloc'ed arrays, NE even: every field starts 16-byte aligned
    for (int f = 0; f < nfields; ++f) {
        const double *a = src + (size_t)f * S->N; double *o = dst + (size_t)f * P.NE;
        if (S->dim == 1) launch_project_dm<1, 0>(false, P.grid, st, a, nullptr, o, S, rx, ry, rz, P.NX, P.NY, P.crows, P.npairs, vec, P.step_rows, P.step_pairs);
        else if (S->dim == 2) launch_project_dm<2, 0>(false, P.grid, st, a, nullptr, o, S, rx, ry, rz, P.NX, P.NY, P.crows, P.npairs, vec, P.step_rows, P.step_pairs);
        else launch_project_dm<3, 0>(false, P.grid, st, a, nullptr, o, S, rx, ry, rz, P.NX, P.NY, P.crows, P.npairs, vec, P.step_rows, P.step_pairs);
    }
}
static int refine_args(const nf_solver *S, int rx, int ry, int rz, const char *who)
{
    if (rx < 1 || ry < 1 || rz < 1) return fail(NF_ERR_ARG, "%s: refine factors must be >= 1 (got %d, %d, %d)", who, rx, ry, rz);
    if ((S->dim < 2 && ry > 1) || (S->dim < 3 && rz > 1))
        return fail(NF_ERR_ARG, "%s: refine factor > 1 on an axis the %dD mesh does not have (%d, %d, %d)", who, S->dim, rx, ry, rz);
    return NF_OK;
}
static int refine_impl(nf_solver *S, int rx, int ry, int rz, nf_handle *out)
{
    RefinePlan P;
    NFCHK(refine_plan(S, rx, ry, rz, "nf_refine", &P));
    if ((long)S->nz * rz >= INT_MAX || (long)S->ny * ry >= INT_MAX) return fail(NF_ERR_ARG, "nf_refine: refined mesh is too large");
    const int dim = S->dim, ng = S->ng;
    auto cut = [](const std::vector<double> &b, int n, int r, bool active) {   // every coarse break is kept exactly
        std::vector<double> f(active ? (size_t)n * r + 1 : 1, active ? 0.0 : b[0]);
        if (!active) return f;
        for (int i = 0; i < n; ++i) for (int a = 0; a < r; ++a) f[(size_t)i * r + a] = b[i] + a * (b[i + 1] - b[i]) / r;
        f[(size_t)n * r] = b[n];
        return f;
    };
    const std::vector<double> xf = cut(S->xb, S->nx, rx, true), yf = cut(S->yb, S->ny, ry, dim >= 2), zf = cut(S->zb, S->nz, rz, dim >= 3);
    nf_handle F = nullptr;
    NFCHK(create_impl(S->k, S->m, ng, (int)xf.size(), xf.data(), (int)yf.size(), yf.data(), (int)zf.size(), zf.data(), 0, 0, S->device, &F));
    *out = F;
    if (F->dim != dim || F->N != P.NE) return fail(NF_ERR_ARG, "nf_refine: the refined mesh lost a dimension");
    for (int a = 0; a < 8; ++a) if (S->bc_set[a]) nf_set_bc(F, a, S->bc_type[a]);
    team_copy_options(F->team, S->team, true);
    const size_t NN = (size_t)P.NE * ng;
    NFCHK(dalloc(&F->d_D, NN)); NFCHK(dalloc(&F->d_SigR, NN)); NFCHK(dalloc(&F->d_NSF, NN)); NFCHK(dalloc(&F->d_Chi, NN));
    refine_replicate(S, P, rx, ry, rz, S->d_D, F->d_D, ng); refine_replicate(S, P, rx, ry, rz, S->d_SigR, F->d_SigR, ng);
    refine_replicate(S, P, rx, ry, rz, S->d_NSF, F->d_NSF, ng); refine_replicate(S, P, rx, ry, rz, S->d_Chi, F->d_Chi, ng);
    for (int b = 0; b < ng * ng; ++b)
        if (S->d_SigS[b]) { NFCHK(dalloc(&F->d_SigS[b], (size_t)P.NE)); refine_replicate(S, P, rx, ry, rz, S->d_SigS[b], F->d_SigS[b], 1); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(S->team->stream));                // the copies ran on the parent's stream; nf_build uses the twin's
    F->xs_uploaded = true;
    return nf_build(F);
}
int nf_refine(nf_handle S, int rx, int ry, int rz, nf_handle *fine)
{
    if (!S || !fine) return fail(NF_ERR_ARG, "nf_refine: bad arguments");
    *fine = nullptr;
    NFCHK(void_refuse(S, "nf_refine"));
    NFCHK(refine_args(S, rx, ry, rz, "nf_refine"));
    if (!team_is_single(S->team)) return fail(NF_ERR_UNSUPPORTED, "nf_refine works on an undivided mesh (not on the slabs of a team)");
    if (!S->xs_uploaded) return fail(NF_ERR_STATE, "nf_refine: call nf_upload_xs first");
    HIPCHK(hipSetDevice(S->device));
    (void)hipGetLastError();
    int rc = refine_impl(S, rx, ry, rz, fine);
    if (rc != NF_OK && *fine) { std::string keep = g_err; nf_destroy(*fine); *fine = nullptr; g_err = keep; (void)hipGetLastError(); }
    return rc;
}

template <int DIM>
static void launch_zoom_d(int m, const RefinePlan &P, hipStream_t st, const double *phi, const double *win, const double *wout, double *q,
                          const nf_solver *C, double inv_k, int rx, int ry, int rz, int *flags, double *part)
{
    const int vec = P.NX % 2 == 0 ? 1 : 0;
#define NF_ZOOM(M) hipLaunchKernelGGL((k_zoom_source<DIM, M>), dim3(P.grid), dim3(256), 0, st, phi, win, wout, q, C->d_hx, C->d_hy, C->d_hz, inv_k, \
                                      C->nx, C->ny, C->N, C->nphi, C->ng, rx, ry, rz, P.NX, P.NY, P.NE, P.crows, P.npairs, vec, P.step_rows, P.step_pairs, flags, part)
    if (m == 0) NF_ZOOM(0); else if (m == 1) NF_ZOOM(1); else NF_ZOOM(2);
#undef NF_ZOOM
}
int nf_zoom_source(nf_handle C, nf_handle F, int adjoint, double keff)
{
    if (!C || !F || C == F) return fail(NF_ERR_ARG, "nf_zoom_source: bad arguments");
    NFCHK(void_refuse(C, "nf_zoom_source")); NFCHK(void_refuse(F, "nf_zoom_source"));
    if (!team_is_single(C->team) || !team_is_single(F->team)) return fail(NF_ERR_UNSUPPORTED, "nf_zoom_source works on undivided meshes (not on the slabs of a team)");
    if (C->device != F->device || C->ng != F->ng || C->dim != F->dim || C->k != F->k || C->m != F->m ||
        F->nx % C->nx || F->ny % C->ny || F->nz % C->nz)
        return fail(NF_ERR_ARG, "nf_zoom_source: %d x %d x %d (RT%d-P%d, %d groups) is not a refinement of %d x %d x %d (RT%d-P%d, %d groups) on the same device",
                    F->nx, F->ny, F->nz, F->k, F->m, F->ng, C->nx, C->ny, C->nz, C->k, C->m, C->ng);
    if (!std::isfinite(keff) || !(keff > 0.0)) return fail(NF_ERR_ARG, "nf_zoom_source: keff must be finite and positive (got %g)", keff);
    if (!C->built || !F->built) return fail(NF_ERR_STATE, "nf_zoom_source: call nf_build first (both handles)");
    if (adjoint && !C->d_phi_adj) return fail(NF_ERR_STATE, "nf_zoom_source: the coarse handle has no adjoint flux (nf_solve_adjoint or nf_set_phi_adj first)");
    const int rx = F->nx / C->nx, ry = F->ny / C->ny, rz = F->nz / C->nz;
    RefinePlan P;
    NFCHK(refine_plan(C, rx, ry, rz, "nf_zoom_source", &P));
    HIPCHK(hipSetDevice(C->device));
    (void)hipGetLastError();
    nf_team *T = F->team;
    hipStream_t st = T->stream;
    HIPCHK(hipStreamSynchronize(C->team->stream));                // the coarse flux is final
    if (!F->d_qsrc) NFCHK(dalloc(&F->d_qsrc, (size_t)F->nphi * F->ng));
    F->src_total = 0.0; F->src_any = false;
    DevTmp<int> flags; NFCHK(dalloc(&flags.p, 1));
    DevTmp<double> part; NFCHK(dalloc(&part.p, (size_t)P.grid + 1));   // the blocks' shares of the source total, then the total
    HIPCHK(hipMemsetAsync(flags.p, 0, sizeof(int), st));
    const double *phi = adjoint ? C->d_phi_adj : C->d_phi;
    const double *win = adjoint ? C->d_Chi : C->d_NSF, *wout = adjoint ? C->d_NSF : C->d_Chi;
    if (C->dim == 1) launch_zoom_d<1>(C->m, P, st, phi, win, wout, F->d_qsrc, C, 1.0 / keff, rx, ry, rz, flags.p, part.p);
    else if (C->dim == 2) launch_zoom_d<2>(C->m, P, st, phi, win, wout, F->d_qsrc, C, 1.0 / keff, rx, ry, rz, flags.p, part.p);
    else launch_zoom_d<3>(C->m, P, st, phi, win, wout, F->d_qsrc, C, 1.0 / keff, rx, ry, rz, flags.p, part.p);
    hipLaunchKernelGGL(k_zoom_total, dim3(1), dim3(256), 0, st, (const double *)part.p, P.grid, part.p + P.grid);
    int hf = 0; double tot = 0.0;
    HIPCHK(hipMemcpyAsync(&hf, flags.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&tot, part.p + P.grid, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (hf & 2) return fail(NF_ERR_NUMERIC, "nf_zoom_source: the frozen source is not finite (non-finite %s flux or keff = %g too small)", adjoint ? "adjoint" : "coarse", keff);
    if (!(hf & 1)) return fail(NF_ERR_ARG, "nf_zoom_source: the frozen source is zero on every cell (a zero %s flux, or no cell with both nuSigf and chi)", adjoint ? "adjoint" : "coarse");
    F->src_total = tot; F->src_any = true;
    return NF_OK;
}
int nf_get_source(nf_handle S, double *q_host)
{
    if (!S || !q_host) return fail(NF_ERR_ARG, "nf_get_source: bad arguments");
    if (!S->d_qsrc) return fail(NF_ERR_STATE, "nf_get_source: the handle has no source (nf_upload_source or nf_zoom_source first)");
    return phi_transfer(S, q_host, false, S->d_qsrc);
}
int nf_set_phi_adj(nf_handle S, const double *phi_adj_host)
{
    if (!S || !phi_adj_host) return fail(NF_ERR_ARG, "nf_set_phi_adj: bad arguments");
    HIPCHK(hipSetDevice(S->device));
    if (!S->d_phi_adj) NFCHK(dalloc(&S->d_phi_adj, (size_t)S->nphi * S->ng));
    return phi_transfer(S, const_cast<double *>(phi_adj_host), true, S->d_phi_adj);
}

static int zoom_solve(nf_handle C, nf_handle F, const nf_keff_opts *o, int adjoint, double keff, nf_zoom_result *res)
{
    NFCHK(nf_zoom_source(C, F, adjoint, keff));
    nf_team *T = F->team;
    Inner in;
    NFCHK(inner_begin(T, o, DIAG_NEVER, &in));
    GroupSweep sw = source_sweep(T, adjoint != 0);
    T->last_path = 0; T->profile = false;
    nf_zoom_result r; memset(&r, 0, sizeof r);
    r.source = F->src_total; r.n_cells = F->N;
    bool conv = false; long outers = 0;
    __atomic_store_n(&T->outers_done, 0L, __ATOMIC_RELEASE);
    NFCHK(nofission_phase(T, o, in.ip, 0, sw, "nf_zoom_resolved", &r.phi_int, &r.production, &r.n_outer, &r.cg_total, &conv, &outers));
    HIPCHK(hipStreamSynchronize(T->stream));
    HIPCHK(hipGetLastError());
    F->raw_valid = true; F->raw_is_diag = false; F->jz_valid = false;
    r.converged = conv ? 1 : 0;
    if (res) *res = r;
    return NF_OK;
}
int nf_zoom_resolved(nf_handle S, const nf_keff_opts *o, int rx, int ry, int rz, int adjoint, double keff, nf_handle *fine, nf_zoom_result *res)
{
    if (!S || !o || !fine) return fail(NF_ERR_ARG, "nf_zoom_resolved: bad arguments");
    *fine = nullptr;
    NFCHK(void_refuse(S, "nf_zoom_resolved"));
    if (o->use_coarse_init || o->use_cmfd || o->use_diagonal_solver)
        return fail(NF_ERR_ARG, "nf_zoom_resolved: coarse start, CMFD and the diagonal solver do not apply to the zoom's fixed-source iteration");
    if (o->max_outer < 1) return fail(NF_ERR_ARG, "nf_zoom_resolved: max_outer must be at least 1");
    if (!std::isfinite(keff) || !(keff > 0.0)) return fail(NF_ERR_ARG, "nf_zoom_resolved: keff must be finite and positive (got %g)", keff);
    NFCHK(refine_args(S, rx, ry, rz, "nf_zoom_resolved"));
    if (!team_is_single(S->team)) return fail(NF_ERR_UNSUPPORTED, "nf_zoom_resolved works on an undivided mesh (slab teams and multi-rank teams are not supported)");
    if (!S->built) return fail(NF_ERR_STATE, "nf_zoom_resolved: call nf_build first");
    if (adjoint && !S->d_phi_adj) return fail(NF_ERR_STATE, "nf_zoom_resolved: no adjoint flux (nf_solve_adjoint or nf_set_phi_adj first)");
    nf_handle F = nullptr;
    NFCHK(nf_refine(S, rx, ry, rz, &F));
    const int rc = zoom_solve(S, F, o, adjoint, keff, res);
    if (rc != NF_OK) { std::string keep = g_err; nf_destroy(F); g_err = keep; (void)hipGetLastError(); return rc; }
    *fine = F;
    return NF_OK;
}

// ---- sensitivity maps: dk/dXS per cell from the current flux, the adjoint flux and an eigenvalue -----------------------
// one launch of a kernel template <DIM, M> over the handle's order: NF_SENS_DM(k_sens_norm, part) / NF_SENS_DM(k_sens_mass, sc, maps...)
#define NF_SENS_FIELDS(S) (const double *)(S)->d_phi, adj, (const double *)(S)->d_Chi, (const double *)(S)->d_NSF, \
                          (const double *)(S)->d_hx, (const double *)(S)->d_hy, (const double *)(S)->d_hz, (S)->nx, (S)->ny, (S)->N, (S)->nphi, (S)->ng
#define NF_SENS_M(KERNEL, DIM, ...) do { \
        if (S->m == 0) hipLaunchKernelGGL((KERNEL<DIM, 0>), dim3(grid), dim3(256), 0, st, NF_SENS_FIELDS(S), __VA_ARGS__); \
        else if (S->m == 1) hipLaunchKernelGGL((KERNEL<DIM, 1>), dim3(grid), dim3(256), 0, st, NF_SENS_FIELDS(S), __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<DIM, 2>), dim3(grid), dim3(256), 0, st, NF_SENS_FIELDS(S), __VA_ARGS__); } while (0)
#define NF_SENS_DM(KERNEL, ...) do { \
        if (S->dim == 1) NF_SENS_M(KERNEL, 1, __VA_ARGS__); else if (S->dim == 2) NF_SENS_M(KERNEL, 2, __VA_ARGS__); else NF_SENS_M(KERNEL, 3, __VA_ARGS__); } while (0)
// adj: the adjoint-side field of the bilinear forms (phi+ for nf_sensitivity, Gamma+ for nf_gpt_sensitivity)
static void launch_sens_norm(const nf_solver *S, const double *adj, int grid, hipStream_t st, double *part) { NF_SENS_DM(k_sens_norm, part); }
static void launch_sens_mass(const nf_solver *S, const double *adj, int grid, hipStream_t st, const double *sc, double *dSigR, double *dNSF, double *dChi, double *dSigS)
{
    NF_SENS_DM(k_sens_mass, sc, dSigR, dNSF, dChi, dSigS);
}
#undef NF_SENS_DM
#undef NF_SENS_M
#undef NF_SENS_FIELDS
template <int DIM>
static void launch_sens_current_d(const nf_solver *S, int grid, hipStream_t st, const Geom &G, const SensJ &O, const double *j, const double *ja,
                                  const double *D, const double *sc, double *dD)
{
    if (S->k == 0) hipLaunchKernelGGL((k_sens_current<DIM, 0>), dim3(grid), dim3(256), 0, st, G, O, j, ja, D, sc, S->N, dD);
    else if (S->k == 1) hipLaunchKernelGGL((k_sens_current<DIM, 1>), dim3(grid), dim3(256), 0, st, G, O, j, ja, D, sc, S->N, dD);
    else hipLaunchKernelGGL((k_sens_current<DIM, 2>), dim3(grid), dim3(256), 0, st, G, O, j, ja, D, sc, S->N, dD);
}
static int gpt_grid(const nf_solver *S, long n) { return grid_for(n, 256, S->team->opt.sens_grid); }
// The bilinear forms of DESIGN.md 14 on (phi, adj) with the three device scalars (Nrm, c, -c / k) of one of two scalar kernels:
// gpt = false: k_sens_norm + k_sens_scalars (c = -k^2 / Nrm; Nrm zero or non-finite is an error) -- nf_sensitivity, launch for launch what
// it always issued; gpt = true: k_fission + k_gpt_defl_dot + k_gpt_scalars (Nrm = <adj, F phi> as measured, c = -1) -- nf_gpt_sensitivity.
// The caller has checked the state; who names it in the messages.
static int sens_body(nf_solver *S, const double *adj, bool gpt, const char *who, double keff, double *dD, double *dSigR, double *dNSF, double *dChi,
                     double *dSigS, double *nrm_out)
{
    hipStream_t st = S->team->stream;
    const long N = S->N;
    const int ng = S->ng, grid = grid_for(N, 256, S->team->opt.sens_grid);
    const int gx = gpt_grid(S, S->nphi), npart = gpt ? std::max(2 * gx * ng, grid) : grid;
    DevTmp<double> part; NFCHK(dalloc(&part.p, (size_t)npart + 3));    // the blocks' shares of Nrm, then Nrm, c, -c / k
    double *sc = part.p + npart;
    DevTmp<double> tf;
    if (gpt) {
        NFCHK(dalloc(&tf.p, (size_t)S->nphi));
        hipLaunchKernelGGL(k_fission, dim3(grid_for(S->nphi)), dim3(256), 0, st, S->d_Mf, S->d_phi, ng, S->nphi, tf.p, S->team->d_partials, (const double *)nullptr, 0L);
        hipLaunchKernelGGL(k_gpt_defl_dot, dim3(gx, ng), dim3(256), 0, st, adj, (const double *)S->d_Chi, (const double *)tf.p, N, S->nphi, part.p, (long)gx * ng);
        hipLaunchKernelGGL(k_gpt_scalars, dim3(1), dim3(256), 0, st, (const double *)part.p, gx * ng, keff, sc);
    } else {
        launch_sens_norm(S, adj, grid, st, part.p);
        hipLaunchKernelGGL(k_sens_scalars, dim3(1), dim3(256), 0, st, (const double *)part.p, grid, keff, sc);
    }
    double nrm = 0.0;
    HIPCHK(hipMemcpyAsync(&nrm, sc, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (!gpt && (!std::isfinite(nrm) || nrm == 0.0))
        return fail(NF_ERR_NUMERIC, "%s: the normalisation phi+^T F phi = %g is not usable (orthogonal, zero or non-finite fields, or no fission)", who, nrm);
    if (gpt && !std::isfinite(nrm))
        return fail(NF_ERR_NUMERIC, "%s: Gamma+^T F phi = %g is not finite (non-finite fields)", who, nrm);
    if (dSigR || dNSF || dChi || dSigS) launch_sens_mass(S, adj, grid, st, sc, dSigR, dNSF, dChi, dSigS);
    DevTmp<double> J, Ja;
    if (dD) {
        NFCHK(dalloc(&J.p, (size_t)S->nJ)); NFCHK(dalloc(&Ja.p, (size_t)S->nJ));
        const Geom G = make_geom(S);
        int ni = S->k; for (int t = 1; t < S->dim; ++t) ni *= S->k + 1;
        const long nJface = S->nJx + S->nJy + S->nJz;
        SensJ O; O.foff[0] = 0; O.foff[1] = S->nJx; O.foff[2] = S->nJx + S->nJy;
        for (int d = 0; d < 3; ++d) O.boff[d] = nJface + (long)d * N * ni;
        for (int g = 0; g < ng; ++g) {                            // group by group: two temporaries of nJ doubles
            NFCHK(flux_to_J(S, g, S->d_phi + (size_t)g * S->nphi, J.p, S->dim, 0, st));
            NFCHK(flux_to_J(S, g, adj + (size_t)g * S->nphi, Ja.p, S->dim, 0, st));
            const double *Dg = S->d_D + (size_t)g * N; double *out = dD + (size_t)g * N;
            if (S->dim == 1) launch_sens_current_d<1>(S, grid, st, G, O, J.p, Ja.p, Dg, sc, out);
            else if (S->dim == 2) launch_sens_current_d<2>(S, grid, st, G, O, J.p, Ja.p, Dg, sc, out);
            else launch_sens_current_d<3>(S, grid, st, G, O, J.p, Ja.p, Dg, sc, out);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));                             // the temporaries are freed on return
    *nrm_out = nrm;
    return NF_OK;
}
static int sens_args(nf_handle S, double keff, const char *who)
{
    if (!S) return fail(NF_ERR_ARG, "%s: bad arguments", who);
    NFCHK(void_refuse(S, who));
    if (!std::isfinite(keff) || !(keff > 0.0)) return fail(NF_ERR_ARG, "%s: keff must be finite and positive (got %g)", who, keff);
    if (!team_is_single(S->team)) return fail(NF_ERR_UNSUPPORTED, "%s works on an undivided mesh (the z currents cross slabs: slab teams and multi-rank teams are not supported)", who);
    if (S->N > 0xFFFFFFFFL) return fail(NF_ERR_UNSUPPORTED, "%s: %ld cells (the kernels index cells with 32 bits)", who, S->N);
    if (!S->built) return fail(NF_ERR_STATE, "%s: call nf_build first", who);
    return NF_OK;
}
int nf_sensitivity(nf_handle S, double keff, double *dD, double *dSigR, double *dNSF, double *dChi, double *dSigS, nf_sens_result *res)
{
    NFCHK(sens_args(S, keff, "nf_sensitivity"));
    if (!S->d_phi_adj) return fail(NF_ERR_STATE, "nf_sensitivity: no adjoint flux (nf_solve_adjoint or nf_set_phi_adj first)");
    HIPCHK(hipSetDevice(S->device));
    (void)hipGetLastError();
    double nrm = 0.0;
    NFCHK(sens_body(S, S->d_phi_adj, false, "nf_sensitivity", keff, dD, dSigR, dNSF, dChi, dSigS, &nrm));
    if (res) { res->norm = nrm; res->keff = keff; res->n_cells = S->N; }
    return NF_OK;
}

// ---- SolveModes: the leading lambda-modes by block power iteration (no counterpart in the reference) ---------------------
// Subspace iteration with a Rayleigh-Ritz step on A = K0^-1 F (adjoint: K0^-T F^T), host-driven like solve_subcritical_impl: per outer
// one application of A to every column of the block (the group sweep of the eigenvalue solve at inv_k = 1 with the group solver of
// inner_plan), one Gram pass, the small algebra on the host (nf_small_eig.h) and one rotate pass.
struct BlockWork {                                                // partial rows and their sums of the block kernels
    DevTmp<double> part, out; long stride = RED_GRID; int rows = 0;
    int ensure(int r)
    {
        if (r <= rows) return NF_OK;
        NFCHK(dalloc(&part.p, (size_t)r * stride)); NFCHK(dalloc(&out.p, (size_t)r));
        rows = r; return NF_OK;
    }
};
// sums of `rows` partial rows of `cnt` blocks each -> host
static int block_sums(nf_team *T, BlockWork &W, int rows, int cnt, double *host)
{
    hipLaunchKernelGGL(k_block_finalize, dim3(rows), dim3(256), 0, T->stream, (const double *)W.part.p, W.stride, cnt, W.out.p);
    HIPCHK(hipMemcpyAsync(host, W.out.p, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, T->stream));
    HIPCHK(stream_wait(T->stream));
    return NF_OK;
}
// H = Q^T Z (b x b, column-major) and G = Z^T Z (full symmetric) of two blocks of b vectors of length n
static int block_gram(nf_team *T, BlockWork &W, int b, long n, const double *Q, const double *Z, double *H, double *G)
{
    const int nt = (b + NF_BLOCK_TILE - 1) / NF_BLOCK_TILE, rows = b * b + b * (b + 1) / 2, gx = grid_for(n);
    NFCHK(W.ensure(rows));
    hipLaunchKernelGGL(k_block_gram, dim3(gx, nt * nt), dim3(256), 0, T->stream, Q, Z, b, n, W.part.p, W.stride);
    double s[NF_BLOCK_MAX * NF_BLOCK_MAX * 2];
    NFCHK(block_sums(T, W, rows, gx, s));
    for (int i = 0; i < b; ++i)
        for (int j = 0; j < b; ++j) {
            H[i + j * b] = s[gram_row_qz(b, i, j)];
            G[i + j * b] = s[i <= j ? gram_row_zz(b, i, j) : gram_row_zz(b, j, i)];
        }
    return NF_OK;
}
// Q <- Z C (C: b x b column-major) and res2[j] = |Z_j - sum_l Q_l Hm[l, j]|^2 for j < m with the old Q (Hm: m x m column-major; m = 0: none)
static int block_rotate(nf_team *T, BlockWork &W, int b, int m, long n, double *Q, const double *Z, const double *C, const double *Hm, double *res2)
{
    BlockCoef cf; memset(&cf, 0, sizeof cf);
    for (int j = 0; j < b; ++j) for (int l = 0; l < b; ++l) cf.C[l + j * b] = C[l + j * b];
    for (int j = 0; j < m; ++j) for (int l = 0; l < m; ++l) cf.H[l + j * b] = Hm[l + j * m];
    const int gx = grid_for(n);
    NFCHK(W.ensure(std::max(m, 1)));
#define NF_ROT(B) case B: hipLaunchKernelGGL((k_block_rotate<B>), dim3(gx), dim3(256), 0, T->stream, Q, Z, m, n, cf, W.part.p, W.stride); break;
    switch (b) { NF_ROT(1) NF_ROT(2) NF_ROT(3) NF_ROT(4) NF_ROT(5) NF_ROT(6) NF_ROT(7) NF_ROT(8) default: return fail(NF_ERR_ARG, "block_rotate: bad block size %d", b); }
#undef NF_ROT
    if (m > 0) NFCHK(block_sums(T, W, m, gx, res2));
    return NF_OK;
}
static int block_args(nf_handle S, int b, int m, long n, const void *Q, const void *Z, const char *who)
{
    if (!S || !Q || !Z) return fail(NF_ERR_ARG, "%s: bad arguments", who);
    if (b < 1 || b > NF_BLOCK_MAX || m < 0 || m > b || n < 1) return fail(NF_ERR_ARG, "%s: needs 1 <= b <= %d, m <= b and n >= 1 (got b = %d, m = %d, n = %ld)", who, NF_BLOCK_MAX, b, m, n);
    HIPCHK(hipSetDevice(S->device));
    return NF_OK;
}
int nf_block_gram(nf_handle S, int b, long n, const double *Q_dev, const double *Z_dev, double *QtZ_host, double *ZtZ_host)
{
    NFCHK(block_args(S, b, 0, n, Q_dev, Z_dev, "nf_block_gram"));
    if (!QtZ_host || !ZtZ_host) return fail(NF_ERR_ARG, "nf_block_gram: bad arguments");
    BlockWork W;
    NFCHK(block_gram(S->team, W, b, n, Q_dev, Z_dev, QtZ_host, ZtZ_host));
    HIPCHK(hipGetLastError());
    return NF_OK;
}
int nf_block_rotate(nf_handle S, int b, int m, long n, double *Q_dev, const double *Z_dev, const double *C_host, const double *H_host, double *res2_host)
{
    NFCHK(block_args(S, b, m, n, Q_dev, Z_dev, "nf_block_rotate"));
    if (!C_host || (m > 0 && (!H_host || !res2_host))) return fail(NF_ERR_ARG, "nf_block_rotate: bad arguments");
    BlockWork W;
    NFCHK(block_rotate(S->team, W, b, m, n, Q_dev, Z_dev, C_host, H_host, res2_host));
    HIPCHK(hipStreamSynchronize(S->team->stream));
    HIPCHK(hipGetLastError());
    return NF_OK;
}

static void modes_drop(nf_solver *S)
{
    if (S->team && S->team->stream && (S->d_modes[0] || S->d_modes[1])) (void)hipStreamSynchronize(S->team->stream);
    for (int a = 0; a < 2; ++a) { dfree(S->d_modes[a]); S->modes_n[a] = 0; S->modes_cap[a] = 0; }
}

// the first nb index triples (i, j, k), i < nx, j < ny, k < nz, in order of i + j + k, then k, then j
static void modes_harmonics(const nf_solver *S, int nb, StartArgs *sa)
{
    int c = 0;
    for (int s = 0; c < nb && s <= S->nx + S->ny + S->nz; ++s)
        for (int k = 0; c < nb && k < S->nz && k <= s; ++k)
            for (int j = 0; c < nb && j < S->ny && j + k <= s; ++j) {
                const int i = s - j - k;
                if (i < S->nx) { sa->hi[c] = i; sa->hj[c] = j; sa->hk[c] = k; ++c; }
            }
}

static int solve_modes_impl(nf_solver *S, const nf_keff_opts *o, int m, int b, int adjoint, nf_modes_result *res)
{
    nf_team *T = S->team;
    const int ng = S->ng; const long N = S->N, NP = S->nphi, NT = NP * ng;
    hipStream_t st = T->stream;
    Inner in;
    NFCHK(inner_begin(T, o, DIAG_LEAN, &in));
    const InnerPlan &ip = in.ip; const int use_diag = in.use_diag;
    T->profile = false;
    DevTmp<double> Qb, Zb;
    NFCHK(dalloc(&Qb.p, (size_t)b * NT)); NFCHK(dalloc(&Zb.p, (size_t)b * NT));
    double *Q = Qb.p, *Z = Zb.p;
    BlockWork W;
    NFCHK(W.ensure(std::max(b * b + b * (b + 1) / 2, 4 * NF_BLOCK_MAX)));
    const double *fis = adjoint ? S->d_Mchi : S->d_Mf, *emi = adjoint ? S->d_NSF : S->d_Chi;
    const int gN = grid_for(NP);
    nf_modes_result r; memset(&r, 0, sizeof r);
    r.n_modes = m; r.n_block = b;
    // z_j = A q_j for the first nc columns: fission source of q_j, then the group sweep (direct: ascending; adjoint: descending on the
    // transposed blocks), in place in z_j; with downscatter only every scatter term reads a group of z_j the sweep has already solved
    GroupSweep sw = sweep_for(T);
    sw.transposed = sw.descending = adjoint != 0;
    sw.slab[0].emis = emi;
    auto apply = [&](int nc) -> int {
        for (int j = 0; j < nc; ++j) {
            const double *q = Q + (size_t)j * NT; double *z = Z + (size_t)j * NT;
            hipLaunchKernelGGL(k_fission, dim3(gN), dim3(256), 0, st, fis, q, ng, NP, S->d_tf, T->d_partials, (const double *)nullptr, 0L);
            sw.slab[0].phi_new = sw.slab[0].phi_old = z; sw.slab[0].sol = z;
            NFCHK(group_sweep(T, ip, use_diag, sw, sweep_no_hook, [&](int, int its) { r.cg_total += its; }));
        }
        return NF_OK;
    };
    double H[64], G[64], V[64], Gp[64], L[64], X[64], C[64], Hm[64], wr[8], wi[8], res2[8], kprev[8];
    // start block: cosine harmonics into Z, orthonormalised into Q with the two block kernels
    {
        StartArgs hs; memset(&hs, 0, sizeof hs);
        modes_harmonics(S, b, &hs);
        hipLaunchKernelGGL(k_modes_start, dim3(grid_for((long)b * NT)), dim3(256), 0, st, Z, b, ng, NP, N, S->nx, S->ny, S->nz, hs);
        HIPCHK(hipMemsetAsync(Q, 0, (size_t)b * NT * sizeof(double), st));
        NFCHK(block_gram(T, W, b, NT, Z, Z, H, G));
        if (small_cholesky(b, G, L) != 0) return fail(NF_ERR_NUMERIC, "nf_solve_modes: block lost rank (the start block of %d cosine harmonics is dependent on this mesh)", b);
        small_inv_lt(b, L, C);
        NFCHK(block_rotate(T, W, b, 0, NT, Q, Z, C, nullptr, nullptr));
    }
    bool conv = false;
    for (int it = 0; it < o->max_outer; ++it) {
        NFCHK(apply(b));
        NFCHK(block_gram(T, W, b, NT, Q, Z, H, G));
        for (int i = 0; i < b * b; ++i) if (!std::isfinite(H[i]) || !std::isfinite(G[i])) return fail(NF_ERR_NUMERIC, "nf_solve_modes: the block iteration produced non-finite sums (outer %d)", it);
        if (small_eig(b, H, wr, wi, V) != 0) return fail(NF_ERR_NUMERIC, "nf_solve_modes: the eigenvalue iteration on the %d x %d projected matrix did not converge (outer %d)", b, b, it);
        for (int i = 0; i < b; ++i)                               // G' = V^T G V
            for (int j = 0; j < b; ++j) {
                double v = 0.0;
                for (int p = 0; p < b; ++p) for (int q = 0; q < b; ++q) v += V[p + i * b] * G[p + q * b] * V[q + j * b];
                Gp[i + j * b] = v;
            }
        const int cr = small_cholesky(b, Gp, L);
        if (cr != 0) return fail(NF_ERR_NUMERIC, "nf_solve_modes: block lost rank (pivot %d of %d at outer %d: A has fewer than n_block independent directions here; use fewer guard vectors)", -cr - 1, b, it);
        small_inv_lt(b, L, X);
        for (int i = 0; i < b; ++i)                               // C = V L^-T
            for (int j = 0; j < b; ++j) { double v = 0.0; for (int p = 0; p < b; ++p) v += V[i + p * b] * X[p + j * b]; C[i + j * b] = v; }
        for (int j = 0; j < m; ++j) for (int l = 0; l < m; ++l) Hm[l + j * m] = H[l + j * b];
        NFCHK(block_rotate(T, W, b, m, NT, Q, Z, C, Hm, res2));
        double rmax = 0.0, dk = 0.0; bool cplx = m < b && wi[m - 1] > 0.0;   // a pair cut by the block of wanted modes counts as complex
        for (int i = 0; i < m; ++i) {
            rmax = std::max(rmax, std::sqrt(res2[i]) / std::fabs(wr[i]));
            dk = std::max(dk, it == 0 ? HUGE_VAL : std::fabs(wr[i] - kprev[i]));
            cplx |= wi[i] != 0.0;
            if (!std::isfinite(res2[i])) return fail(NF_ERR_NUMERIC, "nf_solve_modes: non-finite residual (outer %d)", it);
            kprev[i] = wr[i];
        }
        r.n_outer = it + 1;
        if (!cplx && rmax < o->tol_flux && dk < o->tol_keff) { conv = true; break; }
    }
    // the returned vectors: eigenvectors of H_mm of one more application of A to the leading m columns, X = Q_m W, with their own
    // residuals A x_i - k_i x_i = Z_m w_i - k_i Q_m w_i (a complex pair: the residual of its plane)
    NFCHK(apply(m));
    NFCHK(block_gram(T, W, m, NT, Q, Z, H, G));
    for (int i = 0; i < m * m; ++i) if (!std::isfinite(H[i])) return fail(NF_ERR_NUMERIC, "nf_solve_modes: non-finite projected matrix at the end");
    if (small_eig(m, H, wr, wi, V) != 0) return fail(NF_ERR_NUMERIC, "nf_solve_modes: the eigenvalue iteration on the %d x %d projected matrix did not converge", m, m);
    ExtractCoef ec; memset(&ec, 0, sizeof ec);
    for (int j = 0; j < m; ++j)
        for (int l = 0; l < m; ++l) {
            ec.Wz[l + j * NF_BLOCK_MAX] = V[l + j * m];
            double v = wr[j] * V[l + j * m];                       // W Theta: A (u + i w) = (a + i b)(u + i w) -> A u = a u - b w, A w = b u + a w
            if (wi[j] > 0.0 && j + 1 < m) v -= wi[j] * V[l + (j + 1) * m];
            if (wi[j] < 0.0 && j > 0) v -= wi[j] * V[l + (j - 1) * m];
            ec.Wq[l + j * NF_BLOCK_MAX] = v;
        }
    if (!S->d_modes[adjoint] || S->modes_cap[adjoint] < m) { S->modes_n[adjoint] = 0; NFCHK(dalloc(&S->d_modes[adjoint], (size_t)m * NT)); S->modes_cap[adjoint] = m; }
    S->modes_n[adjoint] = 0;
    double *Xd = S->d_modes[adjoint];
    const int gT = grid_for(NT);
    hipLaunchKernelGGL(k_modes_extract, dim3(gT), dim3(256), 0, st, (const double *)Q, (const double *)Z, m, NT, fis, ec, Xd, W.part.p, W.stride);
    double s[4 * NF_BLOCK_MAX];
    NFCHK(block_sums(T, W, 4 * NF_BLOCK_MAX, gT, s));
    bool cplx = false;
    for (int i = 0; i < m; ++i) {
        const double x2 = s[i], r2 = s[NF_BLOCK_MAX + i], prod = s[2 * NF_BLOCK_MAX + i], aprod = s[3 * NF_BLOCK_MAX + i];
        if (!std::isfinite(x2) || !(x2 > 0.0) || !std::isfinite(r2)) return fail(NF_ERR_NUMERIC, "nf_solve_modes: mode %d came out non-finite or zero", i);
        const double sign = (prod < 0.0 && std::fabs(prod) >= 1e-10 * aprod) ? -1.0 : 1.0;   // sum Mf phi >= 0 where that sum means something
        hipLaunchKernelGGL(k_scale, dim3(gT), dim3(256), 0, st, Xd + (size_t)i * NT, NT, sign * std::sqrt(x2));
        r.k[i] = wr[i];
        r.residual[i] = std::sqrt(r2 / x2) / std::fabs(wr[i]);
        cplx |= wi[i] != 0.0;
    }
    for (int i = 0; i + 1 < m; ++i)
        if (wi[i] > 0.0) {                                        // the plane's residual for both members of a pair
            const double v = std::sqrt((s[NF_BLOCK_MAX + i] + s[NF_BLOCK_MAX + i + 1]) / (s[i] + s[i + 1])) / std::hypot(wr[i], wi[i]);
            r.residual[i] = r.residual[i + 1] = v;
        }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    S->modes_n[adjoint] = m;
    r.dominance_ratio = m > 1 ? r.k[1] / r.k[0] : 0.0;
    r.converged = conv && !cplx ? 1 : 0;
    if (res) *res = r;
    return NF_OK;
}

int nf_solve_modes(nf_handle S, const nf_keff_opts *o, int n_modes, int n_guard, int adjoint, nf_modes_result *res)
{
    if (!S || !o) return fail(NF_ERR_ARG, "nf_solve_modes: bad arguments");
    NFCHK(void_refuse(S, "nf_solve_modes"));
    nf_team *T = S->team;
    if (T->dead) return fail(NF_ERR_COMM, "this team lost a collective (NF_ERR_COMM) and is unusable: destroy the handles and end the process with a non-zero code (never re-exec)");
    if (n_modes < 1 || n_guard < 0 || n_modes + n_guard > NF_MODES_MAX)
        return fail(NF_ERR_ARG, "nf_solve_modes: needs 1 <= n_modes and n_modes + n_guard <= %d (got %d + %d)", NF_MODES_MAX, n_modes, n_guard);
    if (o->use_coarse_init || o->use_cmfd) return fail(NF_ERR_ARG, "nf_solve_modes: coarse start and CMFD do not apply to the block iteration");
    if (o->max_outer < 1) return fail(NF_ERR_ARG, "nf_solve_modes: max_outer must be at least 1");
    if (!team_is_single(T) || T->nproc > 1)
        return fail(NF_ERR_UNSUPPORTED, "nf_solve_modes works on an undivided mesh (slab teams and multi-rank teams are not supported)");
    if (!S->built) return fail(NF_ERR_STATE, "nf_solve_modes: call nf_build first");
    for (int g = 0; g < S->ng; ++g)
        for (int gp = g + 1; gp < S->ng; ++gp)
            if (S->d_Ms[g * S->ng + gp])
                return fail(NF_ERR_UNSUPPORTED, "nf_solve_modes: upscatter (group %d <- group %d) is not supported: the Gauss-Seidel group sweep lags "
                            "those terms, so the iteration operator would no longer be K0^-1 F", g, gp);
    if (S->N < n_modes + n_guard) return fail(NF_ERR_ARG, "nf_solve_modes: the mesh has %ld cells, fewer than the %d vectors of the block", S->N, n_modes + n_guard);
    HIPCHK(hipSetDevice(S->device));
    const int rc = solve_modes_impl(S, o, n_modes, n_modes + n_guard, adjoint ? 1 : 0, res);
    if (rc != NF_OK) { (void)hipStreamSynchronize(T->stream); (void)hipGetLastError(); }
    return rc;
}
int nf_get_mode(nf_handle S, int i, int adjoint, double *phi_host)
{
    if (!S || !phi_host) return fail(NF_ERR_ARG, "nf_get_mode: bad arguments");
    const int a = adjoint ? 1 : 0;
    if (!S->modes_n[a]) return fail(NF_ERR_STATE, "nf_get_mode: no %s modes on this handle (nf_solve_modes first; nf_build and nf_upload_xs drop them)", a ? "adjoint" : "direct");
    if (i < 0 || i >= S->modes_n[a]) return fail(NF_ERR_ARG, "nf_get_mode: mode %d of %d", i, S->modes_n[a]);
    return phi_transfer(S, phi_host, false, S->d_modes[a] + (size_t)i * S->nphi * S->ng);
}

// ---- SolveGPT: the generalized adjoint of a response ratio and its sensitivity maps (no counterpart in the reference) ----
// R = <w_a, phi> / <w_b, phi>; (M - F / k)^T Gamma+ = S+ with <Gamma+, F phi> = 0, by the fixed-source adjoint iteration at criticality with
// the fundamental mode deflated after every outer.  Host-driven like solve_modes_impl, on vectors of its own: phi, phi+, d_raw, the warm
// state and the history are not touched.
static void gpt_drop(nf_solver *S)
{
    if (S->team && S->team->stream && (S->d_gamma || S->d_gpt_w)) (void)hipStreamSynchronize(S->team->stream);
    dfree(S->d_gamma); dfree(S->d_gpt_w); dfree(S->d_gpt_sc); S->gpt_valid = false;
}
// partial rows of the GPT kernels (2 rows of `stride` doubles) and their sums into the device slots sc[slot0], sc[slot0 + 1]
struct GptWork { DevTmp<double> part; long stride = 0; };
static void gpt_finalize(nf_team *T, GptWork &W, int cnt, double *sc, int slot0)
{
    hipLaunchKernelGGL(k_block_finalize, dim3(2), dim3(256), 0, T->stream, (const double *)W.part.p, W.stride, cnt, sc + slot0);
}
// the weights on the device ([w_a | w_b], kept on the handle), <w_a, phi> and <w_b, phi> of the current flux into sc[GPT_WA], sc[GPT_WB]
// and on the host
static int gpt_response(nf_solver *S, GptWork &W, double *sc, double *sums)
{
    nf_team *T = S->team; hipStream_t st = T->stream;
    const long N = S->N; const int ng = S->ng, gc = gpt_grid(S, N);
    hipLaunchKernelGGL(k_gpt_response, dim3(gc, ng), dim3(256), 0, st, (const double *)S->d_phi, (const double *)S->d_gpt_w, (const double *)(S->d_gpt_w + (size_t)ng * N),
                       (const double *)S->d_hx, (const double *)S->d_hy, (const double *)S->d_hz, S->nx, S->ny, N, S->nphi, W.part.p, W.stride);
    gpt_finalize(T, W, gc * ng, sc, GPT_WA);
    HIPCHK(hipMemcpyAsync(sums, sc + GPT_WA, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(st));
    return NF_OK;
}
static int gpt_work(nf_solver *S, GptWork &W)
{
    W.stride = (long)S->team->opt.sens_grid * S->ng;
    return dalloc(&W.part.p, (size_t)2 * W.stride);
}
// the checks every GPT entry shares, before any launch
static int gpt_args(nf_handle S, double keff, const char *who)
{
    if (!S) return fail(NF_ERR_ARG, "%s: bad arguments", who);
    NFCHK(void_refuse(S, who));
    if (S->team->dead) return fail(NF_ERR_COMM, "this team lost a collective (NF_ERR_COMM) and is unusable: destroy the handles and end the process with a non-zero code (never re-exec)");
    if (!std::isfinite(keff) || !(keff > 0.0)) return fail(NF_ERR_ARG, "%s: keff must be finite and positive (got %g)", who, keff);
    if (!team_is_single(S->team) || S->team->nproc > 1)
        return fail(NF_ERR_UNSUPPORTED, "%s works on an undivided mesh (slab teams and multi-rank teams are not supported)", who);
    if (!S->built) return fail(NF_ERR_STATE, "%s: call nf_build first", who);
    if (!S->d_phi_adj) return fail(NF_ERR_STATE, "%s: no adjoint flux (nf_solve_adjoint or nf_set_phi_adj first)", who);
    return NF_OK;
}
// non-finite weights, and weights that make S+ vanish identically (w_a = lambda w_b: R does not depend on phi)
static int gpt_check_weights(const nf_solver *S, const double *wa, const double *wb, const char *who)
{
    const long n = (long)S->ng * S->N;
    long ja = -1, jb = -1;
    for (long i = 0; i < n; ++i) {
        if (!std::isfinite(wa[i]) || !std::isfinite(wb[i]))
            return fail(NF_ERR_ARG, "%s: non-finite weight in group %ld, cell %ld", who, i / S->N, i % S->N);
        if (ja < 0 && wa[i] != 0.0) ja = i;
        if (jb < 0 && wb[i] != 0.0) jb = i;
    }
    if (ja < 0 || jb < 0) return NF_OK;                           // a zero field: its sum is zero, reported as such (NF_ERR_NUMERIC)
    bool prop = true;
    for (long i = 0; i < n && prop; ++i) prop = wa[i] * wb[jb] == wb[i] * wa[jb];
    if (prop) return fail(NF_ERR_ARG, "%s: the source S+ is identically zero (w_a is a multiple of w_b: the ratio does not depend on the flux)", who);
    return NF_OK;
}
static int gpt_upload_weights(nf_solver *S, const double *wa, const double *wb)
{
    const size_t n = (size_t)S->ng * S->N;
    hipStream_t st = S->team->stream;
    if (!S->d_gpt_w) NFCHK(dalloc(&S->d_gpt_w, 2 * n));
    if (!S->d_gpt_sc) NFCHK(dalloc(&S->d_gpt_sc, (size_t)GPT_SLOTS));
    HIPCHK(hipMemsetAsync(S->d_gpt_sc, 0, GPT_SLOTS * sizeof(double), st));
    HIPCHK(hipMemcpyAsync(S->d_gpt_w, wa, n * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S->d_gpt_w + n, wb, n * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                             // the host arrays are the caller's
    return NF_OK;
}
static int gpt_check_sums(const double *sums, const char *who)
{
    if (!std::isfinite(sums[0]) || sums[0] == 0.0) return fail(NF_ERR_NUMERIC, "%s: the numerator <w_a, phi> = %g is not usable (zero or non-finite)", who, sums[0]);
    if (!std::isfinite(sums[1]) || sums[1] == 0.0) return fail(NF_ERR_NUMERIC, "%s: the denominator <w_b, phi> = %g is not usable (zero or non-finite)", who, sums[1]);
    return NF_OK;
}

static int solve_gpt_impl(nf_solver *S, const nf_keff_opts *o, double keff, nf_gpt_result *res)
{
    nf_team *T = S->team;
    const int ng = S->ng; const long N = S->N, NP = S->nphi, NT = NP * ng;
    hipStream_t st = T->stream;
    Inner in;
    NFCHK(inner_begin(T, o, DIAG_NEVER, &in));
    const InnerPlan &ip = in.ip;
    T->profile = false;
    GptWork W; NFCHK(gpt_work(S, W));
    double *sc = S->d_gpt_sc;
    const int gN = grid_for(NP), gx = gpt_grid(S, NP);
    nf_gpt_result r; memset(&r, 0, sizeof r);
    double sums[2];
    NFCHK(gpt_response(S, W, sc, sums));
    NFCHK(gpt_check_sums(sums, "nf_solve_gpt"));
    r.wa_phi = sums[0]; r.wb_phi = sums[1]; r.R = sums[0] / sums[1];
    // tf = sum_g' Mf_g' phi_g', once per call: F phi = chi (x) tf is never stored; the denominator <phi+, F phi> and ||F phi||^2
    DevTmp<double> tfphi, src, old;
    NFCHK(dalloc(&tfphi.p, (size_t)NP)); NFCHK(dalloc(&src.p, (size_t)NT)); NFCHK(dalloc(&old.p, (size_t)NT));
    hipLaunchKernelGGL(k_fission, dim3(gN), dim3(256), 0, st, S->d_Mf, S->d_phi, ng, NP, tfphi.p, T->d_partials, (const double *)nullptr, 0L);
    hipLaunchKernelGGL(k_gpt_defl_dot, dim3(gx, ng), dim3(256), 0, st, (const double *)S->d_phi_adj, (const double *)S->d_Chi, (const double *)tfphi.p, N, NP, W.part.p, W.stride);
    gpt_finalize(T, W, gx * ng, sc, GPT_DEN);
    double den[2];
    HIPCHK(hipMemcpyAsync(den, sc + GPT_DEN, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(st));
    if (!std::isfinite(den[0]) || den[0] == 0.0)
        return fail(NF_ERR_NUMERIC, "nf_solve_gpt: the normalisation phi+^T F phi = %g is not usable (orthogonal, zero or non-finite fields, or no fission)", den[0]);
    const double *wa = S->d_gpt_w, *wb = S->d_gpt_w + (size_t)ng * N;
    hipLaunchKernelGGL(k_gpt_source, dim3(gx, ng), dim3(256), 0, st, (const double *)S->d_phi, wa, wb, (const double *)sc, (const double *)S->d_hx, (const double *)S->d_hy,
                       (const double *)S->d_hz, S->nx, S->ny, N, NP, src.p, (double *)nullptr, (double *)nullptr);
    if (!S->d_gamma) NFCHK(dalloc(&S->d_gamma, (size_t)NT));
    S->gpt_valid = false;                                         // until the iteration has finished
    double *G = S->d_gamma;
    HIPCHK(hipMemsetAsync(G, 0, (size_t)NT * sizeof(double), st));
    HIPCHK(hipMemsetAsync(old.p, 0, (size_t)NT * sizeof(double), st));
    // the sweep runs from the last group to the first on the transposed scatter blocks, in place: in the descending sweep the groups above g
    // are the new ones, k_group_rhs reads both from the one array
    GroupSweep sw = sweep_for(T);
    sw.transposed = sw.descending = true; sw.fscale = 1.0 / keff;
    sw.slab[0].emis = S->d_NSF; sw.slab[0].phi_new = sw.slab[0].phi_old = G; sw.slab[0].sol = G; sw.slab[0].q = src.p;
    double dprev = 0.0, h[3];
    bool conv = false;
    for (int it = 0; it < o->max_outer; ++it) {
        // the adjoint fission term of the previous iterate, then the group sweep from the last group to the first on the transposed
        // scatter blocks, in place: with downscatter only every scatter term reads a group this sweep has already solved
        hipLaunchKernelGGL(k_fission, dim3(gN), dim3(256), 0, st, S->d_Mchi, (const double *)G, ng, NP, S->d_tf, T->d_partials, (const double *)nullptr, 0L);
        NFCHK(group_sweep(T, ip, 0, sw, sweep_no_hook, [&](int, int its) { r.cg_total += its; }));
        // deflation: Gamma -= (<Gamma, F phi> / <phi+, F phi>) phi+, beta formed on the device; norms and old <- Gamma in the same sweep
        hipLaunchKernelGGL(k_gpt_defl_dot, dim3(gx, ng), dim3(256), 0, st, (const double *)G, (const double *)S->d_Chi, (const double *)tfphi.p, N, NP, W.part.p, W.stride);
        hipLaunchKernelGGL(k_block_finalize, dim3(1), dim3(256), 0, st, (const double *)W.part.p, W.stride, gx * ng, sc + GPT_NUM);
        hipLaunchKernelGGL(k_gpt_defl_update, dim3(gx, ng), dim3(256), 0, st, G, (const double *)S->d_phi_adj, old.p, (const double *)sc, NP, W.part.p, W.stride);
        gpt_finalize(T, W, gx * ng, sc, GPT_NN);
        HIPCHK(hipMemcpyAsync(h, sc + GPT_NUM, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(stream_wait(st));
        const double nsq = h[1], dsq = h[2], dg = std::sqrt(dsq / nsq);
        r.n_outer = it + 1;
        __atomic_store_n(&T->outers_done, (long)(it + 1), __ATOMIC_RELEASE);
        if (!std::isfinite(h[0]) || !std::isfinite(nsq) || !std::isfinite(dg))
            return fail(NF_ERR_NUMERIC, "nf_solve_gpt: the iteration produced a non-finite iterate (outer %d: <Gamma, F phi> = %g, ||Gamma||^2 = %g, ||dGamma||^2 = %g)", it, h[0], nsq, dsq);
        r.ratio = dprev > 0.0 ? dg / dprev : 0.0;
        r.dgamma = dg; dprev = dg;
        if (dg < o->tol_flux) { conv = true; break; }
    }
    // what the last deflation left of the fundamental mode: |<Gamma, F phi>| / (||Gamma|| ||F phi||)
    hipLaunchKernelGGL(k_gpt_defl_dot, dim3(gx, ng), dim3(256), 0, st, (const double *)G, (const double *)S->d_Chi, (const double *)tfphi.p, N, NP, W.part.p, W.stride);
    hipLaunchKernelGGL(k_block_finalize, dim3(1), dim3(256), 0, st, (const double *)W.part.p, W.stride, gx * ng, sc + GPT_NUM);
    HIPCHK(hipMemcpyAsync(h, sc + GPT_NUM, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    r.deflation = std::fabs(h[0]) / (std::sqrt(h[1]) * std::sqrt(den[1]));
    if (!std::isfinite(r.deflation)) return fail(NF_ERR_NUMERIC, "nf_solve_gpt: the iterate came out zero or non-finite (<Gamma, F phi> = %g, ||Gamma||^2 = %g)", h[0], h[1]);
    r.norm = den[0];
    r.converged = conv ? 1 : 0;
    S->gpt_valid = true;
    if (res) *res = r;
    return NF_OK;
}

int nf_solve_gpt(nf_handle S, const nf_keff_opts *o, double keff, const double *wa_host, const double *wb_host, nf_gpt_result *res)
{
    if (!S || !o || !wa_host || !wb_host) return fail(NF_ERR_ARG, "nf_solve_gpt: bad arguments");
    NFCHK(gpt_args(S, keff, "nf_solve_gpt"));
    if (o->use_coarse_init || o->use_cmfd || o->use_diagonal_solver)
        return fail(NF_ERR_ARG, "nf_solve_gpt: coarse start, CMFD and the diagonal model do not apply to the generalized adjoint (use_coarse_init, use_cmfd and use_diagonal_solver must be 0)");
    if (o->max_outer < 1) return fail(NF_ERR_ARG, "nf_solve_gpt: max_outer must be at least 1");
    NFCHK(gpt_check_weights(S, wa_host, wb_host, "nf_solve_gpt"));
    HIPCHK(hipSetDevice(S->device));
    (void)hipGetLastError();
    S->gpt_valid = false;                                         // the weights below replace those Gamma+ was solved for
    int rc = gpt_upload_weights(S, wa_host, wb_host);
    if (rc == NF_OK) rc = solve_gpt_impl(S, o, keff, res);
    if (rc != NF_OK) { (void)hipStreamSynchronize(S->team->stream); (void)hipGetLastError(); }
    return rc;
}
int nf_get_gamma(nf_handle S, double *gamma_host)
{
    if (!S || !gamma_host) return fail(NF_ERR_ARG, "nf_get_gamma: bad arguments");
    if (!S->gpt_valid) return fail(NF_ERR_STATE, "nf_get_gamma: no generalized adjoint on this handle (nf_solve_gpt or nf_set_gamma first; nf_upload_xs, nf_build, nf_set_bc and nf_set_void drop it)");
    return phi_transfer(S, gamma_host, false, S->d_gamma);
}
int nf_set_gamma(nf_handle S, const double *gamma_host)
{
    if (!S || !gamma_host) return fail(NF_ERR_ARG, "nf_set_gamma: bad arguments");
    HIPCHK(hipSetDevice(S->device));
    if (!S->d_gamma) NFCHK(dalloc(&S->d_gamma, (size_t)S->nphi * S->ng));
    NFCHK(phi_transfer(S, const_cast<double *>(gamma_host), true, S->d_gamma));
    S->gpt_valid = true;
    return NF_OK;
}
int nf_gpt_source(nf_handle S, const double *wa_host, const double *wb_host, double *src_host, double *sums_host)
{
    if (!S || !wa_host || !wb_host) return fail(NF_ERR_ARG, "nf_gpt_source: bad arguments");
    NFCHK(gpt_args(S, 1.0, "nf_gpt_source"));
    NFCHK(gpt_check_weights(S, wa_host, wb_host, "nf_gpt_source"));
    HIPCHK(hipSetDevice(S->device));
    (void)hipGetLastError();
    hipStream_t st = S->team->stream;
    const int ng = S->ng; const long N = S->N, NP = S->nphi;
    S->gpt_valid = false;
    NFCHK(gpt_upload_weights(S, wa_host, wb_host));
    GptWork W; NFCHK(gpt_work(S, W));
    double sums[2];
    NFCHK(gpt_response(S, W, S->d_gpt_sc, sums));
    if (sums_host) { sums_host[0] = sums[0]; sums_host[1] = sums[1]; }
    NFCHK(gpt_check_sums(sums, "nf_gpt_source"));
    if (!src_host) return NF_OK;
    DevTmp<double> src; NFCHK(dalloc(&src.p, (size_t)NP * ng));
    hipLaunchKernelGGL(k_gpt_source, dim3(gpt_grid(S, NP), ng), dim3(256), 0, st, (const double *)S->d_phi, (const double *)S->d_gpt_w, (const double *)(S->d_gpt_w + (size_t)ng * N),
                       (const double *)S->d_gpt_sc, (const double *)S->d_hx, (const double *)S->d_hy, (const double *)S->d_hz, S->nx, S->ny, N, NP, src.p,
                       (double *)nullptr, (double *)nullptr);
    HIPCHK(hipGetLastError());
    return phi_transfer(S, src_host, false, src.p);
}
int nf_gpt_sensitivity(nf_handle S, double keff, double *dD, double *dSigR, double *dNSF, double *dChi, double *dSigS, double *dWa, double *dWb, nf_sens_result *res)
{
    NFCHK(sens_args(S, keff, "nf_gpt_sensitivity"));
    if (!S->gpt_valid) return fail(NF_ERR_STATE, "nf_gpt_sensitivity: no generalized adjoint on this handle (nf_solve_gpt or nf_set_gamma first)");
    if ((dWa || dWb) && !S->d_gpt_w) return fail(NF_ERR_STATE, "nf_gpt_sensitivity: the maps of the weights need the weights of an nf_solve_gpt (or nf_gpt_source) on this handle");
    HIPCHK(hipSetDevice(S->device));
    (void)hipGetLastError();
    if (dWa || dWb) {                                             // the sums of the flux the maps are taken at, then the two direct maps
        hipStream_t st = S->team->stream;
        const int ng = S->ng; const long N = S->N;
        GptWork W; NFCHK(gpt_work(S, W));
        double sums[2];
        NFCHK(gpt_response(S, W, S->d_gpt_sc, sums));
        NFCHK(gpt_check_sums(sums, "nf_gpt_sensitivity"));
        hipLaunchKernelGGL(k_gpt_source, dim3(gpt_grid(S, N), ng), dim3(256), 0, st, (const double *)S->d_phi, (const double *)S->d_gpt_w, (const double *)(S->d_gpt_w + (size_t)ng * N),
                           (const double *)S->d_gpt_sc, (const double *)S->d_hx, (const double *)S->d_hy, (const double *)S->d_hz, S->nx, S->ny, N, S->nphi, (double *)nullptr, dWa, dWb);
        HIPCHK(hipGetLastError());
    }
    double nrm = 0.0;
    NFCHK(sens_body(S, S->d_gamma, true, "nf_gpt_sensitivity", keff, dD, dSigR, dNSF, dChi, dSigS, &nrm));
    if (res) { res->norm = nrm; res->keff = keff; res->n_cells = S->N; }
    return NF_OK;
}

int nf_get_history(nf_handle S, double *k, double *dk, double *dphi, int *cg, int cap)
{
    if (!S) return fail(NF_ERR_ARG, "null handle");
    nf_team *T = S->team;
    const int n = std::min<int>(cap, T->last_outer);
    for (int i = 0; i < n; ++i) {
        if (k) k[i] = T->hist_k[i];
        if (dk) dk[i] = T->hist_dk[i];
        if (dphi) dphi[i] = T->hist_dphi[i];
        if (cg) for (int g = 0; g < S->ng; ++g) cg[i * S->ng + g] = T->hist_cg[i * S->ng + g];
    }
    return NF_OK;
}

int nf_profile_get(nf_handle S, const char *name, long *count, double *total_ms)
{
    if (!S || !name) return fail(NF_ERR_ARG, "nf_profile_get: bad arguments");
    auto it = S->team->prof.find(name);
    long c = 0, sk = 0; double ms = 0.0;
    if (it != S->team->prof.end()) it->second.stats(&c, &ms, &sk);
    if (count) *count = c;
    if (total_ms) *total_ms = ms;
    return NF_OK;
}
int nf_profile_reset(nf_handle S) { if (!S) return fail(NF_ERR_ARG, "null handle"); S->team->prof.clear(); return NF_OK; }

int nf_time_schur_apply(nf_handle S, int g, int reps, double *avg_ms)
{
    if (!S || g < 0 || g >= S->ng || reps < 1 || !avg_ms) return fail(NF_ERR_ARG, "nf_time_schur_apply: bad arguments");
    nf_team *T = S->team;
    for (auto *X : T->slabs) if (!X->built) return fail(NF_ERR_STATE, "nf_time_schur_apply: call nf_build first");
    HIPCHK(hipSetDevice(S->device));
    NFCHK(team_prepare(T));
    std::vector<const double *> xs; std::vector<double *> ys;
    for (auto *X : T->slabs) {
        hipLaunchKernelGGL(k_fill_pattern, dim3(grid_for(X->nphi)), dim3(256), 0, T->stream, X->d_p, X->nphi);
        xs.push_back(X->d_p); ys.push_back(X->d_q);
    }
    NFCHK(team_schur_apply(T, g, xs, ys, false, ApplyCg()));   // warm-up
    T->profile = true; const int every = T->opt.prof_every; T->opt.prof_every = 1;
    for (int i = 0; i < std::min(reps, 8); ++i) NFCHK(team_schur_apply(T, g, xs, ys, false, ApplyCg()));
    HIPCHK(hipStreamSynchronize(T->stream));
    prof_collect(T); T->profile = false; T->opt.prof_every = every;
    hipEvent_t a, b; HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    HIPCHK(hipEventRecord(a, T->stream));
    for (int i = 0; i < reps; ++i) NFCHK(team_schur_apply(T, g, xs, ys, false, ApplyCg()));
    HIPCHK(hipEventRecord(b, T->stream));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    *avg_ms = ms / reps;
    return NF_OK;
}

// LocalMatrices::Compute on the device, literally (nf_assembly.h): A_loc, B_loc, C_loc of `n_elems` elements of group g by tensor
// quadrature, one element per workgroup.  variant 0 = plain fp64 FMA, 1 = v_mfma_f64_16x16x4_f64.  reps > 1 repeats the launch for timing.
int nf_local_matrices(nf_handle S, int g, int n_elems, const int *elems_host, double *A_host, double *B_host, double *C_host, int variant, int reps, double *avg_ms)
{
    if (!S || g < 0 || g >= S->ng || n_elems < 1 || !elems_host || !A_host || !B_host || !C_host || variant < 0 || variant > 1 || reps < 1)
        return fail(NF_ERR_ARG, "nf_local_matrices: bad arguments");
    if (!S->xs_uploaded) return fail(NF_ERR_STATE, "nf_local_matrices: call nf_upload_xs first");
    for (int i = 0; i < n_elems; ++i) if (elems_host[i] < 0 || elems_host[i] >= S->N) return fail(NF_ERR_ARG, "nf_local_matrices: element %d out of range", elems_host[i]);
    HIPCHK(hipSetDevice(S->device));
    nf_team *T = S->team; hipStream_t st = T->stream;
    AsmArgs P; memset(&P, 0, sizeof P);
    P.dim = S->dim; P.k = S->k; P.m = S->m;
    // Gauss rule of order 2 max(k, m) + 3 (src/NeutFEM.cpp:276): 3 points for RT0, 5 for RT1, and 7 -> the 5-point fallback for RT2
    // (include/FEM.hpp:115-120)
    if (2 * std::max(S->k, S->m) + 3 == 3) {
        P.nq = 3; const double a = std::sqrt(0.6);
        P.qp[0] = -a; P.qp[1] = 0.0; P.qp[2] = a; P.qw[0] = 5.0 / 9.0; P.qw[1] = 8.0 / 9.0; P.qw[2] = 5.0 / 9.0;
    } else {
        P.nq = 5;
        const double p5[5] = { -0.906179845938664, -0.538469310105683, 0.0, 0.538469310105683, 0.906179845938664 };
        const double w5[5] = { 0.236926885056189, 0.478628670499366, 0.568888888888889, 0.478628670499366, 0.236926885056189 };
        for (int i = 0; i < 5; ++i) { P.qp[i] = p5[i]; P.qw[i] = w5[i]; }
    }
    int nf = 1, ni = S->k; for (int t = 1; t < S->dim; ++t) { nf *= S->k + 1; ni *= S->k + 1; }
    const int nJ = S->dim * (2 * nf + ni); int nP = 1; for (int t = 0; t < S->dim; ++t) nP *= S->m + 1;
    P.nx = S->nx; P.ny = S->ny; P.nz = S->nz; P.hx = S->d_hx; P.hy = S->d_hy; P.hz = S->d_hz;
    P.D = S->d_D + (size_t)g * S->N; P.Sig = S->d_SigR + (size_t)g * S->N; P.n_elems = n_elems;
    DevTmp<double> dA, dB, dC; DevTmp<int> dEl; int *&d_el = dEl.p;
    HIPCHK(hipMalloc((void **)&dA.p, (size_t)n_elems * nJ * nJ * sizeof(double))); HIPCHK(hipMalloc((void **)&dB.p, (size_t)n_elems * nP * nJ * sizeof(double)));
    HIPCHK(hipMalloc((void **)&dC.p, (size_t)n_elems * nP * nP * sizeof(double)));
    HIPCHK(hipMalloc((void **)&d_el, (size_t)n_elems * sizeof(int)));
    int rc = NF_OK;
    if (hipMemcpy(d_el, elems_host, (size_t)n_elems * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) rc = fail(NF_ERR_HIP, "nf_local_matrices: upload failed");
    P.elems = d_el; P.A = dA.p; P.B = dB.p; P.C = dC.p;
    const size_t lds = (size_t)(18 + 6 + 6 + 12 + 12 + 128 + 2 * 128 * 48 + 128 * 32) * sizeof(double);
    const void *fn = variant ? (const void *)k_local_matrices<true> : (const void *)k_local_matrices<false>;
    if (rc == NF_OK && !lds_opt_in(fn, lds)) rc = fail(NF_ERR_UNSUPPORTED, "nf_local_matrices needs %zu bytes of LDS per workgroup", lds);
    hipEvent_t a = nullptr, b = nullptr;
    if (rc == NF_OK) {
        (void)hipEventCreate(&a); (void)hipEventCreate(&b);
        for (int r = 0; r <= reps; ++r) {                         // one warm-up launch, then `reps` timed ones
            if (r == 1) (void)hipEventRecord(a, st);
            if (variant) hipLaunchKernelGGL(k_local_matrices<true>, dim3((unsigned)n_elems), dim3(256), lds, st, P);
            else hipLaunchKernelGGL(k_local_matrices<false>, dim3((unsigned)n_elems), dim3(256), lds, st, P);
        }
        (void)hipEventRecord(b, st);
        if (hipEventSynchronize(b) != hipSuccess || hipGetLastError() != hipSuccess) rc = fail(NF_ERR_HIP, "nf_local_matrices: kernel failed");
        float ms = 0.f; (void)hipEventElapsedTime(&ms, a, b);
        if (avg_ms) *avg_ms = ms / reps;
        (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    }
    if (rc == NF_OK && (hipMemcpy(A_host, dA.p, (size_t)n_elems * nJ * nJ * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(B_host, dB.p, (size_t)n_elems * nP * nJ * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(C_host, dC.p, (size_t)n_elems * nP * nP * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
        rc = fail(NF_ERR_HIP, "nf_local_matrices: download failed");
    return rc;
}

int nf_time_device_copy(nf_handle S, size_t bytes, int reps, double *gbps)
{
    if (!S || bytes < 16 || reps < 1 || !gbps) return fail(NF_ERR_ARG, "nf_time_device_copy: bad arguments");
    HIPCHK(hipSetDevice(S->device));
    hipStream_t st = S->team->stream;
    const long n2 = (long)(bytes / 16);
    nf_d2 *a = nullptr, *b = nullptr;
    NFCHK(dalloc(&a, (size_t)n2)); if (dalloc(&b, (size_t)n2) != NF_OK) { dfree(a); return NF_ERR_HIP; }
    (void)hipMemsetAsync(a, 0, (size_t)n2 * 16, st);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    double best = 0.0; hipError_t e = hipSuccess;
    int ncu = 256; (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, S->device);
    const bool verbose = getenv("NEUTFEM_COPY_VERBOSE") != nullptr;
    // best of: plain / non-temporal copy kernels with 4 (or 8) 16-byte loads in flight per lane at 16 ... 256 blocks per CU or one chunk
    // per block, and the runtime's own device-to-device copy (measured on one box, GB/s: 16 per CU 5424 / 5249 nt, 64 per CU 5622 / 5886 nt,
    // 8 in flight 5344 - 5638, hipMemcpyDtoD 4778; round 3's kernel with 8-byte halves: 4790)
    struct V { int kind, per_cu; };                               // kind 0 plain x4, 1 nt x4, 2 nt x8, 3 hipMemcpy ; per_cu 0 = one chunk per block
    const V vs[] = { {0, 16}, {0, 64}, {0, 256}, {0, 0}, {1, 16}, {1, 64}, {1, 256}, {1, 0}, {2, 64}, {2, 0}, {3, 0} };
    const int NV = (int)(sizeof vs / sizeof vs[0]);
    for (int variant = 0; variant < NV && e == hipSuccess; ++variant) {
        const V v = vs[variant];
        const int U = v.kind == 2 ? 8 : 4;
        const long full = (n2 + 256L * U - 1) / (256L * U);
        const int grid = (int)std::min<long>(v.per_cu ? (long)ncu * v.per_cu : full, full);
        auto once = [&]() {
            if (v.kind == 3) { (void)hipMemcpyAsync(b, a, (size_t)n2 * 16, hipMemcpyDeviceToDevice, st); return; }
            if (v.kind == 0) hipLaunchKernelGGL((k_copy<false, 4>), dim3(grid), dim3(256), 0, st, (const nf_d2 *)a, b, n2);
            else if (v.kind == 1) hipLaunchKernelGGL((k_copy<true, 4>), dim3(grid), dim3(256), 0, st, (const nf_d2 *)a, b, n2);
            else hipLaunchKernelGGL((k_copy<true, 8>), dim3(grid), dim3(256), 0, st, (const nf_d2 *)a, b, n2);
        };
        once();
        (void)hipEventRecord(e0, st);
        for (int i = 0; i < reps; ++i) once();
        (void)hipEventRecord(e1, st);
        e = hipEventSynchronize(e1);
        float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
        const double gb = ms > 0.f ? 2.0 * (double)n2 * 16.0 * reps / (ms * 1e-3) / 1e9 : 0.0;   // read + write
        if (verbose) fprintf(stderr, "[copy] variant %2d (%s, grid %d): %.0f GB/s\n", variant,
                             v.kind == 3 ? "hipMemcpyDtoD" : v.kind == 0 ? "plain, 4 in flight" : v.kind == 1 ? "nt, 4 in flight" : "nt, 8 in flight", v.kind == 3 ? 0 : grid, gb);
        if (e == hipSuccess) best = std::max(best, gb);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    dfree(a); dfree(b);
    if (e != hipSuccess) return fail(NF_ERR_HIP, "nf_time_device_copy: %s", hipGetErrorString(e));
    *gbps = best;
    return NF_OK;
}

int nf_set_option(nf_handle S, const char *key, long value)
{
    if (!S || !key) return fail(NF_ERR_ARG, "nf_set_option: bad arguments");
    nf_team *T = S->team;
    const bool own = !strcmp(key, "transient_rebalance");          // the one option kept per handle: the table normalises it
    NfOptions mine; unsigned fx = 0; std::string err;
    if (!nf_options_set(own ? mine : T->opt, key, value, &fx, &err)) return fail(NF_ERR_ARG, "%s", err.c_str());
    if (own) S->opt_tr_rebalance = (int)mine.transient_rebalance;
    if ((fx & NF_FX_RELINK) || ((fx & NF_FX_RELINK_MULTI) && T->nproc > 1)) T->linked_ready = false;
    if (!strcmp(key, "xsol_batch")) { HIPCHK(hipSetDevice(T->device)); for (auto *X : T->slabs) { dfree(X->d_ring); X->ring_m = 0; X->ring_refused = false; } }   // sized under it
    return team_apply_table_effects(T, fx);
}
int nf_get_option(nf_handle S, const char *key, long *value)
{
    if (!S || !key || !value) return fail(NF_ERR_ARG, "nf_get_option: bad arguments");
    if (!nf_options_get(S->team->opt, key, value)) return fail(NF_ERR_ARG, "nf_get_option: unknown key %s", key);
    if (!strcmp(key, "transient_rebalance")) *value = S->opt_tr_rebalance;
    return NF_OK;
}

// ---- raw memory helpers ------------------------------------------------------------------------
int nf_mem_info(int device, size_t *free_bytes, size_t *total_bytes)
{
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail(NF_ERR_ARG, "nf_mem_info: device %d out of range", device); }
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return NF_OK;
}
int nf_dev_alloc(nf_handle S, size_t bytes, void **p)
{
    if (!S || !p) return fail(NF_ERR_ARG, "nf_dev_alloc: bad arguments");
    HIPCHK(hipSetDevice(S->device)); HIPCHK(hipMalloc(p, std::max<size_t>(bytes, 8))); return NF_OK;
}
int nf_dev_free(nf_handle S, void *p) { if (!S) return fail(NF_ERR_ARG, "null handle"); HIPCHK(hipSetDevice(S->device)); if (p) HIPCHK(hipFree(p)); return NF_OK; }
int nf_memcpy_h2d(nf_handle S, void *dst, const void *src, size_t bytes)
{
    if (!S || !dst || !src) return fail(NF_ERR_ARG, "nf_memcpy_h2d: bad arguments");
    HIPCHK(hipSetDevice(S->device)); HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return NF_OK;
}
int nf_memcpy_d2h(nf_handle S, void *dst, const void *src, size_t bytes)
{
    if (!S || !dst || !src) return fail(NF_ERR_ARG, "nf_memcpy_d2h: bad arguments");
    HIPCHK(hipSetDevice(S->device)); HIPCHK(hipStreamSynchronize(S->team->stream)); HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return NF_OK;
}
int nf_synchronize(nf_handle S) { if (!S) return fail(NF_ERR_ARG, "null handle"); HIPCHK(hipSetDevice(S->device)); HIPCHK(hipStreamSynchronize(S->team->stream)); HIPCHK(hipDeviceSynchronize()); return NF_OK; }
void *nf_stream(nf_handle S) { return S ? (void *)S->team->stream : nullptr; }

// diagnostic (not part of the C ABI): the partial / stamp buffer of k_cg_xcd (doubles 384.. hold s_memrealtime sums in -DNF_XSTAMPS builds)
extern "C" int nf_debug_xcd_buffer(void *h, double *out, int n, int coarse)
{
    nf_solver *S = (nf_solver *)h; if (!S || !S->team) return NF_ERR_ARG;
    nf_team *T = S->team;
    (void)coarse;
    if (!T->d_xpart) { for (int i = 0; i < n; ++i) out[i] = 0.0; return NF_OK; }
    HIPCHK(hipMemcpy(out, T->d_xpart, sizeof(double) * std::min(n, 512), hipMemcpyDeviceToHost));
    return NF_OK;
}
