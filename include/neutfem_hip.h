/*
 * neutfem_hip.h -- C ABI of the MI355X (gfx950) hot path of neutfem_amd.
 *
 * This is the drop-in boundary: plain C types, opaque handle, int status
 * (0 = ok, <0 = error; text via nf_last_error()).  No exceptions, no torch or
 * Eigen types cross it.  Each entry point cites the reference interface it
 * replaces (paths relative to the reference repository jujuC31/NeutFEM).
 * Host pointers are marked _host, device pointers _dev (fp64 everywhere).
 *
 * Layouts (identical to the reference's flat arrays, include/NeutFEM.hpp:365-388):
 *   cell e = iz*nx*ny + iy*nx + ix                       (src/FEM.cpp:89-91)
 *   XS      [g*N + e]            SigS [(g_to*ng + g_from)*N + e]
 *   phi     [g*n_phi + e*n_loc + l]                      (n_loc = 1 for P0)   host arrays (nf_set_phi/nf_get_phi)
 *   *_dev vectors (nf_schur_apply, nf_solve_group): device DOF order [l*N + e] (moment-major; same thing for P0)
 *   J       [g*n_J + f]   faces x | y | z | bubbles      (src/FEM.cpp:264-334)
 */
#ifndef NEUTFEM_HIP_H
#define NEUTFEM_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct nf_solver *nf_handle;

enum { NF_OK = 0, NF_ERR_ARG = -1, NF_ERR_NO_DEVICE = -2, NF_ERR_HIP = -3, NF_ERR_UNSUPPORTED = -4,
       NF_ERR_STATE = -5, NF_ERR_NUMERIC = -6,
       NF_ERR_REMOTE = -7,   /* multi-rank team: another rank hit an error inside a solve; every rank returns at the same iteration */
       NF_ERR_COMM = -8 };   /* multi-rank team: a collective did not complete within NEUTFEM_COMM_TIMEOUT_S (a peer is gone or stuck).  The team is
                              * dead afterwards: its streams may hold collectives that never finish, so every further collective call on it
                              * returns NF_ERR_COMM at once and nf_destroy releases the host objects WITHOUT waiting for or freeing device
                              * resources.  The caller must end the process with a non-zero code (a fresh exit -- never an exec of another
                              * program from this process) */
/* BCType, include/NeutFEM.hpp:51-57 */
enum { NF_BC_DIRICHLET = 0, NF_BC_NEUMANN = 1, NF_BC_MIRROR = 2, NF_BC_ROBIN = 3, NF_BC_PERIODIC = 4 };

const char *nf_last_error(void);
/* number of visible HIP devices (0 when there is none); never throws */
int nf_device_count(void);

/* NeutFEM::NeutFEM (src/NeutFEM.cpp:82-300) + CartesianMesh (src/FEM.cpp:23-83) + FESpace
 * (src/FEM.cpp:177-259): mesh from break arrays (a 1-entry y/z array = inactive dimension),
 * RT/P orders clamped like the reference, device = HIP ordinal. */
int nf_create(int rt_order, int p_order, int ng,
              int nxb, const double *xb_host, int nyb, const double *yb_host, int nzb, const double *zb_host,
              int device, nf_handle *out);
int nf_destroy(nf_handle h);

/* ---- multi-GPU: z-slab decomposition (no reference counterpart; the reference is single-process) ------------
 * A slab is an nf_handle over the z-planes [k0,k1) of the global mesh: same x/y breaks, zb_slab = the slab's
 * own k1-k0+1 z-breaks, interface_below/above = 1 where another slab continues the mesh (that side is then not
 * a domain boundary).  Slabs living in one process on one device are chained with nf_link_slabs (bottom to top);
 * slabs of other processes are reached through RCCL: rank 0 calls nf_comm_unique_id, the 128 bytes are broadcast
 * by the launcher (torch.distributed / MPI / a file), every rank calls nf_comm_init.  Rank r must hold the slabs
 * just above rank r-1's.  After that nf_solve_keff / nf_time_schur_apply on any slab of the team run the whole
 * team; nf_set_phi / nf_get_phi / nf_upload_xs / nf_build stay per slab.
 * Collective calls (every rank, same order): nf_comm_init, nf_solve_keff, nf_solve_adjoint, nf_get_J, nf_build_diagonal_cache,
 * nf_team_schur_apply, nf_time_schur_apply.  Decisions that could differ between ranks (slab too thin for the
 * separator sweeps, coarse factors that do not divide a slab) are all-reduced first, so all ranks return the same
 * error.  Any RTk-Pm order; slabs need >= 4 z-planes (>= ~30 for the single-exchange fast path).
 * NEUTFEM_RCCL_LIB overrides the RCCL library path (tests use a host-staged stand-in to run several ranks on one GPU). */
int nf_create_slab(int rt_order, int p_order, int ng,
                   int nxb, const double *xb_host, int nyb, const double *yb_host, int nzb_slab, const double *zb_slab_host,
                   int interface_below, int interface_above, int device, nf_handle *out);
int nf_link_slabs(nf_handle *handles, int n);
int nf_comm_unique_id(void *id128_host);
int nf_comm_init(nf_handle h, const void *id128_host, int nranks, int rank);
/* what carries the data path: *comm_ranks = ncclCommCount of the live communicator (0: none, -1: the library lacks the entry),
 * lib_path = file the RCCL symbols were resolved from ("" without a communicator).  bench.py prints both (rccl_ranks, transport). */
int nf_comm_info(nf_handle h, int *comm_ranks, char *lib_path_host, size_t len);
/* diagnostic: grouped ncclSend/ncclRecv to the own rank on the comm stream + all-reduce(max) through the loaded RCCL */
int nf_comm_selftest(nf_handle h);
/* Schur apply on every local slab: x_dev[i] / y_dev[i] = device vectors of local slab i */
int nf_team_schur_apply(nf_handle h, int g, const double *const *x_dev, double *const *y_dev);

/* sizes: "dim","nx","ny","nz","ne","ng","n_phi","n_J","n_loc","last_outer","last_cg_total",
 * "coarse_outer","device","void_cells","n_local_slabs","n_ranks","rank","cg_reductions" (cross-rank reductions per CG iteration of the last CG solve on a
 * team: 1 single-reduction CG, 2 reference recurrence, 0 undivided mesh),"vec_reduce","xchg_comm","cg_form" (the form of the CG iteration the last CG solve ran -- after a refused one-XCD start
 * the form it continued with -- as an index into xcd, fuse3, lean, fused, classic, team_lean, team_vec, team_sr: the names nf_apply_plan
 * reports as "form") ; returns -1 for an unknown key */
long nf_info(nf_handle h, const char *key);

/* NeutFEM::SetBC (src/NeutFEM.cpp:337-345): attr per BoundaryID (include/NeutFEM.hpp:73-91).
 * Only DIRICHLET changes the operator (src/NeutFEM.cpp:1328-1456); the rest is natural/ignored. */
int nf_set_bc(nf_handle h, int attr, int bc_type);

/* ---- cut-out cells with a vacuum (albedo) condition (no counterpart in the reference) ---------------------------------
 * Cells marked void are cut out of the domain, and every face a kept cell shares with a void one carries J.n = gamma phi, n pointing
 * out of the kept cell (ANL-7416: gamma = 0.4692 on the stepped outline of the core).  In the built operator a void cell adds nothing
 * to A and B; a kept|void face gets A_ff += I_f(a) / gamma, I_f(a) the face integral of the Dirichlet term with the area of the kept
 * cell's face; every current DOF no kept cell touches (void|void faces, natural domain faces and bubbles of void cells) gets the identity;
 * a Dirichlet domain face of a void cell keeps its 2 D I term (it is decoupled).  C keeps the void cells (SigR as uploaded), while nuSigf,
 * chi and every scatter block count as zero there whatever was uploaded; D and SigR of void cells must still pass nf_upload_xs's checks.
 * The flux is exactly zero in void cells, and so are their bubble currents.  Domain faces keep their meaning: NF_BC_DIRICHLET gets the
 * reference's term, every other type is natural -- a vacuum condition on a domain face is posed with one plane of void cells outside it.
 * mask_host: N bytes in cell order, non-zero = void; NULL removes the mask (gamma is then ignored); a mask without a set byte is the
 * same as NULL.  The call takes effect at the next nf_build and marks the handle un-built (solves return NF_ERR_STATE until then); it
 * drops the coarse cache, the tables of distinct lines, the dense S^-1 and the modes, as nf_upload_xs does.  nf_info "void_cells" = the
 * number of void cells (0: no mask).  Errors: gamma non-finite or <= 0, or every cell void -> NF_ERR_ARG; a slab (nf_create_slab, linked
 * or multi-rank) -> NF_ERR_UNSUPPORTED.
 * With a mask: nf_build, nf_schur_apply (y = C x in void cells), nf_solve_group (the right-hand side is taken as 0 in void cells),
 * nf_solve_keff, nf_solve_adjoint, nf_get_phi / nf_get_phi_adj / nf_get_J, nf_set_phi, nf_project_flux / nf_project_power, history, timers
 * and plan reports work.  The CG runs the forms fuse3, lean, fused or classic, never xcd, and the in-kernel paths (resident, one-XCD,
 * diagonal device loop) are not taken: nf_info "last_path" is 0; a direct solver type runs CG to 1e-14 ("last_direct" 2), never the dense
 * S^-1.  NF_ERR_UNSUPPORTED (the text names nf_set_void; before any launch) with a mask for the calls that form A_ff themselves or build
 * a twin handle without the mask -- nf_solve_keff / nf_solve_adjoint with use_diagonal_solver (RT0-P0), use_cmfd or use_coarse_init,
 * nf_build_diagonal_cache, nf_initialize_cmfd, nf_solve_coarse, nf_coarsen, nf_refine, nf_zoom_source, nf_zoom_resolved, nf_sensitivity,
 * nf_transient_begin / nf_transient_step -- and for nf_solve_subcritical, nf_solve_modes, nf_solve_gpt, nf_gpt_source and nf_gpt_sensitivity. */
int nf_set_void(nf_handle h, const unsigned char *mask_host, double gamma);
/* the mask (N bytes, 0 / 1; may be NULL) and gamma (may be NULL) as set; NF_ERR_STATE without a mask */
int nf_get_void(nf_handle h, unsigned char *mask_host, double *gamma);

/* Public XS members D_data_, SigR_data_, NSF_data_, Chi_data_, SigS_data_
 * (include/NeutFEM.hpp:373-388) -> device.  Host arrays in the reference layouts. */
int nf_upload_xs(nf_handle h, const double *D_host, const double *SigR_host, const double *NSF_host,
                 const double *Chi_host, const double *SigS_host);

/* NeutFEM::BuildMatrices (src/NeutFEM.cpp:402-457): AssembleA/B/C, ApplyDirichletToA,
 * AssembleFissionMatrix, AssembleScatteringMatrix as closed-form per-cell coefficients, plus the
 * factorisation SchurSolver::SetMatrices does per solve (A_lu_solver_.compute, src/solvers.cpp:163),
 * done ONCE here as per-grid-line LDL^T.  Invalidates the diagonal cache, keeps the warm start. */
int nf_build(nf_handle h);

/* SchurSolver::SchurProduct (src/solvers.cpp:535-547): y = C_g x + B A_g^-1 B^T x. */
int nf_schur_apply(nf_handle h, int g, const double *x_dev, double *y_dev);

/* SchurSolver::SolveSchurImplicit (src/solvers.cpp:577-636): CG from x0 = 0, stop when
 * ||r||^2 < tol^2 ||b||^2 or after maxit iterations. its/res may be NULL. */
int nf_solve_group(nf_handle h, int g, const double *rhs_dev, double *phi_dev, double tol, int maxit,
                   int *its, double *res);

/* NeutFEM::BuildDiagonalSchurCache (src/NeutFEM.cpp:483-597); S_inv for group g is copied to
 * sinv_host (N doubles) when not NULL. */
int nf_build_diagonal_cache(nf_handle h);
int nf_get_diagonal_cache(nf_handle h, int g, double *sinv_host);

typedef struct nf_keff_opts {
    double tol_keff, tol_flux;      /* NeutFEM::SetTolerance, src/NeutFEM.cpp:327-335 */
    int max_outer, max_inner;
    int use_coarse_init;            /* SolveKeff arguments, src/wrapper.cpp:598-603 */
    int coarse_factors[3];
    int n_coarse_factors;
    int use_diagonal_solver;
    int solver_type;                /* LinearSolverType 0..9 (include/solvers.hpp:176-190) */
    int solver_type_pushed;         /* 0: set_linear_solver never called -> DIRECT_LU */
    int profile;                    /* 1: bracket every Schur-apply pass with HIP events */
    int use_cmfd;                   /* SolveKeff's 4th argument: CMFD correction from outer 2, replaces Chebyshev (:1750-1761,1786) */
} nf_keff_opts;

/* NeutFEM::SolveKeff(bool, vector<int>, bool, bool) (src/NeutFEM.cpp:1627-1815) incl. SolveCoarse
 * (src/NeutFEM.cpp:2380-2611), ChebyshevAccel (src/solvers.cpp:664-756) and SolveGroupInternal
 * (src/NeutFEM.cpp:2084-2105).  State kept between calls exactly like the reference:
 * current flux (nf_set_phi/nf_get_phi) and has_valid_keff_/last_keff_direct_. */
int nf_solve_keff(nf_handle h, const nf_keff_opts *opts, double *keff, int *n_outer);

/* No reference counterpart: nf_solve_keff on n independent handles in one call.  Equivalent to nf_solve_keff(h[i], &opts[n_opts == 1 ? 0 : i],
 * &keff[i], &n_outer[i]) for i = 0 .. n-1 in that order: flux, raw group fluxes, history, warm state, nf_progress and nf_info "last_path" /
 * "last_resident_serial" / "last_outer" / "last_cg_total" of every handle are afterwards bit for bit what those calls leave.  status[i] is
 * the code of handle i, the return value the first one that is not NF_OK; keff, n_outer, status and res may each be NULL.
 * Batched route -- one launch with one workgroup per handle: every handle undivided, built, without a mask (nf_set_void), of the same
 * orders, groups, dimension and nx, ny, nz (cell sizes and cross sections are free), with the same values of the options the one-workgroup
 * solve plans with, and every (handle, opts) pair one that nf_solve_keff alone would run in one workgroup (nf_info "last_path" 2) without
 * use_coarse_init.  The handles' streams are waited for, the launch goes to the stream of h[0].  Anything else that nf_solve_keff
 * would still solve takes the sequential route: nf_solve_keff per handle, in order.  res says which route ran.
 * Refused before any launch, status untouched: n < 1, h or opts NULL, a NULL handle, the same handle twice (two workgroups would write the
 * same vectors), n_opts neither 1 nor n, handles on different devices -> NF_ERR_ARG; a slab (nf_create_slab, linked) or a handle with a
 * communicator (nf_comm_init) -> NF_ERR_UNSUPPORTED (the batch must not reorder collectives); a handle that is not built -> NF_ERR_STATE.
 * nf_info(h[0], "batch_launches") counts the batched launches that went to the stream of that handle, "batch_capacity" is the number of
 * workgroups its argument array holds (it grows, never shrinks, and goes with the handle); nf_info(h, "compute_units") is the number
 * of compute units of the handle's device (hipDeviceAttributeMultiprocessorCount): up to that many workgroups run side by side. */
typedef struct nf_batch_result {
    int n_batched, n_sequential;    /* handles solved by the one launch / by nf_solve_keff one after another */
    int n_launches;                 /* 1 on the batched route, 0 on the sequential one */
    int variant;                    /* the kernel instantiation of the batch: 1 / 2 RT0-P0 line per lane at pitch 1536 / 2560, 3 / 4 RT1-P1 / RT2-P2
                                     * line per lane, 5 + 2 nb + (nx even) the scan variants (nb bubble moments); 0 sequential */
} nf_batch_result;
int nf_solve_keff_batch(nf_handle *h, int n, const nf_keff_opts *opts, int n_opts, double *keff, int *n_outer, int *status, nf_batch_result *res);

/* External source SRC_data_ (include/NeutFEM.hpp:365-388, get_SRC() at src/wrapper.cpp:829; SolveSubcritical reads it,
 * src/wrapper.cpp:699-715) -> device, host layout [g*N + e] like the cross sections; on a slab, the slab's own cells (as nf_upload_xs).
 * SRC is piecewise constant per cell: it loads DOF 0 only, q_g[e, 0] = Q_g(e) |e|.  Needs no nf_build and survives one; a new upload
 * replaces the source.  Non-finite values are refused (NF_ERR_ARG). */
int nf_upload_source(nf_handle h, const double *src_host);

typedef struct nf_subcrit_result {
    double M;                   /* amplification: phi_int / phi_int_nofission (include/NeutFEM.hpp:275-279, src/wrapper.cpp:699-715) */
    double k_source;            /* production / (production + source) */
    double ratio;               /* contraction dP_n / dP_{n-1} of the fission phase (last value with |dP_n| >= 1e-6 P_n; with downscatter only
                                 * it tends to the k-eff of the same core) */
    double phi_int, phi_int_nofission;   /* sum over g, e of |e| phibar_g(e) (phibar = DOF 0, the cell mean) with and without fission */
    double production;          /* sum over g, e of nuSigf_g(e) |e| phibar_g(e) */
    double source;              /* sum over g, e of Q_g(e) |e| */
    int n_outer, n_outer_nofission, cg_total, converged;   /* outers of the fission / no-fission phase, group-solve iterations of both */
} nf_subcrit_result;

/* NeutFEM::SolveSubcritical (declared include/NeutFEM.hpp:275-279 with the contract of src/wrapper.cpp:699-715, never defined there):
 * -div(D grad phi) + Sigma_r phi = F phi + Q, i.e. per group S_g phi_g = chi_g tf(phi) + sum_{g'!=g} Ms[g<-g'] phi_g' + q_g with the fission
 * source not divided by an eigenvalue.  Source iteration in two phases from phi = 0: without fission (phi0), then with it from phi0; each
 * stops when |P_n - P_{n-1}| / P_n < tol_keff (phase 0: phi_int in place of P) and ||phi_n - phi_{n-1}|| / ||phi_n|| < tol_flux, or after
 * max_outer outers (NF_OK, converged = 0).  Reads from opts: tol_keff, tol_flux, max_outer, max_inner, use_diagonal_solver (RT0-P0),
 * solver_type, solver_type_pushed -- the group solver is the one nf_solve_keff picks; use_coarse_init / use_cmfd must be 0 (NF_ERR_ARG).
 * Needs nf_build and nf_upload_source on every slab.  Errors: a zero source -> NF_ERR_ARG; a system that is not subcritical (the fission
 * phase's contraction >= 1 in 5 consecutive outers from its 5th on, or non-finite sums) -> NF_ERR_NUMERIC, current flux reset to 1.
 * Afterwards the converged flux (absolute units per unit source) is the current flux (nf_get_phi, nf_get_J); the warm state
 * (has_valid_keff / last_keff), nf_get_history and nf_info "last_outer" keep what the last nf_solve_keff left; nf_progress counts the
 * outers of both phases; nf_info "last_path" is 0.  Undivided meshes and linked slabs of one process; multi-rank teams: NF_ERR_UNSUPPORTED. */
int nf_solve_subcritical(nf_handle h, const nf_keff_opts *opts, nf_subcrit_result *res);

/* No reference counterpart (the reference is one process): outer iterations the running or last nf_solve_keff has completed
 * (the `it` of the loop at src/NeutFEM.cpp:1694).  May be called from another thread while nf_solve_keff runs -- the watchdog
 * of a multi-rank job tells a slow solve from one whose peers are gone.  On a multi-rank team a rank that fails inside a solve
 * makes every rank return (the failing one with its own code, the others with NF_ERR_REMOTE); a collective that does not complete
 * within NEUTFEM_COMM_TIMEOUT_S seconds (default 120) returns NF_ERR_COMM. */
int nf_progress(nf_handle h, long *outers_done);
/* The progress line of the outer loop (src/NeutFEM.cpp:1791-1796: "It n : k = ... dk = ... dphi = ..." every 5th iteration) WHILE the solve
 * runs: fn(user, it, keff, dk, dphi) is called on the calling thread after every outer iteration of the host-driven loop -- the path every
 * mesh beyond ~28 k unknowns per group takes, where a solve lasts seconds to minutes.  The in-kernel paths (resident, one-XCD, diagonal device
 * loop: milliseconds) have no host between their outers; their lines come from nf_get_history afterwards.  fn = NULL removes it. */
typedef void (*nf_progress_fn)(void *user, int outer, double keff, double dk, double dphi);
int nf_set_progress_callback(nf_handle h, nf_progress_fn fn, void *user);

/* CMFD acceleration (src/NeutFEM.cpp:662-1017, include/NeutFEM.hpp:119-143,232-235): NeutFEM::InitializeCMFD
 * (D-tilde for every direction, D-hat = 0; idempotent until the next nf_build), SetCMFDRelaxation, and a probe that
 * downloads D-tilde / D-hat of (group, direction) in the reference's face numbering (either pointer may be NULL).
 * The correction itself runs inside nf_solve_keff when opts.use_cmfd is set.  On a slab team nf_initialize_cmfd is collective
 * (the D-tilde of an interface z face needs the neighbouring slab's edge cells) and the PCG exchanges one plane per interface
 * and iteration. */
int nf_initialize_cmfd(nf_handle h);
int nf_set_cmfd_relaxation(nf_handle h, double omega);
int nf_get_cmfd_coefficients(nf_handle h, int g, int dir, double *dtilde_host, double *dhat_host);

/* NeutFEM::SolveAdjoint(normalize_to_direct, use_direct_keff) (src/NeutFEM.cpp:1877-2082, BuildFissionRHSAdjoint
 * :1568-1589): tolerances / solver type from opts; the adjoint flux is fetched with nf_get_phi_adj (host layout of phi). */
int nf_solve_adjoint(nf_handle h, const nf_keff_opts *opts, int normalize_to_direct, int use_direct_keff, double *keff_adj, int *n_outer);
int nf_get_phi_adj(nf_handle h, double *phi_adj_host);

/* Sub-cell projection: every cell e is cut into rx x ry x rz equal sub-cells and each gets the exact mean of the cell's flux polynomial
 * sum_p c_p P_i(xi) P_j(eta) P_k(zeta) over it (the Legendre means of every sub-interval in closed form).  Output on the
 * device (out_dev, e.g. from nf_dev_alloc) in the reference's cell order of the refined mesh, x fastest: fine cell
 * (X, Y, Z) = (ix rx + a, iy ry + b, iz rz + c) at (Z NY + Y) NX + X, NX = nx rx, NY = ny ry.  The factors are taken literally: < 1, or > 1
 * on an axis the mesh does not have (ry in 1D, rz in 1D / 2D) -> NF_ERR_ARG.  adjoint = 1 projects the adjoint flux (all ones before
 * any adjoint solve, as nf_get_phi_adj).  Needs nf_build (NF_ERR_STATE); changes no state of the handle.  On a slab: the slab's own
 * planes in slab-local fine numbering (nz_slab rz planes); not collective.
 * NeutFEM::ProjectFluxRefined (include/NeutFEM.hpp:303, src/wrapper.cpp:1003-1022; declared, never defined there):
 * g >= 0 -> N rx ry rz doubles of group g; g = -1 -> all groups, ng N rx ry rz doubles (group-major); other g -> NF_ERR_ARG. */
int nf_project_flux(nf_handle h, int rx, int ry, int rz, int adjoint, int g, double *out_dev);
/* NeutFEM::ProjectPowerRefined (include/NeutFEM.hpp:307, src/wrapper.cpp:1024-1043): P(E) = sum_g ksf_g(e) phibar_g(E), N rx ry rz
 * doubles, no normalisation.  ksf_host: kappa Sigma_f, ng N values in the host layout [g*N + e] (get_KSF()), uploaded for this call only;
 * non-finite values -> NF_ERR_ARG. */
int nf_project_power(nf_handle h, int rx, int ry, int rz, int adjoint, const double *ksf_host, double *out_dev);

/* ---- zoom: re-solve on a refined mesh with the coarse solution's fission source frozen ----
 * NeutFEM::ZoomResolved (declared include/NeutFEM.hpp:311, bound src/wrapper.cpp:1045-1065, never defined there; its docstring: unlike
 * project_flux, which interpolates, this method re-solves the problem on a refined mesh with the sources of the coarse mesh frozen).
 *
 * nf_refine: twin of nf_coarsen.  Returns a BUILT handle of the same RT / P orders, groups and boundary types on the mesh whose every
 * cell is cut into rx x ry x rz equal parts (breaks xb[i] + a (xb[i+1] - xb[i]) / rx, every coarse break kept exactly; cell order of
 * nf_project_flux); a fine cell has the cross sections of its parent.  The factors are taken literally, as nf_project_flux takes them.
 * Undivided meshes only (slab teams: NF_ERR_UNSUPPORTED); needs nf_upload_xs.  On a failure the partial handle is destroyed, *fine is
 * NULL and h stays usable.  The caller destroys the twin.  The fine handle starts with the options (nf_set_option) h has at this call
 * and reports its own solves (nf_info "cg_form", "xcd_solves", "last_direct" ... on the fine handle). */
int nf_refine(nf_handle h, int rx, int ry, int rz, nf_handle *fine);
/* Fills the load vector of `fine` (what nf_upload_source fills) from the coarse handle's current flux (adjoint = 1: its adjoint flux):
 * the fission source chi_g(e) / keff sum_g' nuSigf_g'(e) phi_g'(x) of every coarse cell e, a polynomial, restricted exactly to every
 * fine cell E in e and tested against every moment of E: q_g[E, p'] = chi_g(e) / keff sum_g' Mf'_g'[E, p'] c'_g'[E, p'] with Mf' the
 * fine fission matrix.  All moments are loaded, no 1e-14 drop.  Adjoint: chi and nuSigf swap roles.
 * Errors: fine is not a refinement of coarse (device, groups, orders, divisibility) or keff non-finite / <= 0 -> NF_ERR_ARG; a source
 * that is zero everywhere -> NF_ERR_ARG; a non-finite source -> NF_ERR_NUMERIC; adjoint without an adjoint flux -> NF_ERR_STATE. */
int nf_zoom_source(nf_handle coarse, nf_handle fine, int adjoint, double keff);
/* the load vector (nf_upload_source or nf_zoom_source) in the host DOF layout [g*n_phi + e*n_loc + p]; NF_ERR_STATE without one */
int nf_get_source(nf_handle h, double *q_host);
/* twin of nf_set_phi for the adjoint field Sol_Phi_adj_ (include/NeutFEM.hpp:380-388); allocates it if needed */
int nf_set_phi_adj(nf_handle h, const double *phi_adj_host);

typedef struct nf_zoom_result {
    double source;              /* sum over g, E of q_g[E, dof 0]: the frozen source integrated over the mesh */
    double phi_int;             /* sum over g, E of |E| phibar_g(E) of the zoomed flux */
    double production;          /* sum over g, E of nuSigf_g(E) |E| phibar_g(E) (the same weights for the adjoint field) */
    int n_outer, cg_total, converged;
    long n_cells;               /* cells of the refined mesh */
} nf_zoom_result;
/* nf_refine + nf_zoom_source + the fixed-source solve without fission on the refined mesh: per group
 * S_g phi_g = q_g + sum_{g' != g} Ms[g <- g'] phi_g' (adjoint: the transposed scatter blocks, forward sweep as nf_solve_adjoint), Gauss-Seidel
 * source iteration from phi = 0 with the group solver nf_solve_keff picks, stopped like phase 0 of nf_solve_subcritical (max_outer
 * reached: NF_OK, converged = 0).  No normalisation: the fine flux is in the units of the coarse one; with factors (1, 1, 1) and a
 * converged (phi, keff) it reproduces the coarse flux.  Reads tol_keff, tol_flux, max_outer, max_inner, solver_type, solver_type_pushed
 * from opts; use_coarse_init, use_cmfd and use_diagonal_solver must be 0 (NF_ERR_ARG).  *fine is the refined handle with the zoomed flux
 * as its current flux (nf_get_phi, nf_get_J, nf_project_flux work on it); the caller destroys it (NULL after an error).  Nothing of h
 * changes: flux, warm state, history and nf_progress stay as they are.  Undivided meshes only (NF_ERR_UNSUPPORTED). */
int nf_zoom_resolved(nf_handle h, const nf_keff_opts *opts, int rx, int ry, int rz, int adjoint, double keff, nf_handle *fine, nf_zoom_result *res);

/* ---- sensitivity maps (no counterpart in the reference) ----------------------------------------------------------------
 * First-order perturbation theory on the built operator: with phi the current flux (nf_get_phi), phi+ the adjoint flux (nf_get_phi_adj),
 * the eigenvalue keff, j_g = A_g^-1 B^T phi_g and j+_g = A_g^-1 B^T phi+_g (the line solves of nf_get_J), W_p(e) = detJ(e) C-hat_pp the
 * mass weight of a unit cross section (|e| at P0),
 *   m[g,g',e] = sum_p phi+_g[e,p] W_p(e) phi_g'[e,p]
 *   a[g,e]    = sum_d geometric factor_d(e) j+_loc^T A-hat_d j_loc over the cell's local current DOFs of direction d
 *   b[g,e]    = sum over the Dirichlet boundary faces f of e and their transverse modes of I_f(a) j+_{f,a} j_{f,a} (the build adds I_f(a) 2 D)
 *   Nrm       = sum_{g,g',e} chi_g(e) nuSigf_g'(e) m[g,g',e] = phi+^T F phi,      c = -keff^2 / Nrm
 * the maps are the absolute derivatives dk/dp of every cross section of every cell:
 *   dSigR[g,e] = c m[g,g,e]                      dSigS[g<-g',e] = -c m[g,g',e] (g != g'; 0 for g = g': the solver never reads the diagonal)
 *   dNSF[g',e] = -(c/keff) sum_g chi_g(e) m[g,g',e]          dChi[g,e] = -(c/keff) sum_g' nuSigf_g'(e) m[g,g',e]
 *   dD[g,e]    = c (a[g,e] / D_g(e)^2 - 2 b[g,e])
 * dD, dSigR, dNSF, dChi: ng N doubles [g*N + e]; dSigS: ng ng N doubles [(g_to*ng + g_from)*N + e] (the layouts of nf_upload_xs).  The
 * 1e-14 drop thresholds of the build (chi / k, the scatter blocks, the RT0 line entries) are ignored: the maps describe the operator
 * without them, and always the full operator (never the diagonal model).
 * The outputs are DEVICE buffers; any of them may be NULL and is then skipped (the others come out bit-identical).  res (may be NULL)
 * receives Nrm, the keff used and the cell count.  The call changes no state of the handle and is deterministic.
 * Errors: not built -> NF_ERR_STATE; no adjoint flux (nf_solve_adjoint or nf_set_phi_adj first) -> NF_ERR_STATE; keff non-finite or <= 0 ->
 * NF_ERR_ARG; Nrm non-finite or zero -> NF_ERR_NUMERIC (the outputs are then untouched); slabs and multi-rank teams -> NF_ERR_UNSUPPORTED
 * (the z currents cross slabs), and meshes of 2^32 cells or more.  nf_set_option "sens_grid" = blocks of 256 threads per launch (default 1024; the
 * kernels walk larger meshes with a grid stride). */
typedef struct nf_sens_result {
    double norm;                /* Nrm = phi+^T F phi */
    double keff;                /* the eigenvalue the maps were scaled with */
    long n_cells;               /* N */
} nf_sens_result;
int nf_sensitivity(nf_handle h, double keff, double *dD_dev, double *dSigR_dev, double *dNSF_dev, double *dChi_dev, double *dSigS_dev,
                   nf_sens_result *res);

/* ---- generalized adjoint and response-ratio sensitivity maps (no counterpart in the reference) -------------------------
 * Generalized perturbation theory for a ratio of linear functionals of the flux.  With M phi = (1/k) F phi as in DESIGN.md 14, two weight
 * fields w_a, w_b (ng N doubles [g*N + e], the layout of nf_upload_source; any finite values, fixed data),
 *   <w, phi> = sum_g sum_e w[g,e] |e| phibar_g(e)   (phibar = DOF 0, |e| the cell measure),        R = <w_a, phi> / <w_b, phi>,
 *   S+ = w_a |e| / <w_a, phi> - w_b |e| / <w_b, phi> on the DOF-0 rows, 0 on the higher moments (<S+, phi> = 0 by construction),
 * the generalized adjoint solves (M - F/k)^T Gamma+ = S+ with <Gamma+, F phi> = 0, and for a parameter p the weights do not depend on
 *   (1/R) dR/dp = -Gamma+^T (dM/dp - (1/k) dF/dp) phi:
 * the bilinear forms of nf_sensitivity with Gamma+ in place of phi+ and c = -1 in place of -k^2 / Nrm (so -c/k = 1/k).
 * nf_solve_gpt iterates from Gamma = 0 with the current flux, the adjoint flux and keff: per outer the adjoint fission term of the
 * previous iterate, one Gauss-Seidel group sweep from the LAST group to the first on the transposed scatter blocks, in place (exact for
 * downscatter-only data; nf_solve_adjoint's forward order is the reference's and stays), with the group solver nf_solve_keff picks, then
 * the deflation Gamma -= (<Gamma, F phi> / <phi+, F phi>) phi+.  Stops when ||Gamma_n - Gamma_n-1|| / ||Gamma_n|| < tol_flux or after
 * max_outer outers (NF_OK, converged = 0).  No normalisation, no acceleration: it contracts like the dominance ratio of the core.
 * Reads tol_flux, max_outer, max_inner, solver_type, solver_type_pushed from opts; use_coarse_init, use_cmfd and use_diagonal_solver
 * must be 0 and max_outer >= 1 (NF_ERR_ARG).  Gamma+, the weights and the two sums live on the handle until the next nf_upload_xs,
 * nf_build, nf_set_bc, nf_set_void or nf_destroy; a failed solve leaves no Gamma+.  The current flux, the adjoint flux, nf_get_J, the
 * warm k-eff state and the history are not touched; nf_info "last_direct" / "cg_form" report what ran.  Deterministic.
 * Errors: not built, no adjoint flux (nf_solve_adjoint or nf_set_phi_adj first; the current flux always exists, all ones before a
 * solve) -> NF_ERR_STATE; keff non-finite or <= 0, non-finite
 * weights, w_a a multiple of w_b (S+ identically zero) -> NF_ERR_ARG; <w_a, phi>, <w_b, phi> or phi+^T F phi zero or non-finite, a
 * non-finite iterate -> NF_ERR_NUMERIC; slabs and multi-rank teams, a handle with cut-out cells (nf_set_void) -> NF_ERR_UNSUPPORTED.
 * After any error the handle stays usable. */
typedef struct nf_gpt_result {
    double R;                   /* <w_a, phi> / <w_b, phi> */
    double wa_phi, wb_phi;      /* the two sums */
    double dgamma;              /* ||Gamma_n - Gamma_n-1|| / ||Gamma_n|| of the last outer */
    double ratio;               /* contraction: that change over the one of the outer before (0 after a single outer) */
    double deflation;           /* |<Gamma+, F phi>| / (||Gamma+|| ||F phi||) after the last deflation */
    double norm;                /* phi+^T F phi, the denominator of the deflation */
    int n_outer, cg_total, converged;
} nf_gpt_result;
int nf_solve_gpt(nf_handle h, const nf_keff_opts *opts, double keff, const double *wa_host, const double *wb_host, nf_gpt_result *res);
/* Gamma+ in the host DOF layout of nf_get_phi_adj / nf_set_phi_adj (ng n_phi doubles).  nf_get_gamma: NF_ERR_STATE without one;
 * nf_set_gamma allocates it if needed and keeps the weights the handle holds */
int nf_get_gamma(nf_handle h, double *gamma_host);
int nf_set_gamma(nf_handle h, const double *gamma_host);
/* The response and source kernels on their own: puts the weights on the handle (as nf_solve_gpt does; a Gamma+ solved for other weights
 * is dropped), sums_host[0..1] = <w_a, phi>, <w_b, phi> of the current flux (may be NULL) and S+ in the host DOF layout of nf_get_phi
 * (src_host, may be NULL).  Errors as nf_solve_gpt's for the state, the weights and the sums (the sums are stored before they are judged). */
int nf_gpt_source(nf_handle h, const double *wa_host, const double *wb_host, double *src_host, double *sums_host);
/* The maps (1/R) dR/dp per cell from the current flux, Gamma+ and keff: dD .. dSigS as nf_sensitivity defines them with (phi, Gamma+) and
 * c = -1; dWa[g,e] = |e| phibar_g(e) / <w_a, phi> and dWb[g,e] = -|e| phibar_g(e) / <w_b, phi> (ng N doubles each), the direct maps of the
 * weights themselves, with the sums taken from the current flux -- a caller whose weights are cross sections adds them to the indirect
 * maps.  DEVICE buffers; any may be NULL and is then skipped (the others come out bit-identical).  res: norm = <Gamma+, F phi> as
 * measured (0 up to rounding for a solved Gamma+; the maps do not divide by it), the keff used and the cell count.  Changes no state.
 * Errors: not built, no Gamma+ (nf_solve_gpt or nf_set_gamma first), dWa / dWb without weights on the handle -> NF_ERR_STATE; keff
 * non-finite or <= 0 -> NF_ERR_ARG; the rest as nf_sensitivity.  Option "sens_grid" caps the blocks of every GPT kernel too. */
int nf_gpt_sensitivity(nf_handle h, double keff, double *dD_dev, double *dSigR_dev, double *dNSF_dev, double *dChi_dev, double *dSigS_dev,
                       double *dWa_dev, double *dWb_dev, nf_sens_result *res);

/* ---- lambda-modes: the leading eigenpairs by block power iteration (no counterpart in the reference) -------------------
 * With K0 = blockdiag(S_g) - Ms and F = chi (x) Mf (the matrices of nf_solve_subcritical): the n_modes largest eigenvalues
 * k0 >= k1 >= ... of K0 phi = (1/k) F phi with their eigenvectors; adjoint = 1: K0^T phi+ = (1/k) F^T phi+ (chi and nuSigf swap roles,
 * transposed scatter blocks, groups swept in descending order).  Subspace iteration with a Rayleigh-Ritz step on A = K0^-1 F over a
 * block of n_block = n_modes + n_guard vectors (guard vectors speed the convergence up -- the rate is k[n_block] / k[n_modes - 1] -- and
 * are not returned); the start block is deterministic (cosine harmonics of the cell index).  Stops when the invariant-subspace residual
 * of the wanted block, max_i ||(Z_m - Q_m H_mm)_i|| / |k_i|, is below tol_flux and max_i |k_i - k_i,prev| below tol_keff, or after
 * max_outer outers (NF_OK, converged = 0).  Reads tol_keff, tol_flux, max_outer, max_inner, use_diagonal_solver (RT0-P0), solver_type,
 * solver_type_pushed from opts -- the group solver is the one nf_solve_keff picks; use_coarse_init / use_cmfd must be 0 (NF_ERR_ARG).
 * 1 <= n_modes, n_modes + n_guard <= NF_MODES_MAX <= the number of cells, else NF_ERR_ARG.  Undivided meshes only (slab teams and
 * multi-rank teams: NF_ERR_UNSUPPORTED, before any collective), and no upscatter block (NF_ERR_UNSUPPORTED: the Gauss-Seidel sweep
 * would lag those terms and the iteration operator would no longer be K0^-1 F).  A block that loses rank (A has fewer than n_block
 * independent directions) -> NF_ERR_NUMERIC.  A complex pair among the wanted modes at the stop: converged = 0, the pair's two vectors
 * span its plane, both k are the real part and both residuals the plane's.
 * Each returned mode has unit L2 norm over all groups and DOFs and the sign that makes sum Mf phi >= 0 (adjoint: the M_chi sum; where
 * that sum is below 1e-10 sum |Mf phi| the sign is what the iteration left).  Nothing else of h changes: current flux, adjoint flux,
 * warm state, history and nf_progress stay as they are.  The modes live on the handle until the next nf_build, nf_upload_xs or
 * nf_destroy; direct and adjoint modes are kept side by side.  Device memory during the call: 2 n_block ng n_phi doubles. */
#define NF_MODES_MAX 8
typedef struct nf_modes_result {
    double k[NF_MODES_MAX];        /* eigenvalues, descending; k[0] is k-eff */
    double residual[NF_MODES_MAX]; /* ||A phi_i - k_i phi_i|| / ||k_i phi_i||, A = K0^-1 F, of the returned vectors, from the last outer */
    double dominance_ratio;        /* k[1]/k[0]; 0 with n_modes == 1 */
    int n_modes, n_block, n_outer, cg_total, converged;
} nf_modes_result;
int nf_solve_modes(nf_handle h, const nf_keff_opts *opts, int n_modes, int n_guard, int adjoint, nf_modes_result *res);
/* mode i of the last nf_solve_modes of that kind (adjoint = 0 / 1) in the host DOF layout of nf_get_phi, all groups; NF_ERR_STATE before one */
int nf_get_mode(nf_handle h, int i, int adjoint, double *phi_host);
/* The two streaming kernels of the block iteration on their own, for blocks of b <= NF_MODES_MAX device vectors of length n, column-major
 * with leading dimension n.  nf_block_gram: QtZ = Q^T Z and ZtZ = Z^T Z (full symmetric), b x b, column-major, in one pass.
 * nf_block_rotate: Q <- Z C in place of Q (C: b x b, column-major) and, with the old Q in the same pass, res2[j] = the squared norm of
 * column j of Z_m - Q_m H (H: m x m, column-major; m <= b; m = 0: no residual, H_host / res2_host may be NULL).  Sums are formed in a
 * fixed order: the results are deterministic. */
int nf_block_gram(nf_handle h, int b, long n, const double *Q_dev, const double *Z_dev, double *QtZ_host, double *ZtZ_host);
int nf_block_rotate(nf_handle h, int b, int m, long n, double *Q_dev, const double *Z_dev, const double *C_host, const double *H_host, double *res2_host);

/* ---- space-time kinetics with delayed-neutron precursors (no counterpart in the reference) ----------------------------
 * Implicit Euler in time on the discrete system of nf_solve_subcritical.  With S_g, Ms, Mf, tf(phi) = sum_g' Mf_g' phi_g' as there,
 * W_p(e) = detJ(e) C-hat_pp the mass weight of a unit cross section (|e| at P0, no drop), velocities v_g, precursor families
 * i = 1..I (beta_i, lambda_i, beta = sum beta_i < 1), a delayed spectrum chi_d,g (ng values, the same in every cell; NULL: the handle's
 * Chi per cell) and the eigenvalue k0 given at begin, one step of length dt solves per group
 *   (S_g + diag(W / (v_g dt))) phi_g^{n+1} = chi~_g tf(phi^{n+1}) / k0 + sum_{g' != g} Ms[g <- g'] phi_g'^{n+1} + q_g
 *   q_g = W phi_g^n / (v_g dt) + chi_d,g sum_i lambda_i c_i^n / (1 + lambda_i dt),    chi~_g = chi_g - chi_d,g sum_i beta_i / (1 + lambda_i dt)
 * and then advances c_i^{n+1} = (c_i^n + dt beta_i tf(phi^{n+1}) / k0) / (1 + lambda_i dt).  The handle's Chi is the TOTAL steady-state
 * spectrum (the prompt part is what is left, (1 - beta) chi_p = chi - beta chi_d), so the state at begin is stationary for any chi_d.
 * The precursors live in tf-space: one vector of n_phi doubles per family; c_i^0 = beta_i tf(phi^0) / (lambda_i k0).
 * The left operator is the built operator of the cross sections with SigR_g + 1 / (v_g dt): a built twin of the handle (same mesh,
 * boundary types, device copies of the cross sections), cached and rebuilt only when dt changes or the handle has been built again
 * since (nf_info "transient_rebuilds" counts the builds).  The emission term is what k_group_rhs computes for the fixed-source solve
 * with chi~ for chi and 1 / k0 for the fission scale, its |chi~ / k0| < 1e-14 drop at P >= 1 included. */
#define NF_PRECURSORS_MAX 8
typedef struct nf_kinetics {
    int n_families;                     /* I, 0 .. NF_PRECURSORS_MAX; 0 = prompt neutrons only */
    double beta[NF_PRECURSORS_MAX];     /* delayed fractions beta_i >= 0, sum < 1 */
    double lambda[NF_PRECURSORS_MAX];   /* decay constants lambda_i > 0 */
    const double *velocity_host;        /* ng neutron velocities v_g > 0 */
    const double *chi_delayed_host;     /* ng values of the delayed spectrum, or NULL = the handle's Chi */
} nf_kinetics;
typedef struct nf_transient_result {
    double time;                /* t after the call's last completed step */
    double power;               /* P(t) / P(0) */
    double production;          /* P(t) = sum over g, e of nuSigf_g(e) |e| phibar_g(e) (nf_subcrit_result::production) */
    double phi_int;             /* sum over g, e of |e| phibar_g(e) */
    double precursors;          /* the precursor population: sum over i, e of c_i[e, dof 0] */
    double rebalance;           /* the factor f of the last outer (1 at the solution) */
    long n_steps;               /* steps completed since begin */
    int n_outer;                /* outers of this call, all steps */
    int n_outer_max;            /* the most outers one step of this call took */
    int cg_total;               /* inner iterations of this call */
    int n_unconverged;          /* steps of this call accepted after max_outer outers */
} nf_transient_result;
/* Starts a transient on a BUILT handle (NF_ERR_STATE otherwise) from its current flux phi^0 and the eigenvalue keff: records
 * P(0) (<= 0 or non-finite: NF_ERR_ARG), sets the equilibrium precursors and t = 0; a running transient is replaced.  Invalid data ->
 * NF_ERR_ARG: a v <= 0, a lambda <= 0, a beta < 0, sum beta >= 1, n_families outside 0 .. NF_PRECURSORS_MAX, a non-finite value, keff <= 0.
 * The transient owns a private copy of its flux (ng n_phi doubles) beside the precursors: every other solve on the handle changes the
 * handle's current flux, never the transient's state, and the next step resumes from the transient's own flux.  It survives
 * nf_upload_xs + nf_build on the handle -- that is how the caller perturbs the core; the next step uses the new cross sections.
 * Undivided meshes of one process only (slab teams, multi-rank teams: NF_ERR_UNSUPPORTED before any collective). */
int nf_transient_begin(nf_handle h, const nf_kinetics *kin, double keff);
/* n_steps implicit-Euler steps of length dt.  Per step a source iteration from phi^n on the twin (the handle's current flux is
 * untouched until the step completes): per outer k_fission, the Gauss-Seidel sweep of nf_solve_subcritical with the group solver
 * nf_solve_keff picks on the twin, and one scalar rebalance -- with U the sum of the DOF-0 rows of the right-hand sides the sweep used,
 * E the sum of the same rows of the emission + scatter terms the new iterate would produce and Q the sum of those rows of q, the iterate
 * is scaled by f = Q / (U - E) (f = 1 where that is not finite; exactly 1 at the solution).  Without it the iteration contracts like
 * 1 - beta per outer and is unusable (option "transient_rebalance" = 0, for measurements).  Stop test after the scaling:
 * ||x - x_prev|| / ||x|| < tol_flux and |P - P_prev| / |P| < tol_keff; after max_outer outers the step is accepted and counted in
 * n_unconverged.  On completion of a step the precursors advance, the new flux becomes the handle's current flux (nf_get_phi, nf_get_J,
 * nf_project_* see time t) and the time advances; power_host (n_steps doubles, may be NULL) receives P / P(0) after every step.
 * Reads tol_keff, tol_flux, max_outer, max_inner, solver_type, solver_type_pushed from opts; use_coarse_init, use_cmfd and
 * use_diagonal_solver must be 0, dt > 0 (finite), n_steps >= 1, max_outer >= 1 (NF_ERR_ARG); NF_ERR_STATE without nf_transient_begin or
 * with a handle that is not built.  A non-finite sum in any outer -> NF_ERR_NUMERIC: time, flux and precursors stay those of the last
 * completed step (res reports them) and the handle stays usable.  The warm k-eff state and nf_get_history are untouched; nf_progress
 * counts the outers of the call.  Deterministic.  nf_info "transient_steps": steps completed since begin.  The step operator takes
 * the options (nf_set_option) of h at every call, and nf_info on h reports its last CG solve ("cg_form", "cg_reductions", "last_xcd",
 * "xcd_solves", "xcd_refused", "last_direct"). */
int nf_transient_step(nf_handle h, const nf_keff_opts *opts, double dt, int n_steps, double *power_host, nf_transient_result *res);
/* precursor family `family` (0-based) of the running transient in the host DOF layout of nf_get_phi, one group's length (n_phi) */
int nf_get_precursors(nf_handle h, int family, double *c_host);
/* ends the transient and releases the twin and the precursors (nf_destroy does the same); NF_OK without one */
int nf_transient_end(nf_handle h);

/* ---- adjoint-weighted kinetics parameters and dynamic reactivity (no counterpart in the reference) ---------------------
 * What a state or a transient IS in point-kinetics terms: reactivity rho (also in dollars), beta_eff with its split over the families and
 * the generation time Lambda, as bilinear functionals weighted with the handle's adjoint flux.  Notation of the sections above: all vectors
 * in DOF layout, every product the plain dot product of coefficient vectors (the matrices carry the mass weights);
 *   K0 = blockdiag(S_g) - Ms, the BUILT operator of the handle (never the dt-shifted step operator),  F = chi (x) Mf,
 *   tf(phi) = sum_g' Mf_g' phi_g',  W_p(e) the mass weight of a unit cross section,  w = the handle's adjoint flux (nf_solve_adjoint or
 *   nf_set_phi_adj),  chi_d per group and DOF as nf_transient_begin takes it (the ng given values in every cell, or the handle's Chi per
 *   cell when NULL),  k0 the given eigenvalue.
 * Raw forms, all returned:
 *   production         = w^T F phi = sum_j (sum_g chi_g w_g)_j tf_j                    (nf_sensitivity's Nrm)
 *   delayed_production = sum_j (sum_g chi_d,g w_g)_j tf_j
 *   removal_leakage    = sum_g w_g^T S_g phi_g
 *   scatter            = sum_{g != g'} w_g^T Ms[g <- g'] phi_g'                         (the built blocks)
 *   amplitude          = T = sum_g w_g^T diag(W / v_g) phi_g
 *   c_amp[i]           = C_i = sum_j (sum_g chi_d,g w_g)_j c_i,j                        (nf_transient_kinetics only; 0 otherwise)
 * The 1e-14 drop of chi / k at P >= 1 is ignored, as in nf_sensitivity.  Derived on the host from those, in exactly these expressions:
 *   fw = production / k0                       rho = (production / k0 - removal_leakage + scatter) / fw
 *   beta_eff_i[i] = beta_i delayed_production / production,  beta_eff = their sum (in the order of the families)
 *   gen_time = Lambda = amplitude / fw         rho_dollars = rho / beta_eff (0 when beta_eff = 0)
 * Two identities hold for ANY weight w:
 *   1. exact perturbation: with (phi', k') the eigenpair of the built operator, rho = 1 - k0 / k';
 *   2. discrete point kinetics: after every completed implicit-Euler step of nf_transient_step, with everything evaluated on phi^{n+1},
 *      c^{n+1} and the handle's current cross sections, (T^{n+1} - T^n) / dt = (rho - beta_eff) fw + sum_i lambda_i C_i^{n+1}.
 * beta_eff_i = beta_i exactly when chi_d is NULL.  A caller who wants the classical weighting solves the adjoint at the initial critical
 * state, THEN perturbs and rebuilds: the adjoint flux is kept across nf_upload_xs / nf_build.
 * nf_kinetics_params evaluates the forms on the handle's current flux with the kinetics data and keff given (n_families precursor
 * families enter beta_eff_i only); nf_transient_kinetics on the running transient's own flux and precursors, with the kinetics data and
 * the keff of nf_transient_begin, at the transient's time.  Both form y_g = S_g phi_g with the launch functions of nf_schur_apply under
 * the handle's options, then all 5 + I sums in one streaming pass (k_kin_forms) whose block shares are added in a fixed order: the
 * results are deterministic.  Device memory during the call: ng n_phi doubles for y, n_phi doubles for W when no transient runs (a
 * running transient lends its copy), and 13 x 1024 doubles of block shares.  nf_set_option "kin_grid" = blocks of 256 threads of that pass
 * (default and cap 1024; it walks larger meshes with a grid stride).
 * Neither call changes any state: the flux, the adjoint flux, Gamma+, nf_get_J, the warm k-eff state, the history, nf_progress, the
 * timers and the transient (time, flux, precursors, step operator, nf_info "transient_rebuilds") are untouched; nf_kinetics_params works
 * with a transient running and leaves it alone.
 * Errors (the text names the function): handle not built, no adjoint flux, nf_transient_kinetics without a running transient ->
 * NF_ERR_STATE; invalid kinetics data (the rules of nf_transient_begin), keff non-finite or <= 0, res NULL -> NF_ERR_ARG; production zero
 * or non-finite, or any non-finite form -> NF_ERR_NUMERIC (res then still holds the raw forms, the derived fields are 0); slab teams,
 * multi-rank teams, a handle with cut-out cells (nf_set_void) and meshes of 2^32 cells or more -> NF_ERR_UNSUPPORTED, before any launch
 * or collective.  After any error the handle stays usable. */
typedef struct nf_pk_result {
    double rho, rho_dollars, beta_eff, beta_eff_i[NF_PRECURSORS_MAX], gen_time, fw;
    double production, delayed_production, removal_leakage, scatter, amplitude, c_amp[NF_PRECURSORS_MAX];
    double keff, time;            /* k0 used; t of the transient (0 for nf_kinetics_params) */
    int n_families, from_transient;
} nf_pk_result;
int nf_kinetics_params(nf_handle h, const nf_kinetics *kin, double keff, nf_pk_result *res);  /* the handle's current flux */
int nf_transient_kinetics(nf_handle h, nf_pk_result *res);  /* the running transient's own flux, precursors, kin and k0 of begin */

/* NeutFEM::SolveCoarse (src/NeutFEM.cpp:2380-2611): returns k_coarse and the prolonged flux
 * (ng*n_phi doubles, host) without touching the fine solution. */
int nf_solve_coarse(nf_handle h, const nf_keff_opts *opts, double *k_coarse, double *phi_host);
/* the two halves of SolveCoarse on their own (undivided meshes): nf_coarsen returns a BUILT RT0-P0 handle on the mesh merged by
 * (rx, ry, rz) with block-mean cross sections (src/NeutFEM.cpp:2409-2556; the caller solves and destroys it), nf_prolong
 * injects the coarse handle's current flux into the fine handle's (piecewise constant, higher moments zero, :2585-2606) */
int nf_coarsen(nf_handle h, int rx, int ry, int rz, nf_handle *coarse);
int nf_prolong(nf_handle coarse, nf_handle fine);

/* Sol_Phi_ / Sol_J_ (include/NeutFEM.hpp:380-388) and NeutFEM::ResetFlux (src/NeutFEM.cpp:347-354) */
int nf_set_phi(nf_handle h, const double *phi_host);
int nf_get_phi(nf_handle h, double *phi_host);
int nf_get_J(nf_handle h, double *J_host);   /* on a slab: the slab's own faces (shared interface planes appear in both neighbours); collective */
int nf_reset_flux(nf_handle h);
int nf_set_warm_state(nf_handle h, int has_valid_keff, double last_keff);
int nf_get_warm_state(nf_handle h, int *has_valid_keff, double *last_keff);

/* per-outer history of the last nf_solve_keff: k, dk, dphi (n_outer each), cg (n_outer*ng) */
int nf_get_history(nf_handle h, double *k, double *dk, double *dphi, int *cg, int cap_outer);

/* profiling: kernels timed with HIP events on the solver's stream (opts.profile / nf_time_schur_apply).
 * name in {"schur_x","schur_y","schur_z","schur_apply","schur_z1"}: number of timed launches and their total ms. */
int nf_profile_get(nf_handle h, const char *name, long *count, double *total_ms);
int nf_profile_reset(nf_handle h);
/* the same counters, with the iteration counts of the last solve, as one JSON object */
int nf_timers(nf_handle h, char *json_buf, size_t len);
/* Read-only report of the launch plan: what the next Schur apply on this handle's mesh (or slab) would launch, as one JSON object
 * {"in_cg", "form", "xsol_batch", "slab", "fused", "lean", "single_reduce", "split_dot", "xy_overlap", "passes": [...]}.  in_cg = 0: a plain nf_schur_apply /
 * nf_team_schur_apply; in_cg = 1: the apply inside an iteration of the launch-path CG.  "form": the form of the CG iteration the next
 * CG solve is planned to run (xcd, fuse3, lean, fused, classic, team_lean, team_vec, team_sr; "" for in_cg = 0), from the one function
 * the solve itself asks; "fused", "lean" and "single_reduce" follow from it.  "xsol_batch": the M that solve is planned to run with
 * (option "xsol_batch"; 1 for in_cg = 0 and wherever the batched update does not apply).  The forms xcd and fuse3 launch no Schur pass of their own:
 * for them the passes are those of the launch path (lean) the solve falls back to.
 * One entry of "passes" per direction that exists; the z direction of a slab has two (mode 1 = endpoint pass, mode 2 = accumulation
 * pass).  Per entry: "dir" (x / y / z), "mode", "family" (x = k_schur_x, s = k_schur_s, c = k_schur_c, endpoint_w = k_endpoint_w),
 * "SEG" (cells per segment), "NCH" (chunks per lane / block), "TX" (columns per block; lanes per line for x), "NSEG" (segments per
 * line; NS of the chunked kernel), "grid" [x, y, z], "block", "nt" (streaming loads), "zw" (the pass's share
 * of x.y in the z.w form), "xcd_order" (the XCD-contiguous tile order is requested) and "xcd_permutes" (requested, and the tile count
 * is a multiple of 8 beyond 8: tiles really move), "fold" (accumulation pass of a slab: it forms the separator values
 * itself), "dict" (the pass reads its line factors from the table of distinct lines, see "line_dict") and "early" (level of early vector
 * loads of a table-backed chunked pass, option "c_early"; 0 for every other pass); y / z passes also "stage" (the staged form of
 * k_schur_s, option "s_stage"; "variant" then ends in "stage") and "blocks" (workgroups launched: the tiles of "grid", or the
 * persistent blocks of a staged pass -- "grid" stays the tile grid) and "full" (the whole-tile form of the pass, option "tile_full";
 * never part of "variant"); at the top level "line_dict":
 * {"x", "y", "z"}, the distinct lines of the largest group per direction (0: no table in use).  Built from the predicates the launch functions
 * themselves call.  The one thing it does besides reporting: where the next apply would first build the tables of distinct lines
 * (once per build), the report builds them, since whether a direction verifies is part of the plan; otherwise it launches nothing
 * and changes no state.  A slab team must have been prepared (one team apply or solve since its options last changed). */
int nf_apply_plan(nf_handle h, int in_cg, char *json_buf, size_t len);
/* times `reps` back-to-back Schur applies on group g (random x) with HIP events; average ms per apply */
int nf_time_schur_apply(nf_handle h, int g, int reps, double *avg_ms);
/* LocalMatrices::Compute(e, D, Sigma) (src/FEM.cpp:748-953) on the device, literally: the dense A_loc (n_Jloc x n_Jloc), B_loc
 * (n_loc x n_Jloc) and C_loc (n_loc x n_loc) of `n_elems` elements of group g by the reference's tensor Gauss quadrature (order
 * 2 max(k, m) + 3 with its 7 -> 5-point fallback, include/FEM.hpp:115-120), row-major like GetA / GetB / GetC, D = D_g(e),
 * Sigma = SigR_g(e); local DOF order of src/FEM.cpp:729-745.  One element per workgroup, quadrature points and basis values
 * staged in LDS.  The solver itself never forms these matrices (closed forms); this entry exists to check them
 * against the quadrature on the device and to measure the one dense contraction of the code base in both forms:
 * variant 0 = fp64 FMA, 1 = v_mfma_f64_16x16x4_f64.  reps >= 1 timed launches, average ms in *avg_ms (may be NULL).
 * Needs nf_upload_xs (not nf_build). */
int nf_local_matrices(nf_handle h, int g, int n_elems, const int *elems_host, double *A_host, double *B_host, double *C_host,
                      int variant, int reps, double *avg_ms);
/* HBM microbenchmark: `reps` device-to-device streaming copies of `bytes` (read + write counted) -> GB/s; the
 * roofline is reported against the 8 TB/s spec and against this measured figure */
int nf_time_device_copy(nf_handle h, size_t bytes, int reps, double *gbps);

/* tuning knobs (no reference counterpart):
 *   "s_tx" (0 auto, 8, 16, 32, 64) columns per block and "s_seg" (0 auto, 4, 8, 16, 32) cells per register segment of the y/z line
 *   kernels; "s_wsmin" segments per line from which whole wavefronts scan the segment summaries (default 64);
 *   "xcd" gives each XCD one contiguous range of tiles: bit 0 the y passes, bit 1 the z passes; default -1 = the y passes of meshes
 *   beyond "nt_min_cells" (256^3: y pass 133 -> 123 us; the z passes lose with it, smaller meshes see nothing);
 *   "cg_batch" CG iterations launched between host checks of the device-side stop flag (0 = automatic);
 *   "cg_fuse" (default 1) folds x += alpha p, p = r + beta p into the next pass that reads p (bit-identical iterates);
 *   "cg_lean" (default 1) lets the consumer of a reduction derive the CG scalars itself: no finalize launches on undivided meshes of at
 *   most "cg_lean_max_cells" cells (default 4 Mi; "cg_lean_grid" = blocks of the residual update), no k_cg_logic launches on slab teams;
 *   "cg_fuse3" (default 1) runs the x, y and z passes of an apply as ONE launch (two launches per CG iteration) on undivided meshes of
 *   at most "cg_fuse3_max_cells" cells (default 400 000: above, the four-launch lean iteration is faster);
 *   "cg_xcd" (default 1) runs every CG solve of an undivided mesh (any order, x lines of at most 128 cells) with "cg_xcd_min_cells" ..
 *   "cg_xcd_max_cells" unknowns per group (default 2000 .. 28000) as ONE launch on the workgroups of XCD "cg_xcd_id" (default 0; 8..15 name none: the solve falls back,
 *   for tests), "cg_xcd_groups" (default 32) workgroups per XCD being launched; nf_info "xcd_solves" counts its solves, "xcd_refused"
 *   the times its workgroups did not assemble and the launch path took over; "keff_xcd" (default 1) runs the whole SolveKeff of such a mesh
 *   (iterative full-Schur path, no CMFD) in one launch of the same kind (nf_info "last_path" 3);
 *   "resident" (default 1) runs the whole SolveKeff of an undivided mesh with at most "resident_max_dofs" flux DOFs per group (default
 *   2500) in one workgroup and one launch; "resident_lds" (default 1) keeps its CG vectors and factors in LDS as far as they fit;
 *   "resident_serial" (default 1): meshes whose moments, factors and directions' contributions all fit in LDS run one lane per
 *   (direction, transverse mode, line) with serial sweeps instead of the segmented scans (nf_info "last_resident_serial"), up to
 *   "resident_serial_max_dofs" flux DOFs per group (default 5120, the structural limit; "resident_max_dofs" lowers it too);
 *   "resident_two_sided" (default 1): lines of at least 4 cells are swept by two lanes that meet in the middle;
 *   "direct_max_dofs" (default 6000, at most 8192): explicit-S branch with a dense S^-1 up to this many flux DOFs per group, beyond it
 *   CG to 1e-14 stands in (nf_info "direct_standin_unconverged" counts group solves that did not get there);
 *   "host_pub" (default 1): the host reads the CG scalars and the outer iteration's sums from a mapped host page that a one-thread
 *   kernel fills (polled), not through a device-to-host copy and a stream drain;
 *   "prof_every" (default 8): a profiled solve (nf_keff_opts::profile) brackets every n-th Schur apply with events, not each one;
 *   "nt_loads" (default 1): on undivided RT0-P0 meshes of more than "nt_min_cells" cells (default 8 000 000: from there on the streams no longer live in the
 *   256 MB memory-side cache between launches) the direction passes read their streams with non-temporal loads;
 *   "outer_dev" (default 1) keeps the outer loop of the diagonal-Schur path on the device (undivided mesh, no CMFD);
 *   "sep_fold" (default 1): slab teams form the separator values inside the accumulation pass of the z lines (no k_separators launch);
 *   "cg_single_reduce" (default -1 = while the largest slab of the team has at most "cg_single_reduce_max_cells" cells, default unlimited; 1 always,
 *   0 never): RT0-P0 slab teams run the CG with ONE cross-rank reduction per iteration (p.q, q.q, r.q and the measured |r|^2 in one all-reduce
 *   of five doubles; r -= alpha q rides in the endpoint pass of the z lines; nf_info "cg_reductions" = 1) instead of the reference
 *   recurrence's two ("vec_reduce" then picks between all-reducing the block partials themselves and k_finalize + scalars);
 *   "endpoint_weights" (default 1): that CG's endpoint pass forms the chain-end responses of every z line as weighted sums of the line's cells
 *   (weights measured once per BuildMatrices with the chain solve itself: nz launches per group, 16 B per cell and group of HBM) instead of
 *   solving the chain -- a streaming kernel with the deferred CG update in the same sweep (nf_info "endpoint_weights");
 *   "xchg_comm" (default 0): the interface planes travel on a communicator of their own (created collectively before the next solve;
 *   nf_info "xchg_comm") instead of sharing the one the all-reduces use;
 *   "line_dict" (default -1): undivided RT0-P0 meshes in the streaming regime ("nt_min_cells") whose lines repeat -- cores built from a few
 *   assembly types on a uniform mesh -- read L, 1/d (and the C diagonal, x pass) from a table of the DISTINCT lines of a direction instead of
 *   streaming them per cell.  The lines are identified on the stored factors (128-bit fingerprints, grouped on the host) and every line is
 *   compared bit for bit with its representative before a table is used, so the results are bit-identical to the streaming path; the tables
 *   are built by the first apply, solve or nf_apply_plan after a build.  -1 = the directions that gain at the benchmark size,
 *   0 = off, 1 = every direction whose lines qualify (every group verified, at least fourfold repeats, table within the cap);
 *   "line_dict_dirs" (default 7): bit 0 = x, bit 1 = y, bit 2 = z; "line_dict_max_bytes" (default 524288): cap of one group's table of one
 *   direction; "line_dict_fp_bits" (default 128, tests only): low bits of the fingerprint that are kept, so that collisions can be made.
 *   Changing any option drops the tables; nf_apply_plan reports "dict" per pass and "line_dict": {"x", "y", "z"} = distinct lines of the
 *   largest group (0: the direction streams);
 *   "c_early" (default -1): the chunked y / z pass on its table (family c with "dict") requests the vector loads of its tile ahead of the
 *   sweeps that hide them: 1 = x of both chunks in one round trip, 2 = also y of the upper chunk before that chunk's forward sweep and y of the
 *   lower chunk before the backward half, 0 = each load where it is used, -1 = the level that measurably gains.  Only loads
 *   move: the results are bit-identical at every level.  nf_apply_plan reports the level per pass as "early";
 *   "s_stage" (default -1): staged form of the table-backed y / z passes on k_schur_s (plain RT0-P0 lines, nx a multiple of the tile width): a
 *   launch of "s_stage_grid" blocks (default 0 = one per compute unit) walks the tiles, and the next tile's vector is copied into LDS while
 *   the current one is scanned.  -1 = the directions that measurably gain, where a block has at least two tiles, 0 = off,
 *   1 = wherever eligible.  Only loads move: the results are bit-identical.  nf_apply_plan reports "stage" and "blocks" per pass;
 *   "tile_full" (default -1): whole-tile form of the staged y / z pass on k_schur_s ("stage") and of the chunked pass on its table with early
 *   loads (family c, "dict", "early" 2).  Taken where the tile grid has no partial tile: nx a multiple of the tile width, lines of exactly
 *   8 NSEG cells (chunked: 16 NS), one thread per (column, segment) in the block, summaries not scanned by whole wavefronts ("s_wsmin").  The
 *   per-access predicates of the body are then true at compile time: straight-line loads and stores at 32-bit byte offsets.  Values and
 *   arithmetic are untouched: the results are bit-identical.  -1 and 1 = wherever eligible, 0 = the predicated bodies; a refused staged
 *   launch falls back to the predicated unstaged pass as before.  nf_apply_plan reports "full" per y / z pass;
 *   "xsol_batch" (default -1): the fused form on an undivided RT0-P0 mesh (x lines of at most 1024 cells) updates x_sol in every M-th x pass
 *   only: each new direction goes into the next slot of a ring of M buffers (M - 1 extra vectors of n_phi doubles per handle, allocated at
 *   the first such solve, shared by all groups, dropped when the option is set; a refused allocation leaves the handle at M = 1), every M-th
 *   pass applies the M deferred updates oldest first and the end of the solve applies what is pending.  Same fma chain per cell: the
 *   results are bit-identical.  1 (or 0) = every pass, 2 .. 8 = that M wherever eligible, -1 = 4 beyond "cg_lean_max_cells" cells, else 1
 *   (DESIGN.md 6f).  Other forms, slab teams and higher orders keep M = 1.  nf_apply_plan reports the M as "xsol_batch";
 *   "transient_rebalance" (default 1): nf_transient_step scales the iterate of every outer by the balance factor f; 0 = plain source
 *   iteration (same fixed point, a contraction of about 1 - beta per outer: for measurements);
 *   "kin_grid" (default 1024, at most 1024): blocks of 256 threads of the k_kin_forms pass of nf_kinetics_params / nf_transient_kinetics
 *   (larger meshes are walked with a grid stride; 1 makes the stride wrap on any mesh, for tests); "sens_grid" the same for nf_sensitivity.
 * The handles the library derives from h solve under h's options: the step operator of nf_transient_step (at every call), the fine
 * handle of nf_refine / nf_zoom_resolved (as they are when it is made) and, for the options that choose its solve, the coarse twin of SolveCoarse.
 * nf_info keys beyond the mesh sizes: "last_path" (0 host-driven outer loop, 1 diagonal device loop, 2 resident kernel, 3 one-XCD kernel),
 * "last_direct" (0 CG as configured, 1 dense S^-1, 2 CG to 1e-14 standing in), "line_dict_rejected" (mask of the directions whose table the
 * bit-for-bit verification refused: a fingerprint collision, not an error), "line_dict_bytes" (device memory of the tables and line ids),
 * "transient_steps" (steps completed since nf_transient_begin; 0 without a transient), "transient_rebuilds" (builds of the step operator
 * since nf_transient_begin). */
int nf_set_option(nf_handle h, const char *key, long value);
/* the value a key holds now, as nf_set_option normalised it (retired keys read 0); an unknown key -> NF_ERR_ARG */
int nf_get_option(nf_handle h, const char *key, long *value);

/* raw device-memory helpers so callers without torch can drive the *_dev entry points */
/* free / total HBM of a device (hipMemGetInfo): sizing of decompositions, leak checks */
int nf_mem_info(int device, size_t *free_bytes, size_t *total_bytes);
int nf_dev_alloc(nf_handle h, size_t bytes, void **ptr_dev);
int nf_dev_free(nf_handle h, void *ptr_dev);
int nf_memcpy_h2d(nf_handle h, void *dst_dev, const void *src_host, size_t bytes);
int nf_memcpy_d2h(nf_handle h, void *dst_host, const void *src_dev, size_t bytes);
int nf_synchronize(nf_handle h);
/* the hipStream_t every kernel of this handle is launched on */
void *nf_stream(nf_handle h);

#ifdef __cplusplus
}
#endif
#endif
